"""The NeRF render restricted to 3D boxes on the MI355X (csrc/nerfrender.hip: nerfrender_boxmask / boxzero / boxcount kernels, the
flagged trunk of csrc/nerf_mlp.cuh) through ops.nerf_render_boxes and the nerf_render_boxes command line; DESIGN.md 3.25.

The reference is tests/nerf_boxes_ref.py in float64.  Per case, boxes, mode and tensor the device must lie within 8 x the float32
checker's deviation from the float64 checker, floored at one float32 ulp of the largest magnitude, over the rays without an undecided
sample, with NaN in the same places.  The bounds are computed here; tests/golden/nerf_boxes_bounds.json records what was seen.
Seen on the MI355X: at most 0.39 of a bound (two_pass_6x8, rotated, keep, depth_map), exactly 0 wherever the checker is 0, no ray left out."""
import os

import numpy as np
import pytest

import nerf_boxes_ref as B
import nerf_render_ref as V
from nerf_rpn_amd import lib, ops
from nerf_rpn_amd.scripts import nerf_render_boxes as X
from nerf_boxes_ref import box_refs  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

ALL = [(n, w, m) for n in B.NAMES for w in B.BOXES for m in B.MODES]
IDS = ["-".join(x) for x in ALL]
_WEIGHTS, _RUNS = {}, {}


def weights_of(c, dtype="fp32"):
    if (c.name, dtype) not in _WEIGHTS:
        _WEIGHTS[c.name, dtype] = ops.nerf_grid_pack(c.state, c.cfg, dtype)
    return _WEIGHTS[c.name, dtype]


def frame_args(c, rays=None):
    kw = dict(near=c.near, far=c.far, bb_center=c.bb_center, bb_scale=c.bb_scale, z_samples=c.z_samples, n_samples=c.n_samples,
              return_samples=True, return_stages=True)
    rays = c.rays if rays is None else rays
    if rays is not None:
        kw["rays"] = rays
    else:
        kw.update(H=c.H, W=c.W, intrinsic=c.intrinsic, c2w=c.c2w)
    return kw


def flat(c, out, frame):
    """One row per ray: the maps of a frame call come as (H, W, ...), the stages and tile counts as they are."""
    lead = 2 if frame else 1
    return {k: (v if k in ("raw1", "z2", "tiles_run", "tiles_total") else v.reshape(c.n_rays, *v.shape[lead:])).cpu().numpy()
            for k, v in out.items()}


def run(c, boxes, mode, dtype="fp32", rays=None, **kw):
    args = dict(frame_args(c, rays), **kw)
    return flat(c, ops.nerf_render_boxes(weights_of(c, dtype), c.cfg, boxes, mode, **args), "H" in args)


def plain(c, dtype="fp32"):
    args = frame_args(c)
    return flat(c, ops.nerf_render(weights_of(c, dtype), c.cfg, **args), "H" in args)


def device_run(box_refs, name, which, mode):
    """The default call of a case (skip=True), made once and shared."""
    if (name, which, mode) not in _RUNS:
        c, boxes = box_refs(name, which, mode)[:2]
        _RUNS[name, which, mode] = run(c, boxes, mode)
    return _RUNS[name, which, mode]


def same_bits(a, b, keys=None):
    for k in (keys or a):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k


RESULT_KEYS = ("rgb_map", "depth_map", "acc_map", "disp_map", "depth_std", "z_vals", "weights", "raw1", "z2")


def result_keys(c):
    return tuple(k for k in RESULT_KEYS if k != "z2" or not c.plain)


@pytest.mark.parametrize("name,which,mode", ALL, ids=IDS)
def test_every_tensor_within_bound_of_fp64(dev, box_refs, name, which, mode):
    c, boxes, table, f32, f64, out = box_refs(name, which, mode)
    got = device_run(box_refs, name, which, mode)
    keep, bad = ~out, []
    for k in B.TENSORS:
        if k not in f64:
            continue
        assert got[k].dtype == np.float32 and got[k].shape == f64[k].shape, (k, got[k].shape, f64[k].shape)
        bound, ref_err = B.bound_of(f32, f64, k, keep)
        err, same = B.error_of(got, f64, k, keep)
        print(f"{name} {which} {mode}: {k} error {err:.3g} (bound {bound:.3g}, float32 checker {ref_err:.3g}), NaN positions equal: {same}")
        if not (same and err <= bound):
            bad.append((k, err, bound, same))
    assert not bad, (name, which, mode, bad)


@pytest.mark.parametrize("name", B.NAMES)
@pytest.mark.parametrize("dtype", ops.NERF_DTYPES)
def test_identities_with_the_plain_render(dev, box_refs, name, dtype):
    c = box_refs(name, "all", "keep")[0]
    ref = plain(c, dtype)
    for which, mode in (("all", "keep"), ("none", "remove"), ("k0", "remove")):
        got = run(c, B.case_boxes(c, which), mode, dtype)
        assert sorted(k for k in got if not k.startswith("tiles")) == sorted(ref)
        same_bits(ref, got)
        assert np.array_equal(got["tiles_run"], got["tiles_total"])


@pytest.mark.parametrize("name,which,mode", ALL, ids=IDS)
def test_skipping_changes_no_bit_and_counts_the_checkers_tiles(dev, box_refs, name, which, mode):
    c, boxes, table, f32, f64, out = box_refs(name, which, mode)
    a = device_run(box_refs, name, which, mode)
    b = run(c, boxes, mode, skip=False)
    same_bits(a, b, result_keys(c))
    total = [B.tiles_total(c.n_rays, c.s1), 0 if c.plain else B.tiles_total(c.n_rays, c.s1)]
    assert a["tiles_total"].dtype == np.int64 and a["tiles_total"].tolist() == total and b["tiles_total"].tolist() == total
    assert b["tiles_run"].tolist() == total
    if not out.any():
        want = [B.tiles_counted(f64["counted1"]), 0 if c.plain else B.tiles_counted(f64["counted2"])]
        assert a["tiles_run"].tolist() == want, (a["tiles_run"], want)
    assert (a["tiles_run"] <= a["tiles_total"]).all()
    if which == "rows" and mode == "keep":
        assert a["tiles_run"][0] < a["tiles_total"][0]
    if which == "k0" and mode == "keep":
        assert not a["tiles_run"].any()


@pytest.mark.parametrize("name", B.NAMES)
def test_repeats_chunks_and_rays_are_bit_equal(dev, box_refs, name):
    for which, mode in (("overlap", "keep"), ("rows", "remove")):
        c, boxes, table, f32, f64, out = box_refs(name, which, mode)
        a = device_run(box_refs, name, which, mode)
        same_bits(a, run(c, boxes, mode))
        for chunk in (5, 12 if name != "rays_130x13" else 7):        # 5 rays; 12 x 8 or 7 x 13 points split a 64-point tile
            b = run(c, boxes, mode, chunk=chunk)
            same_bits(a, b, result_keys(c))
            assert b["tiles_total"][0] == B.tiles_total(c.n_rays, c.s1, chunk)
            if not out.any():
                assert b["tiles_run"][0] == B.tiles_counted(f64["counted1"], chunk)
                if not c.plain:
                    assert b["tiles_run"][1] == B.tiles_counted(f64["counted2"], chunk)
        if c.rays is None:
            same_bits(a, run(c, boxes, mode, rays=c.rays32), result_keys(c))


@pytest.mark.parametrize("name,which,mode", [x for x in ALL if x[1] in ("rotated", "overlap", "origin", "aabb6")],
                         ids=[i for x, i in zip(ALL, IDS) if x[1] in ("rotated", "overlap", "origin", "aabb6")])
def test_uncounted_samples_have_weight_zero(dev, box_refs, name, which, mode):
    c, boxes, table = box_refs(name, which, mode)[:3]
    got = device_run(box_refs, name, which, mode)
    o, d = c.rays32[:, None, :3].numpy(), c.rays32[:, None, 3:].numpy()
    pts = o + d * got["z_vals"][:, :, None]                    # float32: the product rounded, then the sum, as the kernels form it
    assert pts.dtype == np.float32
    m = B.counted(pts, table, mode)
    assert (~m).any() and (got["weights"][~m] == 0).all()
    z1 = got["z_vals"][0] if c.plain else np.asarray(c.z_samples, dtype=np.float32)
    first = B.counted(o + d * z1[None, :, None], table, mode)
    assert not got["raw1"][~first].any() and not np.signbit(got["raw1"][~first]).any()          # +0, all four values


def test_refusals_that_reach_the_device_layer(dev, box_refs, monkeypatch):
    c, boxes = box_refs("plain_6x8", "rotated", "keep")[:2]
    too_many = np.tile(B.box_table(boxes), (1025, 1))
    with monkeypatch.context() as m:
        m.setattr(ops, "nerf_box_table", lambda b: too_many)
        with pytest.raises(lib.NrpnError, match="1025 boxes"):
            run(c, boxes, "keep")
    real = ops.call

    def null_table(name, *args):
        args = list(args)
        assert name in ("nerfrender_frame_boxes", "nerfrender_rays_boxes") and args[-5] == 1
        args[-6] = None
        return real(name, *args)
    with monkeypatch.context() as m:
        m.setattr(ops, "call", null_table)
        with pytest.raises(lib.NrpnError, match=r"null box table \(1 boxes\)"):
            run(c, boxes, "keep")
        with pytest.raises(lib.NrpnError, match=r"null box table \(1 boxes\)"):
            run(c, boxes, "keep", rays=c.rays32)
    with pytest.raises(lib.NrpnError, match="mode 2"):
        with monkeypatch.context() as m:
            m.setattr(ops, "nerf_check_box_mode", lambda mode: 2)
            run(c, boxes, "keep")


def test_cli_end_to_end(dev, tmp_path):
    from PIL import Image
    c = V.case_inputs(V.CASES[V.NAMES.index("odd_5x7")])
    argv = V.write_run(tmp_path, c)
    o, d = V.get_rays(c.H, c.W, c.intrinsic, c.c2w)
    centre = (o[c.H // 2, c.W // 2] + 1.2 * d[c.H // 2, c.W // 2]).double().numpy()
    world = np.array([[*centre, 0.9, 0.7, 0.8, 0.3], [*(centre + 0.4), 0.5, 0.5, 0.5, -0.7], [*(centre - 0.3), 0.6, 0.6, 0.6, 0.0]])
    feats = dict(resolution=np.array([64, 48, 40]), bbox_min=centre - np.array([3.0, 2.5, 2.0]), bbox_max=centre + np.array([3.0, 2.0, 2.5]),
                 scale=1.0, offset=0.0, from_mitsuba=False, from_ddp_nerf=True)
    diag = feats["bbox_max"] - feats["bbox_min"]
    grid = np.concatenate([(world[:, :3] - feats["bbox_min"]) / diag * feats["resolution"], world[:, 3:6] / diag * feats["resolution"], world[:, 6:]], 1)
    np.savez(tmp_path / "proposals.npz", proposal=grid, score=np.array([0.8, 0.9, 0.3]))
    np.savez(tmp_path / "features.npz", **feats)
    kept = ops.nerf_boxes_to_world(grid[[1, 0]], feats)              # score > 0.5, best first
    source = ["--proposals", str(tmp_path / "proposals.npz"), "--features", str(tmp_path / "features.npz")]
    kw = dict(H=c.H, W=c.W, intrinsic=c.intrinsic, c2w=c.c2w, near=c.near, far=c.far, bb_center=c.bb_center, bb_scale=c.bb_scale,
              z_samples=c.z_samples)

    written = X.main(argv + source)
    out_dir = str(tmp_path / "out")
    assert written == [(os.path.join(out_dir, "0_rgb.png"), os.path.join(out_dir, "0.npz"))]
    op = {k: v.cpu().numpy() for k, v in ops.nerf_render_boxes(c.state, c.cfg, kept, "keep", **kw).items()}
    img = np.asarray(Image.open(written[0][0]))
    assert img.dtype == np.uint8 and np.array_equal(img, V.to8b(op["rgb_map"]))
    with np.load(written[0][1]) as f:
        for k, name in (("depth", "depth_map"), ("depth_std", "depth_std"), ("acc", "acc_map")):
            assert f[k].dtype == np.float32 and np.array_equal(f[k], op[name]), k
    empty = op["acc_map"] == 0
    assert empty.any() and not empty.all() and not img[empty].any()

    written = X.main(argv + source + ["--each", "--background", "1", "1", "1"])
    assert [os.path.dirname(p) for p, _ in written] == [os.path.join(out_dir, "box_0"), os.path.join(out_dir, "box_1")]
    assert sorted(os.listdir(out_dir)) == ["0.npz", "0_rgb.png", "box_0", "box_1"]
    for k, (png, npz) in enumerate(written):
        op = {key: v.cpu().numpy() for key, v in ops.nerf_render_boxes(c.state, c.cfg, kept[k:k + 1], "keep", **kw).items()}
        img = np.asarray(Image.open(png))
        assert np.array_equal(img, V.to8b(op["rgb_map"] + (np.float32(1.0) - op["acc_map"])[..., None] * np.ones(3, np.float32)))
        empty = op["acc_map"] == 0
        assert empty.any() and (img[empty] == 255).all()
        with np.load(npz) as f:
            assert np.array_equal(f["acc"], op["acc_map"])


def test_recorded_bounds_name_every_case():
    """tests/golden/nerf_boxes_bounds.json only records what was seen; it must cover the cases of this file."""
    rec = B.recorded_bounds()["cases"]
    assert sorted(rec) == sorted(IDS)
