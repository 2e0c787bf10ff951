"""NeRF render kernels (csrc/nerfrender.hip, the shared trunk of csrc/nerf_mlp.cuh) on the MI355X, through ops.nerf_render,
ops.nerf_render_samples and the nerf_render command line.

The reference is tests/nerf_render_ref.py in float64 (render / render_rays of the reference in its order, on the float32 intrinsics,
pose, samples and weights).  Every element of every output of every case must lie within the case's bound of it: 8 x the largest
|float32 checker - float64 checker| of that case and output (tests/golden/nerf_render_bounds.json, written by
make_nerf_render_golden.py, never typed in).  The tests are staged so that a failure points at one kernel: the first MLP pass, the
depth-guided sampling fed the float32 checker's raw, the second pass and compositing fed the float32 checker's samples, then the
whole.  The float64 and float32 checker results are computed once per case and shared."""
import os

import numpy as np
import pytest
import torch

import nerf_render_ref as V
from nerf_rpn_amd import ops
from nerf_rpn_amd.scripts import nerf_render as X
from nerf_render_ref import bounds, refs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TWO_PASS = [c["name"] for c in V.CASES if not c.get("plain")]
MAPS = ("rgb_map", "depth_map", "acc_map", "disp_map", "depth_std")


def render(c, **kw):
    args = dict(H=c.H, W=c.W, intrinsic=c.intrinsic, c2w=c.c2w, near=c.near, far=c.far, bb_center=c.bb_center, bb_scale=c.bb_scale,
                z_samples=c.z_samples, n_samples=c.n_samples, lindisp=c.lindisp, embedded_cam=c.embedded_cam, return_samples=True)
    args.update(kw)
    if args.get("rays") is not None:
        for k in ("H", "W", "intrinsic", "c2w"):
            args.pop(k)
    out = ops.nerf_render(c.state, c.cfg, **args)
    n, frame = c.H * c.W, "H" in args
    # one row per ray: the maps of a frame call come as (H, W, ...), the stages always as (R, ...)
    return {k: (v.reshape(n, *v.shape[2:]) if frame and k not in ("raw1", "z2") else v).cpu().numpy() for k, v in out.items()}


def check(name, got, ref, b, keys):
    """Print every figure, then assert every one."""
    bad = []
    for k in keys:
        assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        err = np.abs(got[k].astype(np.float64) - ref[k]).max()
        print(f"{name}: {k} error {err:.3g} (bound {b[k]['bound']:.3g}, float32 checker {b[k]['fp32_error']:.3g})")
        if not (np.isfinite(got[k]).all() and err <= b[k]["bound"]):
            bad.append((k, err, b[k]["bound"]))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", V.NAMES)
def test_stage1_first_pass_raw(dev, refs, bounds, name):
    c, _, f64 = refs(name)
    got = render(c, return_stages=True)
    raw = got["raw1"]
    assert raw.shape == f64["raw1"].shape
    check(name, {"raw1_rgb": raw[..., :3], "raw1_sigma": raw[..., 3]}, {"raw1_rgb": f64["raw1"][..., :3], "raw1_sigma": f64["raw1"][..., 3]},
          bounds[name], ("raw1_rgb", "raw1_sigma"))


@pytest.mark.parametrize("name", TWO_PASS)
def test_stage2_samples_from_the_checkers_raw(dev, refs, bounds, name):
    c, f32, _ = refs(name)
    rays = np.concatenate([f32["rays_o"], f32["rays_d"]], 1)
    got = ops.nerf_render_samples(f32["raw1"], rays, c.z_samples, c.near, c.far).cpu().numpy()
    ref = V.render_case(c, torch.float64, raw1=f32["raw1"])["z2"].numpy()
    assert (np.diff(got, axis=1) >= 0).all() and got.min() >= np.float32(c.near) and got.max() <= np.float32(c.far)
    check(name, {"z2": got}, {"z2": ref}, bounds[name]["given_raw1"], ("z2",))


@pytest.mark.parametrize("name", TWO_PASS)
def test_stage3_composite_from_the_checkers_samples(dev, refs, bounds, name):
    c, f32, _ = refs(name)
    got = render(c, z2=f32["z2"])
    ref = {k: v.numpy() for k, v in V.render_case(c, torch.float64, z2=f32["z2"]).items()}
    assert np.array_equal(got["z_vals"], f32["z_vals"])          # the merge of float32 lists is exact
    check(name, got, ref, bounds[name]["given_z2"], V.OUTPUTS)


@pytest.mark.parametrize("name", V.NAMES)
def test_stage4_every_element_within_bound_of_fp64(dev, refs, bounds, name):
    c, _, f64 = refs(name)
    got = render(c, return_stages=True)
    if not c.plain:
        check(name, got, f64, bounds[name], ("z2",))
    check(name, got, f64, bounds[name], V.OUTPUTS)


def test_clamped_case_ties_on_the_device(dev, refs):
    c, _, _ = refs("clamped_4x4")
    got = render(c)
    tie = got["z_vals"][:, 1:] == got["z_vals"][:, :-1]
    assert tie.any() and (got["weights"][:, :-1][tie] == 0).all()
    assert (np.diff(got["z_vals"], axis=1) >= 0).all()


@pytest.mark.parametrize("name", ["odd_5x7", "full_3x3", "plain_4x6"])
def test_chunking_and_repeats_are_bit_equal(dev, refs, name):
    c, _, _ = refs(name)
    a = render(c, return_stages=True)
    for other in (render(c, return_stages=True, chunk=1), render(c, return_stages=True, chunk=3), render(c, return_stages=True)):
        for k in a:
            assert np.array_equal(a[k], other[k], equal_nan=True), k


@pytest.mark.parametrize("name", ["odd_5x7", "views_cam_3x5", "plain_lindisp_4x6"])
def test_rays_call_equals_frame_call(dev, refs, name):
    c, f32, _ = refs(name)
    a = render(c, return_stages=True)
    b = render(c, return_stages=True, rays=np.concatenate([f32["rays_o"], f32["rays_d"]], 1))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_shapes_packed_weights_and_errors(dev, refs):
    c, _, _ = refs("odd_5x7")
    w = ops.nerf_grid_pack(c.state, c.cfg)
    kw = dict(H=c.H, W=c.W, intrinsic=c.intrinsic, c2w=c.c2w, near=c.near, far=c.far, bb_center=c.bb_center, bb_scale=c.bb_scale,
              z_samples=c.z_samples)
    out = ops.nerf_render(w, c.cfg, **kw)
    assert sorted(out) == sorted(MAPS) and out["rgb_map"].shape == (5, 7, 3) and out["depth_std"].shape == (5, 7)
    ref = render(c)
    assert np.array_equal(out["rgb_map"].reshape(-1, 3).cpu().numpy(), ref["rgb_map"])
    with pytest.raises(NotImplementedError, match="N_importance"):
        ops.nerf_render(c.state, dict(c.cfg, N_importance=64), **kw)
    with pytest.raises(ops.lib.NrpnError, match="embedded_cam"):
        ops.nerf_render(w, c.cfg, embedded_cam=[1.0], **kw)
    with pytest.raises(ops.lib.NrpnError, match="n_samples"):
        ops.nerf_render(w, c.cfg, **dict(kw, z_samples=None))
    with pytest.raises(ops.lib.NrpnError, match="not both"):
        ops.nerf_render(w, c.cfg, rays=np.zeros((2, 6), np.float32), **kw)
    with pytest.raises(ops.lib.NrpnError, match="or rays"):
        ops.nerf_render(w, c.cfg, **{k: v for k, v in kw.items() if k != "c2w"})
    with pytest.raises(ops.lib.NrpnError, match="near and far"):
        ops.nerf_render(w, c.cfg, **{k: v for k, v in kw.items() if k != "near"})


def test_cli_end_to_end(dev, refs, bounds, tmp_path):
    from PIL import Image
    c, _, f64 = refs("odd_5x7")
    argv = V.write_run(tmp_path, c, frames=2)
    written = X.main(argv + ["--frames", "1"])
    out_dir = str(tmp_path / "out")
    assert written == [(os.path.join(out_dir, "1_rgb.png"), os.path.join(out_dir, "1.npz"))]
    assert sorted(os.listdir(out_dir)) == ["1.npz", "1_rgb.png"]
    op = render(c)
    img = np.asarray(Image.open(written[0][0]))
    assert img.dtype == np.uint8 and np.array_equal(img, V.to8b(op["rgb_map"].reshape(c.H, c.W, 3)))
    with np.load(written[0][1]) as f:
        got = {"depth_map": f["depth"], "depth_std": f["depth_std"], "acc_map": f["acc"]}
    for k, v in got.items():
        assert v.dtype == np.float32 and v.shape == (c.H, c.W) and np.array_equal(v.reshape(-1), op[k]), k
    check("cli", {k: v.reshape(-1) for k, v in got.items()}, f64, bounds["odd_5x7"], tuple(got))
