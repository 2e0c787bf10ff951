"""Host tests of the render restricted to 3D boxes: the checker tests/nerf_boxes_ref.py against the render checker
it restates, the cases it hands the GPU tests, the mutations their bounds must reject, ops.nerf_boxes_to_world against
proposals2ngp, and the argument checks of the op and the command line that need no device."""
import numpy as np
import pytest
import torch

import nerf_boxes_ref as B
import nerf_render_ref as V
from nerf_rpn_amd import ops
from nerf_rpn_amd.scripts import nerf_render as NR
from nerf_rpn_amd.scripts import nerf_render_boxes as X
from nerf_rpn_amd.scripts import proposals2ngp as P2N
from nerf_boxes_ref import box_refs  # noqa: F401  (fixture)

SAME_AS_PLAIN = (("all", "keep"), ("none", "remove"), ("k0", "remove"))


def plain_render(c, dtype):
    """tests/nerf_render_ref.py's render of the case, without boxes."""
    frame = dict(H=c.H, W=c.W, intrinsic=c.intrinsic, c2w=c.c2w) if c.rays is None else dict(rays=c.rays)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)             # as nerf_boxes_ref.refs_of: the float32 sums depend on it
    out = V.render(c.state, c.cfg, c.near, c.far, c.bb_center, c.bb_scale, z_samples=c.z_samples, n_samples=c.n_samples, dtype=dtype,
                   **frame)
    torch.set_num_threads(threads)
    return {k: v.numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", B.NAMES)
def test_checker_without_an_effective_mask_is_the_render_checker_bit_for_bit(box_refs, name):
    c = box_refs(name, "all", "keep")[0]
    plain = {torch.float32: plain_render(c, torch.float32), torch.float64: plain_render(c, torch.float64)}
    for which, mode in SAME_AS_PLAIN:
        _, _, _, f32, f64, out = box_refs(name, which, mode)
        assert not out.any() and f32["counted1"].all() and f64["counted1"].all()
        for dt, got in ((torch.float32, f32), (torch.float64, f64)):
            for k, ref in plain[dt].items():
                assert got[k].dtype == ref.dtype and np.array_equal(got[k], ref, equal_nan=True), (which, mode, dt, k)


@pytest.mark.parametrize("name", B.NAMES)
def test_keep_without_boxes_gives_empty_rays_with_the_references_nan_pattern(box_refs, name):
    for dt_index in (3, 4):
        o = box_refs(name, "k0", "keep")[dt_index]
        n, s = o["z_vals"].shape
        zero_raw = torch.zeros(n, s, 4, dtype=torch.float32 if dt_index == 3 else torch.float64)
        rgb, disp, acc, weights, depth = V.raw2outputs(zero_raw, torch.from_numpy(o["z_vals"].copy()), torch.from_numpy(o["rays_d"].copy()))
        assert disp.isnan().all() and not acc.any() and not rgb.any() and not depth.any()
        assert np.isnan(o["disp_map"]).all() and np.array_equal(np.isnan(o["disp_map"]), disp.isnan().numpy())
        for k in ("acc_map", "rgb_map", "depth_map", "depth_std", "weights", "raw1"):
            assert not o[k].any(), k
        assert not o["counted1"].any() and B.tiles_counted(o["counted1"]) == 0


def _enters_and_leaves(mask):
    """bool [R, S] -> the rays with an uncounted sample, then counted ones, then an uncounted one again."""
    first, last = mask.argmax(1), mask.shape[1] - 1 - mask[:, ::-1].argmax(1)
    return mask.any(1) & (first > 0) & (last < mask.shape[1] - 1)


def test_the_cases_hold_what_they_are_for(box_refs):
    """Conditions on the cases, on the host, before a device is touched."""
    for name in B.NAMES:
        for which in B.BOXES:
            for mode in B.MODES:
                c, boxes, table, f32, f64, out = box_refs(name, which, mode)
                assert out.mean() <= B.MAX_LEFT_OUT, (name, which, mode, out.mean())
                keep = ~out
                for k in ("counted1", "counted2"):       # where nothing is undecided the two checkers count the same samples
                    if k in f64:
                        assert np.array_equal(f32[k][keep], f64[k][keep]), (name, which, mode, k)
                for k in B.TENSORS:
                    if k in f64:
                        assert np.array_equal(np.isnan(f32[k][keep]), np.isnan(f64[k][keep])), (name, which, mode, k)
                print(f"{name} {which} {mode}: {len(table)} boxes, {out.sum()} rays left out, pass 1 counts {f64['counted1'].mean():.2f} "
                      f"of the samples in {B.tiles_counted(f64['counted1'])} of {B.tiles_total(*f64['counted1'].shape)} tiles, nearest "
                      f"sample to a face at {min(B.face_margin(f64[k], table) for k in ('pts1', 'pts2') if k in f64):.2g} of the extent")
    # the frames: an image row is one tile; the rays-only case: tiles straddle rays and the last one is partial
    for name in ("plain_6x8", "two_pass_6x8"):
        c = box_refs(name, "all", "keep")[0]
        assert c.W * c.s1 == B.TILE and c.rays is None
    c = box_refs("rays_130x13", "all", "keep")[0]
    assert c.rays is not None and c.n_rays == 130 and c.s1 == 13 and B.TILE % c.s1 != 0 and (c.n_rays * c.s1) % B.TILE != 0
    for name in B.NAMES:
        c, boxes, table, _, f64, _ = box_refs(name, "rotated", "keep")
        theta = boxes[0, 6]
        assert boxes.shape == (1, 7) and min(abs(theta - k * np.pi / 2) for k in range(-4, 5)) > 0.2
        assert _enters_and_leaves(f64["counted1"]).any(), name
        # a whole tile outside (skippable in pass 1) and a tile partly inside
        c, boxes, table, _, f64, _ = box_refs(name, "rows", "keep")
        m = f64["counted1"]
        flat = np.concatenate([m.reshape(-1), np.zeros(-m.size % B.TILE, dtype=bool)]).reshape(-1, B.TILE)
        assert (~flat.any(1)).any() and (flat.any(1) & ~flat.all(1)).any(), name
        if name != "rays_130x13":
            assert (~m.reshape(c.H, -1).any(1)).any()            # a whole image row
        c, boxes, table, _, f64, _ = box_refs(name, "overlap", "keep")
        both = B.inside(f64["pts1"], table[:1]) & B.inside(f64["pts1"], table[1:])
        only = B.inside(f64["pts1"], table[:1]) ^ B.inside(f64["pts1"], table[1:])
        assert len(table) == 2 and both.any() and only.any(), name
        c, boxes, table, _, f64, _ = box_refs(name, "origin", "keep")
        assert B.inside(c.rays32[:1, :3].numpy(), table).all() and f64["counted1"][:, 0].all() and not f64["counted1"][:, -1].any()
        assert box_refs(name, "all", "keep")[4]["counted1"].all() and not box_refs(name, "none", "keep")[4]["counted1"].any()
        assert box_refs(name, "k0", "keep")[1].shape == (0, 7)
        c, boxes, table, _, f64, _ = box_refs(name, "aabb6", "keep")
        assert boxes.shape == (2, 6) and (table[:, 6] == 1).all() and (table[:, 7] == 0).all() and f64["counted1"].any()
        assert np.allclose(table[:, :3] - table[:, 3:6], boxes[:, :3], rtol=0, atol=1e-15)


MUTATION_PROBES = [("two_pass_6x8", "rotated"), ("two_pass_6x8", "overlap"), ("rays_130x13", "rotated"), ("plain_6x8", "rotated")]


@pytest.mark.parametrize("mutation", B.MUTATIONS)
def test_the_bounds_reject_the_mutations(box_refs, mutation):
    """Each mutation of the float32 checker must exceed the GPU test's bound (8 x the float32 checker's deviation, floored at an ulp)
    of some tensor on some case; every figure is printed."""
    caught = []
    for name, which in MUTATION_PROBES:
        for mode in B.MODES:
            c, boxes, table, f32, f64, out = box_refs(name, which, mode)
            if c.plain and mutation in ("pass2_unmasked", "draw_unmasked"):
                continue
            bad = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in B.render(c, table, mode, torch.float32, mutation).items()}
            for k in B.TENSORS:
                if k not in f64:
                    continue
                bound, _ = B.bound_of(f32, f64, k, ~out)
                err, same = B.error_of(bad, f64, k, ~out)
                print(f"{mutation}: {name} {which} {mode} {k}: error {err:.3g}, bound {bound:.3g}, NaN positions equal: {same}")
                if err > bound or not same:
                    caught.append((name, which, mode, k))
    assert caught, f"{mutation} stays within the bounds on every probed case"


def test_boxes_to_world_against_proposals2ngp():
    rng = np.random.default_rng(5)
    feats = dict(resolution=np.array([160, 121, 97]), bbox_min=np.array([-2.3, -1.1, 0.2]), bbox_max=np.array([3.1, 2.7, 2.9]),
                 scale=1.0, offset=0.0, from_mitsuba=False, from_ddp_nerf=True)
    for_p2n = dict(feats, offset=np.zeros(3))
    obb = np.concatenate([rng.uniform(5, 90, (9, 3)), rng.uniform(3, 40, (9, 3)), rng.uniform(-3, 3, (9, 1))], 1)
    got = ops.nerf_boxes_to_world(obb, feats)
    assert got.dtype == np.float64 and got.shape == (9, 7) and np.array_equal(got[:, 6], obb[:, 6])
    for row, ref in zip(got, P2N.obb_to_ngp_boxes(obb, for_p2n)):
        # obb_to_ngp_boxes -> ngp_matrix_to_nerf at scale 1 / offset 0: the axis cycles cancel, the position is the world centre
        np.testing.assert_allclose(row[:3], ref["position"], rtol=1e-15, atol=1e-15)
        np.testing.assert_allclose(row[3:6], ref["extents"], rtol=1e-15, atol=1e-15)
        rot = np.array(ref["orientation"])
        np.testing.assert_allclose([np.cos(row[6]), np.sin(row[6])], rot[:2, 0], rtol=0, atol=1e-15)
    lo = rng.uniform(5, 60, (7, 3))
    aabb = np.concatenate([lo, lo + rng.uniform(3, 40, (7, 3))], 1)
    got = ops.nerf_boxes_to_world(aabb, feats)
    for row, ref in zip(got, P2N.proposals_to_ngp_boxes(aabb, for_p2n)):
        np.testing.assert_allclose((row[:3] + row[3:]) * 0.5, ref["position"], rtol=1e-15, atol=1e-15)
        np.testing.assert_allclose(row[3:] - row[:3], ref["extents"], rtol=1e-14, atol=1e-15)
    assert ops.nerf_boxes_to_world(np.zeros((0, 7)), feats).shape == (0, 7)
    with pytest.raises(ValueError, match="from_ddp_nerf"):
        ops.nerf_boxes_to_world(obb, dict(feats, from_ddp_nerf=False))
    with pytest.raises(ValueError, match="from_ddp_nerf"):
        ops.nerf_boxes_to_world(obb, {k: v for k, v in feats.items() if k != "from_ddp_nerf"})
    with pytest.raises(ValueError, match="scale 0.5"):
        ops.nerf_boxes_to_world(obb, dict(feats, scale=0.5))
    with pytest.raises(ValueError, match="offset"):
        ops.nerf_boxes_to_world(obb, dict(feats, offset=np.array([0.0, 0.5, 0.0])))
    with pytest.raises(ValueError, match=r"\(9, 5\)"):
        ops.nerf_boxes_to_world(obb[:, :5], feats)


def test_box_table_and_the_checks_that_need_no_device():
    t = ops.nerf_box_table([[1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.5]])
    assert t.dtype == np.float64 and t.shape == (1, 8)
    assert np.array_equal(t[0], np.array([1.0, 2.0, 3.0, 1.0, 2.0, 3.0, np.cos(0.5), np.sin(0.5)]))
    t = ops.nerf_box_table(torch.tensor([[0.0, 1.0, 2.0, 4.0, 2.0, 8.0]]))
    assert np.array_equal(t[0], np.array([2.0, 1.5, 5.0, 2.0, 0.5, 3.0, 1.0, 0.0]))
    assert ops.nerf_box_table([]).shape == (0, 8) and ops.nerf_box_table(np.zeros((0, 6))).shape == (0, 8)
    ok = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0]
    # every refusal comes before the weights are looked at: no device is needed
    for boxes, mode, match in (([ok[:5]], "keep", r"\(1, 5\)"), ([[ok]], "keep", r"\(1, 1, 7\)"),
                               ([ok[:6] + [float("nan")]], "keep", "nan"), ([ok[:3] + [float("inf")] + ok[4:]], "keep", "inf"),
                               ([ok[:4] + [0.0] + ok[5:]], "keep", "extent 0.0 on axis 1"), ([ok[:5] + [-2.0, 0.0]], "remove", "extent -2.0"),
                               ([[0.0, 0.0, 0.0, 1.0, 0.0, 1.0]], "keep", "extent 0.0 on axis 1"), ([ok], "crop", "'crop'"),
                               ([ok] * 1025, "keep", "1025 boxes")):
        with pytest.raises(ValueError, match=match):
            ops.nerf_render_boxes(None, {}, boxes, mode)
    assert ops.nerf_box_table([ok] * 1024).shape == (1024, 8)


def test_the_script_parser():
    p = X.build_parser()
    a = p.parse_args(["--proposals", "p.npz", "--features", "f.npz"])
    assert (a.threshold, a.top_k, a.mode, a.each, a.background, a.boxes_json, a.dtype) == (0.5, 30, "keep", False, [0.0, 0.0, 0.0], None, "fp32")
    a = p.parse_args(["--boxes_json", "b.json", "--mode", "remove", "--each", "--background", "1", "1", "1", "--dtype", "bf16x3"])
    assert (a.mode, a.each, a.background, a.proposals, a.dtype) == ("remove", True, [1.0, 1.0, 1.0], None, "bf16x3")
    for argv in (["--proposals", "p.npz", "--boxes_json", "b.json"], [], ["--boxes_json", "b.json", "--mode", "crop"],
                 ["--boxes_json", "b.json", "--dtype", "bf16"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    # nerf_render's own flags, with its defaults and choices
    plain = {x.dest: x for x in NR.build_parser()._actions}
    boxed = {x.dest: x for x in p._actions}
    for dest, action in plain.items():
        assert boxed[dest].default == action.default and boxed[dest].choices == action.choices, dest
    assert tuple(boxed["dtype"].choices) == ops.NERF_DTYPES
    with pytest.raises(SystemExit, match="--features"):
        X.load_boxes(p.parse_args(["--proposals", "p.npz"]))


def test_the_script_reads_boxes_as_proposals2ngp_does(tmp_path):
    rng = np.random.default_rng(2)
    prop = np.concatenate([rng.uniform(5, 30, (6, 3)), rng.uniform(3, 10, (6, 3)), rng.uniform(-1, 1, (6, 1))], 1)
    score = np.array([0.9, 0.2, 0.7, 0.95, 0.5, 0.6])
    np.savez(tmp_path / "p.npz", proposal=prop, score=score)
    feats = dict(resolution=np.array([40, 40, 30]), bbox_min=np.array([-1.0, -1.0, 0.0]), bbox_max=np.array([1.0, 1.5, 1.2]), scale=1.0,
                 offset=0.0, from_mitsuba=False, from_ddp_nerf=True)
    np.savez(tmp_path / "f.npz", **feats)
    a = X.build_parser().parse_args(["--proposals", str(tmp_path / "p.npz"), "--features", str(tmp_path / "f.npz"), "--top_k", "3"])
    got = X.load_boxes(a)
    assert np.array_equal(got, ops.nerf_boxes_to_world(prop[[3, 0, 2]], feats))          # score > 0.5, best first, top 3
    import json
    with open(tmp_path / "b.json", "w") as f:
        json.dump({"scene_name": "s", "instances": [{"obj_id": 1, "label": "x", "obb": prop[0].tolist()}, {"obj_id": 2, "label": "y", "obb": prop[1].tolist()}]}, f)
    got = X.load_boxes(X.build_parser().parse_args(["--boxes_json", str(tmp_path / "b.json")]))
    assert np.array_equal(got, prop[:2])
    res = {"rgb_map": np.full((2, 2, 3), 0.25, np.float32), "acc_map": np.array([[0.0, 1.0], [0.5, 0.25]], np.float32)}
    out = X.over_background(res, [1.0, 0.5, 0.0])["rgb_map"]
    assert out.dtype == np.float32 and np.array_equal(out[0, 0], np.float32([1.25, 0.75, 0.25])) and np.array_equal(out[0, 1], np.float32([0.25] * 3))
