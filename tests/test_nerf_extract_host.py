"""Host tests of the NeRF grid extraction: the checker (tests/nerf_extract_ref.py) against the reference's recorded results
(tests/golden/nerf_extract.npz, from the reference's own extract_nerf), the bounds the GPU tests use, and everything of
scripts/nerf_extract.py that does not need the device (grid, bounds, checkpoint loading, flags, the file it writes -- with the
checker's float32 hoisted formulation standing in for the op)."""
import json
import os

import numpy as np
import pytest
import torch

import nerf_extract_ref as R
from nerf_extract_ref import GOLDEN, bounds, golden_npz, write_run  # noqa: F401  (fixtures)
from nerf_rpn_amd import datasets, ops
from nerf_rpn_amd.scripts import nerf_extract as X
from nerf_rpn_amd.scripts import scannet_filter_bbox as F

NAMES = [c["name"] for c in R.CASES]
SHARP = 100.0          # a mutation must exceed its bound by this factor


@pytest.fixture(scope="module")
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)         # the golden file was recorded with one thread
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def cases(one_thread):
    """name -> (inputs, float32 checker in reference order, float64 checker); computed once."""
    out = {}
    for i, case in enumerate(R.CASES):
        c = R.case_inputs(case, i)
        args = (c.state, c.cfg, c.xs, c.ys, c.zs, c.bb_center, c.bb_scale, c.poses)
        out[c.name] = (c, R.extract(*args, dtype=torch.float32).numpy(), R.extract(*args, dtype=torch.float64).numpy())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# checker, golden, bounds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fp32_checker_equals_the_reference_bit_for_bit(cases, golden_npz, name):
    c, f32, _ = cases[name]
    assert f32.dtype == np.float32
    assert np.array_equal(f32, golden_npz[f"{name}/rgbsigma"])
    assert list(golden_npz[f"{name}/resolution"]) == c.res == R.CASES[NAMES.index(name)]["res"]
    assert np.array_equal(golden_npz[f"{name}/bbox_min"], c.min_xyz.numpy()) and np.array_equal(golden_npz[f"{name}/bbox_max"], c.max_xyz.numpy())


@pytest.mark.parametrize("name", NAMES)
def test_bounds_are_the_measured_fp32_error(cases, bounds, name):
    _, f32, f64 = cases[name]
    err = np.abs(f32.astype(np.float64) - f64)
    b = bounds[name]
    assert b["rgb"] == 8.0 * err[:, :3].max() and b["sigma"] == 8.0 * err[:, 3].max()
    assert 0 < b["rgb"] < 1e-5


def test_family_b_sigma_takes_both_signs(cases):
    _, _, f64 = cases["tiles_9x8x8"]
    assert f64[:, 3].min() < -5 and f64[:, 3].max() > 50


@pytest.mark.parametrize("name", NAMES)
def test_hoisted_formulation_is_within_the_bounds(cases, bounds, name):
    c, _, f64 = cases[name]
    got = R.extract_hoisted(c.state, c.cfg, c.xs, c.ys, c.zs, c.bb_center, c.bb_scale, c.poses).numpy()
    err = np.abs(got.astype(np.float64) - f64)
    assert err[:, :3].max() <= bounds[name]["rgb"] and err[:, 3].max() <= bounds[name]["sigma"]


@pytest.mark.parametrize("name", ["odd_7x6x5", "views_5x4x3", "half_4x2x2"])
def test_the_kernels_order_of_operations_is_within_the_bounds(cases, bounds, name):
    """The HIP kernels' float32 arithmetic in their own order (k-permuted fmaf chains of the MFMA, padded encoding), emulated in numpy."""
    c, _, f64 = cases[name]
    got = R.extract_kernel_order(c.state, c.cfg, c.xs, c.ys, c.zs, c.bb_center, c.bb_scale, c.poses)
    assert got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - f64)
    assert err[:, :3].max() <= bounds[name]["rgb"] and err[:, 3].max() <= bounds[name]["sigma"]


# which channel group a mutation must break, and the case that shows it (last_pose needs several poses, swap_xz res_x != res_z)
@pytest.mark.parametrize("mutation, group, name", [("no_skip", "both", "odd_7x6x5"), ("swap_sincos", "both", "odd_7x6x5"),
                                                   ("plus_z", "rgb", "odd_7x6x5"), ("last_pose", "rgb", "odd_7x6x5"),
                                                   ("swap_xz", "both", "odd_7x6x5"), ("plus_z", "rgb", "views_5x4x3"),
                                                   ("no_skip", "both", "tiles_9x8x8")])
def test_mutations_exceed_the_bounds(cases, bounds, mutation, group, name):
    c, _, f64 = cases[name]
    bad = R.extract(c.state, c.cfg, c.xs, c.ys, c.zs, c.bb_center, c.bb_scale, c.poses, dtype=torch.float64, mutation=mutation).numpy()
    err = np.abs(bad - f64)
    assert err[:, :3].max() >= SHARP * bounds[name]["rgb"], (mutation, err[:, :3].max())
    if group == "both":
        assert err[:, 3].max() >= SHARP * bounds[name]["sigma"], (mutation, err[:, 3].max())
    else:
        assert err[:, 3].max() == 0            # sigma does not see the view


# ----------------------------------------------------------------------------------------------------------------------
# grid
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_resolution_linspace_and_row_order(cases, golden_npz, tmp_path, name):
    c, _, _ = cases[name]
    path = str(tmp_path / "bbox.json")
    R.write_bbox_json(path, c.bbox)
    lo, hi = X.scene_bounding_box(path)
    assert lo.dtype == torch.float32 and np.array_equal(lo.numpy(), golden_npz[f"{name}/bbox_min"]) and np.array_equal(hi.numpy(), golden_npz[f"{name}/bbox_max"])
    res, xs, ys, zs = X.grid_axes(lo, hi, c.max_res)
    assert res == list(golden_npz[f"{name}/resolution"])
    for a, b in zip((xs, ys, zs), (c.xs, c.ys, c.zs)):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    pts = R.grid_points(xs, ys, zs)
    rx, ry, rz = res
    r = np.arange(rx * ry * rz)
    want = np.stack([xs.numpy()[r % rx], ys.numpy()[(r // rx) % ry], zs.numpy()[r // (rx * ry)]], axis=1)
    assert np.array_equal(pts.numpy(), want)


def test_half_rounds_to_even():
    case = R.CASES[NAMES.index("half_4x2x2")]
    c = R.case_inputs(case)
    ratio = (c.max_xyz - c.min_xyz) / (c.max_xyz - c.min_xyz).max() * c.max_res
    assert ratio.tolist() == [4.0, 2.5, 1.5] and c.res == [4, 2, 2]


def test_wlh_is_the_readme_transform_of_flat(cases):
    c, f32, _ = cases["odd_7x6x5"]
    wlh = R.flat_to_wlh(f32, c.res)
    assert wlh.shape == (7, 6, 5, 4)
    rx, ry, rz = c.res
    for ix, iy, iz in ((0, 0, 0), (6, 5, 4), (3, 1, 2), (1, 4, 0)):
        assert np.array_equal(wlh[ix, iy, iz], f32[(iz * ry + iy) * rx + ix])


# ----------------------------------------------------------------------------------------------------------------------
# the command line
# ----------------------------------------------------------------------------------------------------------------------
def test_cli_flags_match_the_reference():
    with open(os.path.join(GOLDEN, "nerf_extract_cli.json")) as f:
        ref = json.load(f)
    ours = {a.dest: a for a in X.build_parser()._actions}
    for dest, spec in ref.items():
        assert f"--{dest}" in ours[dest].option_strings
        assert ours[dest].default == spec["default"] and ours[dest].type.__name__ == spec["type"]
    assert ours["layout"].default == "flat" and tuple(ours["layout"].choices) == ("flat", "wlh")


def test_unsupported_options_raise():
    assert ops.nerf_grid_config(R.DEFAULT_CFG) == dict(multires=9, multires_views=0, input_ch_cam=4)
    assert ops.nerf_grid_config(dict(R.DEFAULT_CFG, multires_views=4, input_ch_cam=0))["multires_views"] == 4
    for key, value in (("netdepth", 6), ("netwidth", 128), ("multires", 10), ("use_viewdirs", False), ("N_importance", 64), ("i_embed", -1),
                       ("multires_views", -1), ("input_ch_cam", -2), ("multires_views", True)):
        with pytest.raises(NotImplementedError, match=key):
            ops.nerf_grid_config(dict(R.DEFAULT_CFG, **{key: value}))


@pytest.mark.parametrize("prefix", ["module.", ""])
def test_checkpoint_loading(cases, tmp_path, prefix):
    c, _, _ = cases["half_4x2x2"]
    _, paths = write_run(tmp_path, c, prefix=prefix)
    cfg, sd, path = X.load_checkpoint(os.path.dirname(paths["exp"]), "run1")
    assert os.path.basename(path) == "200000.tar" and cfg["multires"] == 9
    assert sorted(sd) == sorted(prefix + k for k in c.state)
    m = R.build_model(sd, cfg)                       # both spellings load into the model
    assert torch.equal(m.alpha_linear.weight, c.state["alpha_linear.weight"])


def test_corner_bounds_equal_the_full_image(cases):
    c, _, _ = cases["odd_7x6x5"]
    H, W = 48, 64
    intr = torch.tensor([[58.0 + k, 58.5, 31.5, 23.5] for k in range(len(c.poses))])
    for far in (4.5, 0.75):
        full = R.scene_bounds(H, W, intr, c.poses, far)
        corner = X.corner_bounds(H, W, intr, c.poses, far)
        for a, b in zip(full, corner):
            assert torch.equal(a, b)


@pytest.fixture()
def host_op(monkeypatch):
    """The checker's float32 hoisted formulation in place of the device op: what the command line does around it is host code."""
    def fake(state_dict, cfg, xs, ys, zs, bb_center, bb_scale, poses, layout="flat", chunk=None):
        ops.nerf_grid_config(cfg)
        flat = R.extract_hoisted(state_dict, cfg, xs, ys, zs, bb_center, bb_scale, poses)
        return flat if layout == "flat" else torch.from_numpy(R.flat_to_wlh(flat.numpy(), [len(xs), len(ys), len(zs)]))
    monkeypatch.setattr(ops, "nerf_grid_query", fake)


def test_npz_keys_and_dtypes(cases, bounds, golden_npz, tmp_path, host_op):
    c, _, _ = cases["odd_7x6x5"]
    argv, _ = write_run(tmp_path, c)
    with np.load(X.main(argv)) as f:
        got = {k: f[k] for k in f.files}
    want = dict(rgbsigma=np.float32, resolution=np.int64, bbox_min=np.float32, bbox_max=np.float32, scale=np.float64, offset=np.float64,
                from_mitsuba=np.bool_, from_ddp_nerf=np.bool_)
    assert {k: v.dtype for k, v in got.items()} == {k: np.dtype(v) for k, v in want.items()}
    assert got["scale"] == 1.0 and got["offset"] == 0.0 and not got["from_mitsuba"] and got["from_ddp_nerf"]
    assert np.array_equal(got["resolution"], golden_npz["odd_7x6x5/resolution"])
    assert np.array_equal(got["bbox_min"], golden_npz["odd_7x6x5/bbox_min"]) and np.array_equal(got["bbox_max"], golden_npz["odd_7x6x5/bbox_max"])
    err = np.abs(got["rgbsigma"].astype(np.float64) - golden_npz["odd_7x6x5/rgbsigma"])
    assert err[:, :3].max() <= bounds["odd_7x6x5"]["rgb"] and err[:, 3].max() <= bounds["odd_7x6x5"]["sigma"]


def test_bounds_from_rays_reach_the_op(cases, tmp_path, monkeypatch):
    c, _, _ = cases["half_4x2x2"]
    argv, paths = write_run(tmp_path, c, bounds_from_rays=(480, 640))
    seen = {}

    def fake(state_dict, cfg, xs, ys, zs, bb_center, bb_scale, poses, layout="flat", chunk=None):
        seen.update(center=bb_center, scale=bb_scale, poses=poses)
        return torch.zeros(len(xs) * len(ys) * len(zs), 4)
    monkeypatch.setattr(ops, "nerf_grid_query", fake)
    X.main(argv)
    poses, intr, far = X.load_transforms(os.path.join(paths["scene"], "transforms_train.json"))
    assert far == 4.5 and torch.equal(poses, c.poses) and intr[1].tolist() == [581.0, 585.0, 319.5, 239.5]
    center, scale, _, _ = R.scene_bounds(480, 640, intr, poses, 4.5)
    assert torch.equal(seen["center"], center) and torch.equal(seen["scale"], scale) and torch.equal(seen["poses"], c.poses)


def test_wlh_file_feeds_the_dataset_and_filter_bbox(cases, tmp_path, host_op):
    c, f32, _ = cases["odd_7x6x5"]
    argv, paths = write_run(tmp_path, c, layout="wlh")
    path = X.main(argv)
    grid = datasets._grid_from_npz(path, normalize_density=False)
    assert tuple(grid.shape) == (4, 7, 6, 5)
    with np.load(path) as f:
        assert np.array_equal(grid.numpy(), np.transpose(f["rgbsigma"], (3, 0, 1, 2)))
    # filter_bbox reads the file's resolution
    inst = [dict(label="chair", obb=[0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0], **b) for b in c.bbox["instances"]]
    obj = str(tmp_path / "obj.json")
    with open(obj, "w") as f:
        json.dump({"instances": inst}, f)
    keep = F.filter_scene(path, obj, str(tmp_path / "boxes.npy"), str(tmp_path / "kept.json"), 1)
    boxes = np.load(str(tmp_path / "boxes.npy"))
    ext = np.array(c.bbox["instances"][1]["max_pt"]) - np.array(c.bbox["instances"][0]["min_pt"])
    assert keep.all() and np.allclose(boxes[0, 3:6], 1.0 / ext * np.array(c.res))
