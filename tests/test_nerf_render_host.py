"""Host tests of the NeRF view rendering: the checker (tests/nerf_render_ref.py) against the reference's recorded results
(tests/golden/nerf_render.npz, from the reference's own render), the bounds the GPU tests use and their sharpness, the merge that
replaces the reference's sort, and everything of scripts/nerf_render.py that does not need the device (flags, to8b, the files)."""
import json
import os

import numpy as np
import pytest
import torch

import nerf_render_ref as V
from nerf_render_ref import bounds, golden_npz, refs  # noqa: F401  (fixtures)
from nerf_rpn_amd.scripts import nerf_render as X

STORED = ("rgb_map", "depth_map", "acc_map", "disp_map", "z_vals", "weights")
TWO_PASS = [c["name"] for c in V.CASES if not c.get("plain")]
SHARP = 10.0          # a mutation must exceed some bound by this factor


def with_raw(o):
    return dict(o, raw1_rgb=o["raw1"][..., :3], raw1_sigma=o["raw1"][..., 3])


@pytest.mark.parametrize("name", V.NAMES)
def test_fp32_checker_equals_the_reference_bit_for_bit(refs, golden_npz, name):
    _, f32, _ = refs(name)
    for k in STORED:
        assert f32[k].dtype == np.float32 and np.array_equal(f32[k], golden_npz[f"{name}/{k}"]), k
    assert list(golden_npz["cases"]) == V.NAMES


@pytest.mark.parametrize("name", V.NAMES)
def test_bounds_are_the_measured_fp32_error(refs, bounds, name):
    c, f32, f64 = refs(name)
    a, b = with_raw(f32), with_raw(f64)
    keys = list(V.OUTPUTS) + ["raw1_rgb", "raw1_sigma"] + ([] if c.plain else ["z2"])
    for k in keys:
        err = np.abs(a[k].astype(np.float64) - b[k]).max()
        rec = bounds[name][k]
        # the recorded error is this one up to what another torch build's float32 summation order may move it by
        assert rec["fp32_error"] == pytest.approx(err, rel=0.25) and rec["bound"] == 8.0 * rec["fp32_error"], (k, err, rec)
        assert err <= rec["bound"] and 0 < rec["bound"] < 1e-3, k          # satisfiable: the float32 checker lies within it
    # compositing is neither empty nor saturated at the first sample
    acc = f64["acc_map"]
    assert (acc.min() < 0.5 and acc.max() > 0.9) if len(acc) > 1 else 0.1 < acc[0] < 0.9
    assert f64["weights"][:, 0].max() < 0.5


def test_the_clamped_case_has_ties_and_clamped_bins(refs):
    c, f32, _ = refs("clamped_4x4")
    z = f32["z_vals"]
    assert (z[:, 1:] == z[:, :-1]).any()
    assert (f32["z2"][:, 0] == np.float32(c.near)).any() and (f32["z2"][:, -1] == np.float32(c.far)).any()


# the outputs a mutation must break and a case that shows it
@pytest.mark.parametrize("mutation, name, keys", [
    ("no_last_dist", "odd_5x7", ("acc_map", "rgb_map")), ("no_last_dist", "plain_4x6", ("acc_map", "weights")),
    ("no_ray_norm", "odd_5x7", ("acc_map", "depth_map")), ("no_ray_norm", "plain_lindisp_4x6", ("weights",)),
    ("no_std_clamp", "odd_5x7", ("z2", "z_vals")), ("no_std_clamp", "clamped_4x4", ("z2",)),
    ("pdf_left_nofloor", "clamped_4x4", ("z2",)), ("raw_viewdir", "views_3x5", ("rgb_map", "raw1_rgb")),
    ("raw_viewdir", "odd_5x7", ("rgb_map",)), ("plus_z", "odd_5x7", ("rgb_map", "depth_map", "raw1_sigma")),
    ("plus_z", "plain_4x6", ("rgb_map", "acc_map")), ("reverse_merge", "odd_5x7", ("z_vals", "weights", "rgb_map")),
    ("reverse_merge", "full_3x3", ("depth_map",))])
def test_mutations_exceed_the_bounds(refs, bounds, mutation, name, keys):
    c, _, f64 = refs(name)
    bad = with_raw({k: v.numpy() for k, v in V.render_case(c, torch.float64, mutation=mutation).items()})
    good = with_raw(f64)
    for k in keys:
        err = np.nanmax(np.abs(bad[k] - good[k]))
        assert not np.isfinite(bad[k]).all() or err >= SHARP * bounds[name][k]["bound"], (mutation, k, err, bounds[name][k]["bound"])


@pytest.mark.parametrize("name", TWO_PASS)
def test_merge_equals_sort(refs, name):
    """Both sample lists are non-decreasing, so the two-pointer merge gives the sorted values, and what it pairs with them differs
    from the reference's sort only inside runs of equal z."""
    c, f32, _ = refs(name)
    n = len(c.z_samples)
    for r in range(f32["z2"].shape[0]):
        assert (np.diff(f32["z2"][r]) >= 0).all() and (np.diff(c.z_samples.numpy()) > 0).all()
        z, src = V.merge_sorted(c.z_samples.numpy(), f32["z2"][r])
        assert np.array_equal(z, f32["z_vals"][r])
        both = np.concatenate([c.z_samples.numpy(), f32["z2"][r]])
        assert sorted(src) == list(range(2 * n)) and np.array_equal(both[src], z)


def test_a_tie_gets_zero_weight(refs):
    _, f32, f64 = refs("clamped_4x4")
    for o in (f32, f64):
        tie = o["z_vals"][:, 1:] == o["z_vals"][:, :-1]
        assert tie.any() and (o["weights"][:, :-1][tie] == 0).all()


def test_quadratic_samples_and_to8b_match_the_checker():
    for near, far, n in ((0.1, 4.0, 8), (1.0, 1.5, 8), (0.5, 6.0, 128)):
        z = X.precompute_quadratic_samples(near, far, n)
        assert z.dtype == torch.float32 and torch.equal(z, V.precompute_quadratic_samples(near, far, n))
        assert abs(float(z[0]) - near) < 1e-6 and abs(float(z[-1]) - far) < 1e-5 and (z[1:] > z[:-1]).all()
    x = np.array([-0.5, 0.0, 0.25, 0.999, 1.0, 7.0], dtype=np.float32)
    assert X.to8b(x).dtype == np.uint8 and X.to8b(x).tolist() == [0, 0, 63, 254, 255, 255]
    assert np.array_equal(X.to8b(x), V.to8b(x))


def test_cli_flags():
    p = X.build_parser()
    a = p.parse_args(["--expname", "e", "--ckpt_dir", "c", "--data_dir", "d", "--scene_id", "s", "--image_hw", "468", "624", "--frames",
                      "0", "7", "--near", "0.1", "--far", "5", "--output_dir", "o", "--bb_center", "1", "2", "3", "--bb_scale", "0.5"])
    assert (a.expname, a.ckpt_dir, a.data_dir, a.scene_id, a.image_hw, a.frames, a.output_dir) == ("e", "c", "d", "s", [468, 624], [0, 7], "o")
    assert (a.near, a.far, a.bb_center, a.bb_scale) == (0.1, 5.0, [1.0, 2.0, 3.0], 0.5)
    assert a.N_samples is None and a.depth_loss_weight is None and a.lindisp is None and a.transforms is None and a.chunk is None
    # the command line wins over args.json, args.json over the reference's defaults
    assert X.render_options(a, {}) == (256, True, False)
    assert X.render_options(a, {"N_samples": 64, "depth_loss_weight": 0.0, "lindisp": True}) == (64, False, True)
    b = p.parse_args(["--N_samples", "32", "--depth_loss_weight", "0.1", "--lindisp"])
    assert X.render_options(b, {"N_samples": 64, "depth_loss_weight": 0.0}) == (32, True, True)
    with pytest.raises(SystemExit):
        X.render_options(p.parse_args(["--N_samples", "4"]), {})
    with pytest.raises(SystemExit, match="expname"):
        X.main([])


def test_frame_files(tmp_path):
    from PIL import Image
    g = np.random.default_rng(0)
    res = {"rgb_map": g.uniform(-0.2, 1.2, (5, 7, 3)).astype(np.float32), "depth_map": g.uniform(0, 4, (5, 7)).astype(np.float32),
           "depth_std": g.uniform(0, 1, (5, 7)).astype(np.float32), "acc_map": g.uniform(0, 1, (5, 7)).astype(np.float32),
           "disp_map": np.ones((5, 7), np.float32)}
    png, npz = X.write_frame(str(tmp_path), 3, res)
    assert (os.path.basename(png), os.path.basename(npz)) == ("3_rgb.png", "3.npz")
    img = np.asarray(Image.open(png))
    assert img.dtype == np.uint8 and img.shape == (5, 7, 3) and np.array_equal(img, V.to8b(res["rgb_map"]))
    with np.load(npz) as f:
        assert sorted(f.files) == ["acc", "depth", "depth_std"]
        for k, src in (("depth", "depth_map"), ("depth_std", "depth_std"), ("acc", "acc_map")):
            assert f[k].dtype == np.float32 and np.array_equal(f[k], res[src])


def test_run_directory_helper(refs, tmp_path):
    c, _, _ = refs("plain_lindisp_4x6")
    argv = V.write_run(tmp_path, c)
    a = X.build_parser().parse_args(argv)
    cfg, state, path = X.load_checkpoint(a.ckpt_dir, a.expname)
    assert X.render_options(a, cfg) == (24, False, True) and path.endswith("200000.tar") and "module.rgb_linear.bias" in state
    poses, intr, far, meta = X.load_transforms(os.path.join(a.data_dir, a.scene_id, "transforms_test.json"), with_meta=True)
    assert torch.equal(poses[0], c.c2w) and torch.equal(intr[0], c.intrinsic) and (meta["near"], far) == (c.near, c.far)
    with open(os.path.join(a.ckpt_dir, a.expname, "args.json")) as f:
        assert json.load(f)["N_samples"] == 24
