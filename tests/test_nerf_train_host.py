"""The checker of the NeRF training front end (tests/nerf_train_ref.py) against the reference's recorded results, the bounds the GPU
tests use, and the host side of nerf_train: the learning-rate schedule, the command line's flags, the checkpoint layout and the data
rules.  No GPU."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import nerf_train_ref as T
from nerf_rpn_amd import nerf_train
from nerf_rpn_amd.scripts import nerf_train as X
from nerf_train_ref import bounds, golden_npz, refs  # noqa: F401  (fixtures)


@pytest.mark.parametrize("name", T.NAMES)
def test_fp32_checker_equals_the_reference_bit_for_bit(refs, golden_npz, name):
    _, f32, _ = refs(name)
    for k in T.STORED:
        got = f32[k].numpy()
        assert got.dtype == golden_npz[f"{name}/{k}"].dtype and np.array_equal(got, golden_npz[f"{name}/{k}"]), k
    assert list(golden_npz["cases"]) == T.NAMES


@pytest.mark.parametrize("name", T.NAMES)
def test_bounds_are_the_measured_fp32_error_and_the_rejected_share_is_capped(refs, bounds, name):
    c, f32, f64 = refs(name)
    bd = bounds["cases"][name]
    rejected = f64["rejected"].numpy()
    assert bd["rejected"] == [int(i) for i in np.nonzero(rejected)[0]] and bd["num_rays"] == c.R
    assert len(bd["rejected"]) <= bounds["reject_cap"] * c.R and bounds["reject_cap"] == T.REJECT_CAP == 0.10
    for k in T.STORED:
        if k == "target_vd":
            assert torch.equal(f32[k], f64[k])
            continue
        err = T.C.max_error(T.kept(f32, k, rejected), T.kept(f64, k, rejected))
        rec = bd[k]
        # the recorded error is this one up to what another torch build's float32 summation order may move it by
        assert rec["fp32_error"] == pytest.approx(err, rel=0.25, abs=1e-12), (k, err, rec)
        assert rec["bound"] == T.bound_of(rec["fp32_error"], T.kept(f64, k, rejected)) and err <= rec["bound"] < 1e-3, (k, err, rec)


def test_the_cases_hold_what_they_are_for(refs):
    seen = set()
    for name in T.NAMES:
        c, f32, f64 = refs(name)
        near, far = np.float32(c.near), np.float32(c.far)
        dr, z2, vd = f32["depth_range"].numpy(), f32["z2"].numpy(), f32["target_vd"].numpy()
        valid = dr[:, 0] >= near
        assert np.array_equal(valid, vd)                                # a pixel without a depth carries 0, below near
        norm = f64["rays"][:, 3:].norm(dim=-1)
        assert 0.5 < norm.min() and norm.max() < 2.0
        if (valid & (dr[:, 0] == near)).any():
            seen.add("depth equals near")
        if (valid & (dr[:, 1] < near) & (dr[:, 2] <= far)).any():
            seen.add("clamped at near")
        if (valid & (dr[:, 2] > far) & (dr[:, 1] >= near)).any():
            seen.add("clamped at far")
        if (valid & (dr[:, 1] < near) & (dr[:, 2] > far)).any():
            seen.add("clamped at both")
        if (valid & (dr[:, 1] > far)).any():
            assert (z2[valid & (dr[:, 1] > far)] == far).all()
            seen.add("every bin of zero width")
        depth, std = T.V.raw2depth(c.raw1.double(), f64["z1"], f64["rays"][:, 3:])
        lower_bound = float(c.z[-1] - c.z[-2])
        if ((~valid) & (std.numpy() < lower_bound)).any():
            seen.add("std below lower_bound")
        if ((~valid) & (depth.numpy() == 0)).any():
            seen.add("no density")
        opaque = (~valid) & (c.raw1[:, c.S // 2:, 3] == 1e4).all(-1).numpy()
        if opaque.any():
            # nothing behind the first opaque sample weighs in: the predicted depth lies at or before it
            assert (depth.numpy()[opaque] <= f64["z1"].numpy()[opaque, c.S // 2]).all() and (depth.numpy()[opaque] > 0).all()
            seen.add("opaque ray")
        if (c.u == 0).any() and (c.u == float(np.nextafter(np.float32(1), np.float32(0)))).any():
            seen.add("u at both ends")
        if len(set(c.pix.tolist())) < c.R and not (np.diff(c.pix.numpy()) >= 0).all():
            seen.add("pix repeated and out of order")
    assert seen == {"depth equals near", "clamped at near", "clamped at far", "clamped at both", "every bin of zero width",
                    "std below lower_bound", "no density", "opaque ray", "u at both ends", "pix repeated and out of order"}, seen


def mutation_factor(refs, bounds, mutation):
    """The largest error of the mutated float64 checker over every case's z1 and z2, in units of the tensor's bound."""
    worst = 0.0
    for name in T.NAMES:
        c, _, f64 = refs(name)
        bd = bounds["cases"][name]
        rejected = f64["rejected"].numpy()
        bad = T.run_case(c, torch.float64, mutation=mutation)
        for k in ("z1", "z2"):
            err = T.C.max_error(T.kept(bad, k, rejected), T.kept(f64, k, rejected))
            worst = max(worst, float("inf") if not np.isfinite(T.kept(bad, k, rejected)).all() else err / bd[k]["bound"])
    return worst


# The factors found (the largest error over the cases' z1 and z2 in units of its bound; inf: a result is not finite):
#   no_floor inf (16 on r3_s4_valid, where it stays finite), no_std_clamp inf, valid_swapped inf, range_cols_swapped 7.4e5,
#   perturb_swapped 1.7e6, shared_z1 2.6e4; searchsorted_left 0 (the test below).
@pytest.mark.parametrize("mutation", [m for m in T.MUTATIONS if m != "searchsorted_left"])
def test_mutations_exceed_the_bounds(refs, bounds, mutation):
    factor = mutation_factor(refs, bounds, mutation)
    print(f"{mutation}: {factor:.3g} x the bound")
    assert factor > 1.0, (mutation, factor)


def test_searching_from_the_left_moves_nothing_outside_the_rejected_rays(refs, bounds):
    """searchsorted from the left differs from the right only where u equals a cdf entry, and there it moves the sample from the top
    of one bin to the bottom of the next: the same point, unless one of the two bins takes sample_pdf's 1e-5 branch -- which is what
    the rejection rule leaves out.  Its factor is 0 on every case (u = 0 included: both searches give the first edge), so no bound can
    tell it from the reference; the mutation is kept in the table to show that."""
    assert mutation_factor(refs, bounds, "searchsorted_left") == 0.0


def test_loop_bounds(bounds):
    loop = bounds["loop"]
    assert len(loop["fp64"]) == len(loop["bound"]) == T.LOOP.steps and loop["fp64"][-1] < loop["fp64"][0]
    for v, e, b in zip(loop["fp64"], loop["fp32_error"], loop["bound"]):
        assert b == max(T.FACTOR * e, float(np.spacing(np.float32(abs(v))))) and b < 1e-3 * v


def test_learning_rate_schedule():
    lr = lambda i: nerf_train.learning_rate(i, 5e-4, 400000, 500000)       # noqa: E731
    assert lr(1) == lr(400000) == 5e-4
    assert lr(400001) == 5e-4 * (0.1 ** (1 / 100000))
    assert lr(450000) == 5e-4 * (0.1 ** 0.5)
    assert lr(500000) == 5e-4 * (0.1 ** 1.0) == lr(500001)
    assert lr(400000) > lr(400001) > lr(450000) > lr(500000)


def test_cli_flags_against_the_reference_defaults(bounds):
    p = X.build_parser()
    a = vars(p.parse_args([]))
    ref = bounds["cli_defaults"]
    assert sorted(ref) == sorted(T.CLI_FLAGS)
    for k, v in ref.items():
        assert a[k] == v and type(a[k]) is type(v), (k, a[k], v)
    assert a["N_iters"] == 500001 and a["depth_std"] is None and a["image_hw"] is None and a["near"] is None and a["far"] is None
    assert a["bb_center"] is None and a["bb_scale"] is None
    b = p.parse_args(["--image_hw", "6", "8", "--bb_center", "1", "2", "3", "--bb_scale", "0.5", "--no_reload", "--lindisp", "--N_iters", "9",
                      "--depth_std", "0.05", "--perturb", "0"])
    assert (b.image_hw, b.bb_center, b.bb_scale, b.no_reload, b.lindisp, b.N_iters, b.depth_std, b.perturb) == (
        [6, 8], [1., 2., 3.], 0.5, True, True, 9, 0.05, 0.)
    with pytest.raises(NotImplementedError, match="N_importance"):
        X.main(["--N_importance", "64"])
    with pytest.raises(NotImplementedError, match="netwidth"):
        X.main(["--netwidth", "128"])
    with pytest.raises(SystemExit, match="image_hw"):
        X.main(["--expname", "e"])


def test_base_samples():
    a = Namespace(depth_loss_weight=0.004, N_samples=26, lindisp=False)
    z, two = nerf_train.base_samples(a, 0.1, 4.0)
    assert two and z.shape == (12,) and torch.equal(z, T.V.precompute_quadratic_samples(0.1, 4.0, 13)[:-1])      # :1079-1080
    a = Namespace(depth_loss_weight=0., N_samples=8, lindisp=False)
    z, two = nerf_train.base_samples(a, 0.1, 4.0)
    t = torch.linspace(0., 1., steps=8)
    assert not two and torch.equal(z, (torch.full((1, 1), 0.1) * (1. - t) + torch.full((1, 1), 4.0) * t).reshape(-1))
    a.lindisp = True
    z, _ = nerf_train.base_samples(a, 0.1, 4.0)
    assert torch.equal(z, (1. / (1. / torch.full((1, 1), 0.1) * (1. - t) + 1. / torch.full((1, 1), 4.0) * t)).reshape(-1))


def test_checkpoint_layout_and_args_json(tmp_path):
    from nerf_rpn_amd import NeRF
    from nerf_rpn_amd.scripts.nerf_extract import load_checkpoint
    args = X.build_parser().parse_args(["--expname", "run1", "--ckpt_dir", str(tmp_path), "--multires_views", "2"])
    run_dir = nerf_train.write_args(args)
    model = NeRF(vars(args))
    opt = torch.optim.Adam(model.parameters(), lr=args.lrate, betas=(0.9, 0.999))
    cam = torch.nn.Embedding(3, args.input_ch_cam)
    assert nerf_train.newest_checkpoint(run_dir) is None
    for step in (4, 1000, 20):
        nerf_train.save_checkpoint(os.path.join(run_dir, "{:06d}.tar".format(step)), step, model, opt, cam)
    assert os.path.basename(nerf_train.newest_checkpoint(run_dir)) == "001000.tar"
    ckpt = torch.load(os.path.join(run_dir, "000004.tar"), map_location="cpu")
    assert sorted(ckpt) == ["embedcam_state_dict", "global_step", "network_fn_state_dict", "optimizer_state_dict"]
    assert ckpt["global_step"] == 4 and sorted(ckpt["network_fn_state_dict"]) == sorted("module." + k for k in model.state_dict())
    assert torch.equal(ckpt["embedcam_state_dict"]["weight"], cam.weight.detach())
    # what nerf_render, nerf_test and nerf_extract read: args.json and the newest checkpoint whose name contains 000.tar
    cfg, state, path = load_checkpoint(str(tmp_path), "run1")
    assert os.path.basename(path) == "001000.tar" and cfg["multires_views"] == 2 and cfg["N_samples"] == 256 and cfg["expname"] == "run1"
    # ... which is the rule train() warns by when it saves under another name
    assert [nerf_train.read_by_the_tools(n) for n in ("000004.tar", "001000.tar", "000020.tar", "004499.tar", "500000.tar")] == [
        False, True, False, False, True]
    assert all(torch.equal(state["module." + k], v) for k, v in model.state_dict().items())
    with open(os.path.join(run_dir, "args.json")) as f:
        assert json.load(f) == vars(args)


def write_scene(tmp, std_files, depth=True):
    from PIL import Image
    scene = os.path.join(tmp, "data", "s")
    os.makedirs(scene)
    raw = np.arange(48, dtype=np.uint16).reshape(6, 8) * 50
    raw[0, :4] = 0
    Image.fromarray(np.full((6, 8, 3), 51, np.uint8)).save(os.path.join(scene, "0.png"))
    Image.fromarray(raw).save(os.path.join(scene, "0_d.png"))
    Image.fromarray(np.full((6, 8), 40, np.uint16)).save(os.path.join(scene, "0_s.png"))
    fr = {"transform_matrix": np.eye(4).tolist(), "fx": 9., "fy": 9., "cx": 4., "cy": 3., "file_path": "0.png"}
    if depth:
        fr["depth_file_path"] = "0_d.png"
    if std_files:
        fr["depth_std_file_path"] = "0_s.png"
    with open(os.path.join(scene, "transforms_train.json"), "w") as f:
        json.dump({"frames": [fr], "near": 0.1, "far": 4.0, "depth_scaling_factor": 1000.0}, f)
    return ["--data_dir", os.path.join(tmp, "data"), "--scene_id", "s", "--image_hw", "6", "8"], raw


def test_json_data_rules(tmp_path):
    flags, raw = write_scene(str(tmp_path / "a"), std_files=True)
    run = X.load_scene(X.build_parser().parse_args(flags))
    assert run.images.shape == (1, 6, 8, 3) and run.images.dtype == torch.float32 and float(run.images[0, 0, 0, 0]) == np.float32(0.2)
    assert run.depths.shape == (1, 6, 8, 2) and run.valid_depths.dtype == torch.bool and (run.near, run.far) == (0.1, 4.0)
    valid = raw > 0
    assert np.array_equal(run.valid_depths[0].numpy(), valid)
    assert np.array_equal(run.depths[0, ..., 0].numpy(), (raw / 1000.).astype(np.float32))
    assert (run.depths[0, ..., 0].numpy()[~valid] == 0).all()           # no depth: 0, below near, so the ray is sampled around its own depth
    assert np.array_equal(run.depths[0, ..., 1].numpy(), np.where(valid, np.float32(0.04), np.float32(0)))
    assert run.bb_center.shape == (3,) and float(run.bb_scale) > 0
    # without a std file --depth_std is required, and used
    flags, _ = write_scene(str(tmp_path / "b"), std_files=False)
    with pytest.raises(SystemExit, match="depth_std"):
        X.load_scene(X.build_parser().parse_args(flags))
    run = X.load_scene(X.build_parser().parse_args(flags + ["--depth_std", "0.07"]))
    assert np.array_equal(run.depths[0, ..., 1].numpy(), np.where(valid, np.float32(0.07), np.float32(0)))
    # without a depth loss nothing of the depth is read or needed
    run = X.load_scene(X.build_parser().parse_args(flags + ["--depth_loss_weight", "0"]))
    assert run.depths is None and run.valid_depths is None
    # a std file without the json's scale is reported, not divided by None
    with pytest.raises(SystemExit, match="depth_scaling_factor"):
        X.load_depth_png(os.path.join(str(tmp_path / "a"), "data", "s"), "0_s.png", 6, 8, None)
    flags, _ = write_scene(str(tmp_path / "c"), std_files=False, depth=False)
    with pytest.raises(SystemExit, match="depth_file_path"):
        X.load_scene(X.build_parser().parse_args(flags + ["--depth_std", "0.07"]))
    assert X.load_scene(X.build_parser().parse_args(flags + ["--depth_loss_weight", "0"])).depths is None
