"""The front end of NeRF training on the MI355X (csrc/nerftrain.hip through ops.nerf_train_batch and ops.nerf_train_samples,
nerf_train.render_rays_train(z2="draw"), nerf_train.train and the nerf_train command line).

The batch is compared with the reference's own results (tests/golden/nerf_train.npz) for equality, the view directions with the
float64 normalisation to one float32 ulp; the drawn samples with tests/nerf_train_ref.py in float64, every element within the case's
bound (tests/golden/nerf_train_bounds.json: 8 x the float32 checker's error, written by make_nerf_train_golden.py, never typed in)
outside the rays the json lists as rejected -- with the golden's staged raw1, and with NeRF.query's raw1 of the case's batch, for which
the checkers, the bound and the rejected rays are evaluated anew.  The checker's results are computed once per case and shared."""
import json
import os
import shutil
from argparse import Namespace

import numpy as np
import pytest
import torch

import nerf_render_ref as V
import nerf_train_ref as T
from nerf_rpn_amd import NeRF, nerf_train, ops
from nerf_train_ref import bounds, golden_npz, refs  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def batch_of(c, **kw):
    args = dict(depth=c.depth, valid=c.valid, z=c.z, t_rand=c.t_rand)
    args.update(kw)
    return ops.nerf_train_batch(c.intrinsic, c.c2w, T.H, T.W, c.pix, c.image, **args)


def samples_of(c, b, raw1=None, **kw):
    args = dict(depth_range=b["depth_range"], u=c.u)
    args.update(kw)
    return ops.nerf_train_samples(c.raw1 if raw1 is None else raw1, b["z1"], b["rays"], c.near, c.far, float(c.z[-1] - c.z[-2]), **args)


@pytest.mark.parametrize("name", T.NAMES)
def test_batch_equals_the_reference(dev, refs, golden_npz, name):
    c, _, f64 = refs(name)
    b = batch_of(c)
    for k in ("rays", "target_s", "target_d", "target_vd", "depth_range", "z1"):
        got = b[k].cpu().numpy()
        assert got.dtype == golden_npz[f"{name}/{k}"].dtype and np.array_equal(got, golden_npz[f"{name}/{k}"]), k
    d = golden_npz[f"{name}/rays"][:, 3:].astype(np.float64)          # the float32 directions, widened
    ref = d / np.sqrt((d * d).sum(-1, keepdims=True))
    err = np.abs(b["viewdirs"].cpu().numpy().astype(np.float64) - ref)
    print(f"{name}: viewdirs error {err.max():.3g}")
    assert (err <= np.spacing(np.abs(ref).astype(np.float32))).all()


def test_batch_without_depth_or_perturbation(dev, refs):
    c, _, _ = refs("r7_s13_mixed")
    full = batch_of(c)
    b = batch_of(c, depth=None, valid=None, z=None, t_rand=None)
    assert sorted(b) == ["rays", "target_s", "viewdirs"]
    for k in b:
        assert torch.equal(b[k], full[k]), k


def test_rays_of_every_pixel_equal_nerf_renders(dev, refs):
    c, _, _ = refs("r7_s13_mixed")
    b = ops.nerf_train_batch(c.intrinsic, c.c2w, T.H, T.W, torch.arange(T.H * T.W), c.image)
    v = V.case_inputs(V.CASES[0])
    st = ops.nerf_camopt_prepare(v.state, v.cfg, torch.zeros(T.H * T.W, 3), H=T.H, W=T.W, intrinsic=c.intrinsic, c2w=c.c2w, near=c.near,
                                 far=c.far, n_samples=4)
    assert torch.equal(b["rays"], st.rays)


@pytest.mark.parametrize("name", T.NAMES)
def test_z2_within_bound_of_fp64(dev, refs, bounds, name):
    c, _, f64 = refs(name)
    bd = bounds["cases"][name]
    rejected = np.zeros(c.R, bool)
    rejected[bd["rejected"]] = True
    assert rejected.sum() <= bounds["reject_cap"] * c.R
    b = batch_of(c)
    got = samples_of(c, b).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (c.R, c.S) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - f64["z2"].numpy())[~rejected].max()
    print(f"{name}: z2 error {err:.3g} (bound {bd['z2']['bound']:.3g}, float32 checker {bd['z2']['fp32_error']:.3g}), "
          f"ratio {err / bd['z2']['bound']:.3g}")
    assert err <= bd["z2"]["bound"]
    assert got.min() >= np.float32(c.near) and got.max() <= np.float32(c.far)


@pytest.mark.parametrize("name", T.NAMES)
def test_z2_through_the_network_query_within_bound_of_fp64(dev, refs, bounds, name):
    """End to end: the first list's raw is NeRF.query's on the device, not a staged one.  Both checkers then run on that raw1 on the
    host, so the bound (8 x the float32 checker's error, floored at one ulp), the rejected rays and their cap are that raw1's."""
    c, _, _ = refs(name)
    L = T.loop_inputs()
    model = loop_model(L, dev)
    b = batch_of(c)
    pts = b["rays"][:, None, :3] + b["rays"][:, None, 3:] * b["z1"][..., :, None]
    raw1 = model.query(pts, b["viewdirs"], L.embedcam[0], T.LOOP.bb_center, T.LOOP.bb_scale).detach()
    assert raw1.shape == (c.R, c.S, 4) and raw1.is_cuda and torch.isfinite(raw1).all()
    got = samples_of(c, b, raw1=raw1).cpu().numpy()
    ref, rejected, err32, bound = T.z2_reference_for(c, raw1)
    assert bound == max(T.FACTOR * err32, float(np.spacing(np.float32(np.abs(ref[~rejected]).max()))))
    assert got.dtype == np.float32 and got.shape == (c.R, c.S) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - ref)[~rejected].max()
    print(f"{name}: z2 error {err:.3g} through NeRF.query (bound {bound:.3g}, float32 checker {err32:.3g}, rejected {int(rejected.sum())}), "
          f"ratio {err / bound:.3g}")
    assert err <= bound
    assert got.min() >= np.float32(c.near) and got.max() <= np.float32(c.far)
    # a ray with a given depth does not read raw1: its samples are those of the staged raw1, bit for bit
    given = (b["depth_range"][:, 0] >= c.near).cpu().numpy()
    assert np.array_equal(got[given], samples_of(c, b).cpu().numpy()[given])


@pytest.mark.parametrize("name", ["r7_s13_mixed", "r130_s32_mixed"])
def test_deterministic_branch_equals_nerf_render_samples(dev, refs, name):
    c, _, _ = refs(name)
    b = batch_of(c)
    lower_bound = float(c.z[-1] - c.z[-2])
    assert np.float64(c.z[-1]) - np.float64(c.z[-2]) == lower_bound          # the float32 difference is exact
    got = ops.nerf_train_samples(c.raw1, c.z, b["rays"], c.near, c.far, lower_bound)
    assert torch.equal(got, ops.nerf_render_samples(c.raw1, b["rays"], c.z, c.near, c.far))
    # a per-ray copy of the shared list takes the other kernel to the same bits
    assert torch.equal(got, ops.nerf_train_samples(c.raw1, c.z[None].expand(c.R, -1).contiguous(), b["rays"], c.near, c.far, lower_bound))


def test_repeats_and_batch_position_are_bit_equal(dev, refs):
    c, _, _ = refs("r130_s32_mixed")
    b = batch_of(c)
    a = samples_of(c, b)
    assert torch.equal(a, samples_of(c, b))
    order = torch.arange(c.R - 1, -1, -1)[:67]                 # 67 of the rays, reversed: another R, other positions, other waves
    dv = a.device
    sub = ops.nerf_train_samples(c.raw1[order], b["z1"][order.to(dv)], b["rays"][order.to(dv)], c.near, c.far, float(c.z[-1] - c.z[-2]),
                                 depth_range=b["depth_range"][order.to(dv)], u=c.u[order])
    assert torch.equal(sub, a[order.to(dv)])
    b2 = ops.nerf_train_batch(c.intrinsic, c.c2w, T.H, T.W, c.pix[order], c.image, c.depth, c.valid, c.z, c.t_rand[order])
    for k in b:
        assert torch.equal(b2[k], b[k][order.to(dv)]), k


def test_arguments_are_checked(dev, refs):
    c, _, _ = refs("r3_s4_valid")
    E = ops.lib.NrpnError
    with pytest.raises(E, match="go together"):
        batch_of(c, valid=None)
    with pytest.raises(E, match="go together"):
        batch_of(c, t_rand=None)
    with pytest.raises(E, match="t_rand"):
        batch_of(c, t_rand=c.t_rand[:, :3])
    with pytest.raises(E, match="pix"):
        ops.nerf_train_batch(c.intrinsic, c.c2w, T.H, T.W, c.pix.float(), c.image)
    with pytest.raises(E, match="outside"):
        ops.nerf_train_batch(c.intrinsic, c.c2w, T.H, T.W, torch.tensor([0, T.H * T.W]), c.image, check=True)
    with pytest.raises(E, match="image"):
        ops.nerf_train_batch(c.intrinsic, c.c2w, T.H, T.W + 1, c.pix, c.image)
    b = batch_of(c)
    with pytest.raises(E, match="supported range"):
        ops.nerf_train_samples(c.raw1[:, :1], c.z[:1], b["rays"], c.near, c.far, 0.1)
    with pytest.raises(E, match="u"):
        samples_of(c, b, u=c.u[:, :2])
    with pytest.raises(E, match="depth_range"):
        samples_of(c, b, depth_range=b["depth_range"][:, :2])
    with pytest.raises(E, match="above far"):
        ops.nerf_train_samples(c.raw1, b["z1"], b["rays"], c.far, c.near, 0.1)
    with pytest.raises(NotImplementedError, match="requires grad"):
        samples_of(c, b, raw1=c.raw1.clone().requires_grad_(True))
    L = ops.lib.load()
    assert L.nrpn_nerftrain_work_bytes(c.R, c.S) == c.R * c.S * 8 and L.nrpn_nerftrain_work_bytes(c.R, 1) == -1
    z2 = torch.empty(c.R, c.S, device=b["rays"].device)
    work = torch.empty(8, dtype=torch.uint8, device=z2.device)
    with pytest.raises(E, match="too small"):
        ops.lib.call("nerftrain_samples", c.raw1.to(z2.device).data_ptr(), b["z1"].data_ptr(), c.S, b["rays"].data_ptr(), None, None, c.S, 0.1,
                 c.near, c.far, c.R, work.data_ptr(), 8, z2.data_ptr(), None)
    with pytest.raises(E, match="z1_stride"):
        ops.lib.call("nerftrain_samples", c.raw1.to(z2.device).data_ptr(), b["z1"].data_ptr(), 1, b["rays"].data_ptr(), None, None, c.S, 0.1,
                 c.near, c.far, c.R, work.data_ptr(), 8, z2.data_ptr(), None)


def loop_model(L, dev):
    model = NeRF(T.LOOP.cfg)
    model.load_state_dict(L.state)
    return model.to(dev)


def test_draw_mode_equals_the_drawn_samples_given(dev, refs):
    c, _, _ = refs("r7_s13_mixed")
    L = T.loop_inputs()
    model = loop_model(L, dev)
    b = batch_of(c)
    kw = dict(depth_range=b["depth_range"], u=c.u, lower_bound=float(c.z[-1] - c.z[-2]), near=c.near, far=c.far)
    args = (model, b["rays"][:, :3], b["rays"][:, 3:], b["viewdirs"], b["z1"])
    rest = (L.embedcam[0], T.LOOP.bb_center, T.LOOP.bb_scale)
    a = nerf_train.render_rays_train(*args, "draw", *rest, **kw)
    drawn = a.pop("z_vals_2")
    assert drawn.shape == (c.R, c.S) and not (drawn[:, 1:] >= drawn[:, :-1]).all()       # in u's order, not sorted
    g = nerf_train.render_rays_train(*args, drawn, *rest)
    assert sorted(a) == sorted(g)
    for k in a:
        assert torch.equal(a[k], g[k]), k
    assert (a["z_vals"][:, 1:] >= a["z_vals"][:, :-1]).all()
    with pytest.raises(ValueError, match="lower_bound"):
        nerf_train.render_rays_train(*args, "draw", *rest)
    with pytest.raises(ValueError, match="draw"):
        nerf_train.render_rays_train(*args, "sample", *rest, **kw)


def loop_args(tmp, **kw):
    a = dict(expname="loop", ckpt_dir=str(tmp), no_reload=True, N_rand=T.LOOP.N_rand, N_samples=T.LOOP.N_samples, lrate=T.LOOP.lrate,
             start_decay_lrate=400000, end_decay_lrate=500000, depth_loss_weight=T.LOOP.depth_loss_weight, perturb=1.,
             raw_noise_std=T.LOOP.raw_noise_std, lindisp=False, i_print=1, i_weights=100000, N_iters=T.LOOP.steps + 1, **T.LOOP.cfg)
    a.update(kw)
    return Namespace(**a)


def test_eight_loop_steps_within_bound_of_fp64(dev, bounds, tmp_path):
    L = T.loop_inputs()
    run = Namespace(images=L.images, depths=L.depths, valid_depths=L.valid_depths, poses=L.poses, intrinsics=L.intrinsics, near=L.near,
                    far=L.far, bb_center=torch.tensor(T.LOOP.bb_center), bb_scale=torch.tensor(T.LOOP.bb_scale, dtype=torch.float32),
                    state_dict=L.state, embedcam=L.embedcam)

    def rand(step, name, shape):
        return getattr(L.steps[step - 1], name)
    out = nerf_train.train(run, loop_args(tmp_path), rand=rand)
    losses = [row[1] for row in out.log]
    ref, bound = bounds["loop"]["fp64"], bounds["loop"]["bound"]
    assert out.step == T.LOOP.steps and len(losses) == len(ref) == T.LOOP.steps
    bad = []
    for i, (g, r, b) in enumerate(zip(losses, ref, bound)):
        print(f"step {i + 1}: loss {g:.9g}, float64 {r:.9g}, error {abs(g - r):.3g} (bound {b:.3g}), ratio {abs(g - r) / b:.3g}")
        if not abs(g - r) <= b:
            bad.append((i + 1, g, r, b))
    assert not bad, bad
    assert losses[-1] < losses[0]
    assert os.path.exists(os.path.join(str(tmp_path), "loop", "{:06d}.tar".format(T.LOOP.steps)))


CLI_HW = 8      # the held-out views are scored with a 7 x 7 SSIM window


def write_scene(tmp):
    """A scene directory with three training views and one held-out view of 8 x 8 pixels, a depth on half the pixels -> the command
    line's common flags."""
    from PIL import Image
    L = T.loop_inputs()
    gen = torch.Generator().manual_seed(7400)
    scene = os.path.join(tmp, "data", "scene0000_00")
    os.makedirs(scene)
    frames = []
    for i in range(T.LOOP.views):
        image = (torch.rand(CLI_HW, CLI_HW, 3, generator=gen) * 255).to(torch.uint8).numpy()
        depth = (torch.rand(CLI_HW, CLI_HW, generator=gen) * 3000 + 500).to(torch.int32).numpy().astype(np.uint16)
        depth.reshape(-1)[1::2] = 0
        Image.fromarray(image).save(os.path.join(scene, f"{i}.png"))
        Image.fromarray(depth).save(os.path.join(scene, f"{i}_d.png"))
        fx, fy, cx, cy = (float(v) for v in L.intrinsics[i])
        frames.append({"transform_matrix": L.poses[i].tolist(), "fx": fx, "fy": fy, "cx": cx, "cy": cy, "file_path": f"{i}.png",
                       "depth_file_path": f"{i}_d.png"})
    for name, fr in (("transforms_train.json", frames), ("transforms_test.json", frames[:1])):
        with open(os.path.join(scene, name), "w") as f:
            json.dump({"frames": fr, "near": L.near, "far": L.far, "depth_scaling_factor": 1000.0}, f)
    return ["--expname", "run1", "--ckpt_dir", os.path.join(tmp, "ckpt"), "--data_dir", os.path.join(tmp, "data"), "--scene_id",
            "scene0000_00", "--image_hw", str(CLI_HW), str(CLI_HW)]


def test_command_line_trains_resumes_and_its_checkpoint_renders(dev, tmp_path):
    from nerf_rpn_amd.scripts import nerf_render, nerf_train as X
    common = write_scene(str(tmp_path))
    flags = common + ["--N_rand", "16", "--N_samples", "8", "--multires_views", "2", "--depth_std", "0.1", "--i_print", "2"]
    # the loop runs steps 1 .. N_iters - 1, as the reference's range(start, N_iters) does
    with pytest.warns(UserWarning, match="000004.tar is resumed from by nerf_train only"):     # not a name the render tools read
        first = X.main(flags + ["--N_iters", "5"])
    run_dir = os.path.join(str(tmp_path), "ckpt", "run1")
    assert first.step == 4 and [row[0] for row in first.log] == [2, 4]
    with open(os.path.join(run_dir, "args.json")) as f:
        cfg = json.load(f)
    assert cfg["N_samples"] == 8 and cfg["multires_views"] == 2 and cfg["input_ch_cam"] == 4 and cfg["netdepth"] == 8
    ckpt = torch.load(os.path.join(run_dir, "000004.tar"), map_location="cpu")
    assert sorted(ckpt) == ["embedcam_state_dict", "global_step", "network_fn_state_dict", "optimizer_state_dict"]
    assert ckpt["global_step"] == 4 and all(k.startswith("module.") for k in ckpt["network_fn_state_dict"])
    assert os.path.exists(os.path.join(run_dir, "test_images_scene0000_00", "metrics.txt"))
    second = X.main(flags + ["--N_iters", "7"])
    assert second.step == 6 and os.path.exists(os.path.join(run_dir, "000006.tar"))
    steps = {int(s["step"]) for s in second.optimizer.state_dict()["state"].values()}
    assert steps == {6}
    assert torch.equal(second.embedcam.weight.cpu(), ckpt["embedcam_state_dict"]["weight"])      # read back, never trained
    with pytest.raises(NotImplementedError, match="N_importance"):
        X.main(flags + ["--N_importance", "64"])
    # the render tools read the newest checkpoint whose name contains 000.tar, as the reference does: the same file under such a name
    shutil.copy(os.path.join(run_dir, "000006.tar"), os.path.join(run_dir, "001000.tar"))
    written = nerf_render.main(common + ["--output_dir", os.path.join(str(tmp_path), "out"), "--frames", "0"])
    assert len(written) == 1 and all(os.path.exists(p) for p in written[0])


@pytest.mark.parametrize("flags", [dict(depth_loss_weight=0., lindisp=True), dict(depth_loss_weight=0., perturb=0.), dict(perturb=0.)])
def test_one_pass_and_unperturbed_paths(dev, tmp_path, flags):
    """depth_loss_weight <= 0 takes render_rays' plain path (:602-614: N_samples between near and far, perturbed by the batch kernel,
    no second list); perturb 0 leaves the base list shared and the second list deterministic."""
    L = T.loop_inputs()
    run = Namespace(images=L.images, depths=L.depths, valid_depths=L.valid_depths, poses=L.poses, intrinsics=L.intrinsics, near=L.near,
                    far=L.far, bb_center=torch.tensor(T.LOOP.bb_center), bb_scale=torch.tensor(T.LOOP.bb_scale, dtype=torch.float32),
                    state_dict=L.state, embedcam=L.embedcam)
    asked = []

    def rand(step, name, shape):
        asked.append(name)
        return getattr(L.steps[step - 1], name) if name in ("image", "pix") else None
    out = nerf_train.train(run, loop_args(tmp_path, N_iters=3, **flags), rand=rand)
    assert out.step == 2 and len(out.log) == 2 and all(np.isfinite(row[1]) and row[1] > 0 for row in out.log)
    two_pass, perturbed = flags.get("depth_loss_weight", 1.) > 0., flags.get("perturb", 1.) > 0.
    assert ("t_rand" in asked) == perturbed and ("u" in asked) == (two_pass and perturbed) and "noise" in asked
