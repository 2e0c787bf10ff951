"""The camera-embedding objective on the MI355X (csrc/nerfrender.hip: nerfcamopt_* kernels) through ops.nerf_camopt_prepare /
ops.nerf_camopt_eval and the nerf_test_opt command line.

The reference is tests/nerf_camopt_ref.py in float64: autograd through the reference's whole graph.  Per element, loss and rgb_map
must lie within 8 x the float32 checker's error of that case (tests/golden/nerf_camopt_bounds.json) and the gradient within that plus
the case's flip allowance (a relu whose float64 pre-activation lies within the pre bound of 0 may come out on the other side).  The
cases are the render cases with a camera embedding: a partial tile (odd_5x7, 280 points per pass), one ray, ties in the merged
samples (clamped_4x4), rays that straddle tiles (full_3x3, 128 samples per pass), the one-pass path (plain_4x6) and view encoding
(views_cam_3x5); at the zero embedding and at (0.7, -1.3, 0.4, 2.1); with equal batches and with a remainder batch.

The command line runs on the two loop cases' networks at 7 x 8 and 8 x 7 pixels: nerf_view_metrics takes no frame below its 7 x 7
SSIM window, so the cases' own 3 x 5 and 5 x 7 frames cannot be measured.  Every figure is printed before it is asserted."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nerf_camopt_ref as C
import nerf_eval_ref as E
from nerf_camopt_ref import camopt_bounds, camopt_refs  # noqa: F401  (fixtures)
from nerf_rpn_amd import lib, ops
from nerf_rpn_amd.scripts import nerf_test as X
from nerf_rpn_amd.scripts import nerf_test_opt as XO

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
ALL = [(n, cam, part) for n in C.CASE_NAMES for cam in C.CAMS for part in C.PARTITIONS]


def frame_args(c):
    return dict(H=c.H, W=c.W, intrinsic=c.intrinsic, c2w=c.c2w, near=c.near, far=c.far, bb_center=c.bb_center, bb_scale=c.bb_scale,
                z_samples=c.z_samples, n_samples=c.n_samples, lindisp=c.lindisp)


def prepare(r, given_z2, **kw):
    c = r["c"]
    z2 = r["z2"] if given_z2 and not c.plain else None
    return ops.nerf_camopt_prepare(c.state, c.cfg, r["target"], ray_weight=r["rw"], z2=z2, **frame_args(c), **kw)


def evaluate(state, cam, rgb=True):
    out = ops.nerf_camopt_eval(state, C.CAMS[cam] if isinstance(cam, str) else cam, return_rgb=rgb)
    n = state.n
    return (out[0], out[1].cpu().numpy()) + ((out[2].reshape(n, 3).cpu().numpy(),) if rgb else ())


def check(tag, got, o64, bound, allow):
    loss, grad, rgb = got
    want_loss, want_grad, want_rgb = float(o64["losses"].sum()), o64["grad"].numpy(), o64["rgb_map"].numpy()
    e_loss, e_rgb, e_grad = abs(loss - want_loss), np.abs(rgb.astype(np.float64) - want_rgb), np.abs(grad - want_grad)
    g_bound = bound["grad"]["bound"] + np.array(allow["allow"])
    print(f"{tag}: loss error {e_loss:.3g} (bound {bound['loss']['bound']:.3g}), rgb_map {e_rgb.max():.3g} ({bound['rgb_map']['bound']:.3g}), "
          f"grad {e_grad.max():.3g} ({bound['grad']['bound']:.3g} + flips {max(allow['allow']):.3g}, |F| {allow['F']}) at |grad| "
          f"{np.abs(want_grad).max():.3g}")
    assert grad.dtype == np.float64 and rgb.dtype == np.float32 and isinstance(loss, float)
    assert e_loss <= bound["loss"]["bound"]
    assert (e_rgb <= bound["rgb_map"]["bound"]).all()
    assert (e_grad <= g_bound).all()


@pytest.mark.parametrize("mode", ["given_z2", "end_to_end"])
@pytest.mark.parametrize("name,cam,part", ALL)
def test_objective_within_the_bounds_of_fp64(dev, camopt_refs, camopt_bounds, name, cam, part, mode):
    r = camopt_refs(name, cam, part, mode == "given_z2")
    b = camopt_bounds["cases"][name]
    got = evaluate(prepare(r, mode == "given_z2"), cam)
    check(f"{name}/{cam}/{part}/{mode}", got, r["o64"], b[mode], b["allow"][mode][cam][part])


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_rgb_map_is_bit_equal_to_nerf_render(dev, camopt_refs, name):
    r = camopt_refs(name, "far", "remainder")
    c = r["c"]
    st = prepare(r, False)
    for cam in C.CAMS:
        _, _, rgb = evaluate(st, cam)
        want = ops.nerf_render(c.state, c.cfg, embedded_cam=C.CAMS[cam], **frame_args(c))["rgb_map"].reshape(-1, 3).cpu().numpy()
        assert np.array_equal(rgb, want), (name, cam, float(np.abs(rgb - want).max()))


@pytest.mark.parametrize("name", ["odd_5x7", "clamped_4x4", "plain_4x6"])
def test_weights_kernel_agrees_with_the_composite_kernel(dev, name):
    """prepare's per-list float64 weights, merged (list 1 first on equal z) and rounded, are nerf_render's weights bit for bit: tiles
    that straddle rays and a partial last tile, ties between the lists, no second list; chunks of 3 rays end mid-frame."""
    c = C.case(name)
    st = ops.nerf_camopt_prepare(c.state, c.cfg, C.target_for(c), chunk=3, **frame_args(c))
    out = ops.nerf_render(c.state, c.cfg, return_samples=True, chunk=3, **frame_args(c))
    n = st.n
    z_vals, weights = (out[k].reshape(n, -1).cpu().numpy() for k in ("z_vals", "weights"))
    z1, w1 = st.inputs.z1.cpu().numpy(), st.w1.cpu().numpy()
    assert (st.z2 is None) == (st.w2 is None) == c.plain
    z2 = np.zeros((n, 0), np.float32) if c.plain else st.z2.cpu().numpy()
    w2 = np.zeros((n, 0), np.float64) if c.plain else st.w2.cpu().numpy()
    assert w1.dtype == w2.dtype == np.float64 and weights.dtype == z_vals.dtype == np.float32
    for r in range(n):
        z_cat = np.concatenate([z1, z2[r]])
        order = np.argsort(z_cat, kind="stable")
        assert np.array_equal(z_vals[r], z_cat[order]), (name, r)
        assert np.array_equal(weights[r], np.concatenate([w1[r], w2[r]])[order].astype(np.float32)), (name, r)


@pytest.mark.parametrize("name", ["full_3x3", "odd_5x7", "plain_4x6"])
def test_chunk_and_cache_do_not_change_the_result(dev, camopt_refs, name):
    r = camopt_refs(name, "far", "remainder")
    c, n = r["c"], C.num_rays(r["c"])
    s1 = c.n_samples if c.plain else c.n_samples // 2
    slot = lib.query("nerfcamopt_work_bytes", 2, n, 3, s1, 0 if c.plain else s1)
    # the budget decides which chunks keep g, nothing else: none, the first, all
    runs = []
    for budget, cached in ((0, 0), (slot, 1), (None, -(-n // 3))):
        st = prepare(r, False, chunk=3, cache_bytes=budget)
        assert st.cached_chunks == cached and st.chunks == -(-n // 3), (st.cached_chunks, st.chunks)
        runs.append(evaluate(st, "far"))
        again = evaluate(st, "far")
        assert runs[-1][0] == again[0] and all(np.array_equal(a, b) for a, b in zip(runs[-1][1:], again[1:]))      # repeatable
    for other in runs[1:]:
        assert other[0] == runs[0][0] and np.array_equal(other[1], runs[0][1]) and np.array_equal(other[2], runs[0][2])
    # the chunk size: per-ray results bit-equal, the sums over rays within their rounding
    t = C.head_terms(c, C.CAMS["far"], torch.float64)
    fg = C.fixed_gradient(c, t, r["target"], r["rw"])
    terms = t["pre"].numel() * 3
    tol_grad, tol_loss = 2 * terms * U64 * fg["abs_terms"].numpy(), 2 * 3 * n * U64 * float(fg["loss"])
    for chunk in (1, n):
        got = evaluate(prepare(r, False, chunk=chunk), "far")
        assert np.array_equal(got[2], runs[0][2])
        d_loss, d_grad = abs(got[0] - runs[0][0]), np.abs(got[1] - runs[0][1])
        print(f"{name}: chunk {chunk} against 3: loss differs by {d_loss:.3g} (tolerance {tol_loss:.3g}), grad by {d_grad.max():.3g} "
              f"({tol_grad.min():.3g})")
        assert d_loss <= tol_loss and (d_grad <= tol_grad).all()


def test_arguments_are_checked(dev, camopt_refs):
    r = camopt_refs("one_ray", "far", "equal")
    c = r["c"]
    with pytest.raises(lib.NrpnError, match="camera embedding"):
        v0 = C.V.case_inputs(C.V.CASES[C.V.NAMES.index("views_3x5")])
        ops.nerf_camopt_prepare(v0.state, v0.cfg, torch.zeros(15, 3), **frame_args(v0))
    with pytest.raises(lib.NrpnError, match="pixels"):
        ops.nerf_camopt_prepare(c.state, c.cfg, torch.zeros(2, 3), **frame_args(c))
    with pytest.raises(lib.NrpnError, match="ray_weight"):
        ops.nerf_camopt_prepare(c.state, c.cfg, r["target"], ray_weight=torch.ones(2), **frame_args(c))
    st = prepare(r, False)
    with pytest.raises(lib.NrpnError, match="input_ch_cam"):
        ops.nerf_camopt_eval(st, [0., 1.])
    # the default ray weight is the image's mean squared error
    loss, _, rgb = evaluate(ops.nerf_camopt_prepare(c.state, c.cfg, r["target"], **frame_args(c)), "far")
    want = float(((rgb.astype(np.float64) - r["target"].numpy()) ** 2).mean())
    assert abs(loss - want) <= 1e-6 * want           # rgb is rounded to float32 on its way out, the loss is not


def cli_run(tmp_path, name):
    c, target, batches = C.cli_case(name)
    single = SimpleNamespace(**dict(vars(c), poses=c.c2w[None], frames=1))
    argv = E.write_run(tmp_path, single, c.rgb8, np.zeros((1, c.H, c.W), np.uint16))
    return c, target, batches, argv


@pytest.mark.parametrize("name", list(C.CLI_FRAMES))
def test_cli_test_opt(dev, camopt_bounds, tmp_path, name):
    c, target, batches, argv = cli_run(tmp_path, name)
    res = XO.main(argv + ["--opt_steps", str(C.CLI_STEPS), "--N_rand", str(C.CLI_N_RAND), "--opt_seed", str(C.CLI_SEED)])
    exp = os.path.join(str(tmp_path), "ckpt", "run1")
    assert res["dir"] == os.path.join(exp, "test_images_with_optimization_scene0000_00")
    code = np.loadtxt(os.path.join(exp, "test_latent_codes_scene0000_00", "0.txt"))
    b = camopt_bounds["loop4"][name]
    diff = np.abs(code - np.array(b["embedding64"]))
    print(f"{name}: latent code {code.tolist()}, float64 loop {b['embedding64']}, off by {diff.max():.3g}, bound {b['bound']:.3g}")
    assert code.shape == (4,) and (diff <= b["bound"]).all()
    for f in ("metrics.txt", "0_rgb.jpg", "0_d.png"):
        assert os.path.exists(os.path.join(res["dir"], f)), f
    with open(os.path.join(res["dir"], "metrics.txt")) as f:
        keys = [line.split(":")[0] for line in f.read().splitlines()]
    assert keys == ["img_loss", "psnr", "ssim"] and len(res["frames"]) == 1
    # the frame was measured on the render at the written vector
    out = ops.nerf_render(c.state, c.cfg, embedded_cam=code.astype(np.float32), **frame_args(c))
    want = ops.nerf_view_metrics(out["rgb_map"], target.reshape(c.H, c.W, 3), out["depth_map"], torch.zeros(c.H, c.W),
                                 torch.zeros(c.H, c.W, dtype=torch.bool), far=c.far)
    for k in ("img_loss", "psnr", "ssim"):
        assert res["frames"][0][k] == want[k], k


def test_cli_test_task_does_not_touch_the_new_code(dev, tmp_path):
    """nerf_test --task test writes the same bytes whether or not the loop's module can be imported, and no latent codes."""
    _, _, _, argv = cli_run(tmp_path, "odd_5x7")
    files = {}
    for tag, blocked in (("blocked", True), ("plain", False)):
        saved = sys.modules.get("nerf_rpn_amd.camopt")
        if blocked:
            sys.modules["nerf_rpn_amd.camopt"] = None          # an import of it raises ImportError
        try:
            res = X.main(argv + ["--task", "test", "--output_dir", os.path.join(str(tmp_path), tag)])
        finally:
            if saved is not None:
                sys.modules["nerf_rpn_amd.camopt"] = saved
            else:
                sys.modules.pop("nerf_rpn_amd.camopt", None)
        files[tag] = {f: open(os.path.join(res["dir"], f), "rb").read() for f in sorted(os.listdir(res["dir"]))}
    assert sorted(files["plain"]) == ["0_d.png", "0_rgb.jpg", "metrics.txt"] and files["plain"] == files["blocked"]
    assert not os.path.exists(os.path.join(str(tmp_path), "ckpt", "run1", "test_latent_codes_scene0000_00"))
