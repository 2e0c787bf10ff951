"""GPU tests of the differentiable NeRF query (ops.nerf_query, NeRF.query) against the float64 checker, with the
per-tensor bounds of tests/golden/nerf_query_bounds.json (8 x the float32 checker's own error)."""
import numpy as np
import pytest
import torch

import nerf_query_ref as Q
import nerf_render_ref as V
from nerf_query_ref import bounds, golden_npz, refs  # noqa: F401

from nerf_rpn_amd import NeRF, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev_state(c):
    return {k: v.to(DEV) for k, v in c.state.items()}


def run(c, chunk=None, params=None):
    """ops.nerf_query on case inputs and the gradients of sum(raw * cot) -> dict of numpy over raw, the 24 gradients and dcam."""
    params = {k: v.clone().requires_grad_(True) for k, v in (params or dev_state(c)).items()}
    cam = None if c.cam is None else c.cam.to(DEV).requires_grad_(True)
    raw = ops.nerf_query(params, c.cfg, c.pts, c.viewdirs, cam, c.bb_center, c.bb_scale, chunk=chunk)
    assert raw.shape == (*c.pts.shape[:2], 4) and raw.dtype == torch.float32 and raw.is_cuda
    wrt = [params[k] for k in Q.PARAMS] + ([] if cam is None else [cam])
    g = torch.autograd.grad((raw * c.cot.to(DEV)).sum(), wrt)
    out = {k: v.cpu().numpy() for k, v in zip(Q.PARAMS, g)}
    assert all(out[k].shape == tuple(params[k].shape) and out[k].dtype == np.float32 for k in Q.PARAMS)
    if cam is not None:
        out["dcam"] = g[-1].cpu().numpy()
    out["raw"] = raw.detach().cpu().numpy()
    return out


def assert_within(name, got, o64, b, tag=""):
    worst = []
    for k in got:
        err = float(np.abs(got[k].astype(np.float64) - o64[k]).max())
        ratio = err / b[k]["bound"] if b[k]["bound"] else (0.0 if err == 0 else float("inf"))      # bound 0: an exact one-term sum
        print(f"{name}{tag}/{k}: error {err:.3g}, bound {b[k]['bound']:.3g}, ratio {ratio:.3g}")
        if not err <= b[k]["bound"]:
            worst.append((k, err, b[k]["bound"]))
    assert not worst, worst


@pytest.fixture(scope="module")
def many(refs):
    """many_tiles at its three chunkings, twice each."""
    c, _, _ = refs("many_tiles")
    return {chunk: (run(c, chunk), run(c, chunk)) for chunk in Q.MANY_TILES_CHUNKS}


@pytest.mark.parametrize("name", [n for n in Q.NAMES if n != "many_tiles"])
def test_within_bounds(name, refs, bounds):
    c, _, o64 = refs(name)
    got = run(c)
    assert sorted(got) == sorted(Q.tensor_names(c.cfg))
    assert_within(name, got, o64, bounds["cases"][name]["tensors"])


@pytest.mark.parametrize("chunk", Q.MANY_TILES_CHUNKS)
def test_many_tiles_within_bounds(chunk, many, refs, bounds):
    _, _, o64 = refs("many_tiles")
    assert_within("many_tiles", many[chunk][0], o64, bounds["cases"]["many_tiles"]["tensors"], f"[chunk={chunk}]")


def test_chunk_invariance_and_repeatability(many):
    """raw is bit-equal across the chunkings; at each chunking two calls give bit-equal gradients."""
    first = many[None][0]
    for chunk, (a, b) in many.items():
        assert np.array_equal(a["raw"], first["raw"]), chunk
        for k in a:
            assert np.array_equal(a[k], b[k]), (chunk, k)


def test_sigma_bit_equal_to_render():
    """On plain_4x6's rays and samples, with pts = o + d z formed as a separately rounded multiply and add, sigma is nerf_render's."""
    c = V.case_inputs(V.CASES[V.NAMES.index("plain_4x6")])
    ref = V.render_case(c, torch.float32)
    rays = torch.cat([ref["rays_o"], ref["rays_d"]], -1).contiguous()
    out = ops.nerf_render(c.state, c.cfg, rays=rays, near=c.near, far=c.far, bb_center=c.bb_center, bb_scale=c.bb_scale,
                          n_samples=c.n_samples, return_samples=True, return_stages=True)
    z = out["z_vals"].cpu()
    pts = rays[:, None, :3] + rays[:, None, 3:] * z[..., None]
    viewdirs = rays[:, 3:] / torch.norm(rays[:, 3:], dim=-1, keepdim=True)
    raw = ops.nerf_query(dev_state(c), c.cfg, pts, viewdirs, None, c.bb_center, c.bb_scale)
    assert torch.equal(raw[..., 3], out["raw1"][..., 3])
    assert float((raw[..., :3] - out["raw1"][..., :3]).abs().max()) <= 1e-5        # the head adds the same terms; viewdirs are given here


@pytest.mark.parametrize("name", ["plain_4x6", "views_cam_3x5"])
def test_raw_bit_equal_to_render(name):
    """On a render's rays and first-pass samples, with pts = o + d z formed as a separately rounded multiply and add and viewdirs
    formed in unit_dir's order (csrc/nerf_mlp.cuh), all four channels of raw are nerf_render's: the two run one view branch and one
    rgb head.  Tiles of 64 points hold several rays in both cases (24 and 8 samples a ray); the 15 x 8 points of views_cam_3x5 end in
    a partial tile, and it has two view frequencies and four camera channels."""
    c = V.case_inputs(V.CASES[V.NAMES.index(name)])
    ref = V.render_case(c, torch.float32)
    rays = torch.cat([ref["rays_o"], ref["rays_d"]], -1).contiguous()
    out = ops.nerf_render(c.state, c.cfg, rays=rays, near=c.near, far=c.far, bb_center=c.bb_center, bb_scale=c.bb_scale,
                          z_samples=c.z_samples, n_samples=c.n_samples, embedded_cam=c.embedded_cam, return_samples=True,
                          return_stages=True)
    raw1 = out["raw1"]
    z =(out["z_vals"] if c.plain else c.z_samples.expand(rays.shape[0], -1)).cpu()
    assert z.shape == raw1.shape[:2]
    pts = rays[:, None, :3] + rays[:, None, 3:] * z[..., None]
    d = rays[:, 3:].to(DEV)           # on the device: its float32 square root and division are the kernel's
    viewdirs = d / torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    raw = ops.nerf_query(dev_state(c), c.cfg, pts, viewdirs, c.embedded_cam, c.bb_center, c.bb_scale)
    assert torch.equal(raw, raw1)


def test_module_matches_op_and_fills_grads(refs):
    c, _, _ = refs("tile_plus_one")
    want = run(c)
    model = NeRF(c.cfg).to(DEV)
    model.load_state_dict(c.state)
    raw = model.query(c.pts, c.viewdirs, c.cam, c.bb_center, c.bb_scale)
    (raw * c.cot.to(DEV)).sum().backward()
    assert np.array_equal(raw.detach().cpu().numpy(), want["raw"])
    grads = {k: p.grad for k, p in model.named_parameters()}
    assert len(grads) == 24 and all(g is not None for g in grads.values())
    for k in Q.PARAMS:
        assert np.array_equal(grads[k].cpu().numpy(), want[k]), k


def test_grad_of_cam_alone(refs, bounds):
    """torch.autograd.grad with respect to embedded_cam with no weight requiring grad."""
    c, _, o64 = refs("straddle")
    cam = c.cam.to(DEV).requires_grad_(True)
    raw = ops.nerf_query(dev_state(c), c.cfg, c.pts, c.viewdirs, cam, c.bb_center, c.bb_scale)
    (dcam,) = torch.autograd.grad((raw * c.cot.to(DEV)).sum(), [cam])
    assert_within("straddle", {"dcam": dcam.cpu().numpy()}, o64, bounds["cases"]["straddle"]["tensors"], "[cam only]")


def test_inputs_that_require_grad_are_refused(refs):
    c, _, _ = refs("one_point")
    with pytest.raises(NotImplementedError):
        ops.nerf_query(dev_state(c), c.cfg, c.pts.clone().requires_grad_(True), c.viewdirs, c.cam)
    with pytest.raises(NotImplementedError):
        ops.nerf_query(dev_state(c), c.cfg, c.pts, c.viewdirs.clone().requires_grad_(True), c.cam)


def test_eight_adam_steps(refs, bounds):
    """Eight Adam steps through NeRF.query, the objective composed in torch on the device: every loss within 8 x the float32 host
    run's deviation from the float64 host run, and the last loss below the first."""
    c, _, _ = refs(Q.TRAIN_CASE)
    tr = bounds["train"]
    model = NeRF(c.cfg).to(DEV)
    model.load_state_dict(c.state)
    z, target = Q.train_inputs(c)
    pts, viewdirs, cam = c.pts.to(DEV), c.viewdirs.to(DEV), c.cam.to(DEV)
    losses = Q.train_loop(model.parameters(), lambda: model.query(pts, viewdirs, cam, c.bb_center, c.bb_scale), z.to(DEV), viewdirs,
                          target.to(DEV))
    dev = [abs(a - b) for a, b in zip(losses, tr["losses_fp64"])]
    for i, (l, d) in enumerate(zip(losses, dev)):
        print(f"step {i}: loss {l:.9g}, deviation from the float64 host run {d:.3g}, bound {tr['bound']:.3g}, ratio {d / tr['bound']:.3g}")
    assert losses[-1] < losses[0]
    assert max(dev) <= tr["bound"], (dev, tr["bound"])
