"""GPU tests of the differentiable ray stage (ops.nerf_composite, ops.nerf_ray_losses, render_rays_train, training_loss; DESIGN.md
3.21) against the float64 checker, with the per-tensor bounds of tests/golden/nerf_composite_bounds.json (8 x the float32 checker's
own error, floored at a float32 ulp; zero where the tensor is exactly zero)."""
import json
import os

import numpy as np
import pytest
import torch

import nerf_composite_ref as C
import nerf_query_ref as Q
import nerf_render_ref as V
from nerf_composite_ref import bounds, refs  # noqa: F401

from nerf_rpn_amd import NeRF, lib, ops, render_rays_train, training_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORDER = ("rgb_map", "disp_map", "acc_map", "weights", "depth_map", "z_vals")      # of ops.nerf_composite's tuple


def dev(x):
    return None if x is None else x.to(DEV)


def run(c):
    """The ops on case inputs -> dict of numpy over C.tensor_names: the six outputs, draw1 / draw2 for the seeded cotangent of every
    differentiable output, both losses and their gradients down to raw1 / raw2."""
    raw1 = dev(c.raw1).requires_grad_(True)
    raw2 = None if c.raw2 is None else dev(c.raw2).requires_grad_(True)
    wrt = [raw1] + ([] if raw2 is None else [raw2])
    names = ["draw1"] + ([] if raw2 is None else ["draw2"])
    outs = ops.nerf_composite(raw1, dev(c.z1), dev(c.rays_d), raw2, dev(c.z2), dev(c.noise))
    out = dict(zip(ORDER, outs))
    nr, s = c.raw1.shape[0], c.g_w.shape[1]
    assert all(v.dtype == torch.float32 and v.is_cuda for v in outs)
    assert [tuple(out[k].shape) for k in ORDER] == [(nr, 3), (nr,), (nr,), (nr, s), (nr,), (nr, s)]
    assert not out["disp_map"].requires_grad and not out["z_vals"].requires_grad
    res = {k: v.detach().cpu().numpy() for k, v in out.items()}
    cot = (out["rgb_map"] * dev(c.g_rgb)).sum() + (out["depth_map"] * dev(c.g_depth)).sum() + (out["acc_map"] * dev(c.g_acc)).sum() \
        + (out["weights"] * dev(c.g_w)).sum()
    res.update(zip(names, (g.cpu().numpy() for g in torch.autograd.grad(cot, wrt, retain_graph=True))))
    img, dep = ops.nerf_ray_losses(out["rgb_map"], dev(c.target_s), out["depth_map"], out["z_vals"], out["weights"], dev(c.target_d),
                                   dev(c.target_vd))
    assert img.shape == dep.shape == () and img.dtype == dep.dtype == torch.float32
    res.update(img_loss=img.detach().cpu().numpy(), depth_loss=dep.detach().cpu().numpy())
    for tag, loss in (("img_", img), ("depth_", dep)):
        res.update(zip([tag + n for n in names], (g.cpu().numpy() for g in torch.autograd.grad(loss, wrt, retain_graph=True))))
    return res


@pytest.fixture(scope="module")
def runs(refs):
    """case name -> two runs of it."""
    cache = {}

    def get(name):
        if name not in cache:
            c, _, _ = refs(name)
            cache[name] = (run(c), run(c))
        return cache[name]
    return get


@pytest.mark.parametrize("name", C.NAMES)
def test_within_bounds(name, refs, runs, bounds):
    c, _, o64 = refs(name)
    got = runs(name)[0]
    assert sorted(got) == sorted(C.tensor_names(c.case))
    b, worst = bounds["cases"][name]["tensors"], []
    for k in got:
        err = C.max_error(got[k], o64[k])
        ratio = err / b[k]["bound"] if b[k]["bound"] else (0.0 if err == 0 else float("inf"))
        print(f"{name}/{k}: error {err:.3g}, bound {b[k]['bound']:.3g}, ratio {ratio:.3g}")
        if not err <= b[k]["bound"]:
            worst.append((k, err, b[k]["bound"]))
    assert not worst, worst


@pytest.mark.parametrize("name", C.NAMES)
def test_two_calls_are_bit_equal(name, runs):
    a, b = runs(name)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


@pytest.mark.parametrize("name", ["shared_3x4", "uneven_7x18"])
def test_no_valid_or_no_applied_ray_gives_exact_zeros(name, runs):
    got = runs(name)[0]
    assert got["depth_loss"] == 0
    assert not any(np.any(got[k]) for k in got if k.startswith("depth_draw"))


def test_empty_ray(runs):
    """A ray whose sigma is all <= 0: acc 0, disparity NaN as nerf_render keeps it, zero gradients."""
    got = runs("two_lists_5x12")[0]
    assert got["acc_map"][3] == 0 and np.isnan(got["disp_map"][3]) and not np.any(got["weights"][3])
    assert not any(np.any(got[k][3]) for k in got if "draw" in k)


def test_bit_equal_to_render():
    """With noise=None, the shared z1 and the raw of plain_4x6, the outputs are nerf_render's bit for bit.  nerf_render exposes the
    first pass's raw only, so no two-pass case can be composited from its stages: the one-pass case stands alone."""
    c = V.case_inputs(V.CASES[V.NAMES.index("plain_4x6")])
    ref = V.render_case(c, torch.float32)
    rays = torch.cat([ref["rays_o"], ref["rays_d"]], -1).contiguous()
    out = ops.nerf_render(c.state, c.cfg, rays=rays, near=c.near, far=c.far, bb_center=c.bb_center, bb_scale=c.bb_scale,
                          n_samples=c.n_samples, return_samples=True, return_stages=True)
    z1 = out["z_vals"][0].contiguous()
    assert torch.equal(out["z_vals"], z1.expand_as(out["z_vals"]))
    got = dict(zip(ORDER, ops.nerf_composite(out["raw1"], z1, rays[:, 3:].contiguous())))
    for k in ORDER:
        assert np.array_equal(got[k].cpu().numpy(), out[k].cpu().numpy(), equal_nan=True), k
    per_ray = dict(zip(ORDER, ops.nerf_composite(out["raw1"], out["z_vals"], rays[:, 3:].contiguous())))      # z1 given per ray
    for k in ORDER:
        assert np.array_equal(per_ray[k].cpu().numpy(), out[k].cpu().numpy(), equal_nan=True), k


def test_arguments_are_checked(refs):
    c, _, _ = refs("two_lists_5x12")
    z2 = c.z2.flip(-1)
    with pytest.raises(lib.NrpnError, match="non-decreasing"):
        ops.nerf_composite(dev(c.raw1), dev(c.z1), dev(c.rays_d), dev(c.raw2), dev(z2), check=True)
    ops.nerf_composite(dev(c.raw1), dev(c.z1), dev(c.rays_d), dev(c.raw2), dev(c.z2), check=True)
    with pytest.raises(lib.NrpnError):
        ops.nerf_composite(dev(c.raw1), dev(c.z1), dev(c.rays_d), dev(c.raw2))
    with pytest.raises(lib.NrpnError):
        ops.nerf_composite(dev(c.raw1), dev(c.z1)[:, :-1], dev(c.rays_d))
    with pytest.raises(NotImplementedError):
        ops.nerf_composite(dev(c.raw1), dev(c.z1).requires_grad_(True), dev(c.rays_d))
    with pytest.raises(lib.NrpnError):
        ops.nerf_ray_losses(torch.zeros(5, 3, device=DEV), torch.zeros(4, 3, device=DEV))
    with pytest.raises(lib.NrpnError):
        ops.nerf_ray_losses(torch.zeros(5, 3, device=DEV), torch.zeros(5, 3, device=DEV), target_d=torch.zeros(5, 2))


def test_img_loss_alone(refs, runs, bounds):
    c, _, o64 = refs("uneven_7x18")
    got = runs("uneven_7x18")[0]
    rgb = torch.tensor(got["rgb_map"], device=DEV).requires_grad_(True)
    img, dep = ops.nerf_ray_losses(rgb, dev(c.target_s))
    assert np.array_equal(img.detach().cpu().numpy(), got["img_loss"]) and dep.item() == 0
    (g,) = torch.autograd.grad(img, [rgb])
    want = 2 * (got["rgb_map"].astype(np.float64) - c.target_s.numpy()) / rgb.numel()
    assert np.abs(g.cpu().numpy() - want).max() <= np.spacing(np.float32(np.abs(want).max()))


def test_eight_adam_steps(bounds):
    """Eight Adam steps through render_rays_train + training_loss: every loss within 8 x the float32 host loop's deviation from the
    float64 host loop, and the last loss below the first."""
    with open(os.path.join(Q.GOLDEN, "nerf_query_bounds.json")) as f:
        c = Q.case_inputs(Q.CASES[Q.NAMES.index(Q.TRAIN_CASE)], json.load(f)["cases"][Q.TRAIN_CASE]["tau"])
    tr = bounds["train"]
    t = C.train_inputs(c)
    model = NeRF(c.cfg).to(DEV)
    model.load_state_dict(c.state)
    viewdirs, cam = dev(t.rays_d), dev(c.cam)

    def loss_fn():
        out = render_rays_train(model, dev(t.rays_o), dev(t.rays_d), viewdirs, dev(t.z1), dev(t.z2), cam, C.TRAIN_BB_CENTER, C.TRAIN_BB_SCALE)
        assert sorted(out) == sorted(ORDER)
        return training_loss(out, dev(t.target_s), dev(t.target_d), dev(t.target_vd), tr["depth_loss_weight"])[0]
    losses = C.train_loop(model.parameters(), loss_fn)
    deviation = [abs(a - b) for a, b in zip(losses, tr["losses_fp64"])]
    for i, (l, d) in enumerate(zip(losses, deviation)):
        print(f"step {i}: loss {l:.9g}, deviation from the float64 host run {d:.3g}, bound {tr['bound']:.3g}, ratio {d / tr['bound']:.3g}")
    assert losses[-1] < losses[0]
    assert max(deviation) <= tr["bound"], (deviation, tr["bound"])
