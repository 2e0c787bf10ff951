"""GPU tests of the bf16x3 backward of the NeRF query (backward_dtype="bf16x3"): ops.nerf_query, the NeRF module and
nerf_train.

The yardstick is the float64 checker on the same float32 parameters and inputs; the allowance is the host emulation's
(tests/nerf_split_backward_ref.py), computed at run time and never taken from the kernel: per case and per tensor
max|gpu - float64| <= 8 x max|emulation - float64|, floored at one float32 ulp.  The checkers' results are computed once per case and
shared, and so are the GPU runs.  Every test here needs ``backward_dtype=``, which the tree without the mode lacks."""
import contextlib
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import nerf_extract_ref as R
import nerf_query_ref as Q
import nerf_split_backward_ref as B
import nerf_split_ref as S
import nerf_train_ref as T
from nerf_split_backward_ref import brefs  # noqa: F401  (fixture)

from nerf_rpn_amd import NeRF, nerf_train, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODE = "bf16x3"


def run(c, chunk=None, backward_dtype=MODE):
    """ops.nerf_query on case inputs in dtype bf16x3 -> dict of numpy: raw, the 24 gradients of sum(raw * cot) and dcam."""
    params = {k: v.to(DEV).requires_grad_(True) for k, v in c.state.items()}
    cam = None if c.cam is None else c.cam.to(DEV).requires_grad_(True)
    raw = ops.nerf_query(params, c.cfg, c.pts, c.viewdirs, cam, c.bb_center, c.bb_scale, chunk=chunk, dtype=MODE, backward_dtype=backward_dtype)
    wrt = [params[k] for k in Q.PARAMS] + ([] if cam is None else [cam])
    g = torch.autograd.grad((raw * c.cot.to(DEV)).sum(), wrt)
    out = {"raw": raw.detach().cpu().numpy()}
    out.update({k: v.cpu().numpy() for k, v in zip(Q.PARAMS, g)})
    assert all(out[k].shape == tuple(params[k].shape) and out[k].dtype == np.float32 for k in Q.PARAMS)
    if cam is not None:
        out["dcam"] = g[-1].cpu().numpy()
    return out


@pytest.fixture(scope="module")
def gpu(brefs):
    """(case name, chunk, switch) -> the run, made once."""
    cache = {}

    def get(name, chunk=None, backward_dtype=MODE):
        key = (name, chunk, backward_dtype)
        if key not in cache:
            cache[key] = run(brefs(name).c, chunk, backward_dtype)
        return cache[key]
    return get


def assert_all_within(tag, got, r):
    assert sorted(got) == sorted(Q.tensor_names(r.c.cfg))
    bad = []
    for k in Q.tensor_names(r.c.cfg):
        assert np.isfinite(got[k]).all(), k
        try:
            S.assert_within(f"{tag}/{k}", got[k], r.split[k], r.f64[k])
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_every_gradient_within_bound(name, brefs, gpu):
    r = brefs(name)
    assert r.c.nudge["holds"] and S.margins_hold(r.c)       # on the float64 reference, before the GPU is touched
    assert_all_within(name, gpu(name), r)


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_switch_leaves_raw_and_the_head_and_changes_the_trunk(name, brefs, gpu):
    on, off = gpu(name), gpu(name, backward_dtype="fp32")
    assert np.array_equal(on["raw"], off["raw"])
    for k in B.untouched_names(brefs(name).c.cfg):
        assert np.array_equal(on[k], off[k]), k
    assert not np.array_equal(on["pts_linears.0.weight"], off["pts_linears.0.weight"])


def test_switch_off_is_the_call_without_it(brefs, gpu):
    c = brefs("p65").c
    params = {k: v.to(DEV).requires_grad_(True) for k, v in c.state.items()}
    raw = ops.nerf_query(params, c.cfg, c.pts, c.viewdirs, None, c.bb_center, c.bb_scale, dtype=MODE)
    g = torch.autograd.grad((raw * c.cot.to(DEV)).sum(), [params[k] for k in Q.PARAMS])
    off = gpu("p65", backward_dtype="fp32")
    assert np.array_equal(off["raw"], raw.detach().cpu().numpy())
    for k, v in zip(Q.PARAMS, g):
        assert np.array_equal(off[k], v.cpu().numpy()), k


@pytest.mark.parametrize("name", ["p130", "p65x65"])
def test_two_calls_are_bit_equal(name, brefs, gpu):
    a, b = gpu(name), run(brefs(name).c)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("chunk", [128, 64])
def test_chunks_leave_raw_and_stay_within_bound(chunk, brefs, gpu):
    got = gpu("p130", chunk)
    assert np.array_equal(got["raw"], gpu("p130")["raw"])
    assert_all_within(f"p130/chunk{chunk}", got, brefs("p130"))


def test_chunk_loop_over_slices_of_two_tiles(brefs, gpu):
    """4225 points in chunks of 2048: two chunks of 32 tiles and one of 3, added in float64."""
    got = gpu("p65x65", 2048)
    assert np.array_equal(got["raw"], gpu("p65x65")["raw"])
    assert_all_within("p65x65/chunk2048", got, brefs("p65x65"))
    again = run(brefs("p65x65").c, 2048)
    assert all(np.array_equal(got[k], again[k]) for k in got)


def test_module_carries_the_switch(brefs, gpu):
    c = brefs("p130").c
    want = gpu("p130")
    model = NeRF(c.cfg, dtype=MODE, backward_dtype=MODE).to(DEV)
    model.load_state_dict(c.state)
    cam = c.cam.to(DEV).requires_grad_(True)
    raw = model.query(c.pts, c.viewdirs, cam, c.bb_center, c.bb_scale)
    (raw * c.cot.to(DEV)).sum().backward()
    assert np.array_equal(raw.detach().cpu().numpy(), want["raw"])
    for k, p in model.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy(), want[k]), k
    assert np.array_equal(cam.grad.cpu().numpy(), want["dcam"])


def test_switch_needs_the_forward_mode(brefs):
    c = brefs("p1").c
    params = {k: v.to(DEV) for k, v in c.state.items()}
    for dtype, bad in (("fp32", MODE), (MODE, "bf16"), (MODE, "fp16")):
        with pytest.raises(ValueError, match="backward_dtype"):
            ops.nerf_query(params, c.cfg, c.pts, c.viewdirs, c.cam, c.bb_center, c.bb_scale, dtype=dtype, backward_dtype=bad)


# ---- the loop -----------------------------------------------------------------------------------------------------------------------
LOOP_STEPS = 4


@contextlib.contextmanager
def built_models():
    """While active, the models the host loop builds (R.build_model, whatever it is at that time) are collected."""
    saved, built = R.build_model, []

    def build(*a, **kw):
        built.append(saved(*a, **kw))
        return built[-1]
    R.build_model = build
    try:
        yield built
    finally:
        R.build_model = saved


def test_four_loop_steps_parameters_within_bound_of_fp64(tmp_path):
    """Four steps of nerf_train.train with both switches on the 6 x 8, 3-view loop case: args.json records them, every loss and every
    parameter after the four steps within 8 x the emulated host loop's deviation from the float64 host loop."""
    L = T.loop_inputs()
    L.steps = L.steps[:LOOP_STEPS]
    with built_models() as m64:
        ref = T.train_loop_host(L, torch.float64)
    with S.emulated(), B.backward_emulated(), built_models() as memu:
        emu = T.train_loop_host(L, torch.float32)
    p64, pemu = m64[-1].state_dict(), memu[-1].state_dict()
    args = Namespace(expname="loop", ckpt_dir=str(tmp_path), no_reload=True, N_rand=T.LOOP.N_rand, N_samples=T.LOOP.N_samples,
                     lrate=T.LOOP.lrate, start_decay_lrate=400000, end_decay_lrate=500000, depth_loss_weight=T.LOOP.depth_loss_weight,
                     perturb=1., raw_noise_std=T.LOOP.raw_noise_std, lindisp=False, i_print=1, i_weights=100000, N_iters=LOOP_STEPS + 1,
                     dtype=MODE, backward_dtype=MODE, **T.LOOP.cfg)
    with open(os.path.join(nerf_train.write_args(args), "args.json")) as f:
        recorded = json.load(f)
    assert recorded["dtype"] == MODE and recorded["backward_dtype"] == MODE
    run_ns = Namespace(images=L.images, depths=L.depths, valid_depths=L.valid_depths, poses=L.poses, intrinsics=L.intrinsics, near=L.near,
                       far=L.far, bb_center=torch.tensor(T.LOOP.bb_center), bb_scale=torch.tensor(T.LOOP.bb_scale, dtype=torch.float32),
                       state_dict=L.state, embedcam=L.embedcam)
    out = nerf_train.train(run_ns, args, rand=lambda step, name, shape: getattr(L.steps[step - 1], name))
    assert out.model.compute_dtype == MODE and out.model.backward_dtype == MODE and out.step == LOOP_STEPS
    losses = [row[1] for row in out.log]
    assert len(losses) == len(ref) == LOOP_STEPS and np.isfinite(losses).all()
    bad = []
    for i, (g, r, e) in enumerate(zip(losses, ref, emu)):
        b = max(T.FACTOR * abs(e - r), float(np.spacing(np.float32(abs(r)))))
        print(f"step {i + 1}: loss {g:.9g}, float64 {r:.9g}, emulation {e:.9g}, error {abs(g - r):.3g} (bound {b:.3g}), ratio {abs(g - r) / b:.3g}")
        if not abs(g - r) <= b:
            bad.append((i + 1, g, r, b))
    got = {k: v.detach().cpu() for k, v in out.model.state_dict().items()}
    assert sorted(got) == sorted(p64)
    for k in sorted(got):
        try:
            S.assert_within(f"loop/{k}", got[k], pemu[k], p64[k])
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad
