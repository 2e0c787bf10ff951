"""Host tests of the differentiable NeRF query: the checker against the golden file recorded from the reference, the
flip-free condition on the test points, the bounds file, the sharpness of the bounds, the NeRF module's state dict.  No GPU."""
import numpy as np
import pytest
import torch

import nerf_extract_ref as R
import nerf_query_ref as Q
from nerf_query_ref import bounds, golden_npz, refs  # noqa: F401

from nerf_rpn_amd import NeRF, lib, ops


@pytest.mark.parametrize("name", Q.NAMES)
def test_checker_matches_golden(name, refs, golden_npz, bounds):
    """The float64 checker reproduces the reference's float64 run within 1e-12 of each tensor's largest magnitude (for the recorded sum
    and absolute sum: of the absolute sum, which is what their own rounding scales with); the float32 checker reproduces the
    reference's float32 run bit for bit where the generator found that it does."""
    c, o32, o64 = refs(name)
    index = Q.NAMES.index(name)
    for k in Q.tensor_names(c.cfg):
        want = golden_npz[f"{name}/{k}"]
        top = float(np.abs(o64[k]).max())
        if k == "raw":
            assert np.abs(o64[k] - want).max() <= 1e-12 * top, k
        else:
            have = Q.summary(k, index, torch.tensor(o64[k]))
            assert np.abs(have[2:] - want[2:]).max() <= 1e-12 * top, k
            assert np.abs(have[:2] - want[:2]).max() <= 1e-12 * max(top, want[1]), k
        if bounds["f32_bit_equal"]:
            want32 = golden_npz[f"{name}/f32/{k}"]
            have32 = o32[k] if k == "raw" else Q.summary(k, index, torch.tensor(o32[k]))
            assert np.array_equal(have32, want32), k


@pytest.mark.parametrize("name", Q.NAMES)
def test_rejection_cap(name, refs, bounds):
    """At most 10 % of the candidates have a pre-activation within tau of zero; tau is the recorded 8 x pool error."""
    c, _, _ = refs(name)
    b = bounds["cases"][name]
    assert b["tau"] == bounds["factor"] * b["pre_error"] and 0 < b["tau"] < 2e-5
    assert (c.info["candidates"], c.info["rejected"]) == (b["candidates"], b["rejected"])
    assert c.info["rejected"] <= 0.10 * c.info["candidates"]
    o = Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, dtype=torch.float64)
    assert o["pre"].shape == (c.pts.shape[0] * c.pts.shape[1], 2176) and float(o["pre"].abs().min()) >= b["tau"]


def test_bounds_file_complete(bounds):
    assert bounds["factor"] == 8.0 and sorted(bounds["cases"]) == sorted(Q.NAMES)
    for case in Q.CASES:
        t = bounds["cases"][case["name"]]["tensors"]
        assert sorted(t) == sorted(Q.tensor_names(Q.case_cfg(case)))
        for k, v in t.items():
            assert v["bound"] == 8.0 * v["fp32_error"] >= 0, (case["name"], k)      # 0: a one-term sum, exact in every dtype
    tr = bounds["train"]
    assert tr["case"] == Q.TRAIN_CASE and len(tr["deviation"]) == Q.TRAIN_STEPS + 1 and tr["bound"] == 8.0 * max(tr["deviation"]) > 0
    assert tr["losses_fp64"][-1] < tr["losses_fp64"][0]


def test_manual_backward_is_autograd(refs):
    """The layer-by-layer formulas (what the kernels implement) give torch autograd's gradients in float64."""
    c, _, o64 = refs("straddle")
    g = Q.manual_grads(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot)
    for k in Q.tensor_names(c.cfg)[1:]:
        assert np.abs(g[k].numpy() - o64[k]).max() <= 1e-12 * np.abs(o64[k]).max(), k


@pytest.mark.parametrize("mutation", Q.MUTATIONS)
def test_sharpness(mutation, refs, bounds):
    """Every mutation of the backward exceeds the committed bound of some tensor by more than 10 x on straddle."""
    c, _, o64 = refs("straddle")
    g = Q.manual_grads(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot, mutation=mutation)
    b = bounds["cases"]["straddle"]["tensors"]
    ratio = max(float(np.abs(g[k].numpy() - o64[k]).max()) / b[k]["bound"] for k in Q.tensor_names(c.cfg)[1:])
    print(f"{mutation}: {ratio:.3g} x the bound")
    assert ratio > 10.0


@pytest.mark.parametrize("cfg", [{}, dict(multires_views=4, input_ch_cam=0)])
def test_module_state_dict(cfg):
    """NeRF().state_dict() has the keys and shapes of a checkpoint's network_fn_state_dict, loads one, and has torch's Linear init."""
    full = dict(R.DEFAULT_CFG, **cfg)
    want = R.make_state(3, "a", full)
    model = NeRF(full)
    have = model.state_dict()
    assert list(have) and sorted(have) == sorted(want) and len(have) == 24
    assert all(tuple(have[k].shape) == tuple(want[k].shape) and have[k].dtype == torch.float32 for k in want)
    model.load_state_dict(want)
    assert all(torch.equal(model.state_dict()[k], want[k]) for k in want)
    assert sorted(k for k, _ in model.named_parameters()) == sorted(ops.NERF_QUERY_PARAMS)
    torch.manual_seed(5)
    a = NeRF(full).state_dict()
    torch.manual_seed(5)
    b = R.NeRF(D=8, W=256, input_ch=57, input_ch_views=3 + 6 * full["multires_views"], input_ch_cam=full["input_ch_cam"], use_viewdirs=True)
    assert all(torch.equal(a[k], v) for k, v in b.state_dict().items())       # the checker model is made of default nn.Linear
    with pytest.raises(NotImplementedError):
        NeRF(dict(full, netwidth=128))


def test_query_needs_a_device_or_rejects_grad_inputs():
    state = R.make_state(3, "a", R.DEFAULT_CFG)
    pts, dirs = torch.zeros(1, 1, 3), torch.zeros(1, 3)
    if not torch.cuda.is_available():
        with pytest.raises(lib.NrpnError):
            ops.nerf_query(state, R.DEFAULT_CFG, pts, dirs)
        with pytest.raises(lib.NrpnError):
            NeRF(R.DEFAULT_CFG).query(pts, dirs)
    with pytest.raises(NotImplementedError):
        ops.nerf_query(state, dict(R.DEFAULT_CFG, netdepth=4), pts, dirs)
