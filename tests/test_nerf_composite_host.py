"""Host tests of the differentiable ray stage: the checker against the golden file, the decision margins of the test
rays, the bounds file, the written-out backward, the sharpness of the bounds, the header.  No GPU."""
import numpy as np
import pytest
import torch

import nerf_composite_ref as C
import nerf_query_ref as Q
from nerf_composite_ref import bounds, golden_npz, refs  # noqa: F401

from nerf_rpn_amd import lib

# the case each mutation is judged on; list2_first on two_lists_5x12 with an exact tie put into every ray (C.with_ties)
SHARPNESS_CASE = dict(no_eps="two_lists_5x12", no_suffix="two_lists_5x12", no_relu_mask="two_lists_5x12", finite_last_dist="two_lists_5x12",
                      v_no_eps="two_lists_5x12", clamp_zero_grad="two_lists_5x12", detached_m="two_lists_5x12", no_noise="two_lists_5x12",
                      list2_first="two_lists_5x12")


def ratio_of(err, bound):
    return err / bound if bound else (0.0 if err == 0 else float("inf"))


@pytest.mark.parametrize("name", C.NAMES)
def test_checker_matches_golden(name, refs, golden_npz):
    """The float64 checker reproduces the recorded summaries (taken after the generator compared it with the reference's
    forward_with_additonal_samples, raw2outputs and compute_weights) within 1e-12 of each tensor's largest magnitude; for the sum
    and absolute sum, of the absolute sum."""
    c, _, o64 = refs(name)
    index = C.NAMES.index(name)
    for k in C.tensor_names(c.case):
        want = golden_npz[f"{name}/{k}"]
        have = Q.summary(k, index, torch.tensor(o64[k]))
        top = C.top_of(o64[k])
        assert C.max_error(have[2:], want[2:]) <= 1e-12 * top, k
        assert C.max_error(have[:2], want[:2]) <= 1e-12 * max(top, 0.0 if np.isnan(want[1]) else want[1]), k


@pytest.mark.parametrize("name", C.NAMES)
def test_decision_margins_and_rejection_cap(name, refs, bounds):
    """Every decision of every ray is at least the recorded tau (8 x the pool error) from its boundary in float64, no z is shared by
    the two lists, and at most 10 % of the candidates were rejected."""
    c, _, _ = refs(name)
    b = bounds["cases"][name]
    assert sorted(b["tau"]) == sorted(C.DECISIONS) and all(b["tau"][k] == bounds["factor"] * b["pool_error"][k] for k in C.DECISIONS)
    assert (c.info["candidates"], c.info["rejected"]) == (b["candidates"], b["rejected"])
    assert c.info["rejected"] <= 0.10 * c.info["candidates"]
    q, gap, _ = C.margins(c)
    assert all(float(q[k].abs().min()) >= b["tau"][k] for k in C.DECISIONS) and float(gap.min()) > 0


def test_bounds_file_complete_and_cases_cover(bounds):
    assert bounds["factor"] == C.FACTOR and sorted(bounds["cases"]) == sorted(C.NAMES) and bounds["f32_bit_equal"] is True
    for case in C.CASES:
        t = bounds["cases"][case["name"]]["tensors"]
        assert sorted(t) == sorted(C.tensor_names(case))
        for k, v in t.items():
            floor = float(np.spacing(np.float32(v["top"]))) if v["top"] else 0.0
            assert v["bound"] == (max(C.FACTOR * v["fp32_error"], floor) if v["top"] else 0.0), (case["name"], k)
    cover = {n: bounds["cases"][n]["cover"] for n in C.NAMES}
    assert sum(v["applied_v_below"] for v in cover.values()) >= 1 and sum(v["applied_v_above"] for v in cover.values()) >= 1
    assert cover["shared_3x4"]["valid"] == 0 and cover["uneven_7x18"]["valid"] == 7 and cover["uneven_7x18"]["applied"] == 0
    assert cover["two_lists_5x12"]["valid"] == cover["two_lists_5x12"]["applied"] == 5
    assert any(v["empty_rays"] for v in cover.values()) and any(v["opaque_rays"] for v in cover.values())
    assert all(abs(v["norm_min"] - 1) > 0.01 or abs(v["norm_max"] - 1) > 0.01 for v in cover.values())
    tr = bounds["train"]
    assert tr["case"] == Q.TRAIN_CASE and len(tr["deviation"]) == Q.TRAIN_STEPS + 1 and tr["bound"] == C.FACTOR * max(tr["deviation"]) > 0
    assert tr["losses_fp64"][-1] < tr["losses_fp64"][0] and tr["depth_loss_weight"] == C.DEPTH_LOSS_WEIGHT


@pytest.mark.parametrize("name", C.NAMES)
def test_bounds_are_satisfiable(name, refs, bounds):
    """The float32 checker is inside every bound; an exactly zero tensor is exactly zero there too."""
    _, o32, o64 = refs(name)
    for k, v in bounds["cases"][name]["tensors"].items():
        assert C.max_error(o32[k], o64[k]) <= v["bound"], k


@pytest.mark.parametrize("name", C.NAMES)
def test_manual_backward_is_autograd(name, refs):
    """The per-sample formulas (what the kernels implement) give the checker's outputs and torch autograd's gradients in float64."""
    c, _, o64 = refs(name)
    man = C.manual(c)
    for k in C.tensor_names(c.case):
        assert C.max_error(man[k], o64[k]) <= 1e-12 * C.top_of(o64[k]), k


def test_empty_rays_and_unapplied_losses_are_exact(refs):
    """A ray whose sigma is all <= 0 has acc 0, a NaN disparity and zero gradients; without a valid or an applied ray the depth loss
    and its gradients are exactly zero."""
    c, _, o64 = refs("two_lists_5x12")
    assert o64["acc_map"][3] == 0 and np.isnan(o64["disp_map"][3])
    assert not np.any(o64["draw1"][3]) and not np.any(o64["draw2"][3]) and not np.any(o64["depth_draw1"][3])
    for name in ("shared_3x4", "uneven_7x18"):
        _, o32, o64 = refs(name)
        for o in (o32, o64):
            assert o["depth_loss"] == 0 and not any(np.any(o[k]) for k in o if k.startswith("depth_draw"))


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_sharpness(mutation, refs, bounds):
    """Every mutation of the written-out stage exceeds the committed bound of some tensor by more than 10 x."""
    name = SHARPNESS_CASE[mutation]
    c, _, o64 = refs(name)
    want = o64
    if mutation == "list2_first":
        c = C.with_ties(c)
        want = {k: v.detach().numpy() for k, v in C.manual(c).items()}
        chk = C.check_case(c, torch.float64)      # the stable sort of the checker puts list 1 first, as the written-out stage does
        assert all(C.max_error(chk[k], want[k]) <= 1e-12 * C.top_of(want[k]) for k in C.tensor_names(c.case))
    got = C.manual(c, mutation)
    b = bounds["cases"][name]["tensors"]
    ratios = {k: ratio_of(C.max_error(got[k], want[k]), b[k]["bound"]) for k in C.tensor_names(c.case)}
    worst = max(ratios, key=ratios.get)
    print(f"{mutation}: {ratios[worst]:.3g} x the bound of {worst}")
    assert ratios[worst] > 10.0


def test_header_declares_the_entries():
    want = ["nrpn_nerfcomposite_work_bytes", "nrpn_nerfcomposite_forward", "nrpn_nerfcomposite_backward", "nrpn_nerfraylosses_forward",
            "nrpn_nerfraylosses_backward"]
    declared = lib.declared_symbols(tools=False)
    assert all(k in declared for k in want)
    text = open(lib.HEADER).read()
    assert "[f10]" in text and all(ref in text for ref in ("419-469", "504-512", "837-847"))
