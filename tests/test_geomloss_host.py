"""CPU tests of the fp64 reference that the rotated-IoU loss kernel is judged by (tests/geomloss_ref.py): its gradient against finite
differences, its loss against the oracle's fp32 chain and the reference-captured pairs, and the share of pairs that its stability
probe may exclude from (or must put on) a decision of the piecewise formulation.  No kernel runs here."""
import numpy as np
import pytest
import torch

import geomloss_ref as R


def oracle_loss32(mode, b1, b2):
    from oracle import geometry as OG
    b1, b2 = b1.unsqueeze(0), b2.unsqueeze(0)
    if mode in ("iou", "linear_iou"):
        iou, _, _, _, u = OG.iou_3d(b1, b2, verbose=True)
        r = (iou * u + 1.0) / (u + 1.0)
        return (-torch.log(r) if mode == "iou" else 1 - r)[0]
    return (OG.giou_3d(b1, b2)[0] if mode == "giou" else OG.diou_3d(b1, b2)[0])[0]


@pytest.mark.parametrize("mode", R.MODES)
def test_fp64_autograd_matches_central_differences(mode):
    """eps 1e-6 on fp64 boxes: truncation ~eps^2 |f'''|, rounding ~1e-16 / eps = 1e-10; a decision within eps of a pair would show as
    a large difference and fail -- `generic` has none at this seed."""
    b1, b2 = R.gen("generic")
    _, g, _ = R.loss_grad64(mode, b1, b2)
    eps = 1e-6
    fd = torch.zeros_like(g)
    for k in range(7):
        e = torch.zeros(7, dtype=torch.float64)
        e[k] = eps
        fd[:, k] = (R.loss64(mode, b1.double() + e, b2)[0] - R.loss64(mode, b1.double() - e, b2)[0]) / (2 * eps)
    err = (g - fd).abs()
    print(mode, "max |autograd - fd|", float(err.max()), "max |g|", float(g.abs().max()))
    assert (err <= 1e-3 + 1e-2 * g.abs()).all(), float(err.max())


@pytest.mark.parametrize("mode", R.MODES)
def test_fp64_loss_matches_fp32_oracle(mode, golden):
    g = golden("geometry")
    sets = [R.gen("generic"), (torch.from_numpy(g["b1"])[0, 9:209], torch.from_numpy(g["b2"])[0, 9:209])]
    for b1, b2 in sets:
        l64 = R.loss64(mode, b1, b2)[0]
        l32 = oracle_loss32(mode, b1, b2)
        err = (l64 - l32.double()).abs().max()
        print(mode, "max |l64 - l32|", float(err))
        assert err <= 5e-5, float(err)
    if mode in ("giou", "diou"):                                  # and what the reference itself produced
        l64 = R.loss64(mode, torch.from_numpy(g["b1"])[0, 9:209], torch.from_numpy(g["b2"])[0, 9:209])[0]
        assert (l64 - torch.from_numpy(g[mode + "_loss"])[0, 9:209].double()).abs().max() <= 5e-5


@pytest.mark.parametrize("kind,mode", R.STABLE_CASES)
def test_stable_classes_flag_at_most_5_percent(kind, mode):
    """The cap on what the GPU test may exclude.  A condition on the class and seed, not on the kernel."""
    flagged = R.case(kind, mode)[2]["flagged"]
    print(kind, mode, "flagged", int(flagged.sum()), "of", flagged.numel())
    assert flagged.sum() <= 0.05 * flagged.numel(), int(flagged.sum())


@pytest.mark.parametrize("kind,mode", R.TIE_CASES)
def test_tie_classes_flag_at_least_25_percent(kind, mode):
    """A tie class that the probe does not flag is not on the decision it claims to test."""
    flagged = R.case(kind, mode)[2]["flagged"]
    print(kind, mode, "flagged", int(flagged.sum()), "of", flagged.numel())
    assert flagged.sum() >= 0.25 * flagged.numel(), int(flagged.sum())


def test_stability_is_seeded_and_leaves_its_inputs_alone():
    b1, b2 = R.gen("equal_yaw", 32)
    keep = b1.clone()
    a, b = R.stability("giou", b1, b2), R.stability("giou", b1, b2)
    assert torch.equal(b1, keep) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(R.gen("equal_yaw", 32)[0], b1) and np.isfinite(a["g64"].numpy()).all()
    assert a["dev"].shape == (32, 7) and a["gmax"].shape == (32,) and a["ldev"].shape == (32,)
