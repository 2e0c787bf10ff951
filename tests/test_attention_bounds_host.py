"""Host side of tests/test_gpu_attention.py (no GPU): the float64 attention-core reference of tests/attention_ref.py is anchored to
oracle.nets.window_attention (pinned to the reference implementation by the goldens), and its per-element bounds are shown to be both
satisfiable and sharp on the CPU: torch's fp32 evaluation stays inside the fp32 term T32, an emulation of the bf16 MFMA kernels' rounding
points stays inside the bf16 bounds, and the same emulation with a transposed relative-position bias lands far outside them.

Measured here (max |err| / bound over every element, the larger of the two geometries of BOUND_GEOMS; seed 11):
    family      torch fp32 vs T32 (out / dqkv / dtable / dbias_pad)      MFMA emulation vs bf16 bounds      transposed bias (out)
    normal      0.10 / 0.09 / 0.03 / 0.002                               0.74 / 0.77 / 0.02 / 0.02          260 - 430
    peaked      0.43 / 0.49 / 0.29 / 0.02   (Lambda up to 137)           0.88 / 0.97 / 0.25 / 0.20          1800 - 2000
    offset_v    0.10 / 0.93 / 0.01 / 0.002  (dq: dP - rowdot cancels)    0.62 / 0.77 / 0.01 / 0.01          4.8
    selector    0.14 / 0.11 / 0.02 / 0.002                               0.90 / 0.92 / 0.03 / 0.05          > 1e6"""
import pytest
import torch
import torch.nn.functional as F

import attention_ref as AR


def _oracle_case(shape, heads, shift, seed):
    from oracle import nets as ON
    g = torch.Generator().manual_seed(seed)
    c = AR.HD * heads
    rnd = lambda *s, k=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * k).requires_grad_()      # noqa: E731
    x, dy = rnd(*shape, c), torch.randn(*shape, c, generator=g, dtype=torch.float64)
    wq, bq, wp, bp = rnd(3 * c, c, k=c ** -0.5), rnd(3 * c, k=0.5), rnd(c, c, k=c ** -0.5), rnd(c, k=0.5)
    table = rnd(343, heads, k=0.5)
    index = ON.WindowAttention(c, heads, shift).relative_position_index
    return ON, x, dy, wq, bq, wp, bp, table, index


# padded + shifted, padded + partly shifted (an axis one window long), unpadded partly shifted, unpadded shifted / unshifted, axes shorter
# than a window, padded unshifted
ORACLE_CASES = [((1, 10, 7, 6), 6, 2), ((2, 5, 4, 3), 3, 2), ((1, 8, 4, 4), 3, 2), ((2, 8, 8, 8), 3, 2), ((2, 8, 8, 8), 3, 0),
                ((1, 3, 2, 2), 3, 2), ((1, 9, 8, 5), 3, 0), ((1, 1, 1, 1), 3, 2)]


@pytest.mark.parametrize("shape,heads,shift", ORACLE_CASES)
def test_reference_equals_oracle(shape, heads, shift):
    """proj(attn_core_ref(linear(x))) == oracle.nets.window_attention to 1e-12, and so do the gradients: the oracle's qkv-bias gradient is
    the sum of dqkv over the real tokens plus the reference's dbias_pad (whose q third is exactly zero)."""
    ON, x, dy, wq, bq, wp, bp, table, index = _oracle_case(shape, heads, shift, 7)
    yo = ON.window_attention(x, wq, bq, wp, bp, table, index, heads, shift)
    gx, gwq, gbq, gt = torch.autograd.grad(yo, (x, wq, bq, table), dy)
    with torch.no_grad():
        qkv = F.linear(x, wq, bq)
        dctx = dy @ wp                                   # gradient reaching the core through the proj Linear
    r = AR.attn_core_ref(qkv, bq.detach(), table.detach(), index, heads, shift, dout=dctx)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12 * (1.0 + b.abs().max().item()))      # noqa: E731
    c = AR.HD * heads
    assert close(F.linear(r.out, wp.detach(), bp.detach()), yo.detach())
    assert close(r.dqkv @ wq.detach(), gx)
    assert close(r.dtable, gt)
    assert torch.equal(r.dbias_pad[:c], torch.zeros(c, dtype=torch.float64))
    assert close(r.dqkv.reshape(-1, 3 * c).sum(0) + r.dbias_pad, gbq)
    if not any(r.frame.pad):
        assert torch.equal(r.dbias_pad, torch.zeros_like(r.dbias_pad))
    # the written-out backward (the form the fp32 evaluation and the MFMA emulation use) is the same function
    out, dqkv, dtable, dpad = AR.attn_core_explicit(qkv, bq.detach(), table.detach(), index, heads, shift, dctx)
    assert close(out, r.out) and close(dqkv, r.dqkv) and close(dtable, r.dtable) and close(dpad, r.dbias_pad)
    # the magnitudes are made of the same dS as the gradients: scattered onto the table entries it is the table gradient
    assert close(AR._scatter_table(index, r.ds), r.dtable) and close(r.s.grad, r.ds)
    assert (r.terms["dtable"] >= r.dtable.abs() * (1 - 1e-12)).all()


def test_reference_without_bias_pads_with_zeros():
    ON, x, dy, wq, bq, wp, bp, table, index = _oracle_case((1, 6, 5, 3), 3, 2, 9)
    with torch.no_grad():
        yo = ON.window_attention(x, wq, None, wp, bp, table, index, 3, 2)
        r = AR.attn_core_ref(F.linear(x, wq), None, table.detach(), index, 3, 2, dout=dy @ wp)
        assert r.dbias_pad is None
        assert torch.allclose(F.linear(r.out, wp, bp), yo, rtol=1e-12, atol=1e-12)


BOUND_GEOMS = [((3, 13, 10, 9), 3, 2), ((2, 8, 8, 8), 6, 0)]      # padded + shifted (108 windows), unpadded (16 windows)


@pytest.mark.parametrize("shape,heads,shift", BOUND_GEOMS)
@pytest.mark.parametrize("family", AR.FAMILIES[:4])
def test_bounds_hold_for_emulation_and_catch_transposed_bias(family, shape, heads, shift):
    index = AR.relative_position_index()
    # torch fp32 on fp32 inputs against T32
    qkv, bias, table, dout = AR.make_case(family, shape, heads, 11)
    ref = AR.attn_core_ref(qkv.double(), bias.double(), table.double(), index, heads, shift, dout=dout.double())
    r32 = AR.torch32_ratios(ref, AR.attn_core_explicit(qkv, bias, table, index, heads, shift, dout))
    print(family, shape, "torch fp32 / T32:", {k: round(v, 3) for k, v in r32.items()}, "Lambda max", round(ref.lam_max, 1))
    assert all(v <= 1.0 for v in r32.values()), r32
    # the MFMA kernels' rounding points on bf16 inputs against the bf16 bounds, k measured on torch fp32 for the same inputs
    qkv, bias, table, dout = AR.make_case(family, shape, heads, 11, bf16=True)
    ref = AR.attn_core_ref(qkv.double(), bias.double(), table.double(), index, heads, shift, dout=dout.double())
    r32 = AR.torch32_ratios(ref, AR.attn_core_explicit(qkv, bias, table, index, heads, shift, dout))
    assert all(v <= 1.0 for v in r32.values()), r32
    emu = AR.attn_core_explicit(qkv, bias, table, index, heads, shift, dout, mfma_rounding=True)
    for name, got in zip(AR.NAMES, emu):
        AR.check(ref, name, "bf16_mfma", got, AR.allowance(r32[name]), f"{family} {shape} emulation")
    # transposed relative-position bias: out, dqkv and dtable all leave their bounds
    bug = AR.attn_core_explicit(qkv, bias, table, index, heads, shift, dout, mfma_rounding=True, transpose_bias=True)
    for name, got in zip(AR.NAMES[:3], bug):
        worst = AR.ratio_map(ref, name, "bf16_mfma", got, 2.0).max().item()
        print(family, shape, "transposed bias", name, "err/bound =", round(worst, 1))
        assert worst > 1.5, (name, worst)
        with pytest.raises(AssertionError):
            AR.check(ref, name, "bf16_mfma", got, 2.0)


@pytest.mark.parametrize("shape,shift", [((2, 8, 8, 8), 0), ((2, 8, 8, 8), 2), ((1, 8, 4, 4), 2), ((2, 5, 4, 3), 2), ((1, 10, 7, 6), 0)])
def test_uniform_family_closed_form(shape, shift):
    """Family 5: q = 0 and a zero table make every softmax row uniform over its window-and-region set, so the first five v channels of
    every head come out as the mean of (x, y, z, 1, b) over that set - computed here by index arithmetic alone."""
    heads = 3
    qkv, _, table, dout = AR.make_case("uniform", shape, heads, 13, with_bias=False)
    ref = AR.attn_core_ref(qkv.double(), None, table.double(), AR.relative_position_index(), heads, shift)
    want = AR.uniform_closed_form(shape, shift)
    for h in range(heads):
        assert torch.allclose(ref.out[..., h * AR.HD:h * AR.HD + 5], want, rtol=0, atol=1e-12)
    if shift == 0 and not any(ref.frame.pad):          # every token carries the mean coordinate of its own window
        x = torch.arange(shape[1], dtype=torch.float64)
        assert torch.equal(want[0, :, 0, 0, 0], (x // 4) * 4 + 1.5)
