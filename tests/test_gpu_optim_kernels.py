"""GPU: the five kernels of csrc/elementwise.hip that end every training step -- nrpn_adamw_step / nrpn_adamw_step_zero_grad,
nrpn_grad_sumsq, nrpn_transpose_weights, nrpn_reduce_slices, nrpn_cast -- called directly against the float64 references of
tests/optim_ref.py: every element inside its own derived bound (AdamW, the norm), or equal where the kernel only moves, rounds or adds in
a fixed order.  The bounds, their derivation, the cases and what is left out are in optim_ref's docstring; tests/test_optim_bounds_host.py
shows on the CPU that they are satisfiable and sharp.  No tolerance here is a bare constant: each is an equality or a bound of optim_ref
times the allowance k = max(1, min(2, 4 r)) measured on torch's fp32 CPU evaluation of the same case (never on the kernel).  Every check
prints its max |err| / bound (run with -s).

Loops reached: AdamW's scalar tail alone (1, 3), its remainder loop (4, 5, 1023, 10007), its paired loop (8 392 611: pair or one quad per
lane) and pair-then-remainder (16 781 217); every loop of the three read patterns of the norm through nrpn_set_sumsq_form, restored to
(0, 1024) in a finally; the binary search and the ragged tile edges of transpose_weights; the second and third trip of reduce_slices'
grid-stride loop, its bias block and the wrows > cout stride; the second trip of cast.  Every output buffer is followed by a guard that
must keep its sentinel."""
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GUARD = 64


def _guarded(t, dev, dtype=None):
    """``t`` on the device as the head of a buffer whose last GUARD elements hold the sentinel -> (view, guard)."""
    dtype = dtype or t.dtype
    buf = torch.full((t.numel() + GUARD,), R.SENTINEL, dtype=dtype, device=dev)
    buf[:t.numel()] = t.to(dev).to(dtype).reshape(-1)
    return buf[:t.numel()], buf[t.numel():]


def _intact(*guards):
    return all(bool((g == R.SENTINEL).all()) for g in guards)


# ======================================================================================================================
# AdamW
# ======================================================================================================================
def _adamw_run(case, h, dev, zero, shadow):
    """One launch on fresh copies -> namespace of device tensors p, g, m, v, shadow (or None), ok (guards and sentinels intact)."""
    from nerf_rpn_amd import lib, ops
    import types
    (p, gp), (g, gg), (m, gm), (v, gv) = (_guarded(t, dev) for t in case[:4])
    ss = None
    if h.sumsq is not None:
        ss = torch.full((lib.query("grad_sumsq_floats"),), R.SENTINEL, device=dev)
        ss[0] = R.f32(h.sumsq)
    sh, gs = _guarded(torch.full((p.numel(),), R.SENTINEL), dev, BF16) if shadow else (None, None)
    spare = torch.full((p.numel() + GUARD,), R.SENTINEL, dtype=BF16, device=dev)             # a buffer no kernel receives: only a wild write reaches it
    ops.adamw_step(p, g, m, v, ss, h.max_norm, h.lr, (h.b1, h.b2), h.eps, h.wd, h.step, grad_scale=h.grad_scale, shadow=sh, zero_grad=zero)
    torch.cuda.synchronize()
    ok = _intact(gp, gg, gm, gv, spare) and (gs is None or _intact(gs)) and (ss is None or (_intact(ss[1:]) and ss[0].item() == R.f32(h.sumsq)))
    return types.SimpleNamespace(p=p, g=g, m=m, v=v, shadow=sh, ok=ok)


def _adamw_exact(case, runs, what):
    """The equalities of one case: runs = {(zero, shadow): result}."""
    p0, g0, m0, v0, pad = case
    first = next(iter(runs.values()))
    for (zero, shadow), r in runs.items():
        assert r.ok, (what, zero, shadow, "a guard, the buffer no kernel received or the sumsq buffer was written")
        assert torch.equal(R.bits(r.p), R.bits(first.p)) and torch.equal(R.bits(r.m), R.bits(first.m)) and torch.equal(R.bits(r.v), R.bits(first.v)), \
            (what, zero, shadow, "the variants differ")
        if zero:
            assert not R.bits(r.g).any(), (what, "gradient not +0 everywhere after zero_grad")
        else:
            assert torch.equal(R.bits(r.g), R.bits(g0)), (what, "gradient changed without zero_grad")
        if shadow:
            assert torch.equal(R.bits(r.shadow), R.bits(r.p.cpu().to(BF16))), (what, "shadow is not the round-to-nearest-even of p'")
            assert not r.shadow.cpu()[pad].any()
        for t in (r.p, r.m, r.v):
            assert not t.cpu()[pad].any(), (what, "arena padding moved")


def _adamw_bounds(case, h, r, what):
    p0, g0, m0, v0, _ = case
    ref = R.adamw_ref(p0, g0, m0, v0, h)
    e = R.adamw_eval(p0, g0, m0, v0, h, F32)
    out = []
    for name, got, want, tol, t32 in (("p'", r.p, ref.p, ref.p_bound, e.p), ("m'", r.m, ref.m, ref.m_bound, e.m), ("v'", r.v, ref.v, ref.v_bound, e.v)):
        out.append(R.check(got, want, tol, R.allowance(R.ratio(t32, want, tol)), f"adamw {what} {name}"))
    return out


@pytest.mark.parametrize("step", R.STEPS)
def test_adamw_configurations_match_fp64(step, dev):
    """Count 10007, every configuration of optim_ref.ADAMW_CONFIGS at this step: p', m', v' of the plain variant inside their bounds, and
    the zero_grad + shadow variant bit-equal to it."""
    worst = [0.0, 0.0, 0.0]
    for name, h in R.ADAMW_CONFIGS[step]:
        case = R.adamw_case(10007, h)
        runs = {(z, s): _adamw_run(case, h, dev, z, s) for z, s in ((False, False), (True, True))}
        _adamw_exact(case, runs, name)
        worst = [max(a, b) for a, b in zip(worst, _adamw_bounds(case, h, runs[(False, False)], f"step {step} {name}"))]
    print(f"adamw step {step}: worst err / (k bound) p' {worst[0]:.3f} m' {worst[1]:.3f} v' {worst[2]:.3f}")


@pytest.mark.parametrize("count", R.ADAMW_SMALL_COUNTS)
def test_adamw_small_counts_match_fp64(count, dev):
    """Scalar tail alone (1, 3), one quad (4), quad + tail (5), 1023, 10007: all four variants, twice."""
    for h in (R.BASE, R.PRODUCTION._replace(step=1000)):
        case = R.adamw_case(count, h)
        runs = {(z, s): _adamw_run(case, h, dev, z, s) for z in (False, True) for s in (False, True)}
        _adamw_exact(case, runs, f"n{count}")
        again = _adamw_run(case, h, dev, True, True)
        assert all(torch.equal(R.bits(getattr(again, n)), R.bits(getattr(runs[(True, True)], n))) for n in ("p", "m", "v", "shadow")), "run to run"
        _adamw_bounds(case, h, runs[(False, False)], f"n{count} step {h.step}")


def _same_bits(a, b, what):
    """Bit equality of two device tensors; a failure names the first and last differing flat index."""
    it = torch.int32 if a.dtype == F32 else torch.int16
    if not torch.equal(a.view(it), b.view(it)):
        bad = (a.view(it) != b.view(it)).nonzero().reshape(-1)
        raise AssertionError((what, "differ at", int(bad.numel()), "elements, flat indices", int(bad[0]), "...", int(bad[-1]),
                              "trip of the paired loop", int(bad[0]) // (4 * R.ADAMW_S)))


@pytest.mark.parametrize("name,h,zero,shadow", R.BIG_CONFIGS, ids=[c[0] for c in R.BIG_CONFIGS])
@pytest.mark.parametrize("count", [R.ADAMW_PAIRED, R.ADAMW_PAIRED_REMAINDER], ids=["paired", "paired_then_remainder"])
def test_adamw_paired_loop_matches_fp64(count, name, h, zero, shadow, dev):
    """The two-quads-per-trip loop: exact checks over every element on the device, the bound over optim_ref.adamw_sample (windows round every
    loop boundary + every 64th element); a failure names the flat index."""
    case = R.adamw_case(count, h)
    pad = case[4].to(dev)
    run = _adamw_run(case, h, dev, zero, shadow)
    other = _adamw_run(case, h, dev, not zero, False)
    again = _adamw_run(case, h, dev, zero, shadow)
    assert run.ok and other.ok and again.ok, "a guard, the buffer no kernel received or the sumsq buffer was written"
    g0 = case[1].to(dev)
    for n in ("p", "m", "v"):
        _same_bits(getattr(run, n), getattr(other, n), f"{n}' of the two variants")
        _same_bits(getattr(run, n), getattr(again, n), f"{n}' run to run")
        assert not getattr(run, n)[pad].any(), (n, "arena padding moved")
    for r, z in ((run, zero), (other, not zero)):
        _same_bits(r.g, torch.zeros_like(g0) if z else g0, "gradient after zero_grad (+0 everywhere)" if z else "gradient without zero_grad (kept)")
    if shadow:
        _same_bits(run.shadow, run.p.to(BF16), "shadow against the round-to-nearest-even of p'")
        _same_bits(run.shadow, again.shadow, "shadow run to run")
        assert not run.shadow[pad].any()
    idx = R.adamw_sample(count)
    sub = [t[idx] for t in case[:4]]
    ref = R.adamw_ref(*sub, h)
    e = R.adamw_eval(*sub, h, F32)
    di = idx.to(dev)
    for nm, got, want, tol, t32 in (("p'", run.p, ref.p, ref.p_bound, e.p), ("m'", run.m, ref.m, ref.m_bound, e.m), ("v'", run.v, ref.v, ref.v_bound, e.v)):
        R.check_at(got[di], want, tol, R.allowance(R.ratio(t32, want, tol)), f"adamw {count} {name} {nm}", idx)


# ======================================================================================================================
# gradient norm
# ======================================================================================================================
@pytest.mark.parametrize("form,grid,count", R.SUMSQ_CASES)
def test_grad_sumsq_forms_match_fp64(form, grid, count, dev):
    from nerf_rpn_amd import lib, ops
    g = R.sumsq_case(count)
    gd = g.to(dev)
    floats = lib.query("grad_sumsq_floats")
    try:
        lib.call("set_sumsq_form", form, grid)
        for scale in R.SUMSQ_SCALES:
            want, bound = R.sumsq_ref(g, scale, form, grid)
            k = R.allowance(abs(R.sumsq_emulate(g, scale, grid) - want) / bound)
            a, b = (torch.full((floats,), R.SENTINEL, device=dev) for _ in range(2))
            ops.grad_sumsq(gd, a, scale)
            ops.grad_sumsq(gd, b, scale)
            torch.cuda.synchronize()
            assert torch.equal(R.bits(a), R.bits(b)), "run to run"
            assert a[1].item() == R.SENTINEL and _intact(a[2 + grid:]), "buf[1] or a partial slot beyond the grid was written"
            R.check(a[0], torch.tensor(want, dtype=F64), bound, k, f"sumsq form {form} grid {grid} count {count} scale {scale:.3f}")
    finally:
        lib.call("set_sumsq_form", 0, 1024)


# ======================================================================================================================
# transpose_weights
# ======================================================================================================================
def _transpose_run(master, rows, prefix, dtype, dev):
    from nerf_rpn_amd import lib
    from nerf_rpn_amd.ops import _p, _s
    md = master.to(dev)
    dst, guard = _guarded(torch.full((master.numel(),), R.SENTINEL), dev, dtype)
    tab = torch.tensor(rows, dtype=torch.int64, device=dev)
    pre = torch.tensor(prefix, dtype=torch.int32, device=dev)
    lib.call("transpose_weights", _p(md), _p(dst), _p(tab), _p(pre), len(rows), prefix[-1], lib.F32 if dtype == F32 else lib.BF16, _s())
    torch.cuda.synchronize()
    assert _intact(guard) and torch.equal(R.bits(md), R.bits(master)), "the guard or the master arena was written"
    return dst


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_transpose_weights_is_the_permutation(dtype, dev):
    """One table of eleven weights (ragged 64 x 64 tile edges, one-job entries at the edges of the binary search) laid out with gaps: the
    permuted master bit for bit (bf16: torch's round to nearest even of it), gaps and tail untouched; then a table of one weight."""
    master, rows, prefix, gap = R.transpose_case()
    got = _transpose_run(master, rows, prefix, dtype, dev)
    R.check_equal(R.bits(got), R.bits(R.transpose_expected(master, rows, dtype)), f"transpose_weights {dtype}")
    assert (got.cpu()[gap] == R.SENTINEL).all()
    for entry in ((1, 70, 36), (1, 8, 8), (27, 4, 130)):
        master, rows, prefix, gap = R.transpose_case([entry], seed=1)
        got = _transpose_run(master, rows, prefix, dtype, dev)
        R.check_equal(R.bits(got), R.bits(R.transpose_expected(master, rows, dtype)), f"transpose_weights {dtype} single {entry}")


# ======================================================================================================================
# reduce_slices
# ======================================================================================================================
@pytest.mark.parametrize("slices,count", R.REDUCE_CASES)
def test_reduce_slices_is_the_ordered_sum(slices, count, dev):
    """dst and the bias gradient equal the same additions in the same order in torch fp32 on the CPU (itself within slices u sum|.| of
    float64); without bias, and with it (cout 300 of wrows 320: two turns of the channel loop, the stride wider than cout, the last block
    doing bias only while every element of dst is still written)."""
    from nerf_rpn_amd import lib
    from nerf_rpn_amd.ops import _p, _s
    part, dst0, bias_part, gbias0 = R.reduce_case(slices, count)
    pd, bd = part.to(dev), bias_part.to(dev)
    for accumulate in (0, 1):
        want = R.reduce_expected(part, dst0, accumulate)
        w64 = R.reduce_expected(part, dst0, accumulate, F64)
        assert R.ratio(want, w64, slices * R.U * R.reduce_magnitude(part, dst0, accumulate) + R.ETA) <= 1.0
        for bias in (None, 0, 1):
            dst, guard = _guarded(dst0, dev)
            gb, gguard = _guarded(gbias0, dev)
            if bias is None:
                lib.call("reduce_slices", _p(pd), slices, count, _p(dst), accumulate, 0, 0, 0, 0, 0, _s())
            else:
                lib.call("reduce_slices", _p(pd), slices, count, _p(dst), accumulate, _p(bd), R.REDUCE_WROWS, R.REDUCE_COUT, _p(gb), bias, _s())
            torch.cuda.synchronize()
            assert _intact(guard, gguard) and torch.equal(R.bits(pd), R.bits(part)) and torch.equal(R.bits(bd), R.bits(bias_part))
            R.check_equal(R.bits(dst), R.bits(want), f"reduce_slices {slices} x {count} accumulate {accumulate} bias {bias}")
            wb = gbias0 if bias is None else R.reduce_bias_expected(bias_part, gbias0, bias, R.REDUCE_COUT)
            R.check_equal(R.bits(gb), R.bits(wb), f"reduce_slices {slices} x {count} bias gradient (accumulate_bias {bias})")


# ======================================================================================================================
# cast
# ======================================================================================================================
@pytest.mark.parametrize("count", R.CAST_COUNTS)
def test_cast_rounds_to_nearest_even_and_copies(count, dev):
    from nerf_rpn_amd import lib
    from nerf_rpn_amd.ops import _p, _s
    x = R.cast_case(count)
    xb = x.to(BF16)
    code = {F32: lib.F32, BF16: lib.BF16}
    for src, ddt, want in ((x, BF16, xb), (xb, F32, xb.float()), (x, F32, x), (xb, BF16, xb)):
        sd = src.to(dev)
        dst, guard = _guarded(torch.full((count,), R.SENTINEL), dev, ddt)
        lib.call("cast", _p(sd), _p(dst), count, code[src.dtype], code[ddt], _s())
        torch.cuda.synchronize()
        got = dst.cpu()
        assert _intact(guard) and torch.equal(R.bits(sd), R.bits(src))
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), "a NaN stays a NaN, and nothing else becomes one"
        R.check_equal(R.bits(got)[~nan], R.bits(want)[~nan], f"cast {src.dtype} -> {ddt} count {count}")
