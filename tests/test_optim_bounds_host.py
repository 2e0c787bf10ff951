"""Host side of tests/test_gpu_optim_kernels.py (no GPU): the float64 AdamW reference of tests/optim_ref.py is anchored to
torch.optim.AdamW(foreach=False) in float64, and its per-element bounds are shown on the CPU to be satisfiable (a torch fp32 evaluation of
the kernel's expressions stays inside, its worst |err| / bound r is printed: run with -s) and sharp (every mutation lands outside).  The
share of the bias-correction line in the p' bound is printed per step, for the launcher's fp32 powf form and for a double form.
The norm's bound is held by a torch fp32 emulation of sumsq_kernel<0>'s partition; the expected values of the three exact kernels are checked
against their index formula / float64; the limits of nrpn_set_sumsq_form are refused with an error code."""
import pytest
import torch

import optim_ref as R

F32, F64 = torch.float32, torch.float64


# ======================================================================================================================
# AdamW
# ======================================================================================================================
@pytest.mark.parametrize("clip", [False, True])
def test_adamw_reference_is_torch_adamw(clip):
    """Five steps of torch.optim.AdamW in float64 (with clip_grad_norm_ when ``clip``) against the reference iterated on its own results.
    Without the clip they agree to 1e-12; with it to 1e-6 of the distance travelled: sumsq[0] and the 1e-6 reach the kernel as floats."""
    n = 4001
    h = R.BASE._replace(sumsq=None)
    p, g, _, _, _ = R.adamw_case(n, h)
    ref = torch.nn.Parameter(p.double().clone())
    opt = torch.optim.AdamW([ref], lr=R.f32(h.lr), betas=(R.f32(h.b1), R.f32(h.b2)), eps=R.f32(h.eps), weight_decay=R.f32(h.wd), foreach=False)
    mine, m, v = p.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in range(1, 6):
        gs = g.double().roll(step) * step
        ref.grad = gs.clone()
        hs = h._replace(step=step)
        if clip:
            torch.nn.utils.clip_grad_norm_([ref], R.f32(h.max_norm), foreach=False)
            hs = hs._replace(sumsq=R.f32(gs.pow(2).sum().item()))
        opt.step()
        e = R.adamw_eval(mine, gs, m, v, hs)
        mine, m, v = e.p, e.m, e.v
    st = opt.state[ref]
    tol = 1e-6 if clip else 1e-12
    moved = (mine - p.double()).abs().max().item()
    assert (mine - ref.detach()).abs().max().item() <= tol * moved
    assert (m - st["exp_avg"]).abs().max().item() <= tol * m.abs().max().item()
    assert (v - st["exp_avg_sq"]).abs().max().item() <= 2 * tol * v.abs().max().item()


def _torch_r(count, h):
    p, g, m, v, _ = R.adamw_case(count, h)
    ref = R.adamw_ref(p, g, m, v, h)
    e = R.adamw_eval(p, g, m, v, h, F32)
    return (R.ratio(e.p, ref.p, ref.p_bound), R.ratio(e.m, ref.m, ref.m_bound), R.ratio(e.v, ref.v, ref.v_bound)), ref


@pytest.mark.parametrize("step", R.STEPS)
def test_adamw_bounds_hold_for_torch_fp32(step):
    worst = [0.0, 0.0, 0.0]
    for name, h in R.ADAMW_CONFIGS[step]:
        r, ref = _torch_r(10007, h)
        assert torch.isfinite(ref.p).all() and torch.isfinite(ref.p_bound).all()
        print(f"adamw step {step} {name}: torch fp32 r p' {r[0]:.3f} m' {r[1]:.3f} v' {r[2]:.3f}")
        assert max(r) <= 1.0, (name, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
    for count in R.ADAMW_SMALL_COUNTS:
        r, _ = _torch_r(count, R.BASE._replace(step=step))
        assert max(r) <= 1.0, (count, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"adamw step {step}: worst torch fp32 r p' {worst[0]:.3f} m' {worst[1]:.3f} v' {worst[2]:.3f}, k up to {R.allowance(max(worst)):.2f}")


def test_adamw_case_holds_what_it_promises():
    h = R.BASE
    p, g, m, v, pad = R.adamw_case(10007, h)
    assert (g == 0).sum() > 900 and ((g != 0) & (g.abs() < 1.17e-38)).sum() == 1
    assert ((v == 0) & (g != 0)).sum() >= 30 and ((v == 0) & (g == 0) & (p != 0)).sum() >= 32
    assert pad.sum() == 37 and not (p[pad].any() or g[pad].any() or m[pad].any() or v[pad].any())
    assert p.abs()[p != 0].min() < 2e-5 and p.abs().max() > 5 and g.abs()[g != 0].min() < 1e-7 and g.abs().max() > 0.5
    e = R.adamw_eval(p, g, m, v, h)
    blk = slice(300, 428)
    live = g[blk] != 0
    cancel = (e.m[blk].abs() / (e.s.b1 * m[blk].double()).abs().clamp(min=1e-300))[live]
    assert cancel.max().item() < 8 * R.U, "b1 m and (1 - b1) g coef cancel to within a few ulps"
    # the large case: elements one trip of the paired loop apart never hold the same values
    big = R.adamw_case(R.ADAMW_PAIRED, h)[0]
    s4 = 4 * R.ADAMW_S
    assert (big[:4000] != big[s4:s4 + 4000]).float().mean() > 0.99
    idx = R.adamw_sample(R.ADAMW_PAIRED_REMAINDER)
    for b in (0, 4000, s4, s4 + 4000, 2 * s4, 2 * s4 + 4000, R.ADAMW_PAIRED_REMAINDER - 1):
        assert b in idx[torch.searchsorted(idx, torch.tensor([b]))], b
    assert idx.numel() < 400_000


def test_bias_correction_share_of_the_bound():
    """Prints the share of the bias-correction line in the p' bound, per step, for the launcher's `1.0f - powf(beta, step)` (POW_ULPS ulps
    of powf) and for corrections computed in double and rounded once; the double form never carries the bound."""
    for step in R.STEPS:
        h = R.BASE._replace(step=step)
        p, g, m, v, pad = R.adamw_case(10007, h)
        live = ~pad
        f32_form = R.adamw_ref(p, g, m, v, h, pow_ulps=R.POW_ULPS).share[live]
        dbl_form = R.adamw_ref(p, g, m, v, h, pow_ulps=0).share[live]
        print(f"bias-correction share of the p' bound at step {step}: fp32 powf form median {f32_form.median().item():.2f} max {f32_form.max().item():.2f}"
              f"; double form median {dbl_form.median().item():.2f} max {dbl_form.max().item():.2f}")
        assert dbl_form.max().item() < 0.5


def test_bias_corrections_of_the_fp32_form_stay_inside_their_line():
    """torch's float32 pow, difference and square root against float64, per tested step and both betas: within bias_errors; at step 1 the
    power is exact."""
    for step in R.STEPS:
        for b1 in (0.9, 0.85):
            h = R.BASE._replace(step=step, b1=b1)
            s = R._scalars(h, F32)
            e1, e2 = R.bias_errors(h, R.POW_ULPS)
            got1 = (R.f32(h.lr) / s.step.double()).item()             # bc1 as the fp32 evaluation formed it (to within the u of lr / bc1)
            assert abs(got1 - s.bc1) <= (e1 + R.U) * s.bc1, (step, b1, got1, s.bc1)
            assert abs(s.bc2s.double().item() - s.bc2 ** 0.5) <= e2 * s.bc2 ** 0.5, (step, s.bc2s.item(), s.bc2 ** 0.5)
    assert torch.pow(torch.tensor(R.f32(0.999)), torch.tensor(1.0)).item() == R.f32(0.999)


@pytest.mark.parametrize("mutation", sorted(R.ADAMW_MUTATIONS))
def test_adamw_mutations_land_outside_the_bound(mutation):
    h = R.ADAMW_MUTATIONS[mutation]
    for name, hh in (("asserted", h), ("production", R.PRODUCTION)):
        p, g, m, v, pad = R.adamw_case(10007, hh)
        ref = R.adamw_ref(p, g, m, v, hh)
        e = R.adamw_eval(p, g, m, v, hh, F32, mutate=mutation)
        sel = ~pad & (g != 0)
        q = R._ratio((e.p.double() - ref.p).abs()[sel], 2 * ref.p_bound[sel])
        print(f"mutation {mutation} ({name}: lr {hh.lr} wd {hh.wd} max_norm {hh.max_norm} sumsq {hh.sumsq}): |err| / (2 bound) of p' median {q.median().item():.3g},"
              f" outside on {(q > 1).float().mean().item():.1%}")
        if name == "asserted":
            assert q.median().item() > R.MUTATION_THRESHOLD
            with pytest.raises(AssertionError):
                R.check(e.p, ref.p, ref.p_bound, 2.0, mutation)


def test_dropped_clip_epsilon_is_invisible_at_zero_sumsq():
    """max_norm / (0 + 1e-6) and max_norm / 0 = +inf both leave min(1, .) = 1: the mutation the issue names cannot be observed at
    sumsq = 0 in IEEE arithmetic; ADAMW_MUTATIONS tests it where the norm is of the size of the 1e-6."""
    h = R.BASE._replace(sumsq=0.0)
    assert R._scalars(h, F32, "no_clip_eps").coef.item() == R._scalars(h, F32).coef.item() == R.f32(h.grad_scale)
    assert R._scalars(R.BASE._replace(sumsq=0.0025, grad_scale=1.0 / 3), F32).coef.item() == R.f32(1.0 / 3), "inactive clip: coef == grad_scale exactly"


# ======================================================================================================================
# gradient norm
# ======================================================================================================================
def test_sumsq_depth_follows_the_loops():
    assert R.sumsq_trips(0, 64, R.SUMSQ_COUNT_ALL_LOOPS) == (0, 2, 2) and R.sumsq_trips(1, 64, R.SUMSQ_COUNT_ALL_LOOPS) == (1, 0, 2)
    assert R.sumsq_trips(2, 64, R.SUMSQ_COUNT_ALL_LOOPS) == (1, 0, 2) and R.sumsq_trips(1, 64, R.SUMSQ_COUNT_8_THEN_4) == (1, 1, 1)
    assert R.sumsq_trips(0, 1024, R.SUMSQ_COUNT_PRODUCTION) == (0, 1, 1) and R.sumsq_trips(0, 1024, 3) == (0, 0, 0)
    assert R.sumsq_trips(0, 1024, 74_815_925) == (0, 18, 0)
    assert R.sumsq_depth(0, 64, R.SUMSQ_COUNT_ALL_LOOPS) == 16 + 2 + 8 + 1 + 8 and R.sumsq_depth(0, 2048, 3) == 1 + 2 + 8 + 8 + 8


@pytest.mark.parametrize("grid,count", sorted({(gr, c) for _, gr, c in R.SUMSQ_CASES}))
def test_sumsq_bound_holds_for_the_emulated_partition(grid, count):
    g = R.sumsq_case(count)
    for scale in R.SUMSQ_SCALES:
        want, bound = R.sumsq_ref(g, scale, 0, grid)
        got = R.sumsq_emulate(g, scale, grid)
        r = abs(got - want) / bound
        print(f"sumsq grid {grid} count {count} scale {scale:.3f}: torch fp32 emulation r {r:.4f} (depth {R.sumsq_depth(0, grid, count)})")
        assert r <= 1.0
        plain = (g * torch.tensor(R.f32(scale))).pow(2).sum().item()             # torch's own order: another partition, same bound class
        assert abs(plain - want) <= bound * 4


def test_set_sumsq_form_refuses_what_the_kernels_cannot_run():
    from nerf_rpn_amd import lib
    for form, grid in ((3, 1024), (-1, 1024), (0, 63), (0, 2049)):
        with pytest.raises(lib.NrpnError, match="set_sumsq_form"):
            lib.call("set_sumsq_form", form, grid)
    lib.call("set_sumsq_form", 0, 1024)          # the default, and what a refused call leaves in place


# ======================================================================================================================
# the exact kernels' expected values
# ======================================================================================================================
def test_transpose_expected_is_the_index_formula():
    master, rows, prefix, gap = R.transpose_case()
    want = R.transpose_expected(master, rows, F32)
    assert prefix[:7] == [0, 27, 29, 110, 118, 461, 465] and prefix[-1] == 470 and len(prefix) == len(rows) + 1
    assert torch.equal(want[gap], torch.full((int(gap.sum()),), R.SENTINEL)) and gap[:5].all() and gap[-11:].all()
    for off, taps, cout, cin in (rows[1], rows[2], rows[6]):
        for t, o, c in ((0, 0, 0), (taps - 1, cout - 1, cin - 1), (taps // 2, cout // 3, cin // 2), (0, cout - 1, 0)):
            assert R.bits(want)[off + (taps - 1 - t) * cin * cout + c * cout + o] == R.bits(master)[off + t * cout * cin + o * cin + c]
    off = rows[0][0]
    planted = master[off + 3:off + 3 + 17 * 7:17]           # the seven special values of the first weight
    assert planted.bfloat16().float().tolist()[:3] == [1.0, 1.0 + 2.0 ** -6, -1.0], "ties go to even, both ways"
    assert R.bits(planted)[3].item() == -2 ** 31 and 0 < planted[4].item() < 1.17e-38 and torch.isinf(planted[5:]).all()


def test_reduce_expected_is_within_float64():
    for slices, count in ((1, 1028), (2, 1028), (7, 1028)):
        part, dst, bias_part, gbias = R.reduce_case(slices, count)
        for acc in (0, 1):
            got = R.reduce_expected(part, dst, acc)
            want = R.reduce_expected(part, dst, acc, F64)
            assert R.ratio(got, want, slices * R.U * R.reduce_magnitude(part, dst, acc) + R.ETA) <= 1.0
            gb = R.reduce_bias_expected(bias_part, gbias, acc, R.REDUCE_COUT)
            assert torch.equal(gb[R.REDUCE_COUT:], gbias[R.REDUCE_COUT:])
            wb = R.reduce_bias_expected(bias_part, gbias, acc, R.REDUCE_COUT, F64)
            mag = bias_part.double().abs().sum(0) + gbias.double().abs()
            assert R.ratio(gb, wb, (slices + 1) * R.U * mag + R.ETA) <= 1.0


def test_cast_case_values():
    x = R.cast_case(257)
    y = x.bfloat16()
    assert torch.isnan(x).sum() == 1 and torch.isinf(x).sum() == 2 and torch.isinf(y).sum() == 4, "the largest finite fp32 rounds to inf in bf16"
    assert y[0].item() == 1.0 and y[13].item() == 1.0 + 2.0 ** -6 and R.bits(y)[39].item() == -32768, "ties to even; -0.0 keeps its sign"
    assert R.cast_case(1).item() == 1.0 + 2.0 ** -8
