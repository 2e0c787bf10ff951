"""float64 references of the five optimiser / arena kernels of csrc/elementwise.hip (nrpn_adamw_step[_zero_grad], nrpn_grad_sumsq,
nrpn_transpose_weights, nrpn_reduce_slices, nrpn_cast) with per-element error bounds built from float64 magnitudes; the same expressions
evaluated in torch fp32 on the CPU (what the allowance k is measured on), with the mutations the bounds have to catch; the seeded cases
shared by tests/test_optim_bounds_host.py (no GPU) and tests/test_gpu_optim_kernels.py.  ratio / allowance / check are fcos_ref's.

AdamW.  Reference: the kernel's formula in float64 from the same fp32 inputs, hyper-parameters at the fp32 values the C ABI receives,
bc = 1 - beta^step in float64 (anchored to torch.optim.AdamW(foreach=False) in float64 by the host test):
    coef = grad_scale min(1, max_norm / (sqrt(sumsq[0]) + 1e-6f)) with a sumsq pointer and max_norm > 0, else grad_scale
    gi = g coef;  m' = b1 m + (1 - b1) gi;  v' = b2 v + (1 - b2) gi^2;  den = sqrt(v') / sqrt(bc2) + eps
    p' = p (1 - lr wd) - (lr / bc1) m' / den
Bounds (u = 2^-24, first order through the kernel's intermediates; the unit is built with contraction allowed, which only removes
roundings; every output bound also holds the absolute floor ETA = 2^-126, every intermediate 2^-147 for results below the normal range):

    quantity   magnitude                    rounded operations counted                                             constant
    gi         |g coef|                     product 1; coef with the clip: sqrt, + 1e-6, divide, grad_scale 4      cg = 5 (1 without clip)
    m'         A = |b1 m|                   product 1, sum 1                                                       2u A
               B = |(1 - b1) gi|            gi cg, 1 - b1 1, product 1, sum 1                                      (cg + 3) u B
    v'         A = b2 v                     product 1, sum 1                                                       2u A
               B = (1 - b2) gi^2            gi twice 2 cg, 1 - b2 1, two products 2, sum 1                         (2 cg + 4) u B
    sqrt(v')   d = min(dv' / (2 sqrt v'), sqrt(dv'))   (|sqrt a - sqrt b| <= sqrt|a - b| where v' is 0 or below its own error)
    den        d / sqrt(bc2) + (sqrt(v') / sqrt(bc2)) (sqrt 1 + divide 1 + e2) u + u den (the sum)
    p'         |p decay|                    lr wd and 1 - . 2, product 1, final difference 1                       4u
               |upd| = (lr / bc1) |m'| / den   m' / den 1, lr / bc1 1, product 1, final difference 1, + e1         (4 + e1) u
               + (lr / bc1) dm' / den + |upd| dden / den
    e1, e2: relative error of bc1 and sqrt(bc2) as the launcher hands them over, in units of u -- the bias-correction line of the bound.

Bias corrections.  The launcher forms them as `1.0f - powf(beta, (float)step)` and sqrtf(bc2).  One ulp of powf at x = beta^step
(ulp32(x), the exact spacing: u for x in [0.5, 1)) is ulp32(x) / bc of the correction: with beta2 = 0.999, 500 u of bc2 at step 2 and
100 u at step 10.  The line allows POW_ULPS = 1 ulp, and none at step 1, where pow(x, 1) is x: e1 = ulp32(b1^step) / bc1 + u (the
difference), e2 = (ulp32(b2^step) / bc2 + u) / 2 + u (the square root).  Its share of the p' bound (median / largest over the elements
of the 10007 case, host test): 0.00 / 0.10 at step 1, 0.11 / 0.96 at step 2, 0.02 / 0.83 at step 10, 0.00 / 0.22 at step 1000,
0.00 / 0.20 at step 100000 -- above the sum of all other terms on some elements (small |p|) at steps 2 and 10.  Corrections computed in
double and rounded once (e1 = e2 = u, bias_errors(h, 0)) would hold the share <= 0.16 at every step; the launcher keeps the fp32 form
because changing it moves the last bit of every weight from step 2 on, which the chaotic 40-step trajectory of
tests/test_gpu_convergence.py does not absorb inside its bands.  The reference models the fp32 form, and its fp32 evaluation forms the
corrections with torch.pow in float32 (held inside the line by the host test).

Every assertion is |err| <= k * bound, k = max(1, min(2, 4 r)) with r the largest |err| / bound of the torch fp32 CPU evaluation of the
same case (never of the kernel).  r as measured on the CPU over every configuration of ADAMW_CONFIGS at count 10007 (host test):
    p' <= 0.57, m' <= 0.97, v' <= 0.98 (the two-addend bounds of m' and v' are nearly attained where one addend carries the result)
    -- k = 2 at 10007 and the large counts, 1.0 - 2.0 at the tiny ones; the ordered norm (form 0 emulated with the kernel's partition):
    r <= 0.062, k = 1.
Mutations (host test, applied to the fp32 evaluation, |err| / (2 bound) of p', median over the elements with g != 0 that are not padding):
    at the PRODUCTION hyper-parameters (lr 3e-4, wd 0.01, step 10, clip active, grad_scale 1/3): bc1 = 1: 969; bc2 for sqrt(bc2): 2.5e3;
    eps inside the square root: 35; grad_scale dropped from coef: 21; decay applied after the update: 0.09 and coupled L2: 6 -- at
    lr wd = 3e-6 decay-after differs from AdamW by less than the roundings of p' on most elements, so no test at those values can see it;
    at the LOUD configuration (lr 1e-2, wd 0.1) the two reach 55 and 1.9e3.  Asserted: median > MUTATION_THRESHOLD = 10 at the
    configuration named in ADAMW_MUTATIONS (the weakest, the dropped grad_scale, reaches 21).  The 1e-6 of the clip dropped: at sumsq = 0
    the quotient is huge or +inf and min(1, .) returns the same 1 -- not observable in IEEE arithmetic, asserted as such; at the TINY_NORM
    configuration (max_norm 1e-6, sumsq 1e-12: norm = 1e-6) coef doubles: median 428.  LOUD and TINY_NORM are in ADAMW_CONFIGS so that
    the device test can see all seven.

Large counts (8 392 611 and 16 781 217; S = 8192 x 256 quads): the data is a 1 000 003-element seeded case repeated (a prime length: the
elements q and q + S of a lane's pair never hold the same values).  The exact checks (gradient cleared or kept, shadow, padding, the two
variants bit-equal, run-to-run) cover every element; the bound is applied to windows of 4096 elements on both sides of every loop boundary
(0, 4 x 1000, 4S, 4(S + 1000), 8S, 4(2S + 1000), the tail) plus every 64th element -- adamw_sample -- and failures name the flat index.

Gradient norm.  Reference: sum (g scale)^2 in float64, scale at its fp32 value.  Bound (3 + depth) u sum t^2 + ETA: product, square and
the accumulate of each term, depth = the longest chain of additions (sumsq_depth: four per 16-byte load a lane adds into one accumulator,
the (s0 + s1) + (s2 + s3) join, 8 LDS levels, ceil(grid / 256) strided adds of the finish kernel, 8 more).

transpose_weights, reduce_slices, cast: equalities (a permutation; additions in a fixed order repeated in torch fp32 on the CPU, held
to float64 within slices u sum|.|; round to nearest even).

Left out: nrpn_cast bf16 -> bf16 is tested as a copy only at the small counts; sumsq_kernel forms 1 and 2 take their allowance from the
emulation of form 0 (same terms, other partition).  The grid cap of adamw / reduce_slices / cast (8192 blocks) IS reached: the large counts."""
import collections
import math
import types

import numpy as np
import torch

from fcos_ref import ETA, F32, F64, U, _ratio, allowance, check, check_equal, ratio  # noqa: F401  (re-exported to the two test files)

TINY = 2.0 ** -147            # four roundings into the subnormal range (2^-149 each)
SENTINEL = -12288.0           # exact in bf16


def f32(x):
    """The value a C `float` argument holds."""
    return float(np.float32(x))


# ======================================================================================================================
# AdamW
# ======================================================================================================================
ADAMW_S = 8192 * 256                                        # lanes of the capped grid = quads per trip of the paired loop
ADAMW_SMALL_COUNTS = (1, 3, 4, 5, 1023, 10007)
ADAMW_PAIRED, ADAMW_PAIRED_REMAINDER = 4 * (ADAMW_S + 1000) + 3, 4 * (2 * ADAMW_S + 1000) + 1
ADAMW_PERIOD = 1_000_003
POW_ULPS = 1                                                # of powf, allowed to the launcher's fp32 bias corrections
STEPS = (1, 2, 10, 1000, 100000)

Hyper = collections.namedtuple("Hyper", "lr b1 b2 eps wd step grad_scale max_norm sumsq")      # sumsq: None = null pointer, else sumsq[0]
BASE = Hyper(3e-4, 0.9, 0.999, 1e-8, 0.01, 10, 1.0, 0.1, 7.3)
CLIPS = {"active": dict(sumsq=7.3), "inactive": dict(sumsq=0.0025), "zero_sumsq": dict(sumsq=0.0), "no_pointer": dict(sumsq=None),
         "max_norm0": dict(max_norm=0.0)}
LOUD = BASE._replace(lr=1e-2, wd=0.1, grad_scale=1.0 / 3)
TINY_NORM = BASE._replace(max_norm=1e-6, sumsq=1e-12)
PRODUCTION = BASE._replace(grad_scale=1.0 / 3)


def adamw_configs(step):
    """Every configuration run at count 10007 for one step number: clip mode x grad_scale, then wd = 0, beta1 = 0.85 (what one_cycle
    passes) and both, and the two configurations the mutations need."""
    out = [(f"{c}-gs{gs:.3f}", BASE._replace(step=step, grad_scale=gs, **kw)) for c, kw in CLIPS.items() for gs in (1.0, 0.125, 1.0 / 3)]
    out += [("wd0", BASE._replace(step=step, wd=0.0)), ("b1_085", BASE._replace(step=step, b1=0.85)),
            ("wd0-b1_085-gs0.333", BASE._replace(step=step, wd=0.0, b1=0.85, grad_scale=1.0 / 3)),
            ("loud", LOUD._replace(step=step)), ("tiny_norm", TINY_NORM._replace(step=step))]
    return out


ADAMW_CONFIGS = {s: adamw_configs(s) for s in STEPS}
BIG_CONFIGS = [("base", BASE, False, False), ("zero_grad-shadow-clip", PRODUCTION._replace(step=1000), True, True)]
# mutation -> the configuration at which it has to land outside the bound (module docstring)
ADAMW_MUTATIONS = {"bc1_one": PRODUCTION, "bc2_nosqrt": PRODUCTION, "eps_inside": PRODUCTION, "no_grad_scale": PRODUCTION,
                   "decay_after": LOUD, "coupled_l2": LOUD, "no_clip_eps": TINY_NORM}
MUTATION_THRESHOLD = 10.0


def _scalars(h, dtype, mutate=None):
    """The kernel's and the launcher's scalars as 0-d tensors of ``dtype``, every operation rounded in ``dtype`` (the bias corrections too: in float32 they
    are the launcher's `1.0f - powf(beta, (float)step)` and sqrtf)."""
    def t(x):
        return torch.tensor(f32(x), dtype=dtype)
    one = torch.ones((), dtype=dtype)
    gs = one.clone() if mutate == "no_grad_scale" else t(h.grad_scale)
    coef = gs
    clip = h.sumsq is not None and f32(h.max_norm) > 0
    if clip:
        norm = torch.sqrt(t(h.sumsq))
        if mutate != "no_clip_eps":
            norm = norm + t(1e-6)
        coef = gs * torch.minimum(one, t(h.max_norm) / norm)
    b1, b2 = f32(h.b1), f32(h.b2)
    bc1, bc2 = 1.0 - b1 ** h.step, 1.0 - b2 ** h.step
    if dtype == F32:           # the launcher's own form: 1.0f - powf(beta, (float)step), sqrtf
        bc1_t, bc2_t = one - torch.pow(t(h.b1), t(float(h.step))), one - torch.pow(t(h.b2), t(float(h.step)))
    else:
        bc1_t, bc2_t = torch.tensor(bc1, dtype=dtype), torch.tensor(bc2, dtype=dtype)
    bc1_t = one.clone() if mutate == "bc1_one" else bc1_t
    bc2s_t = bc2_t if mutate == "bc2_nosqrt" else torch.sqrt(bc2_t)
    return types.SimpleNamespace(coef=coef, clip=clip, decay=one - t(h.lr) * t(h.wd), b1=t(h.b1), b2=t(h.b2), omb1=one - t(h.b1), omb2=one - t(h.b2),
                                 eps=t(h.eps), wd=t(h.wd), step=t(h.lr) / bc1_t, bc2s=bc2s_t, bc1=bc1, bc2=bc2)


def adamw_eval(p, g, m, v, h, dtype=F64, mutate=None):
    """The kernel's expressions in ``dtype`` (float64: the reference; float32: the torch evaluation k is measured on) -> namespace with
    p, m, v (the results) and the intermediates the bounds are built from.  ``mutate``: a key of ADAMW_MUTATIONS."""
    s = _scalars(h, dtype, mutate)
    p, g, m, v = p.to(dtype), g.to(dtype), m.to(dtype), v.to(dtype)
    if mutate == "coupled_l2":
        g = g + s.wd * p
    gi = g * s.coef
    pd = p if mutate in ("coupled_l2", "decay_after") else p * s.decay
    m2 = s.b1 * m + s.omb1 * gi
    v2 = s.b2 * v + s.omb2 * gi * gi
    if mutate == "eps_inside":
        den = torch.sqrt(v2 + s.eps) / s.bc2s
    else:
        den = torch.sqrt(v2) / s.bc2s + s.eps
    upd = s.step * (m2 / den)
    p2 = (pd - upd) * s.decay if mutate == "decay_after" else pd - upd
    return types.SimpleNamespace(p=p2, m=m2, v=v2, gi=gi, pd=pd, den=den, upd=upd, s=s, m_in=m, v_in=v)


def ulp32(x):
    """The spacing of fp32 at |x| (2^-149 in the subnormal range and at 0)."""
    return 2.0 ** max(math.floor(math.log2(abs(x))) - 23, -149) if x else 2.0 ** -149


def bias_errors(h, pow_ulps=0):
    """Relative errors of bc1 and sqrt(bc2) as handed to the kernel.  pow_ulps = 0: computed in double, rounded once (u each).  Otherwise
    `1.0f - powf(beta, step)`: ``pow_ulps`` ulps of powf at beta^step (none at step 1: pow(x, 1) is x), the difference rounded, and for
    bc2 the square root rounded."""
    if not pow_ulps:
        return U, U
    b1s, b2s = f32(h.b1) ** h.step, f32(h.b2) ** h.step
    k = 0 if h.step == 1 else pow_ulps
    return k * ulp32(b1s) / (1 - b1s) + U, 0.5 * (k * ulp32(b2s) / (1 - b2s) + U) + U


def adamw_ref(p, g, m, v, h, pow_ulps=POW_ULPS):
    """float64 p', m', v' with their bounds (module docstring) and ``share``: the part of the p' bound that is the bias-correction line."""
    e = adamw_eval(p, g, m, v, h)
    s = e.s
    cg = 5.0 if s.clip else 1.0
    a, b = (s.b1 * e.m_in).abs(), (s.omb1 * e.gi).abs()
    dm = U * (2 * a + (cg + 3) * b) + TINY
    a2, b2 = s.b2 * e.v_in, s.omb2 * e.gi * e.gi
    dv = U * (2 * a2 + (2 * cg + 4) * b2) + TINY
    sq = torch.sqrt(e.v)
    dsq = torch.minimum(dv / (2 * sq).clamp(min=1e-300), torch.sqrt(dv))
    e1, e2 = bias_errors(h, pow_ulps)
    d1 = sq / s.bc2s
    dden = dsq / s.bc2s + d1 * 2 * U + U * e.den
    upd = e.upd.abs()
    bias = upd * (d1 * e2 / e.den + e1)
    other = 4 * U * e.pd.abs() + s.step * dm / e.den + upd * dden / e.den + 4 * U * upd + ETA
    return types.SimpleNamespace(p=e.p, m=e.m, v=e.v, p_bound=bias + other, m_bound=dm + ETA, v_bound=dv + ETA, share=bias / (bias + other))


def _base_case(n, h, seed):
    rs = np.random.RandomState((5000 + seed + n) % (2 ** 31))

    def signed(lo, hi):
        return np.where(rs.random_sample(n) < 0.5, -1.0, 1.0) * 10.0 ** rs.uniform(lo, hi, n)
    p = signed(-5, 1).astype(np.float32)                   # six decades, 1e-5 ... 10
    g = signed(-8, 0).astype(np.float32)                   # eight decades
    if h.step > 1:                                         # plausible running moments: |m| <= |g|, v = (0.5 ... 2 g)^2, from g before its zeros
        m = (g * rs.uniform(-1.0, 1.0, n)).astype(np.float32)
        v = ((g * rs.uniform(0.5, 2.0, n)) ** 2).astype(np.float32)
    else:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    g[7::11] = 0.0                                         # exact zeros over moments that are not
    if n > 5:
        g[5] = 1e-40                                       # one fp32 denormal
    pad = slice(0, 0)
    if n >= 600:
        v[100:140] = 0.0                                   # v = 0 under g != 0 (and under the g = 0 of 106, 117, 128, 139)
        g[200:232] = 0.0                                   # g = m = v = 0, p alive: p' = p decay
        m[200:232] = 0.0
        v[200:232] = 0.0
        # b1 m and (1 - b1) g coef cancel to within a few ulps: m = -(1 - b1) g coef / b1 rounded, every other one moved by 1 - 3 ulps
        s = _scalars(h, F64)
        blk = slice(300, 428)
        mc = (-(float(s.omb1) / float(s.b1)) * float(s.coef) * g[blk].astype(np.float64)).astype(np.float32)
        far = np.where(mc < 0, -np.inf, np.inf).astype(np.float32)
        away, toward = np.nextafter(mc, far), np.nextafter(mc, np.float32(0))
        mc[1::4], mc[2::4], mc[3::4] = away[1::4], toward[2::4], np.nextafter(np.nextafter(away, far), far)[3::4]
        m[blk] = np.where(g[blk] == 0, np.float32(0), mc)
        pad = slice(500, 537)                              # arena padding: everything zero
        for arr in (p, g, m, v):
            arr[pad] = 0.0
    return p, g, m, v, pad


def adamw_case(count, h, seed=0):
    """Seeded fp32 (p, g, m, v) of ``count`` elements from numpy's legacy generator and ``pad``, the bool mask of the arena padding.
    Beyond ADAMW_PERIOD elements the case of that length is repeated (module docstring)."""
    n = min(count, ADAMW_PERIOD)
    p, g, m, v, pad = _base_case(n, h, seed)
    mask = np.zeros(n, bool)
    mask[pad] = True
    if count > n:
        p, g, m, v, mask = (np.resize(a, count) for a in (p, g, m, v, mask))
    assert all(np.isfinite(a).all() for a in (p, g, m, v)) and (v >= 0).all()
    return tuple(torch.from_numpy(a) for a in (p, g, m, v)) + (torch.from_numpy(mask),)


def adamw_sample(count):
    """Flat indices the bound is applied to: every element up to 2^20, beyond that windows of 4096 on both sides of every loop boundary of
    adamw_kernel plus every 64th element (module docstring)."""
    if count <= 1 << 20:
        return torch.arange(count)
    s4 = 4 * ADAMW_S
    marks = [0, 4000, s4, s4 + 4000, 2 * s4, 2 * s4 + 4000, count - (count % 4), count]
    idx = [torch.arange(0, count, 64)]
    for b in (b for b in marks if b - 4096 < count):
        idx.append(torch.arange(max(0, b - 4096), min(count, b + 4096)))
    return torch.unique(torch.cat(idx))


def check_at(got, want, tol, k, what, index):
    """fcos_ref.check over the sampled elements ``index``; a failure names the flat index in the whole array."""
    try:
        return check(got, want, tol, k, what)
    except AssertionError as exc:
        bad = _ratio((got.detach().double().cpu().reshape(want.shape) - want).abs(), tol * k) > 1
        where = index[bad.reshape(-1)]
        raise AssertionError((what, "flat indices", int(where.min()), "...", int(where.max()), "in quads of", ADAMW_S, "lanes: trips",
                              sorted(set((where // (4 * ADAMW_S)).tolist()))[:4], exc.args[0])) from None


# ======================================================================================================================
# gradient norm
# ======================================================================================================================
SUMSQ_SCALES = (1.0, 0.5, 1.0 / 3)
SUMSQ_COUNT_ALL_LOOPS = 4 * 64 * 2348 + 3                  # grid 64: 8-wide loop of forms 1 and 2, 4-wide of form 0, singles, tail
SUMSQ_COUNT_8_THEN_4 = 4 * 64 * 3116 + 3                   # grid 64, form 1: one 8-wide trip, then one 4-wide, then a single
SUMSQ_COUNT_PRODUCTION = 4 * 1024 * 1100 + 2               # form 0 at grid 1024 inside its 4-wide loop
# (form, grid, count)
SUMSQ_CASES = ([(f, 64, SUMSQ_COUNT_ALL_LOOPS) for f in (0, 1, 2)] + [(f, 64, SUMSQ_COUNT_8_THEN_4) for f in (0, 1, 2)]
               + [(f, gr, c) for f in (0, 1, 2) for gr in (1024, 2048) for c in (3, 1000, SUMSQ_COUNT_ALL_LOOPS)]
               + [(0, 1024, SUMSQ_COUNT_PRODUCTION)])


def sumsq_trips(form, grid, count):
    """(8-wide, 4-wide, single) loop trips of the lane that takes the most: lane 0 of block 0."""
    n4 = count // 4
    length, stride = (n4, grid * 256) if form == 2 else (-(-n4 // grid), 256)
    it8 = max(0, -(-(length - 7 * stride) // (8 * stride))) if form in (1, 2) else 0
    pos = it8 * 8 * stride
    it4 = max(0, -(-(length - pos - 3 * stride) // (4 * stride))) if form in (0, 1) else 0
    pos += it4 * 4 * stride
    return it8, it4, max(0, -(-(length - pos) // stride))


def sumsq_depth(form, grid, count):
    it8, it4, single = sumsq_trips(form, grid, count)
    lane = max(4 * (2 * it8 + it4 + single), 4 * (2 * it8 + it4) + 1)          # s0 takes the singles, s1 the scalar tail
    return lane + 2 + 8 + -(-grid // 256) + 8


def sumsq_case(count, seed=0):
    return torch.from_numpy((np.random.RandomState(6000 + seed + count % 100003).standard_normal(count) * 1e-3).astype(np.float32))


def sumsq_ref(g, scale, form, grid):
    t2 = (g.double() * f32(scale)) ** 2
    total = t2.sum().item()
    return total, (3 + sumsq_depth(form, grid, g.numel())) * U * total + ETA


def _tree256(x):
    """sh[t] += sh[t + off], off = 128 ... 1, over the last dimension (256 wide)."""
    off = 128
    while off:
        x = x[..., :off] + x[..., off:2 * off]
        off //= 2
    return x[..., 0]


def sumsq_emulate(g, scale, grid):
    """sumsq_kernel<0> + sumsq_finish_kernel in torch fp32 on the CPU: the same block ranges, four accumulators per lane, the join, both trees."""
    count = g.numel()
    n4 = count // 4
    sc = torch.tensor(f32(scale), dtype=F32)
    t = g.float() * sc
    sq = t * t
    per = -(-n4 // grid)
    trips = -(-per // 256) if per else 0
    padded = torch.zeros(grid * max(trips, 1) * 256 * 4, dtype=F32).view(grid, max(trips, 1) * 256, 4)
    length = (torch.clamp(torch.tensor(n4) - torch.arange(grid) * per, min=0, max=per)).view(grid, 1)             # b1 - b0 per block
    if n4:
        body = sq[:n4 * 4].view(n4, 4)
        for b in range(min(grid, -(-n4 // per))):
            ln = int(length[b])
            padded[b, :ln] = body[b * per:b * per + ln]
    lane = torch.arange(256).view(1, 256)
    acc = torch.zeros(grid, 256, 4, dtype=F32)
    for j in range(trips):
        wide = lane + 1024 * (j // 4) + 768 < length                       # this load belongs to a four-wide trip of its lane
        which = torch.where(wide, torch.tensor(j % 4), torch.tensor(0))
        for kk in range(4):
            val = padded[:, j * 256:(j + 1) * 256, kk]                     # zero beyond the range: x + 0 is exact
            for a in range(4):
                acc[:, :, a] = torch.where(which == a, acc[:, :, a] + val, acc[:, :, a])
    tail = count - n4 * 4
    if tail:
        acc[0, :tail, 1] = acc[0, :tail, 1] + sq[n4 * 4:]
    parts = _tree256((acc[:, :, 0] + acc[:, :, 1]) + (acc[:, :, 2] + acc[:, :, 3]))
    fin = torch.zeros(256, dtype=F32)
    for k0 in range(0, grid, 256):
        chunk = parts[k0:k0 + 256]
        fin[:chunk.numel()] = fin[:chunk.numel()] + chunk
    return _tree256(fin).item()


# ======================================================================================================================
# transpose_weights
# ======================================================================================================================
TRANSPOSE_ENTRIES = [(27, 64, 64), (1, 70, 36), (27, 4, 130), (8, 1, 1), (343, 16, 4), (1, 128, 65)] + [(1, 8, 8)] * 5
SPECIALS = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -0.0, 1e-40, float("inf"), float("-inf"))


def plant(a, values=SPECIALS, first=3, step=17):
    """Special values at fixed flat positions of the fp32 numpy array ``a`` (as many as fit)."""
    for i, val in enumerate(values):
        if first + step * i < a.size:
            a[first + step * i] = val
    return a


def transpose_case(entries=TRANSPOSE_ENTRIES, seed=0):
    """-> master fp32 (gaps and a tail between the weights), table rows (offset, taps, cout, cin), tile_prefix, the bool mask of the gaps.
    Every weight holds the special values (bf16 ties both ways, -0.0, a denormal, +-inf) as far as it has room."""
    rs = np.random.RandomState(7000 + seed)
    rows, prefix, off = [], [0], 5
    for i, (t, co, ci) in enumerate(entries):
        rows.append([off, t, co, ci])
        prefix.append(prefix[-1] + t * ((co + 63) // 64) * ((ci + 63) // 64))
        off += t * co * ci + (3, 1, 7, 2)[i % 4]
    total = off + 11
    master = rs.standard_normal(total).astype(np.float32)
    gap = np.ones(total, bool)
    for o, t, co, ci in rows:
        plant(master[o:o + t * co * ci])
        gap[o:o + t * co * ci] = False
    return torch.from_numpy(master), rows, prefix, torch.from_numpy(gap)


def transpose_expected(master, rows, dtype):
    """dst[off + (taps - 1 - t) cin cout + c cout + o] = master[off + t cout cin + o cin + c], cast by torch (round to nearest even);
    the gaps hold SENTINEL."""
    out = torch.full((master.numel(),), SENTINEL, dtype=dtype)
    for o, t, co, ci in rows:
        w = master[o:o + t * co * ci].view(t, co, ci)
        out[o:o + t * co * ci] = w.flip(0).permute(0, 2, 1).contiguous().view(-1).to(dtype)
    return out


def bits(t):
    """Integer view for bit comparisons (-0.0 against 0.0, infinities)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


# ======================================================================================================================
# reduce_slices
# ======================================================================================================================
REDUCE_BIG = 4 * (8192 * 256 + 5)
REDUCE_CASES = [(s, c) for s in (1, 2, 7) for c in (4, 1028)] + [(2, REDUCE_BIG)]      # (slices, count)
REDUCE_COUT, REDUCE_WROWS = 300, 320


def reduce_case(slices, count, seed=0):
    """-> partials [slices, count], dst prefill [count], bias partials [slices, wrows], gbias prefill [wrows]: seeded normals over
    three decades (sums that round at every step)."""
    rs = np.random.RandomState(8000 + seed + slices + count % 100003)

    def draw(*shape):
        return torch.from_numpy((rs.standard_normal(shape) * 10.0 ** rs.randint(-2, 2, shape)).astype(np.float32))
    return draw(slices, count), draw(count), draw(slices, REDUCE_WROWS), draw(REDUCE_WROWS)


def reduce_expected(part, dst, accumulate, dtype=F32):
    acc = part[0].to(dtype).clone()
    for s in range(1, part.shape[0]):
        acc += part[s].to(dtype)
    if accumulate:
        acc += dst.to(dtype)
    return acc


def reduce_bias_expected(bias_part, gbias, accumulate, cout, dtype=F32):
    s = torch.zeros(cout, dtype=dtype)
    for k in range(bias_part.shape[0]):
        s += bias_part[k, :cout].to(dtype)
    out = gbias.to(dtype).clone()
    out[:cout] = out[:cout] + s if accumulate else s
    return out


def reduce_magnitude(part, dst, accumulate):
    mag = part.double().abs().sum(0)
    return mag + dst.double().abs() if accumulate else mag


# ======================================================================================================================
# cast
# ======================================================================================================================
CAST_COUNTS = (1, 257, 8192 * 256 + 3)
F32_MAX = 3.4028234663852886e38                             # rounds to +inf in bf16


def cast_case(count, seed=0):
    """Seeded fp32 with the special values of the transpose case, the largest finite fp32 and one NaN (as far as ``count`` has room; at
    count 1 the single element is the first bf16 tie)."""
    a = np.random.RandomState(9000 + seed + count % 100003).standard_normal(count).astype(np.float32)
    plant(a, SPECIALS + (F32_MAX, -F32_MAX, float("nan")), first=0, step=13)
    return torch.from_numpy(a)
