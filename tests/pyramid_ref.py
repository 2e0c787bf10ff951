"""float64 / integer references of the "copy / select / add" companions of csrc/elementwise.hip -- nrpn_maxpool3d_fwd / _bwd,
nrpn_upsample_add_fwd / _bwd, nrpn_subsample3d, nrpn_add_relu, nrpn_relu_backward, nrpn_ncdhw_to_ndhwc / nrpn_ndhwc_to_ncdhw -- written
from the definition of each operation in numpy, the seeded data they are run on, and the one bound the multi-term backwards need.  Shared
by tests/test_pyramid_ref_host.py (no GPU: the references against torch in float64, the mutations) and tests/test_gpu_pyramid_kernels.py.
ratio / allowance / check are fcos_ref's.  Tensors are channels-last [N, X, Y, Z, C] numpy float64 arrays holding values of the storage
type (fp32 or bf16), so float64 arithmetic on them is the exact operation up to float64's own rounding.

Definitions.
    max pool     y[w] = max over the window of w, padding = -inf and never the argmax: the in-grid positions of the window are scanned in
                 ascending (a, b, d) order, the first one is taken whatever it holds (a window of -inf data reports its first in-grid
                 position, torch's rule), a later one only if strictly greater -- the first maximum wins.  code = (a k + b) k + d.
                 Output size: torch's, floor or ceil of (g + 2p - k) / s, + 1, and a ceil-mode window must start inside input + left pad.
                 dx[v] = sum of dy[w] over the windows w whose argmax is v.
    upsample-add fine[v] += coarse[src(v)], per axis src(dst) = min(floor(dst * ((float)in / out)), in - 1) with the quotient, the
                 product and the floor in fp32 (np.float32 here).  dcoarse[u] = sum of d[v] over src(v) = u (+ the old dcoarse[u] with
                 accumulate = 1).  For (in, out) = (14, 46), (26, 44), (28, 46), (30, 58) -- the only pairs with in <= out <= 64 -- the
                 fp32 rule is NOT the integer floor(dst in / out): the rounded quotient, times dst, lands on the next integer.
    subsample    y[x, y, z] = x[s x, s y, s z]; backward: dy at the multiples of s, +0 everywhere else.
    add_relu     round(a + b), then max(., +0) if relu (-0 < +0: a sum of -0.0 comes out as +0.0 under relu, as -0.0 without).
    relu_bwd     dx = dy where y > 0, else +0: y = -0.0 and y = +0.0 give +0, a positive denormal y passes dy.
    layouts      [N][C][V] fp32 <-> [N][V][C] T: the permutation and one round-to-nearest-even.

Rounding.  round_to(dtype) rounds a float64 ONCE to nearest even at 24 (fp32) or 8 (bf16) significant bits, with the subnormal spacing
2^-149 (both share fp32's exponent range: bf16's is 2^-133), overflow to inf.  The kernels add in fp32 and then store: for bf16 that is
two roundings of a + b.  Double rounding is harmless for a two-term sum: the exact sum of two p-bit numbers rounded first to q >= 2p + 2
bits and then to p bits equals the one-step rounding (Figueroa), and 24 >= 2 * 8 + 2 (bf16 through fp32), 53 >= 2 * 24 + 2 (fp32 through the
float64 sum formed here), so round_to(dtype)(a64 + b64) is what a correct kernel stores, bit for bit.

Data.  "exact": signed integers times 2^-3, |value| <= 8.  Every partial sum of such values is an integer multiple of 2^-3 below 2^21:
exact in fp32 in any order, so every backward must equal round_to(dtype)(float64 sum) bit for bit.  In fp32 the rounding is the identity;
in bf16 it is not (27 gradients plus a prefill reach 224 = 1792 eighths, 11 bits against bf16's 8), but it is ONE rounding of an exactly
known number, whatever the order of the additions -- the equality holds all the same, as it does for the 105-term sums of the
7x5x3-over-1 pair.  "rounding": seeded normal data, NOT ReLU'd (the pool inputs are drawn around POOL_MEAN = -1.5, so that all-negative windows
occur in every configuration, the 64-element windows of k = 4 included: the clipped windows at the border), with planted bf16 ties (+-(1 + 2^-8),
+-(1 + 3 2^-8)), one fp32 denormal, -0.0, and with inf=True one +inf and one -inf -- only ever in the first operand of a sum, the second is
finite, so no inf - inf arises; gradients hold no infinity.  plant_pairs writes operand pairs into (a, b) at the named positions PAIRS:
a = -b (sum +0.0), -0.0 + -0.0, a positive denormal + 0, and the two sums that land on a rounding tie of the storage type (to even
downwards, to even upwards).  No NaN: outside what these kernels promise.

The bound of a multi-term backward on "rounding" data (u = 2^-24), per element, from the terms t_1 .. t_n that the reference itself
summed (n and sum|t| come out of the reference, not out of the kernel):
    fp32 sum in any fixed order     e32 = g(n - 1) sum|t|,  g(m) = m u / (1 - m u)      (Higham, Accuracy and Stability, (4.4))
    one rounding to the store type  fp32: none (the sum is an fp32);  bf16: 2^-8 (|ref| + e32) + 2^-134 (half the subnormal spacing)
    n <= 1                          0: nothing is added, and a stored value is returned as it was -- equality.
Every bounded assertion is |err| <= k bound, k = allowance(r) = max(1, min(2, 4 r)), r = the largest |err| / bound of torch's fp32 CPU
evaluation of the same case (F.max_pool3d / F.interpolate(mode="nearest") and autograd in float32, the result cast to the store type;
never the kernel).  Measured on the CPU over the cases of the two test files: max pool fp32 r = 1.00 (a two-term sum attains u sum|t|),
bf16 r = 0.996; upsample-add fp32 r = 0.00 - 0.99, bf16 r = 0.45 - 0.996 (the half-ulp line of the final rounding is attained wherever
the mantissa is near 1) -> k = 1.0 where one term or none is summed, 2.0 on nearly every multi-term case.
Mutations the host test shows to land outside (counts of mismatching elements there): 0-padding instead of -inf, "last maximum wins",
the integer-floor index rule, the mask y >= 0."""
import types

import numpy as np
import torch
import torch.nn.functional as Fn

from fcos_ref import F32, F64, U, allowance, check, ratio  # noqa: F401  (re-exported to the two test files)

BF16 = torch.bfloat16
SENTINEL = -12288.0           # exact in bf16
SIG = {F32: 24, BF16: 8}
TIES = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8))
DENORMAL = 1e-40
EXACT_MAX = 8.0


# ======================================================================================================================
# rounding, bits, equality
# ======================================================================================================================
def round_to(dtype):
    """-> f(x64): one round-to-nearest-even of float64 values to ``dtype`` (fp32 / bf16), returned as float64."""
    sig = SIG[dtype]

    def f(x):
        x = np.asarray(x, dtype=np.float64)
        _, ex = np.frexp(np.where(np.isfinite(x), x, 0.0))                  # |x| in [2^(ex - 1), 2^ex)
        ulp = np.ldexp(1.0, np.maximum(ex - 1, -126) - (sig - 1))
        r = np.rint(x / ulp) * ulp                                         # power-of-two scalings are exact; rint rounds to even
        r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, x), r)
        return np.where(np.isfinite(x), r, x)
    return f


def to_torch(x64, dtype):
    """float64 values of ``dtype`` as a torch tensor of that type (exact: the values are representable)."""
    return torch.from_numpy(np.ascontiguousarray(x64, dtype=np.float64)).to(F32).to(dtype)


def bits(t):
    """Integer view for bit comparisons (-0.0 against 0.0, infinities)."""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()])


def check_equal(got, want64, what, dtype=None):
    """``got`` (a tensor of fp32 / bf16 / int8) holds the bits of ``want64`` in its own type."""
    dtype = dtype or got.dtype
    want = torch.from_numpy(np.ascontiguousarray(want64)).to(dtype) if dtype == torch.int8 else to_torch(want64, dtype)
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.numel() == w.numel(), (what, "sizes", g.numel(), w.numel())
    if not torch.equal(g, w):
        bad = (g != w).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError((what, "bits differ at", int(bad.numel()), "of", g.numel(), "first flat index", i, "got",
                              got.detach().cpu().reshape(-1)[i].item(), "want", want.reshape(-1)[i].item()))
    print(f"{what}: bit-equal ({g.numel()} elements)")


# ======================================================================================================================
# data
# ======================================================================================================================
def exact(seed, shape):
    """Signed integers times 2^-3, |value| <= 8 (float64)."""
    return np.random.RandomState(seed).randint(-64, 65, size=shape).astype(np.float64) / 8.0


def rounding(seed, shape, dtype, inf=False, mean=0.0):
    """Seeded normal fp32 data around ``mean`` with the planted values (module docstring), rounded to ``dtype``, as float64."""
    n = int(np.prod(shape))
    a = (np.random.RandomState(seed).standard_normal(n) + mean).astype(np.float32)
    planted = [(7 + 13 * i, v) for i, v in enumerate(TIES)] + [(31, DENORMAL), (11, -0.0)]
    if inf:
        planted += [(43, np.inf), (n - 5, -np.inf)]
    for i, v in planted:
        if 0 <= i < n:
            a[i] = v
    return round_to(dtype)(a.astype(np.float64)).reshape(shape)


def data(kind, seed, shape, dtype, inf=False, mean=0.0):
    return exact(seed, shape) if kind == "exact" else rounding(seed, shape, dtype, inf, mean)


POOL_MEAN = -1.5      # of the pool inputs: 93 % of the values are negative, so the clipped windows at the border are often all-negative


PAIRS = {"cancel": 3, "neg_zero": 5, "denormal": 9, "tie_down": 14, "tie_up": 17}


def plant_pairs(a, b, dtype):
    """Operand pairs at the flat positions PAIRS of (a, b) (in place; arrays of at least 18 elements)."""
    p = SIG[dtype]
    fa, fb = a.reshape(-1), b.reshape(-1)
    fa[PAIRS["cancel"]], fb[PAIRS["cancel"]] = 1.375, -1.375
    fa[PAIRS["neg_zero"]], fb[PAIRS["neg_zero"]] = -0.0, -0.0
    fa[PAIRS["denormal"]], fb[PAIRS["denormal"]] = float(round_to(dtype)(DENORMAL)), 0.0
    fa[PAIRS["tie_down"]], fb[PAIRS["tie_down"]] = 1.0, 2.0 ** -p                       # exactly between 1 and 1 + 2^-(p-1): to even, 1
    fa[PAIRS["tie_up"]], fb[PAIRS["tie_up"]] = 1.0 + 2.0 ** -(p - 1), 2.0 ** -p         # between 1 + 2^-(p-1) and 1 + 2^-(p-2): up
    return a, b


MASKS = {"neg_zero": 3, "pos_zero": 5, "denormal": 9, "negative": 14, "positive": 17}


def plant_mask(y, dtype):
    """The values that decide the ReLU mask at the flat positions MASKS of ``y`` (in place)."""
    f = y.reshape(-1)
    f[MASKS["neg_zero"]], f[MASKS["pos_zero"]], f[MASKS["denormal"]] = -0.0, 0.0, float(round_to(dtype)(DENORMAL))
    f[MASKS["negative"]], f[MASKS["positive"]] = -0.5, 0.5
    return y


# ======================================================================================================================
# the bound
# ======================================================================================================================
def sum_bound(count, mag, ref, dtype):
    """Per-element bound of an fp32 ordered sum of ``count`` terms of total magnitude ``mag`` stored as ``dtype`` (module docstring)."""
    m = np.maximum(count - 1, 0) * U
    e32 = m / (1 - m) * mag
    store = 0.0 if dtype == F32 else 2.0 ** -8 * (np.abs(ref) + e32) + 2.0 ** -134
    return np.where(count <= 1, 0.0, e32 + store)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ======================================================================================================================
# max pool
# ======================================================================================================================
def pool_out(g, k, s, p, ceil):
    num = g + 2 * p - k
    assert num + (s - 1 if ceil else 0) >= 0 and 2 * p <= k      # torch refuses anything else (no output, or padding over half a window)
    o = (-(-num // s) if ceil else num // s) + 1
    if ceil and (o - 1) * s >= g + p:
        o -= 1
    return o


def maxpool_ref(x, k, s, p, ceil, mutate=None):
    """x [N, X, Y, Z, C] -> namespace y, code (int8), o (output grid) and dx(dy64) -> (sum, sum|t|, number of terms) per input element.
    ``mutate``: "zero_pad" (out-of-grid positions are zeros that take part) or "last_wins" (>= instead of >)."""
    n, c = x.shape[0], x.shape[4]
    g = x.shape[1:4]
    o = tuple(pool_out(q, k, s, p, ceil) for q in g)
    size = tuple(max(p + q, (oo - 1) * s + k) for q, oo in zip(g, o))
    inner = (slice(None),) + tuple(slice(p, p + q) for q in g)
    xp = np.full((n,) + size + (c,), 0.0 if mutate == "zero_pad" else -np.inf, dtype=x.dtype)
    xp[inner] = x
    ingrid = np.zeros(size, bool)
    ingrid[inner[1:]] = True
    if mutate == "zero_pad":
        ingrid[:] = True

    def window(a, b, d):
        return (slice(None),) + tuple(slice(t, t + (oo - 1) * s + 1, s) for t, oo in zip((a, b, d), o))

    shape = (n,) + o + (c,)
    best = np.full(shape, -np.inf, dtype=x.dtype)
    code = np.zeros(shape, np.int8)
    taken = np.zeros((1,) + o + (1,), bool)
    for a in range(k):
        for b in range(k):
            for d in range(k):
                w = window(a, b, d)
                cand, inm = xp[w], ingrid[w[1:]][None, ..., None]
                upd = inm & (~taken | ((cand >= best) if mutate == "last_wins" else (cand > best)))
                best = np.where(upd, cand, best)
                code = np.where(upd, np.int8((a * k + b) * k + d), code)
                taken = taken | inm
    assert taken.all(), "a window without an in-grid position"

    def dx(dy):
        acc, mag, cnt = (np.zeros(xp.shape, np.float64) for _ in range(3))
        for a in range(k):
            for b in range(k):
                for d in range(k):
                    w = window(a, b, d)                      # one (a, b, d): a strided view, every element once
                    hit = code == (a * k + b) * k + d
                    acc[w] += np.where(hit, dy, 0.0)
                    mag[w] += np.where(hit, np.abs(dy), 0.0)
                    cnt[w] += hit
        return acc[inner], mag[inner], cnt[inner]

    return types.SimpleNamespace(y=best, code=code, o=o, dx=dx)


def _ncdhw32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(F32).permute(0, 4, 1, 2, 3).contiguous()


def maxpool_dx_torch32(x, dy, k, s, p, ceil, dtype):
    """torch's float32 CPU max_pool3d backward of the same case, cast to ``dtype`` (what the allowance is measured on) -> float64 numpy."""
    xt = _ncdhw32(x).requires_grad_(True)
    Fn.max_pool3d(xt, k, s, p, ceil_mode=bool(ceil)).backward(_ncdhw32(dy))
    return xt.grad.permute(0, 2, 3, 4, 1).to(dtype).double().numpy()


# ======================================================================================================================
# nearest upsample + add
# ======================================================================================================================
def nearest_index(out, inn, rule="fp32"):
    """Source index of every destination index 0 .. out - 1.  "fp32": the rule as stated; "integer": floor(dst in / out) in integers."""
    if rule == "integer":
        return np.minimum(np.arange(out) * inn // out, inn - 1)
    scale = np.float32(inn) / np.float32(out)
    prod = np.arange(out, dtype=np.float32) * scale
    assert prod.dtype == np.float32 and isinstance(scale, np.float32)
    return np.minimum(np.floor(prod).astype(np.int64), inn - 1)


def _indices(fshape, cshape, rule):
    return [nearest_index(f, c, rule) for f, c in zip(fshape[1:4], cshape[1:4])]


def upsample_add_ref(fine, coarse, rule="fp32"):
    """fine + nearest(coarse) in float64, not yet rounded to the store type."""
    ix, iy, iz = _indices(fine.shape, coarse.shape, rule)
    return fine + coarse[:, ix][:, :, iy][:, :, :, iz]


def upsample_add_bwd_ref(d, cshape, prefill=None, rule="fp32"):
    """d [N, fx, fy, fz, C] -> (dcoarse, sum|t|, number of terms) per coarse element; ``prefill`` = the old dcoarse of accumulate = 1
    (one more term), None = accumulate 0."""
    onehot = [(np.arange(c)[:, None] == idx[None, :]).astype(np.float64) for idx, c in zip(_indices(d.shape, cshape, rule), cshape[1:4])]
    acc = np.einsum("xa,yb,zd,nabdc->nxyzc", *onehot, d, optimize=True)
    mag = np.einsum("xa,yb,zd,nabdc->nxyzc", *onehot, np.abs(d), optimize=True)
    cnt = np.einsum("xa,yb,zd->xyz", *onehot)[None, ..., None] * np.ones(acc.shape)
    if prefill is not None:
        acc, mag, cnt = acc + prefill, mag + np.abs(prefill), cnt + 1
    return acc, mag, cnt


def upsample_bwd_torch32(d, cshape, prefill, dtype):
    """torch's float32 CPU backward of F.interpolate(mode="nearest") on the same case (+ the prefill in float32), cast to ``dtype``."""
    n, cx, cy, cz, c = cshape
    ct = torch.zeros((n, c, cx, cy, cz), dtype=F32, requires_grad=True)
    Fn.interpolate(ct, size=tuple(d.shape[1:4]), mode="nearest").backward(_ncdhw32(d))
    g = ct.grad.permute(0, 2, 3, 4, 1)
    if prefill is not None:
        g = g + torch.from_numpy(np.ascontiguousarray(prefill)).to(F32)
    return g.to(dtype).double().numpy()


# ======================================================================================================================
# subsample, joins, layouts
# ======================================================================================================================
def subsample_ref(x, s):
    return x[:, ::s, ::s, ::s]


def subsample_bwd_ref(dy, shape, s):
    dx = np.zeros(shape, np.float64)            # +0 everywhere else
    dx[:, ::s, ::s, ::s] = dy
    return dx


def add_relu_ref(a, b, relu, dtype):
    y = round_to(dtype)(a + b)
    return np.where(y > 0, y, 0.0) if relu else y


def relu_backward_ref(y, dy, mutate=None):
    return np.where((y >= 0) if mutate == "ge" else (y > 0), dy, 0.0)


def to_channels_last_ref(x, dtype):
    """[N, C, V] fp32 values -> [N, V, C] rounded to ``dtype``."""
    return round_to(dtype)(np.transpose(x, (0, 2, 1)))


def to_channels_first_ref(x):
    """[N, V, C] -> [N, C, V] (fp32 holds every bf16 and fp32 value: a pure permutation)."""
    return np.transpose(x, (0, 2, 1))


# ======================================================================================================================
# the cases both test files run
# ======================================================================================================================
POOL_CONFIGS = [(3, 2, 1, 0), (2, 2, 0, 1), (3, 1, 1, 0), (2, 2, 1, 0), (2, 1, 1, 1), (4, 2, 2, 0), (5, 3, 2, 1), (1, 2, 0, 0), (1, 1, 0, 0)]
POOL_GRIDS = [(9, 7, 5), (2, 1, 3)]
UPSAMPLE_PAIRS = [((10, 10, 10), (5, 5, 5)), ((9, 7, 5), (5, 4, 3)), ((46, 3, 2), (14, 2, 1)), ((5, 4, 3), (5, 4, 3)), ((7, 5, 3), (1, 1, 1)),
                  ((3, 2, 2), (7, 5, 3))]
FP32_RULE_PAIRS = [(14, 46), (26, 44), (28, 46), (30, 58)]      # (in, out), in <= out <= 64, where the fp32 rule is not the integer floor
SUBSAMPLE_GRIDS = [(9, 7, 5), (8, 6, 4)]
WIDTHS = [(4, F32), (12, F32), (36, BF16), (8, BF16), (64, BF16)]      # 4 per lane: fp32 and bf16 C = 36; 8 per lane: bf16 C = 8, 64
