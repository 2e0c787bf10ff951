"""float64 reference of the conv3d kernel family on EXACTLY SUMMABLE data (no GPU; used by test_conv_exact_host.py and test_gpu_conv_exact.py).

Why exact families.  The only order-independent bound for a K-term dot product is (K-1) u sum|a||b|; at K = 27 Cin it is far looser than the
tolerances of test_gpu_conv.py, which in turn let a dropped bias or a truncating bf16 store through.  Here the operands are seeded integers
(or integers times a power of two) chosen so that every product and every partial sum, in ANY order and ANY K split, is representable in
fp32: sum|a||b| < 2^24 units for every output element.  A correct kernel then has to EQUAL the float64 result -- bit for bit in fp32, its
single round-to-nearest-even rounding in bf16 -- whatever its tile shape, MFMA order, slice count or epilogue staging.

Reference.  Channels-last rows.  ``Geometry`` lists, per kernel tap, the input row each output row reads (and whether it exists): dense
grids of several scenes, ragged lists of grids laid end to end, the strided 7x7x7 stem, and a subset of output rows.  forward = one float64
matmul [M, Cin] @ [Cin, Cout] per tap (27; 343 for the stem); the same routine on |x|, |w|, |bias| gives the magnitude sum|a||b|.  dx, dw, db
are written from their definitions (correlation with the flipped taps, sum_v x[v + off] (x) gy[v], sum_v gy[v]) -- no autograd.  The
epilogue models bias, ReLU, the ReLU mask of a dgrad, scale/shift of a folded eval BatchNorm (y = acc * scale + shift), fp32 or bf16 storage,
the BatchNorm statistics partials of the STORED outputs, and the bf16x3 mode (x = hi + lo; result = sum(hi hi + hi lo + lo hi), the dropped
lo lo term computed on its own).

Families (``Member.kind``).
  i8    x in [-8, 8], w in [-4, 4] ([-6, 6] where K < 1500; x, w in [-16, 16] for 1x1x1), bias in +-[1, 16], gy in [-8, 8] on 30 % of the
        rows: the bf16 kernels (every operand is a bf16 number)
  st    i8 with amplitudes scaled down (sigma(y) ~ 120) so that sum y_stored^2 over ANY 128 rows of a channel stays < 2^24: the launches
        with fused statistics.  128 y^2 < 2^24 keeps |y| below 362, so few of its outputs need a rounding (0.3 - 1.2 %, all of them ties):
        the rounding mutations are caught on i8, these members catch "statistics from the accumulator" (81 % of the channel sums change)
  f32   a quarter of the x / gy entries and 3 % of w are odd 9-bit integers (257 .. 511): the fp32 kernels -- a path that drops to bf16
        operands is not equal
  x3    512 h + l, h in +-{1, 2}, l in {-1, 0, 1}: 10-11 significant bits, hi = 512 h, lo = l on two thirds of the entries.  The kept terms
        of the split evaluation are multiples of 2^9 below 2^33, hence exact in fp32 (figures below are in units of 2^9).  The FULL product
        of such operands is no fp32 number at K = 27 Cin -- two 9-bit-plus operands leave no room for 1728 terms -- so "mode off == plain
        fp32 evaluation" is asserted on the f32 family instead.
Every member: bias / shift nonzero, scales powers of two in {1/4, 1/2, 2, 4, 8}, shift a multiple of scale (acc * scale + shift needs no more
bits than acc + bias), nonzero inputs on every face of every grid, some pre-activations exactly 0 (f32 / x3: no zero occurs by chance at
their magnitudes, so the bias of channels 0..3 is minus one accumulator of the channel).

Measured on the CPU (test_conv_exact_host.py -s prints these lines for EVERY member; largest sum|a||b| per tensor, all < 2^24 = 1.68e7):

  member              y        dx       dw       db     | bf16 rounds  ties   pre <= 0  pre == 0
  g765_c32_64      1.3e4    1.4e4    3.0e3    6.3e2     |   33.9 %    21.0 %   49.8 %    0.119 %
  g765_c64_96      1.7e4    1.2e4    2.8e3    5.7e2     |   33.6 %    21.3 %   50.2 %    0.067 %
  g555_c128_256    3.4e4    3.3e4    1.0e3    2.0e2     |   43.9 %    22.4 %   49.6 %    0.053 %
  g443_k1_c128_256 1.1e4    1.1e4    1.5e3    1.3e2     |   60.0 %    20.4 %   51.0 %    0.016 %
  rag_c64_128      1.8e4    1.5e4    2.3e3    4.6e2     |   28.7 %    19.6 %   50.3 %    0.129 %     (the lowest rounding share of any i8 member)
  stem_s2_16_14_13 2.1e4      -      1.6e4    3.5e3     |   40.7 %    22.0 %   49.7 %    0.084 %
  g765_f32_c32_64  2.8e6    2.5e6    3.0e6    1.7e4     |      -        -      49.9 %    0.015 %
  stem_f32_s1_9_8_7 3.9e6     -      1.3e7    1.1e5     |      -        -      49.6 %    0.006 %
  x3_g765_c64_96   2.1e6    1.5e6    1.6e5    9.9e4     |  lo lo != 0 on 98.1 % of the outputs; pre == 0 on 0.012 %
  x3_g555_c128_256 7.2e6    1.4e7    7.6e4    3.8e4     |  lo lo != 0 on 98.7 %   (dx: the largest figure of any member, 1.418e7)
  st_gG2_c64_96    1.0e4    4.1e4    1.2e5    3.9e4     |  1.2 % rounded; largest sum of ANY 128 y_stored^2 of a channel 1.65e7 (its partials hold 64 rows)
  the large members (gG*, gH1, gk20, gtail, gw*): bound K max|x| max|w| + max|bias| <= 2.2e5, rows(gy) max|x| max|gy| <= 1.6e6;
  their shares: bf16 rounds 35 - 59 %, ties 20.6 - 22.4 %, pre <= 0 49.8 - 50.2 %, pre == 0 0.04 - 0.09 %

  mutation (smallest share of changed elements over the members it applies to)
  bias dropped 100 % | bias added once per K slice 100 % | last input channel of one tap dropped 31.6 % | last K-step (32 channels) dropped 40.5 %
  dgrad with unflipped taps 93.2 % | zero padding -> wrap-around into the next z-row / y-row / scene 64.0 % | ragged list read as one dense grid 99.9 %
  last partial 256-row tile unwritten 2.0 % (= all of its rows) | bf16 store by truncation 0.29 % (st; >= 14.4 % on i8) | round-half-up 0.31 % (st;
  >= 9.8 % on i8) | K-slice partials rounded to bf16 0.01 % (st; >= 31.4 % on i8) | (acc + shift) * scale 100 % | statistics from the fp32
  accumulator 80.7 % | lo lo included 97.9 % (dw: 91.6 %) | lo terms dropped 99.2 %

Row lists (ROW_CASES; the row-list kernels of the cone head, test_gpu_conv_rows_exact.py).  A list = ascending voxel ids of a member's voxel
space in the device format of csrc/cone.hip (``tap_words``: {voxel id, in-bounds bits of the 27 taps | segment id << 27}); the four sums take
``rows=`` (conv_dw: gy restricted to the listed rows, db their sum).  Lists: ragA = all 314 voxels of the ragged members, ragB = a seeded
half + every corner of every segment (179); cone0 c cone1 c cone2 = the S_0 / S_1 / S_2 of 18 + 20 sampled anchors on the pyramid (10,8,6),
(5,4,3), (3,2,2) x 2 scenes (35 / 483 / 935 of 1104 voxels; the GPU test builds them with the real cone_build and compares); r26 = 16421
seeded voxels of 26^3, r26s the same count over 26^3 + an 8 x 3 x 3 grid, r30 = 24653 of 30 x 30 x 28, w2100 = 2100 of (12,10,9) x 2, r18 = 5200 of
18^3.  The long lists (r26, r26s, r30, r18) evaluate y / dx on 512 seeded rows + every row of the last two tiles, dw / db whole.  Data rules on
top of the families' own (test_row_lists_are_not_vacuous): no list length is a multiple of 32; a listed row reads an unlisted voxel (all
but ragA); listed rows on all six faces of a segment deeper than one voxel; gy nonzero on listed rows of the last partial tile and chunk
(``RowList.gy`` copies a nonzero row there where the seeded 30 % left none) and off the list.  Voxels that no tap of the list reads -- the
GPU test holds NaN there -- exist for the cone lists (56 %, 15 % and 4 % of the voxels at 3x3x3) and for every list at 1x1x1; dy and the ReLU mask hold NaN off every list.

Plans reached (the size / plan queries; asserted without a GPU by test_row_cases_reach_their_plans and again before every GPU launch):
  rag* / cone*, 35 - 935 rows      forward on 4 (Cin 64 bf16) or 9 (Cin 128 bf16, Cin 64 fp32) K slices over all rows; weight gradient on 1 slice
  cone_k1_*, 35 rows               1x1x1 at Cout 256 and at the head's packed widths 128 / 192: never sliced
  gr26_c64_128 / r26, 16421 rows   129 tiles: unsliced, no tail        gr30_c64_256 / r30, 24653 rows: 386 tiles of 128 rows unsliced = 97 tiles of
  gr26(s)_c64_512 / r26(s)         516 tiles: tail split, the last tile (37 rows) on 4 K slices          256 rows with set_rows_big_tile(1)
  gw2_c64_128 / gw2_f32_c64_128 / w2100, 2100 rows   weight gradient on 2 (bf16) and 4 (fp32) slices; forward on 4 / 9 K slices
  gr18_c256_256 / r18, 5200 rows   weight gradient in the 256x256 form (conv_wgrad_big_kernel<ROWS>) on 5 slices; forward on 4 K slices.  Threshold
                                   of that form at Cin = Cout = 256: 5057 rows (80 chunks of 64 rows -> k = 5 slices, 135 tiles = 53 % of a round)

  case (member / list)        y        dx       dw       db          (largest sum|a||b| on the evaluated rows; dw, db over the listed rows, + 8)
  rag_c64_128 / ragA, ragB   1.8e4    1.5e4    2.3e3    4.8e2
  rag_f32_c64_128 / ragA     4.5e6    4.7e6    2.5e6    1.5e4
  rag_x3_c64_128 / ragA        -        -      1.3e5    8.0e4       (units of 2^9; lo lo != 0 on 88.2 % of dw at ragB, the smaller share)
  cone_c64_96 / cone2        1.8e4    1.4e4    6.2e3    1.3e3
  cone_c128_264 / cone2      3.5e4    3.6e4    6.4e3    1.4e3
  cone_k1_c128_{256,128,192} 1.2e4    1.0e4    1.1e3    1.1e2
  gr26_c64_128 / r26         1.8e4    1.9e4      -        -
  gr26(s)_c64_512 / r26(s)   1.8e4    7.9e4      -        -
  gr30_c64_256 / r30         1.8e4    3.7e4      -        -
  gw2_c64_128 / w2100        1.8e4    1.9e4    1.4e4    3.1e3
  gw2_f32_c64_128 / w2100    5.1e6    4.5e6    1.04e7   8.1e4       (the largest figure of a row case)
  gr18_c256_256 / r18        6.8e4    4.2e4    3.1e4    6.9e3
  as members (all rows): y <= 2.2e5, dx <= 4.4e5, dw <= 4.8e5 (gw2_f32_c64_128: y 5.1e6, dw 1.06e7); bf16 rounds 33.9 - 60.1 %, ties 20.4 - 22.2 %

  row-list mutation (smallest share of changed elements over the cases it applies to)
  tap word ignored 14.3 % | segment id of the word ignored 10.2 % | x gathered by list position 96.7 % | y written by list position 6.2 % | ReLU
  mask read by list position 16.0 % | last partial tile unwritten 2.5 % (= all of its rows) | bias once per K slice on the tail rows 100 % | tail
  rows summed without the first slice 99.8 % | without the last slice 78.1 % (r26s; on r26 it CANNOT show: an ascending list over one grid
  ends on the face x = X - 1, where the taps 18..26 -- the whole fourth slice at Cin 64 -- are out of bounds; r26s is there for this) | dW
  over all rows 99.5 % | db over all rows 97.7 %
"""
import numpy as np
import torch

TWO24 = float(2 ** 24)


# ----------------------------------------------------------------------------------------------------------------------
# geometry: which input row every output row reads, per tap
# ----------------------------------------------------------------------------------------------------------------------
class Geometry:
    """segs: [(X, Y, Z)] grids laid end to end (a dense batch of n scenes = n equal segments).  ksize k, padding k // 2, stride s.
    wrap=True (MUTATION): a tap is read wherever its linear row index lands inside the tensor -- the neighbouring z-row, y-row or scene."""

    def __init__(self, segs, ksize=3, stride=1, wrap=False, seg0=False):
        self.segs = [tuple(int(v) for v in s) for s in segs]
        self.k, self.stride, self.pad, self.wrap = ksize, stride, ksize // 2, wrap
        self.seg0 = seg0        # MUTATION (row lists): every row steps with the y / z strides of segment 0; the in-bounds test stays the row's own
        assert not seg0 or stride == 1
        self.osegs = [tuple((g - 1) // stride + 1 for g in s) for s in self.segs]
        self.m_in = sum(x * y * z for x, y, z in self.segs)
        self.m_out = sum(x * y * z for x, y, z in self.osegs)
        co, base, b = [], [], 0
        for (X, Y, Z), (OX, OY, OZ) in zip(self.segs, self.osegs):
            g = np.stack(np.meshgrid(np.arange(OX), np.arange(OY), np.arange(OZ), indexing="ij"), -1).reshape(-1, 3)
            co.append(np.concatenate([g, np.broadcast_to(np.array([X, Y, Z]), g.shape)], 1))
            base.append(np.full(len(g), b))
            b += X * Y * Z
        self.co, self.base = np.concatenate(co).astype(np.int64), np.concatenate(base).astype(np.int64)

    def taps(self):
        k = self.k
        return [(a, b, c) for a in range(k) for b in range(k) for c in range(k)]

    def tap(self, t, rows=None, shift=None):
        """-> (input row index [R], valid [R]) of tap t = (a, b, c) for the output rows ``rows`` (default: all)."""
        co, base = (self.co, self.base) if rows is None else (self.co[rows], self.base[rows])
        i = [co[:, d] * self.stride + t[d] - self.pad for d in range(3)]
        X, Y, Z = co[:, 3], co[:, 4], co[:, 5]
        idx = base + (i[0] * Y + i[1]) * Z + i[2]
        if self.seg0:
            Y0, Z0 = self.segs[0][1], self.segs[0][2]
            idx = base + (co[:, 0] * Y + co[:, 1]) * Z + co[:, 2] + ((t[0] - self.pad) * Y0 + (t[1] - self.pad)) * Z0 + (t[2] - self.pad)
        if self.wrap:
            ok = (idx >= 0) & (idx < self.m_in)
        else:
            ok = (i[0] >= 0) & (i[0] < X) & (i[1] >= 0) & (i[1] < Y) & (i[2] >= 0) & (i[2] < Z)
        if shift is not None:       # MUTATION (row lists): the row's own offset is taken from somewhere else (its list position)
            idx = idx + shift
        if self.seg0 or shift is not None:
            ok = ok & (idx >= 0) & (idx < self.m_in)       # a kernel's buffer bounds: reads outside the tensor give 0
        return torch.from_numpy(np.where(ok, idx, 0)), torch.from_numpy(ok)


# ----------------------------------------------------------------------------------------------------------------------
# the four sums
# ----------------------------------------------------------------------------------------------------------------------
def conv_acc(x, w, geom, rows=None, krange=None, shift=None):
    """x f64 [m_in, Cin], w f64 [Cout, Cin, k, k, k] -> f64 [rows, Cout] = sum over taps of x[row + off] @ w[tap]^T.
    krange = (k0, k1): only the terms k0 <= tap * Cin + ci < k1 of the flattened K axis (one K slice).  shift [rows]: MUTATION, see tap."""
    cin = x.shape[1]
    out = None
    for j, t in enumerate(geom.taps()):
        c0, c1 = 0, cin
        if krange is not None:
            c0, c1 = max(0, krange[0] - j * cin), min(cin, krange[1] - j * cin)
            if c0 >= c1:
                continue
        idx, ok = geom.tap(t, rows, shift)
        part = (x[idx, c0:c1] * ok[:, None]) @ w[:, c0:c1, t[0], t[1], t[2]].t()
        out = part if out is None else out + part
    return out


def flip_t(w):
    """forward weight [Cout, Cin, k, k, k] -> the dgrad's [Cin, Cout, k, k, k] with flipped taps."""
    return w.flip(2, 3, 4).transpose(0, 1).contiguous()


def conv_dx(gy, w, geom, rows=None, flipped=True):
    """dx[u] = sum_{v + off = u} gy[v] w[:, :, off] (stride 1): a correlation of gy with the flipped taps.  flipped=False: MUTATION."""
    assert geom.stride == 1
    return conv_acc(gy, flip_t(w) if flipped else w.transpose(0, 1).contiguous(), geom, rows)


def conv_dw(x, gy, geom, rows=None):
    """dw[co, ci, tap] = sum_v x[v + off] (x) gy[v]; db = sum_v gy[v].  rows: the sums run over these rows only (a row list)."""
    k = geom.k
    if rows is not None:
        listed = torch.zeros_like(gy)
        listed[rows] = gy[rows]
        gy = listed
    dw = torch.zeros(gy.shape[1], x.shape[1], k, k, k, dtype=torch.float64)
    rows = (gy != 0).any(1).nonzero().reshape(-1).numpy()          # rows with a zero gradient add nothing
    g = gy[rows].t().contiguous()
    for t in geom.taps():
        idx, ok = geom.tap(t, rows)
        dw[:, :, t[0], t[1], t[2]] = g @ (x[idx] * ok[:, None])
    return dw, gy.sum(0)


# ----------------------------------------------------------------------------------------------------------------------
# storage and epilogue
# ----------------------------------------------------------------------------------------------------------------------
def _bits(v):
    f = v.float()
    assert torch.equal(f.double(), v), "value is not an fp32 number: the family violates exact_ok"
    return f.contiguous().view(torch.int32)


def store(v, dtype, how="rne"):
    """f64 exact value -> f64 value of what a kernel stores.  how: 'rne' (correct), 'trunc', 'half_up' (MUTATIONS; magnitude-wise)."""
    if dtype == torch.float32:
        _bits(v)
        return v.clone()
    if how == "rne":
        _bits(v)
        return v.float().bfloat16().double()
    b = _bits(v)
    b = (b & -65536) if how == "trunc" else ((b + 0x8000) & -65536)
    return b.view(torch.float32).double()


def epilogue(acc, bias=None, scale=None, relu=False, mask=None, swapped=False, bias_times=1):
    """y = acc * scale + bias (bias = the fold's shift when scale is given), ReLU, dgrad mask (0 where the saved activation <= 0).
    swapped: MUTATION (acc + shift) * scale; bias_times: MUTATION bias added once per K slice."""
    y = acc
    if swapped:
        y = (y + bias) * scale
    else:
        if scale is not None:
            y = y * scale
        if bias is not None:
            y = y + bias * bias_times
    if relu:
        y = y.clamp_min(0.0)
    if mask is not None:
        y = torch.where(mask > 0, y, torch.zeros_like(y))
    return y


def stats_partials(y_stored, group, partials=None):
    """[M, C] stored outputs -> [P, 2, C]: (sum, sum of squares) of each group of ``group`` consecutive rows; P = ceil(M / group), or
    ``partials`` where the kernel's last tile carries groups past the end (all zero)."""
    m, c = y_stored.shape
    p = max(-(-m // group), partials or 0)
    pad = torch.zeros(p * group, c, dtype=torch.float64)
    pad[:m] = y_stored
    g = pad.view(p, group, c)
    return torch.stack([g.sum(1), (g * g).sum(1)], 1)


def halo_partials(y_stored, n, grid):
    """Statistics partials of the halo form: [2 * blocks, 2, C], blocks = the 4 x 8 x 8 voxel blocks of every scene in (scene, bx, by, bz)
    order; partial 2 b + h = (sum, sum of squares) over the voxels of block b in its x-planes [2 h, 2 h + 2) that lie inside the grid."""
    X, Y, Z = grid
    c = y_stored.shape[1]
    v = y_stored.view(n, X, Y, Z, c)
    tx, ty, tz = -(-X // 4), -(-Y // 8), -(-Z // 8)
    pad = torch.zeros(n, tx * 4, ty * 8, tz * 8, c, dtype=torch.float64)
    pad[:, :X, :Y, :Z] = v
    g = pad.view(n, tx, 2, 2, ty, 8, tz, 8, c).permute(0, 1, 4, 6, 2, 3, 5, 7, 8).reshape(n * tx * ty * tz * 2, 128, c)
    return torch.stack([g.sum(1), (g * g).sum(1)], 1)


def stats_exact_ok(y_stored, group=128):
    """sum y^2 over ANY ``group`` rows of a channel < 2^24 (the ``group`` largest squares): every partial a kernel can form over at most
    that many rows is an exact fp32 sum, whatever rows it groups."""
    sq = (y_stored * y_stored)
    top = sq.topk(min(group, sq.shape[0]), dim=0).values.sum(0)
    return top.max().item()


def split(v):
    """fp32-valued f64 tensor -> (hi, lo) f64: hi = bf16(v), lo = bf16(v - hi)."""
    hi = v.float().bfloat16().float()
    lo = (v.float() - hi).bfloat16().float()
    return hi.double(), lo.double()


def x3_terms(a, b, fn):
    """bf16x3 evaluation of the bilinear ``fn(a, b)``: -> (kept = hi hi + hi lo + lo hi, dropped = lo lo)."""
    ah, al = split(a)
    bh, bl = split(b)
    return fn(ah, bh) + fn(ah, bl) + fn(al, bh), fn(al, bl)


# ----------------------------------------------------------------------------------------------------------------------
# exact families
# ----------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, lo, hi, nonzero=False):
    v = torch.randint(lo, hi + 1, shape, generator=g).double()
    if nonzero:
        v = torch.where(v == 0, torch.full_like(v, float(hi)), v)
    return v


def _big(g, shape, share):
    """odd 9-bit integers +-(257 .. 511) on ``share`` of the entries, 0 elsewhere."""
    mag = torch.randint(128, 256, shape, generator=g).double() * 2 + 1
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    return mag * sign * (torch.rand(shape, generator=g) < share)


def _x3(g, shape, scale_only=False):
    h = (torch.randint(1, 3, shape, generator=g).double()) * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)
    l = torch.randint(-1, 2, shape, generator=g).double()
    return 512.0 * h + (0.0 if scale_only else l)


class Member:
    """One seeded member: x [m_in, Cin], w [Cout, Cin, k, k, k], bias / scale / shift [Cout], gy [m_out, Cout] (all f64, fp32-exact)."""

    def __init__(self, name, kind, segs, cin, cout, ksize=3, stride=1, n=None, gy_density=0.3, seed=0):
        self.name, self.kind, self.cin, self.cout, self.k, self.stride = name, kind, cin, cout, ksize, stride
        if n is not None:                       # dense batch
            self.n, self.grid, self.ragged = n, tuple(segs), False
            segs = [tuple(segs)] * n
        else:
            self.n, self.grid, self.ragged = 1, None, True
        self.geom = Geometry(segs, ksize, stride)
        g = torch.Generator().manual_seed(1000 + seed + 7 * cin + cout + self.geom.m_in)
        mi, mo, K = self.geom.m_in, self.geom.m_out, ksize ** 3 * cin
        wshape = (cout, cin, ksize, ksize, ksize)
        rows_on = (torch.rand(mo, 1, generator=g) < gy_density).double()
        if kind in ("i8", "st"):
            ax, aw = 8, (6 if K < 1500 else 4)       # short K: wider weights, so that enough outputs pass 2^8 and need a bf16 rounding
            if K < 200:                              # 1x1x1: K = Cin
                ax = aw = 16
            if kind == "st":      # sigma(y)^2 = K E[x^2] E[w^2] ~ 120^2, so that the 128 largest y^2 of a channel sum below 2^24
                aw = 2
                ax = max(1, int((3 * 120.0 ** 2 / (2.0 * K)) ** 0.5))
            self.x, self.w = _ints(g, (mi, cin), -ax, ax), _ints(g, wshape, -aw, aw)
            self.bias = _ints(g, (cout,), -16, 16, True)
            self.gy = _ints(g, (mo, cout), -8, 8) * rows_on
            self.unit = 1.0
        elif kind == "f32":
            self.x = torch.where((b := _big(g, (mi, cin), 0.25)) != 0, b, _ints(g, (mi, cin), -8, 8))
            self.w = torch.where((b := _big(g, wshape, 0.03)) != 0, b, _ints(g, wshape, -4, 4))
            self.bias = _big(g, (cout,), 1.1)
            self.gy = torch.where((b := _big(g, (mo, cout), 0.25)) != 0, b, _ints(g, (mo, cout), -8, 8)) * rows_on
            self.unit = 1.0
        elif kind == "x3":
            self.x, self.w = _x3(g, (mi, cin)), _x3(g, wshape)
            self.bias = _x3(g, (cout,), True)
            self.gy = _x3(g, (mo, cout)) * rows_on
            self.unit = 512.0       # every kept term of the split evaluation is a multiple of 2^9
        else:
            raise ValueError(kind)
        if kind in ("f32", "x3"):
            # at these magnitudes no pre-activation is 0 by chance: the bias of channels 0..3 is set to minus one accumulator of the channel, so
            # that each of them has an exact zero at the ReLU (still a nonzero fp32 integer / multiple of 2^9)
            rows = np.array([(7 + 97 * c) % mo for c in range(4)])
            fn = lambda a, b: conv_acc(a, b, self.geom, rows)
            a0 = x3_terms(self.x, self.w, fn)[0] if kind == "x3" else fn(self.x, self.w)
            for c in range(4):
                if a0[c, c] != 0:
                    self.bias[c] = -a0[c, c]
        e = torch.randint(-2, 3, (cout,), generator=g).double()
        self.scale = 2.0 ** torch.where(e == 0, torch.full_like(e, 3.0), e)          # powers of two other than 1
        # a multiple of scale * unit, the lowest bit of acc * scale: acc * scale + shift then needs no more bits than acc + bias
        self.shift = _ints(g, (cout,), -16, 16, True) * self.scale.clamp_min(1.0) * self.unit

    # ---- reference results (f64, exact) ----
    def acc(self, rows=None, geom=None, w=None, krange=None):
        return conv_acc(self.x, self.w if w is None else w, geom or self.geom, rows, krange)

    def pre(self, rows=None, fold=False, **kw):
        return epilogue(self.acc(rows, **kw), self.shift if fold else self.bias, self.scale if fold else None)

    def magnitude(self, rows=None, fold=False):
        m = conv_acc(self.x.abs(), self.w.abs(), self.geom, rows)
        return (m * self.scale.abs() + self.shift.abs()) if fold else (m + self.bias.abs())

    def bound(self):
        """Cheap rigorous bound of sum|a||b| for the members too large to evaluate on the host: K max|x| max|w| + max|bias|."""
        K = self.k ** 3 * self.cin
        return K * self.x.abs().max().item() * self.w.abs().max().item() + self.bias.abs().max().item()

    def reference(self, relu, dtype, x3=False, geom=None):
        """What conv(+ReLU) and its backward from ``gy`` must give with ``dtype`` activations: dict of f64 tensors -- pre (exact
        pre-activation), y, dx (as stored), dw, db (fp32 sums), and for x3 the dropped lo lo parts (y_lolo, dx_lolo, dw_lolo)."""
        key = ("ref", relu, dtype, x3, id(geom))
        if key in _CACHE.setdefault(self.name + "/ref", {}):
            return _CACHE[self.name + "/ref"][key]
        geom = geom or self.geom
        r = {}
        if x3:
            acc, r["y_lolo"] = x3_terms(self.x, self.w, lambda a, b: conv_acc(a, b, geom))
        else:
            acc = conv_acc(self.x, self.w, geom)
        r["pre"] = acc + self.bias
        r["y"] = store(epilogue(r["pre"], relu=relu), dtype)
        gy = self.gy * (r["y"] > 0) if relu else self.gy
        r["db"] = gy.sum(0)
        if x3:
            if self.stride == 1:
                dx, r["dx_lolo"] = x3_terms(gy, self.w, lambda a, b: conv_dx(a, b, geom))
                r["dx"] = dx
            r["dw"], r["dw_lolo"] = x3_terms(self.x, gy, lambda a, b: conv_dw(a, b, geom)[0])
        else:
            if self.stride == 1:
                r["dx"] = store(conv_dx(gy, self.w, geom), dtype)
            r["dw"] = conv_dw(self.x, gy, geom)[0]
        _CACHE[self.name + "/ref"][key] = r
        return r

    def nchw(self, t2d, out=True):
        """rows [M, C] -> [N, X, Y, Z, C] of a dense member."""
        g = self.geom.osegs[0] if out else self.geom.segs[0]
        return t2d.view(self.n, *g, t2d.shape[1])


def members():
    """name -> constructor arguments of every member (built lazily: the large ones are only built where they are used)."""
    R = [(6, 5, 4), (3, 3, 2), (9, 2, 1), (1, 1, 1)]
    spec = {}

    def add(name, kind, segs, cin, cout, **kw):
        spec[name] = (name, kind, segs, cin, cout, kw)
    G = (24, 20, 17)                  # 8160 voxels: x 2 scenes = 127 whole 128-row tiles + 64 rows, enough tiles for the unsliced kernels
    for kind in ("i8", "st"):
        p = "" if kind == "i8" else "st_"
        add(p + "g765_c32_64", kind, (7, 6, 5), 32, 64, n=2)
        add(p + "g765_c64_96", kind, (7, 6, 5), 64, 96, n=2)
        add(p + "gG2_c64_96", kind, G, 64, 96, n=2)
        add(p + "gG1_c64_256", kind, G, 64, 256, n=1)
        add(p + "g59a_c96_256", kind, (5, 9, 10), 96, 256, n=2)
        add(p + "g59a_c128_264", kind, (5, 9, 10), 128, 264, n=2)
    add("gG2_c32_64", "i8", G, 32, 64, n=2)
    add("gG1_c256_256", "i8", G, 256, 256, n=1)                 # forward AND dgrad on the 256x256 tiles
    add("g59a_c256_256", "i8", (5, 9, 10), 256, 256, n=2)       # forward AND dgrad in the halo form
    add("gH1_c64_264", "i8", (20, 17, 16), 64, 264, n=1)
    add("g987_c64_256", "i8", (9, 8, 7), 64, 256, n=1)          # 504 rows: K-sliced whatever tile is asked for
    add("g987_c64_264", "i8", (9, 8, 7), 64, 264, n=1)
    add("g555_c128_256", "i8", (5, 5, 5), 128, 256, n=1)
    add("gk20_c128_512", "i8", (20, 20, 16), 128, 512, n=1)
    add("gtail_c64_256", "i8", (50, 50, 33), 64, 256, n=1)
    add("g443_k1_c128_256", "i8", (4, 4, 3), 128, 256, n=1, ksize=1)
    add("g443_k1_c32_64", "i8", (4, 4, 3), 32, 64, n=1, ksize=1)
    add("rag_c64_128", "i8", [g for g in R for _ in range(2)], 64, 128)
    add("rag_f32_c64_128", "f32", [g for g in R for _ in range(2)], 64, 128)
    add("rag_x3_c64_128", "x3", [g for g in R for _ in range(2)], 64, 128)
    add("g765_f32_c16_32", "f32", (7, 6, 5), 16, 32, n=2)
    add("g765_f32_c32_64", "f32", (7, 6, 5), 32, 64, n=2)
    add("gG2_f32_c16_32", "f32", G, 16, 32, n=2, gy_density=0.05)       # 16320 rows: a sparser gy keeps sum|x||gy| of dw below 2^24
    add("gG2_f32_c32_64", "f32", G, 32, 64, n=2, gy_density=0.05)
    add("gw2_c32_64", "i8", (12, 10, 9), 32, 64, n=2)
    add("gw2_c64_128", "i8", (12, 10, 9), 64, 128, n=2)
    add("gw2_f32_c32_64", "f32", (12, 10, 9), 32, 64, n=2)
    add("gw_c256_512", "i8", (16, 14, 14), 256, 512, n=1)
    add("gw_c128_256", "i8", (24, 22, 20), 128, 256, n=1)
    add("gw2_k1_c64_96", "i8", (12, 10, 9), 64, 96, n=2, ksize=1)
    for kind in ("i8", "f32"):
        p = "stem_" if kind == "i8" else "stem_f32_"
        add(p + "s1_9_8_7", kind, (9, 8, 7), 4, 64, n=2, ksize=7, stride=1, gy_density=1.0)
        add(p + "s2_16_14_13", kind, (16, 14, 13), 4, 64, n=2, ksize=7, stride=2, gy_density=1.0)
        add(p + "s2_18_15_12", kind, (18, 15, 12), 4, 64, n=2, ksize=7, stride=2, gy_density=1.0)
    add("stem_s2_34_26_20", "i8", (34, 26, 20), 4, 64, n=2, ksize=7, stride=2, gy_density=1.0)
    add("x3_g555_c128_256", "x3", (5, 5, 5), 128, 256, n=1)
    add("x3_g765_c64_96", "x3", (7, 6, 5), 64, 96, n=2)
    # members of the row-list kernels (ROW_CASES below): the cone pyramid of test_gpu_cone.py as one ragged space, and single grids long
    # enough for the unsliced, tail-split, 256-row-tile and 256x256 weight-gradient plans
    cone = [g for g in CONE_GRIDS for _ in range(CONE_SCENES)]
    add("cone_c64_96", "i8", cone, 64, 96)
    add("cone_c128_264", "i8", cone, 128, 264)
    add("cone_k1_c128_256", "i8", cone, 128, 256, ksize=1)
    for width in HEAD_WIDTHS:
        add(f"cone_k1_c128_{width}", "i8", cone, 128, width, ksize=1)
    add("gr26_c64_128", "i8", (26, 26, 26), 64, 128, n=1)
    add("gr26_c64_512", "i8", (26, 26, 26), 64, 512, n=1)
    # the last rows of an ascending list over ONE grid lie on its face x = X - 1, where the taps 18..26 (the whole last K slice of a tail
    # split at Cin 64) are out of bounds: a small second grid puts rows with every tap in bounds into the tail
    add("gr26s_c64_512", "i8", [(26, 26, 26), (8, 3, 3)], 64, 512)
    add("gr30_c64_256", "i8", (30, 30, 28), 64, 256, n=1)
    add("gw2_f32_c64_128", "f32", (12, 10, 9), 64, 128, n=2)
    add("gr18_c256_256", "i8", (18, 18, 18), 256, 256, n=1)
    return spec


CONE_GRIDS, CONE_SCENES, CONE_ANCHORS = [(10, 8, 6), (5, 4, 3), (3, 2, 2)], 2, 13
# ((anchors * (1 + delta width) + 63) // 64) * 64 for 13 / 15 anchors with 6- and 8-wide deltas: 91, 117, 105 -> 128; 135 -> 192.  The GPU test
# asks RPNHead for these widths and compares.
HEAD_WIDTHS = (128, 192)


_SPEC = members()
_CACHE = {}
# members small enough for the full host treatment (anchors, measured magnitude, every mutation)
HOST_FULL = ["g765_c32_64", "g765_c64_96", "st_g765_c64_96", "g555_c128_256", "g443_k1_c128_256", "rag_c64_128", "rag_f32_c64_128", "rag_x3_c64_128",
             "g765_f32_c16_32", "g765_f32_c32_64", "gw2_k1_c64_96", "stem_s1_9_8_7", "stem_s2_16_14_13", "stem_f32_s2_16_14_13", "x3_g765_c64_96",
             "cone_c64_96", "cone_k1_c128_192"]


def names():
    return list(_SPEC)


def get(name):
    if name not in _CACHE:
        n, kind, segs, cin, cout, kw = _SPEC[name]
        _CACHE[name] = Member(n, kind, segs, cin, cout, **kw)
    return _CACHE[name]


def first_diff(a, b):
    """Message for a failed torch.equal: first differing flat index and both values."""
    if a.shape != b.shape:
        return f"shapes {tuple(a.shape)} != {tuple(b.shape)}"
    d = (a != b).reshape(-1).nonzero()
    if d.numel() == 0:
        return "equal"
    i = int(d[0])
    return f"{d.numel()} of {a.numel()} differ; first at flat index {i}: got {a.reshape(-1)[i].item()!r}, want {b.reshape(-1)[i].item()!r}"


# ----------------------------------------------------------------------------------------------------------------------
# row lists: the device list format of csrc/cone.hip and the cases of the row-list kernels
# ----------------------------------------------------------------------------------------------------------------------
def tap_words(segs, ids):
    """(segments laid end to end, ascending voxel ids of that space) -> uint32 [n, 2] = {voxel id, tap word}: bit t of the word says that the
    neighbour (dx, dy, dz) = (t / 9 - 1, (t / 3) % 3 - 1, t % 3 - 1) lies inside the voxel's own segment, bits 27.. hold the segment id.  Bit 13
    (the voxel itself) is therefore always set."""
    dims = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
    first = np.concatenate([[0], np.cumsum(dims.prod(1))])
    ids = np.asarray(ids, dtype=np.int64)
    assert ids.ndim == 1 and (np.diff(ids) > 0).all() and ids[0] >= 0 and ids[-1] < first[-1] and len(dims) <= 16
    seg = np.searchsorted(first, ids, side="right") - 1
    local, d = ids - first[seg], dims[seg]
    pos = np.stack([local // (d[:, 1] * d[:, 2]), local // d[:, 2] % d[:, 1], local % d[:, 2]], 1)
    word = seg.astype(np.uint32) << np.uint32(27)
    for t in range(27):
        q = pos + np.array([t // 9 - 1, t // 3 % 3 - 1, t % 3 - 1])
        word |= ((q >= 0) & (q < d)).all(1).astype(np.uint32) << np.uint32(t)
    assert ((word >> np.uint32(13)) & 1).all()
    return np.stack([ids.astype(np.uint32), word], 1)


class RowList:
    """One list over the voxel space ``segs``: ``ids`` ascending voxel ids (= output rows of a stride-1 geometry), ``words`` their device
    format, ``ev`` the list POSITIONS on which the forward / dgrad reference is evaluated (all of them unless the list is long), ``tile``
    the row tile whose last partial tile the vacuity checks look at."""

    def __init__(self, name, segs, ids, ev=None, tile=128):
        self.name, self.segs, self.tile = name, [tuple(s) for s in segs], tile
        self.ids = np.asarray(ids, dtype=np.int64)
        self.n = len(self.ids)
        self.words = tap_words(self.segs, self.ids)
        self.ev = np.arange(self.n) if ev is None else np.asarray(ev, dtype=np.int64)
        self.total = sum(x * y * z for x, y, z in self.segs)
        self.whole = self.n == self.total           # every voxel listed: position == voxel id

    def listed(self):
        m = np.zeros(self.total, dtype=bool)
        m[self.ids] = True
        return m

    def reads(self, ksize=3):
        """bool [total]: the voxels some in-bounds tap of a listed row reads (1x1x1: the listed voxels)."""
        m = self.listed()
        if ksize == 3:
            g = Geometry(self.segs)
            for t in g.taps():
                idx, ok = g.tap(t, self.ids)
                m[idx.numpy()[ok.numpy()]] = True
        return m

    def vox(self):
        """voxel ids of the evaluated positions"""
        return self.ids[self.ev]

    def gy(self, m):
        """m.gy with a nonzero row (a copy of a nonzero row of the member: the family's number format) on the first and last listed row of
        the list's last partial tile and last partial 64- and 32-row chunk, should the member's seeded 30 % have left them zero."""
        gy = m.gy.clone()
        src = m.gy[(m.gy != 0).any(1)]
        for j, p in enumerate(sorted({self.n - 1, self.n // self.tile * self.tile, self.n // 128 * 128, self.n // 64 * 64, self.n // 32 * 32} - {self.n})):
            if not (gy[self.ids[p]] != 0).any():
                gy[self.ids[p]] = src[j % len(src)]
        return gy


def _seeded_ids(total, n, seed):
    return np.sort(np.random.default_rng(seed).permutation(total)[:n])


def _long_ev(n, tile, seed):
    """512 seeded positions before the last two tiles + every position of the last two tiles."""
    t0 = (-(-n // tile) - 2) * tile
    return np.concatenate([_seeded_ids(t0, 512, seed), np.arange(t0, n)])


def cone_sample(seed=5, kp=8, kn=10):
    """Sampled anchor indices of the cone cases: per scene, (positives, negatives) drawn without replacement from one scene's flat
    (level, x, y, z, anchor) order -- the draw of tests/test_gpu_cone.py with fewer anchors, so that S_2 (935 of the 1104 voxels; 35 and 483
    in S_0 and S_1) stays a proper subset: every list then has unlisted neighbours, and voxels that no tap of S_0 or S_1 reads."""
    rng = np.random.default_rng(seed)
    T = sum(g[0] * g[1] * g[2] for g in CONE_GRIDS) * CONE_ANCHORS
    pos = [np.sort(rng.choice(T, size=kp - 3 * i, replace=False)).astype(np.int64) for i in range(CONE_SCENES)]
    neg = [np.sort(rng.choice(T, size=kn + 2 * i, replace=False)).astype(np.int64) for i in range(CONE_SCENES)]
    return pos, neg


def cone_sets(pos, neg, depth=2):
    """S_0 c S_1 c ... of the sample: S_0 = the voxels that hold a sampled anchor, S_{k+1} = S_k and its 26 neighbours inside the same grid;
    ascending ids of the ragged (level-major, scene-major) space of the cone members."""
    segs = [g for g in CONE_GRIDS for _ in range(CONE_SCENES)]
    first = np.concatenate([[0], np.cumsum([x * y * z for x, y, z in segs])])
    on = np.zeros(first[-1], dtype=bool)
    for s in range(CONE_SCENES):
        a, lvl0 = np.concatenate([pos[s], neg[s]]), 0
        for l, g in enumerate(CONE_GRIDS):
            cells = g[0] * g[1] * g[2]
            here = a[(a >= lvl0) & (a < lvl0 + cells * CONE_ANCHORS)] - lvl0
            on[first[l * CONE_SCENES + s] + here // CONE_ANCHORS] = True
            lvl0 += cells * CONE_ANCHORS
    out, geom = [np.flatnonzero(on)], Geometry(segs)
    for _ in range(depth):
        ids = out[-1]
        for t in geom.taps():
            idx, ok = geom.tap(t, ids)
            on[idx.numpy()[ok.numpy()]] = True
        out.append(np.flatnonzero(on))
    return out


RAG_SEGS = [g for g in [(6, 5, 4), (3, 3, 2), (9, 2, 1), (1, 1, 1)] for _ in range(2)]
_LISTS = {}


def row_list(name):
    """The lists of ROW_CASES, built on first use."""
    if name in _LISTS:
        return _LISTS[name]
    if name.startswith("cone"):
        segs = [g for g in CONE_GRIDS for _ in range(CONE_SCENES)]
        for k, ids in enumerate(cone_sets(*cone_sample())):
            _LISTS[f"cone{k}"] = RowList(f"cone{k}", segs, ids)
    elif name == "ragA":            # every voxel: 2 whole tiles + 58 rows
        _LISTS[name] = RowList(name, RAG_SEGS, np.arange(314))
    elif name == "ragB":            # a seeded half + every corner voxel of every segment
        first, corners = 0, []
        for X, Y, Z in RAG_SEGS:
            corners += [first + (x * Y + y) * Z + z for x in (0, X - 1) for y in (0, Y - 1) for z in (0, Z - 1)]
            first += X * Y * Z
        _LISTS[name] = RowList(name, RAG_SEGS, np.union1d(_seeded_ids(314, 157, 314), corners))
    elif name == "r26":             # 128 whole tiles + 37 rows
        _LISTS[name] = RowList(name, [(26, 26, 26)], _seeded_ids(26 ** 3, 16421, 16421), _long_ev(16421, 128, 1))
    elif name == "r26s":            # the same count over 26^3 + an 8 x 3 x 3 grid: the 37 tail rows lie in the small grid
        _LISTS[name] = RowList(name, [(26, 26, 26), (8, 3, 3)], _seeded_ids(26 ** 3 + 72, 16421, 16422), _long_ev(16421, 128, 1))
    elif name == "r30":             # 96 whole tiles of 256 rows + 77 rows
        _LISTS[name] = RowList(name, [(30, 30, 28)], _seeded_ids(25200, 24653, 24653), _long_ev(24653, 256, 2), tile=256)
    elif name == "r18":             # 81 whole 64-row chunks + 16 rows
        _LISTS[name] = RowList(name, [(18, 18, 18)], _seeded_ids(18 ** 3, 5200, 5200), _long_ev(5200, 128, 3))
    elif name == "w2100":           # 32 whole 64-row chunks + 52 rows
        _LISTS[name] = RowList(name, [(12, 10, 9)] * 2, _seeded_ids(2160, 2100, 2100))
    else:
        raise KeyError(name)
    return _LISTS[name]


# (member, list, forward / dgrad launches run, weight gradient run).  The forward plan of each case is asserted by both test files through
# rows_plan_class; the dgrad swaps Cin and Cout and is run where Cout is a legal Cin (Cout * elemsize a multiple of 128 bytes).
ROW_CASES = (
    [(m, l, True, True) for m in ("rag_c64_128", "rag_f32_c64_128") for l in ("ragA", "ragB")]
    + [("rag_x3_c64_128", l, False, True) for l in ("ragA", "ragB")]                  # the bf16x3 weight gradient only
    + [(m, l, True, True) for m in ("cone_c64_96", "cone_c128_264") for l in ("cone0", "cone1", "cone2")]
    + [(m, "cone0", True, True) for m in ("cone_k1_c128_256", "cone_k1_c128_128", "cone_k1_c128_192")]
    + [("gr26_c64_128", "r26", True, False), ("gr26_c64_512", "r26", True, False), ("gr26s_c64_512", "r26s", True, False), ("gr30_c64_256", "r30", True, False)]
    + [("gw2_c64_128", "w2100", True, True), ("gw2_f32_c64_128", "w2100", True, True), ("gr18_c256_256", "r18", True, True)])


# plan every case must reach, forward and (where Cout is a legal Cin) dgrad: ("unsliced",), ("ksplit",) on any slice count >= 2, ("tail", ks)
ROW_PLANS = {"gr26_c64_128-r26": (("unsliced",), ("unsliced",)), "gr26_c64_512-r26": (("tail", 4), ("unsliced",)),
             "gr26s_c64_512-r26s": (("tail", 4), ("unsliced",)),
             "gr30_c64_256-r30": (("unsliced",), ("unsliced",)), "cone_k1_c128_256-cone0": (("unsliced",), ("unsliced",)),
             "cone_k1_c128_128-cone0": (("unsliced",), ("unsliced",)), "cone_k1_c128_192-cone0": (("unsliced",), ("unsliced",))}


def rows_plan_class(ws_bytes, nrows, cout):
    """Workspace bytes of the row-list forward -> ("unsliced",), ("ksplit", slices) or ("tail", ks, first tail tile of 128 rows)."""
    per = nrows * cout * 4
    if ws_bytes == 0:
        return ("unsliced",)
    if ws_bytes % per == 0:
        return ("ksplit", ws_bytes // per)
    assert ws_bytes < per, (ws_bytes, per)
    for tile0 in range(nrows // 128, -1, -1):          # the shortest tail first
        part = (nrows - tile0 * 128) * cout * 4
        if ws_bytes % part == 0 and ws_bytes // part >= 2:
            return ("tail", ws_bytes // part, tile0)
    raise AssertionError(f"{ws_bytes} bytes are no K-slice or tail-split workspace of {nrows} x {cout}")
