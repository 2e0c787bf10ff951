"""float64 references of the seven FCOS kernels of csrc/fcos.hip (head epilogue forward / backward, GT summary, target assignment, focal
loss, candidate scores, candidate decode) with per-element error bounds built from float64 magnitudes; the same expressions evaluated in
torch fp32 on the CPU (what the allowance k is measured on), with the mutations the bounds have to catch; the seeded input families shared
by tests/test_fcos_bounds_host.py (no GPU) and tests/test_gpu_fcos_kernels.py.

Bounds (u = 2^-24, fp32 round to nearest; every bound also holds an absolute floor ETA = 2^-126 for results below the normal range):

    kernel / output            reference                              bound
    focal term, dloss/dlogit   closed form in fp64 (anchored to        first order through the kernel's intermediates: dp = 4u p,
                               autograd of oracle focal_loss_sum)      dq = 4u p + 2u q (q is FORMED as 1 - p: at logit +16.6 the absolute
                                                                       error of p is 7e7 u q), dlog = 4u |log|, + 8u |value| for the rest
    focal sum, d_scale         fp64 sum                                sum of the per-term bounds + depth u sum|term|, depth = adds per
                                                                       thread + 8 (LDS tree) + ceil(blocks / 256) + 8 (ticket holder's tree)
    head, norm_reg branch      torch fp32, the kernel's order          equality: max(raw sc, 0) stride and (dv stride) sc are correctly
                                                                       rounded operations (the unit is built with -ffp-contract=off)
    head, expf branch          fp64                                    4u |value| (per d_scale term too; 2u per term on the norm_reg branch)
    GT summary, AABB           the box itself                          equality
    GT summary, OBB            oracle obb_summary in fp64              footprint: 4u Mc; alpha, beta: 8u Mc / extent, Mc = max |corner coord.|
    targets                    oracle targets_for_scene in fp64        equality (labels and regression targets: quarter-grid coordinates,
                                                                       on which fp32 and fp64 agree exactly)
    scores                     sigmoid sigmoid in fp64                 8u value; the candidate mask is exact (fixture: no sigmoid within
                                                                       4u of the threshold)
    decode, AABB               clip in fp64 on quarter-grid inputs     equality, sqrt(score): 2u value, keep rule exact
    decode, OBB                oracle decode_obb in fp64               centre, height: 16u M (Mz = M + max|z| for cz and the height);
                                                                       width, length: 16u M amp; angle: 16u M amp / (width / 2) modulo 2 pi,
                                                                       M = max(|x0|, |x1|, |y0|, |y1|) + max(|a|, |b|) max(x1 - x0, y1 - y0),
                                                                       amp = 1 + dmax / (min(d0, d1) + 1e-7)

An OBB row is *vacuous* for width / length / angle where amp > 1e3, and for the angle alone where its bound exceeds 0.1 rad; its centre,
height, level and finiteness are still checked.  The keep decision of an OBB row is asserted where every size is further from min_size
than its bound.

Every assertion is |err| <= k * bound, k = max(1, min(2, 4 r)) with r the largest |err| / bound of the torch fp32 CPU evaluation of the
same case (never of the kernel); the cap of 2 keeps the allowance from hiding a real error.  r as measured on the CPU (host test):
    focal term / gradient 0.37 / 0.46 (label 1; label 0: 0.31 / 0.32), focal sum <= 0.04; head expf forward / d_box_out / d_scale
    0.41 / 0.62 / 0.013, norm_reg d_scale 0.013; OBB summary footprint / alpha, beta 0.12 / 0.06; rotated targets 0.10; scores 0.43;
    decode sqrt(score) 0.54 - 0.65 (of its 2u); decode OBB centre+height / width+length / angle 0.075 / 0.087 / 0.03 on the regular half
    and 0.074 / 0.08 / 0.047 on the degenerate half (vacuous rows: 0 % and 17.8 %).
Mutations (host test, |err| / bound at k = 2): alpha <-> 1 - alpha median 5e4 - 6e5; the factor 2 of the focal gradient dropped: median
9e3 - 3e4 (label 1), 1e5 (label 0) over |logit| < 8 (beyond, one of p, q is below u and the factor with it); the 1e-7 dropped: NaN on
whole-zero rows; the others break an equality.

Equal volumes: of two GTs of equal volume over the same location both torch's ``min`` on the CPU and the kernel's strict ``vol < best``
return the FIRST (lower index).  The decode kernel's grid cap (8192 blocks) lies beyond the post-processor's k * L <= 16384 candidates
and is not reachable through ops.fcos_decode's callers: it is left out."""
import math
import types

import torch

U = 2.0 ** -24
ETA = 2.0 ** -126
F32, F64 = torch.float32, torch.float64


# ======================================================================================================================
# the checker
# ======================================================================================================================
def _ratio(err, tol):
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    return torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def ratio(got, want, tol):
    """max |got - want| / tol over every element (inf where got is not finite or tol is zero and the error is not)."""
    got = got.detach().double().cpu().reshape(want.shape)
    tol = tol if torch.is_tensor(tol) else torch.full_like(want, tol)
    if want.numel() == 0:
        return 0.0
    return _ratio((got - want).abs(), tol.expand_as(want)).max().item()


def allowance(r_torch):
    return max(1.0, min(2.0, 4.0 * r_torch))


def check(got, want, tol, k, what):
    """Every element of ``got`` within k * tol of ``want``; prints and returns the worst |err| / (k * tol)."""
    got = got.detach().double().cpu().reshape(want.shape)
    tol = (tol if torch.is_tensor(tol) else torch.full_like(want, tol)).expand_as(want) * k
    m = _ratio((got - want).abs(), tol)
    worst = m.max().item() if m.numel() else 0.0
    print(f"{what}: max err/bound = {worst:.3f} (k = {k:.2f})")
    if not worst <= 1.0:
        flat = int(m.reshape(-1).argmax())
        raise AssertionError((what, "bad elements", int((m > 1).sum()), "of", m.numel(), "worst ratio", worst, "at", flat, "got",
                              got.reshape(-1)[flat].item(), "want", want.reshape(-1)[flat].item(), "k", k))
    return worst


def check_equal(got, want, what):
    got = got.detach().cpu().reshape(want.shape)
    if not torch.equal(got, want.to(got.dtype)):
        bad = got != want.to(got.dtype)
        flat = int(bad.reshape(-1).to(torch.uint8).argmax())
        raise AssertionError((what, "not equal", int(bad.sum()), "of", bad.numel(), "first at", flat, "got", got.reshape(-1)[flat].item(),
                              "want", want.reshape(-1)[flat].item()))
    print(f"{what}: equal ({want.numel()} elements)")


def sum_depth(count, cap, per_row=1):
    """Summation depth of the ordered grid sum: adds per thread + LDS tree + the ticket holder's strided adds + its tree."""
    blocks = min(max((count + 255) // 256, 1), cap)
    trips = -(-count // (blocks * 256))
    return trips * per_row + 8 + -(-blocks // 256) + 8


# ======================================================================================================================
# focal loss
# ======================================================================================================================
FOCAL_COUNTS = (1, 255, 256, 257, 1024 * 256 + 77)
FOCAL_CAP = 1024


def _softplus(v):
    return v.clamp(min=0) + torch.log1p(torch.exp(-v.abs()))


def focal_eval(logits, labels, alpha=0.25, mutate=None):
    """The kernel's expressions in the dtype of ``logits`` (float64: the reference; float32: the torch evaluation k is measured on)
    -> per-element loss term and d loss / d logit, zero where the label is negative.  ``mutate``: 'swap_alpha' | 'drop2'."""
    x = logits
    one = torch.ones((), dtype=x.dtype)
    a1, a0 = (1.0 - alpha, alpha) if mutate == "swap_alpha" else (alpha, 1.0 - alpha)
    a1, a0 = torch.tensor(a1, dtype=x.dtype), torch.tensor(a0, dtype=x.dtype)
    two = torch.tensor(1.0 if mutate == "drop2" else 2.0, dtype=x.dtype)
    p = one / (one + torch.exp(-x))
    q = one - p
    logp, log1mp = -_softplus(-x), -_softplus(x)
    t1 = -a1 * q * q * logp
    d1 = a1 * q * q * (two * p * logp - q)
    t0 = -a0 * p * p * log1mp
    d0 = a0 * p * p * (p - two * q * log1mp)
    zero = torch.zeros_like(x)
    term = torch.where(labels > 0, t1, torch.where(labels == 0, t0, zero))
    grad = torch.where(labels > 0, d1, torch.where(labels == 0, d0, zero))
    return term, grad


def focal_ref(logits, labels, alpha=0.25):
    """float64 focal terms and gradients with their bounds (module docstring) and the bound of the ordered sum."""
    x = logits.double()
    term, grad = focal_eval(x, labels, alpha)
    p = torch.sigmoid(x)
    q = torch.sigmoid(-x)                       # 1 - p without the cancellation
    logp, log1mp = _softplus(-x), _softplus(x)  # magnitudes
    dp, dq = 4 * U * p, 4 * U * p + 2 * U * q
    # label 1: T = a q^2 |logp|, d = a q^2 I, I = 2 p |logp| + q (one sign)
    i1 = 2 * p * logp + q
    bt1 = alpha * (2 * q * dq * logp + q * q * 4 * U * logp)
    bd1 = alpha * (2 * q * dq * i1 + q * q * (2 * (dp * logp + p * 4 * U * logp) + dq))
    # label 0: T = (1 - a) p^2 |log1mp|, d = (1 - a) p^2 I, I = p + 2 q |log1mp|
    i0 = p + 2 * q * log1mp
    bt0 = (1 - alpha) * (2 * p * dp * log1mp + p * p * 4 * U * log1mp)
    bd0 = (1 - alpha) * (2 * p * dp * i0 + p * p * (dp + 2 * (dq * log1mp + q * 4 * U * log1mp)))
    zero = torch.zeros_like(x)
    bt = torch.where(labels > 0, bt1, torch.where(labels == 0, bt0, zero))
    bd = torch.where(labels > 0, bd1, torch.where(labels == 0, bd0, zero))
    live = (labels >= 0).double()
    bt = bt + (8 * U * term.abs() + ETA) * live
    bd = bd + (8 * U * grad.abs() + ETA) * live
    n = x.numel()
    sum_bound = bt.sum().item() + sum_depth(n, FOCAL_CAP) * U * term.abs().sum().item()
    return types.SimpleNamespace(term=term, grad=grad, term_bound=bt, grad_bound=bd, sum=term.sum().item(), sum_bound=sum_bound)


def focal_case(count, kind="mixed", seed=0):
    """Seeded (logits fp32, labels int8).  'mixed': N(0, 3) logits and a dense sweep of [-87, 87], ~1 % positives and ~5 % ignored;
    'ignored': every label -1; 'negative': every label 0."""
    g = torch.Generator().manual_seed(1000 + seed + count)
    logits = torch.randn(count, generator=g) * 3.0
    ns = count // 2
    if ns > 1:
        logits[:ns] = torch.linspace(-87.0, 87.0, ns)
    elif count == 1:
        logits[0] = 0.75
    r = torch.rand(count, generator=g)
    labels = torch.where(r < 0.01, 1, torch.where(r < 0.06, -1, 0)).to(torch.int8)
    if count > 4:
        labels[:ns:3] = 1            # the sweep sees every label over the whole range
        labels[1:ns:7] = -1
    if count == 1:
        labels[0] = 1
    if kind == "ignored":
        labels.fill_(-1)
    elif kind == "negative":
        labels.fill_(0)
    return logits, labels


# ======================================================================================================================
# head epilogue
# ======================================================================================================================
HEAD_BWD_COUNTS = FOCAL_COUNTS
HEAD_FWD_BIG = 8192 * 256 + 300
HEAD_SCALES, HEAD_STRIDES = (0.8, 1.25, -0.5), (1.0, 4.0, 32.0)


def head_case(rows, wrows, D, seed=0, grads=True):
    """Seeded fused-GEMM outputs cls_out / box_out [rows, wrows] and incoming gradients (80 % zeros).  |raw| <= 1: the product raw * sc is
    rounded before expf, an error of u |raw sc| exp() that the 4u bound of the expf branch has to hold next to expf's own."""
    g = torch.Generator().manual_seed(2000 + seed + rows + D)
    cls_out = torch.randn(rows, wrows, generator=g)
    box_out = (torch.randn(rows, wrows, generator=g) * 0.5).clamp(-1.0, 1.0)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.0, -1.0])      # raw * sc underflows to +-0 or stays a denormal
    flat = box_out.view(-1)
    n = min(special.numel(), flat.numel())
    flat[:n] = special[:n]
    if not grads:
        return cls_out, box_out

    def sparse(*shape):
        return torch.randn(*shape, generator=g) * (torch.rand(*shape, generator=g) < 0.2)
    return cls_out, box_out, sparse(rows), sparse(rows, D), sparse(rows)


def head_fwd_eval(cls_out, box_out, sc, stride_mul, norm_reg, D, ctr_on_reg):
    """Kernel order in the dtype of the inputs -> logits, reg, ctr."""
    dt = box_out.dtype
    v = box_out[:, :D] * torch.tensor(sc, dtype=dt)
    if norm_reg:
        v = torch.cat([v[:, :6].clamp(min=0) * torch.tensor(stride_mul, dtype=dt), v[:, 6:]], dim=1)
    else:
        v = torch.exp(v)
    return cls_out[:, 0].clone(), v, (box_out[:, D] if ctr_on_reg else cls_out[:, 1]).clone()


def head_bwd_eval(box_out, sc, stride_mul, norm_reg, D, ctr_on_reg, d_logits, d_reg, d_ctr, mutate=None):
    """Kernel order in the dtype of the inputs -> d_cls_out, d_box_out [rows, wrows] (zero in every padded column), the d_scale terms
    dv * raw [rows, D].  ``mutate`` 'mask_raw': the ReLU mask taken on raw instead of raw * sc."""
    dt = box_out.dtype
    rows, wrows = box_out.shape
    s = torch.tensor(sc, dtype=dt)
    raw = box_out[:, :D]
    dv = d_reg.to(dt).clone()
    if norm_reg:
        on = (raw[:, :6] > 0) if mutate == "mask_raw" else (raw[:, :6] * s > 0)
        dv[:, :6] = torch.where(on, dv[:, :6] * torch.tensor(stride_mul, dtype=dt), torch.zeros((), dtype=dt))
    else:
        dv = dv * torch.exp(raw * s)
    d_cls, d_box = torch.zeros(rows, wrows, dtype=dt), torch.zeros(rows, wrows, dtype=dt)
    d_cls[:, 0] = d_logits.to(dt)
    if ctr_on_reg:
        d_box[:, D] = d_ctr.to(dt)
    else:
        d_cls[:, 1] = d_ctr.to(dt)
    d_box[:, :D] = dv * s
    return d_cls, d_box, dv * raw


def head_scale_bound(terms64, norm_reg, rows, D):
    per_term = (2.0 if norm_reg else 4.0) * U * terms64.abs().sum().item()
    return per_term + sum_depth(rows, 1024, per_row=D) * U * terms64.abs().sum().item() + ETA


# ======================================================================================================================
# geometry of the flat location list
# ======================================================================================================================
class Geometry:
    """Level-major, then scene, then voxel (x, y, z) with z fastest; location = index * stride + stride // 2 (float64)."""

    def __init__(self, n, dims, strides, ori_sizes=None):
        self.n, self.dims, self.strides = n, [tuple(d) for d in dims], list(strides)
        self.ori = ori_sizes
        self.counts = [d[0] * d[1] * d[2] for d in self.dims]
        self.off = [0]
        for c in self.counts:
            self.off.append(self.off[-1] + n * c)
        self.total = self.off[-1]
        self.locations = []
        for d, s in zip(self.dims, self.strides):
            g = torch.meshgrid(*[torch.arange(0, k * s, step=s, dtype=F64) for k in d], indexing="ij")
            self.locations.append(torch.stack([t.reshape(-1) for t in g], dim=1) + s // 2)

    def valid(self):
        """[total] bool: the location lies inside its scene's un-padded size (strictly below it on every axis)."""
        out = []
        for loc in self.locations:
            for i in range(self.n):
                if self.ori is None:
                    out.append(torch.ones(loc.shape[0], dtype=torch.bool))
                else:
                    w, l, h = self.ori[i]
                    out.append((loc[:, 0] < w) & (loc[:, 1] < l) & (loc[:, 2] < h))
        return torch.cat(out)

    def flat_locations(self):
        return torch.cat([loc for loc in self.locations for _ in range(self.n)])

    def flat_levels(self):
        return torch.cat([torch.full((self.n * c,), l, dtype=torch.long) for l, c in enumerate(self.counts)])

    def flat_scenes(self):
        return torch.cat([torch.full((c,), i, dtype=torch.long) for c in self.counts for i in range(self.n)])


# ======================================================================================================================
# GT summary and targets
# ======================================================================================================================
def summary_ref(gt):
    """[G, 6|7] -> float64 [G, 8] summary (footprint AABB + z range, alpha, beta) and its bound (zero = equality for AABB input)."""
    from oracle import fcos as OF
    gt = gt.double()
    if gt.shape[1] == 6:
        out = torch.cat([gt, torch.zeros(gt.shape[0], 2, dtype=F64)], dim=1)
        return out, torch.zeros_like(out)
    aabb, alpha, beta = OF.obb_summary(gt)
    out = torch.cat([aabb, alpha[:, None], beta[:, None]], dim=1)
    mc = torch.stack([aabb[:, [0, 3]].abs().amax(1), aabb[:, [1, 4]].abs().amax(1)], 1).amax(1) + gt[:, 3:5].amax(1)
    mz = gt[:, 2].abs() + gt[:, 5]
    ext = torch.stack([aabb[:, 3] - aabb[:, 0], aabb[:, 4] - aabb[:, 1]], 1)
    bound = torch.stack([4 * U * mc, 4 * U * mc, 4 * U * mz, 4 * U * mc, 4 * U * mc, 4 * U * mz, 8 * U * mc / ext[:, 0], 8 * U * mc / ext[:, 1]], 1)
    return out, bound + ETA


def summary_threshold_distance(gt):
    """Smallest distance of any corner's (ymax - y, xmax - x) to the 0.1 threshold of encode_fcos_obb (fp64)."""
    from oracle import geometry as G
    c = G.corners_2d(gt.double()[:, [0, 1, 3, 4, 6]].unsqueeze(0)).squeeze(0)
    xs, ys = c[:, :, 0], c[:, :, 1]
    dx, dy = xs.max(1, keepdim=True)[0] - xs, ys.max(1, keepdim=True)[0] - ys
    return min((dx - 0.1).abs().min().item(), (dy - 0.1).abs().min().item())


OBB_SUMMARY_GTS = torch.tensor([[20.0, 18.0, 16.0, 14.0, 12.0, 10.0, 0.0], [20.0, 18.0, 16.0, 14.0, 12.0, 10.0, 0.3],
                                [12.25, 24.0, 30.0, 10.0, 9.0, 12.0, -0.3], [40.0, 33.5, 21.0, 22.0, 8.0, 6.0, 0.8],
                                [31.0, 52.0, 12.0, 7.0, 19.0, 30.0, -0.8], [64.0, 64.0, 40.0, 30.0, 24.0, 18.0, 1.2],
                                [5.0, 6.0, 7.0, 3.0, 3.0, 2.0, 0.0], [90.5, 10.25, 33.0, 16.0, 4.0, 5.0, 0.3]])


def targets_ref(geom, targets, radius, norm_reg, use_obb, mutate=None, dtype=F64):
    """oracle targets_for_scene in float64, wrapped into the kernel's flat order: labels int8 [total] (-1 = padding), reg_targets [total, D].
    ``mutate``: 'lo_strict' (mx > lo), 'inside_ge' (>= 0 in the sampling region); ``dtype`` float32: the oracle's own fp32 evaluation."""
    from oracle import fcos as OF
    D = 8 if use_obb else 6
    allp = torch.cat(geom.locations).to(dtype)
    saved = OF.sample_region
    per_scene = []
    try:
        if mutate == "inside_ge":
            def region(gt, strides, counts, loc, rad):
                K, n = loc.shape[0], gt.shape[0]
                g = gt[None].expand(K, n, 6)
                ctr = (g[..., :3] + g[..., 3:]) / 2
                r = torch.cat([torch.full((c,), s * rad, dtype=F64) for c, s in zip(counts, strides)])[:, None, None]
                lo = torch.where(ctr - r > g[..., :3], ctr - r, g[..., :3])
                hi = torch.where(ctr + r > g[..., 3:], g[..., 3:], ctr + r)
                return torch.cat([loc[:, None, :] - lo, hi - loc[:, None, :]], dim=-1).min(-1)[0] >= 0
            OF.sample_region = region
        for gt in targets:
            gt = gt.to(dtype)
            if mutate == "lo_strict" and gt.shape[0]:
                lab, reg = _targets_lo_strict(OF, allp, geom, gt, radius, use_obb)
            else:
                lab, reg = OF.targets_for_scene(allp, geom.counts, geom.strides, gt, radius, use_obb)
            per_scene.append((lab.double(), reg.double()))
    finally:
        OF.sample_region = saved
    labels, regs = [], []
    for l, s in enumerate(geom.strides):
        for lab, reg in per_scene:
            labels.append(torch.split(lab, geom.counts)[l])
            rt = torch.split(reg, geom.counts)[l].clone()
            if norm_reg:
                rt[:, :6] = rt[:, :6] / s
            regs.append(rt)
    labels, regs = torch.cat(labels).to(torch.int8), torch.cat(regs)
    valid = geom.valid()
    labels[~valid] = -1
    regs[~valid] = 0
    return labels, regs


def _targets_lo_strict(OF, allp, geom, gt, radius, use_obb):
    """targets_for_scene with `mx > lo` in place of `mx >= lo` (the oracle has no hook for it: its lines, with that one change)."""
    aabb, alpha, beta = OF.obb_summary(gt) if use_obb else (gt, None, None)
    reg = torch.cat([allp[:, None, :] - aabb[None, :, :3], aabb[None, :, 3:] - allp[:, None, :]], dim=2)
    inside = OF.sample_region(aabb, geom.strides, geom.counts, allp, radius) if radius > 0 else reg.min(2)[0] > 0
    soi = torch.cat([torch.tensor(OF.SIZES_OF_INTEREST[min(l, 3)], dtype=F64)[None].expand(c, -1) for l, c in enumerate(geom.counts)])
    mx = reg.max(2)[0]
    cared = (mx > soi[:, [0]]) & (mx <= soi[:, [1]])
    vol = ((aabb[:, 3] - aabb[:, 0]) * (aabb[:, 4] - aabb[:, 1]) * (aabb[:, 5] - aabb[:, 2]))[None].repeat(allp.shape[0], 1)
    vol[~inside] = OF.INF
    vol[~cared] = OF.INF
    best, which = vol.min(dim=1)
    if use_obb:
        reg = torch.cat([reg, alpha[None, :, None].expand(allp.shape[0], -1, 1), beta[None, :, None].expand(allp.shape[0], -1, 1)], dim=2)
    return (best != OF.INF).double(), reg[torch.arange(allp.shape[0]), which]


TARGET_STRIDES = (4, 8, 16, 32)
TARGET_SIZES = [(96, 80, 64), (70, 60, 50)]       # scene 1 ends ON locations: x = 70 and z = 50 (level 0), y = 60 (level 1)
TARGET_DIMS = [(24, 20, 16), (12, 10, 8), (6, 5, 4), (3, 3, 2)]
SOI_LIMITS = (16.0, 32.0, 64.0)


def _limit_box(s, L, delta, loc):
    """A GT whose left face lies L + delta from the location ``loc`` of the stride-s level, 1.5 L wide, L in y and z around it: the
    location's largest distance is exactly L + delta and it lies inside the radius-1.5 sampling region."""
    x, y, z = loc
    a0 = x - L - delta
    return [a0, y - L / 2, z - L / 2, a0 + 1.5 * L, y + L / 2, z + L / 2]


def targets_case(empty_second=False):
    """Two scenes of different un-padded size on strides (4, 8, 16, 32); quarter-grid AABB GTs (module docstring):
    scene 0: for every size-of-interest limit L a GT with a location at max-distance exactly L seen from the level below (hi) and from the
    level above (lo), and one a quarter voxel beyond; scene 1: nested GTs, two GTs of equal volume over the same locations, a GT whose
    sampling-region face and whose own face pass through locations."""
    s0 = []
    for s, L in ((4, 16.0), (8, 32.0), (16, 64.0)):
        loc = tuple(float(3 * s + s // 2 + 2 * s * k) for k in (1, 0, 0))
        s0.append(_limit_box(s, L, 0.0, loc))                      # hi limit of the stride-s level, hit exactly
        s0.append(_limit_box(s, L, 0.25, loc))                     # ... and a quarter voxel beyond
        loc2 = tuple(float(2 * s + s) for _ in range(3))           # a location of the stride-2s level (index 1)
        s0.append(_limit_box(2 * s, L, 0.0, loc2))                 # lo limit of the stride-2s level, hit exactly
    s1 = [[2.0, 4.0, 4.0, 30.0, 28.0, 26.0],                       # faces of the region (x = 10, 22) and of the box (x = 2) on locations
          [36.0, 30.0, 16.0, 66.0, 58.0, 44.0], [42.0, 36.0, 20.0, 58.0, 50.0, 36.0],      # nested: the smaller wins
          [40.0, 8.0, 20.0, 60.0, 24.0, 40.0], [42.0, 6.0, 20.0, 62.0, 22.0, 40.0]]        # equal volume (6400), overlapping
    t0, t1 = torch.tensor(s0), torch.tensor(s1)
    if empty_second:
        t1 = torch.zeros(0, 6)
    return Geometry(2, TARGET_DIMS, TARGET_STRIDES, TARGET_SIZES), [t0, t1]


def as_obb(gt):
    """(x0, y0, z0, x1, y1, z1) -> (cx, cy, cz, w, l, h, 0): angle exactly 0, so the footprint is the box, alpha = 0.5, beta = -0.5."""
    if gt.shape[0] == 0:
        return torch.zeros(0, 7)
    return torch.cat([(gt[:, :3] + gt[:, 3:]) / 2, gt[:, 3:] - gt[:, :3], torch.zeros(gt.shape[0], 1)], dim=1)


def targets_big_case():
    """One level of 81^3 locations (531 441 > 2048 x 256), stride 4, one scene, 3 GTs."""
    gts = torch.tensor([[100.0, 100.0, 100.0, 130.0, 124.0, 122.0], [96.0, 96.0, 96.0, 140.0, 140.0, 140.0], [200.25, 40.0, 300.0, 212.0, 52.5, 311.0]])
    return Geometry(1, [(81, 81, 81)], [4], None), [gts]


def targets_boundaries(geom, targets, radius):
    """Which decision boundaries the fp64 quantities of the fixture sit on (each must be hit by at least one location)."""
    allp = torch.cat(geom.locations)
    level = torch.cat([torch.full((c,), l) for l, c in enumerate(geom.counts)])
    s = torch.tensor(geom.strides, dtype=F64)[level]
    out = {f"hi=={L}": False for L in SOI_LIMITS}
    out.update({f"lo=={L}": False for L in SOI_LIMITS})
    out.update({f"beyond {L}": False for L in SOI_LIMITS})
    out.update({"region face": False, "equal volume": False, "nested": False})
    soi = [[-1, 16], [16, 32], [32, 64], [64, 1e8]]
    for gt in targets:
        if not gt.shape[0]:
            continue
        g = gt.double()
        reg = torch.cat([allp[:, None, :] - g[None, :, :3], g[None, :, 3:] - allp[:, None, :]], dim=2)
        if radius > 0:
            ctr = (g[:, :3] + g[:, 3:]) / 2
            r = (s * radius)[:, None, None]
            lo = torch.maximum(ctr[None] - r, g[None, :, :3])
            hi = torch.minimum(ctr[None] + r, g[None, :, 3:])
            dmin = torch.cat([allp[:, None, :] - lo, hi - allp[:, None, :]], dim=-1).min(-1)[0]
        else:
            dmin = reg.min(2)[0]
        inside = dmin > 0
        mx = reg.max(2)[0]
        lim = torch.tensor([soi[l] for l in level.tolist()], dtype=F64)
        for L in SOI_LIMITS:
            out[f"hi=={L}"] |= bool((inside & (mx == L) & (lim[:, [1]] == L)).any())
            out[f"lo=={L}"] |= bool((inside & (mx == L) & (lim[:, [0]] == L)).any())
            out[f"beyond {L}"] |= bool((inside & (mx == L + 0.25) & (lim[:, [1]] == L)).any())
        out["region face"] |= bool((dmin == 0).any())
        cared = inside & (mx >= lim[:, [0]]) & (mx <= lim[:, [1]])
        vol = ((g[:, 3] - g[:, 0]) * (g[:, 4] - g[:, 1]) * (g[:, 5] - g[:, 2]))[None].expand_as(mx)
        v = torch.where(cared, vol, torch.full_like(vol, float("inf")))
        best = v.min(1, keepdim=True)[0]
        out["equal volume"] |= bool((((v == best) & cared).sum(1) > 1).any())
        out["nested"] |= bool(((cared.sum(1) > 1) & ((v == best).sum(1) == 1)).any())
    if geom.ori is not None:
        for i, size in enumerate(geom.ori):
            for d in range(3):
                out[f"scene {i} axis {d} location == ori"] = bool((allp[:, d] == size[d]).any()) or size[d] == max(z[d] for z in geom.ori)
    return out


OBB_TARGET_GTS = [torch.tensor([[30.0, 28.0, 20.0, 24.0, 16.0, 18.0, 0.3], [60.0, 50.0, 30.0, 40.0, 28.0, 30.0, -0.8],
                                 [40.0, 40.0, 32.0, 70.0, 60.0, 50.0, 1.2]]),
                   torch.tensor([[24.0, 24.0, 20.0, 20.0, 14.0, 16.0, 0.8], [36.0, 30.0, 24.0, 30.0, 40.0, 28.0, -0.3]])]
DECISION_MARGIN = 1e-3          # 100 x the fp32 error of a footprint coordinate (4u x 100)


def rotated_targets_ref(geom, targets, radius, norm_reg):
    """Rotated GTs: labels and targets in float64 from the float64 summary, with per location the distance ``margin`` of the nearest
    decision quantity (sampling-region distance, max-distance against both size-of-interest limits) to its threshold - a label is
    asserted where the margin exceeds DECISION_MARGIN - and the bound of the targets: the summary's bound of the scene's GTs (largest)
    plus 2u |value| for the subtraction and the division, over the stride where normalised."""
    labels, regs = targets_ref(geom, targets, radius, norm_reg, True)
    allp = torch.cat(geom.locations)
    level = torch.cat([torch.full((c,), l) for l, c in enumerate(geom.counts)])
    s = torch.tensor(geom.strides, dtype=F64)[level]
    lim = torch.tensor([[-1.0, 16.0], [16.0, 32.0], [32.0, 64.0], [64.0, 1e8]], dtype=F64)[level.clamp(max=3)]
    margins, bounds = [], []
    for gt in targets:
        summ, sb = summary_ref(gt)
        g = summ[:, :6]
        reg = torch.cat([allp[:, None, :] - g[None, :, :3], g[None, :, 3:] - allp[:, None, :]], dim=2)
        if radius > 0:
            ctr = (g[:, :3] + g[:, 3:]) / 2
            r = (s * radius)[:, None, None]
            lo, hi = torch.maximum(ctr[None] - r, g[None, :, :3]), torch.minimum(ctr[None] + r, g[None, :, 3:])
            dmin = torch.cat([allp[:, None, :] - lo, hi - allp[:, None, :]], dim=-1).min(-1)[0]
        else:
            dmin = reg.min(2)[0]
        mx = reg.max(2)[0]
        m = torch.minimum(dmin.abs(), torch.minimum((mx - lim[:, [0]]).abs(), (mx - lim[:, [1]]).abs())).min(1)[0]
        vol = (g[:, 3] - g[:, 0]) * (g[:, 4] - g[:, 1]) * (g[:, 5] - g[:, 2])
        assert (vol[:, None] - vol[None, :]).abs().add(torch.eye(len(vol)) * 1e9).min() > 1.0, "volumes of the rotated GTs must be distinct"
        margins.append(m)
        bounds.append(sb.amax(0))
    margin, bound = [], []
    for l, st in enumerate(geom.strides):
        for m, b in zip(margins, bounds):
            margin.append(torch.split(m, geom.counts)[l])
            dn = float(st) if norm_reg else 1.0
            bound.append(torch.cat([b[:6] / dn, b[6:]])[None].expand(geom.counts[l], 8))
    bound = torch.cat(bound) + 2 * U * regs.abs()
    return labels, regs, torch.cat(margin), bound


# ======================================================================================================================
# scores
# ======================================================================================================================
SCORE_THRESH = 0.05


def scores_ref(geom, logits, ctr, thresh):
    """-> float64 scores (-1 where not a candidate), bound, and the distance |sigmoid - thresh| / (4u sigmoid) of the closest logit."""
    c = torch.sigmoid(logits.double())
    t = float(torch.tensor(thresh, dtype=F32))
    cand = geom.valid() & (c > t)
    val = c * torch.sigmoid(ctr.double())
    want = torch.where(cand, val, torch.full_like(val, -1.0))
    bound = torch.where(cand, 8 * U * val + ETA, torch.zeros_like(val))
    return want, bound, ((c - t).abs() / (4 * U * c)).min().item()


def scores_eval32(geom, logits, ctr, thresh):
    one = torch.ones((), dtype=F32)
    c = one / (one + torch.exp(-logits))
    cand = geom.valid() & (c > torch.tensor(thresh, dtype=F32))
    return torch.where(cand, c * (one / (one + torch.exp(-ctr))), -one)


def scores_case(big=False, seed=0):
    if big:
        geom = Geometry(1, [(129, 128, 128)], [4], None)           # 2 113 536 > 8192 x 256
    else:
        geom = Geometry(2, [(9, 7, 6), (5, 4, 3), (3, 2, 2)], [4, 8, 16], [(36, 28, 24), (22, 20, 14)])
    g = torch.Generator().manual_seed(3000 + seed + geom.total)
    logits, ctr = torch.randn(geom.total, generator=g) * 3.0, torch.randn(geom.total, generator=g) * 3.0
    ns = min(geom.total // 3, 4096)
    logits[:ns] = torch.linspace(-87.0, 87.0, ns)
    ctr[:ns] = torch.linspace(87.0, -87.0, ns).roll(ns // 3)
    near = (torch.sigmoid(logits.double()) - float(torch.tensor(SCORE_THRESH, dtype=F32))).abs() <= 64 * U
    logits[near] += 0.01                                           # no sigmoid within 4u of the threshold
    return geom, logits, ctr


# ======================================================================================================================
# decode
# ======================================================================================================================
DECODE_SEG = 37
DECODE_K = 16.0


def decode_case(kind, seed=0):
    """Two scenes x three levels, seg_len 37 -> idx int32 [6, 37] (-1 slots), score [6, 37] (-1, NaN, 0 slots), reg [total, D].
    kind: 'aabb' (quarter-grid distances, extents exactly min_size) | 'obb_regular' | 'obb_degenerate'."""
    geom = Geometry(2, [(9, 7, 6), (5, 4, 3), (3, 2, 2)], [4, 8, 16], [(36, 28, 24), (22, 20, 14)])
    g = torch.Generator().manual_seed(4000 + seed + len(kind))
    segs = geom.n * len(geom.dims)
    idx = torch.stack([torch.randint(0, geom.counts[sg // geom.n], (DECODE_SEG,), generator=g) for sg in range(segs)]).to(torch.int32)
    score = torch.rand(segs, DECODE_SEG, generator=g)
    idx[:, 5::11] = -1
    score[:, 3::13] = -1.0
    score[:, 4::17] = float("nan")
    score[:, 6::19] = 0.0
    D = 6 if kind == "aabb" else 8
    if kind == "aabb":
        reg = torch.randint(0, 40, (geom.total, 6), generator=g).float() * 0.25
        reg[::5, 0], reg[::5, 3] = 0.75, 1.25                      # x extent exactly min_size = 2 (where the clip does not act)
        reg[1::7, 1], reg[1::7, 4] = 0.75, 1.0                     # y extent 1.75 < min_size
        min_size = 2.0
    elif kind == "obb_regular":
        reg = torch.cat([1.0 + torch.rand(geom.total, 6, generator=g) * 11.0, torch.rand(geom.total, 2, generator=g) * 0.9 - 0.45], dim=1)
        min_size = 1.0
    else:
        reg = torch.cat([torch.rand(geom.total, 6, generator=g) * 12.0, torch.rand(geom.total, 2, generator=g) * 1.6 - 0.8], dim=1)
        reg[:, :6] *= (torch.rand(geom.total, 6, generator=g) >= 0.2)
        reg[::9] = 0.0                                             # whole rows zero
        reg[1::9, 6:] = 0.0                                        # alpha = beta = 0
        reg[2::9, 6], reg[2::9, 7] = 0.5, -0.5
        min_size = 1.0
    return geom, idx, score, reg, D, min_size


def decode_ref(geom, idx, score, reg, D, min_size, dtype=F64, mutate=None):
    """Reference of the candidate decode in ``dtype`` (float64: the reference; float32: torch's evaluation).  -> namespace with boxes
    [count, 6|7], scores, levels, live (slot decoded), and for D = 8 the bound magnitudes.  ``mutate``: 'swap_seg' | 'no_eps' | 'gt_min'."""
    from oracle import fcos as OF
    segs, k = idx.shape
    count = segs * k
    seg = torch.arange(count) // k
    level, scene = (seg % len(geom.dims), seg // len(geom.dims)) if mutate == "swap_seg" else (seg // geom.n, seg % geom.n)
    idf, sc = idx.reshape(-1).long(), score.reshape(-1).to(dtype)
    live = (idf >= 0) & (sc >= 0)
    W = 7 if D == 8 else 6
    boxes = torch.zeros(count, W, dtype=dtype)
    out_s = torch.full((count,), -1.0, dtype=dtype)
    cnt = torch.tensor(geom.counts)[level]
    vox = idf.clamp(min=0) % cnt                 # (the modulo acts under 'swap_seg' only)
    flat = torch.tensor(geom.off[:-1])[level] + scene * cnt + vox
    loc = torch.stack([geom.locations[l][i] for l, i in zip(level.tolist(), vox.tolist())]).to(dtype)
    r = reg.to(dtype)[flat]
    ori = torch.tensor(geom.ori, dtype=dtype)[scene]
    res = types.SimpleNamespace(live=live, levels=level.to(dtype), sqrt_in=torch.sqrt(torch.nan_to_num(sc, nan=0.0).clamp(min=0)))
    if D == 6:
        det = torch.cat([loc - r[:, :3], loc + r[:, 3:6]], dim=1)
        det = torch.minimum(det.clamp(min=0), torch.cat([ori, ori], dim=1))
        ext = det[:, 3:] - det[:, :3]
        keep = (ext > min_size).all(1) if mutate == "gt_min" else (ext >= min_size).all(1)
    else:
        if mutate == "no_eps":
            det = _decode_obb_no_eps(loc, r)
        else:
            det = OF.decode_obb(loc, r)
        keep = (det[:, 3:6] >= min_size).all(1)
        x0, x1, y0, y1 = loc[:, 0] - r[:, 0], loc[:, 0] + r[:, 3], loc[:, 1] - r[:, 1], loc[:, 1] + r[:, 4]
        z0, z1 = loc[:, 2] - r[:, 2], loc[:, 2] + r[:, 5]
        M = torch.stack([x0.abs(), x1.abs(), y0.abs(), y1.abs()], 1).amax(1) + r[:, 6:].abs().amax(1) * torch.maximum(x1 - x0, y1 - y0)
        vx = torch.minimum(torch.maximum((x1 + x0) / 2 + r[:, 6] * (x1 - x0), x0), x1)
        vy = torch.minimum(torch.maximum((y1 + y0) / 2 + r[:, 7] * (y1 - y0), y0), y1)
        cx, cy = (x0 + x1) / 2, (y0 + y1) / 2
        d0, d1 = torch.hypot(vx - cx, y1 - cy), torch.hypot(x1 - cx, vy - cy)
        res.M, res.Mz = M, M + torch.maximum(z0.abs(), z1.abs())
        res.amp = 1 + torch.maximum(d0, d1) / (torch.minimum(d0, d1) + 1e-7)
        res.zero_row = (r[:, :6] == 0).all(1)
        res.loc = loc
    boxes[live] = det[live]
    out_s[live] = torch.where(keep[live], torch.sqrt(sc[live]), torch.full_like(sc[live], -1.0))
    res.boxes, res.scores, res.keep = boxes, out_s, keep
    return res


def _decode_obb_no_eps(loc, reg):
    """decode_fcos_obb with the 1e-7 of its normalisation dropped (the mutation; its lines otherwise)."""
    x0, y0, z0 = loc[:, 0] - reg[:, 0], loc[:, 1] - reg[:, 1], loc[:, 2] - reg[:, 2]
    x1, y1, z1 = loc[:, 0] + reg[:, 3], loc[:, 1] + reg[:, 4], loc[:, 2] + reg[:, 5]
    vx = torch.minimum(torch.maximum((x1 + x0) / 2 + reg[:, 6] * (x1 - x0), x0), x1)
    vy = torch.minimum(torch.maximum((y1 + y0) / 2 + reg[:, 7] * (y1 - y0), y0), y1)
    ctr = torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, (z0 + z1) / 2], dim=1)
    v0, v1 = torch.stack([vx, y1], dim=1) - ctr[:, :2], torch.stack([x1, vy], dim=1) - ctr[:, :2]
    d0, d1 = torch.norm(v0, dim=1), torch.norm(v1, dim=1)
    dmax = torch.max(d0, d1)
    v0 = v0 / d0[:, None] * dmax[:, None] + ctr[:, :2]
    v1 = v1 / d1[:, None] * dmax[:, None] + ctr[:, :2]
    mid = (v0 + v1) / 2 - ctr[:, :2]
    return torch.stack([ctr[:, 0], ctr[:, 1], ctr[:, 2], torch.norm(mid, dim=1) * 2, torch.norm(v0 - v1, dim=1), z1 - z0,
                        torch.atan2(mid[:, 1], mid[:, 0])], dim=1)


def decode_obb_bounds(ref):
    """Per-row bounds of the OBB decode (module docstring) and the vacuous masks: -> centre_height [count, 4] (cx, cy, cz, h), size
    [count] (width, length), angle [count], vac_size, vac_angle (bool)."""
    k = DECODE_K * U
    ch = torch.stack([k * ref.M, k * ref.M, k * ref.Mz, k * ref.Mz], dim=1) + ETA
    size = k * ref.M * ref.amp + ETA
    angle = size / (ref.boxes[:, 3] / 2).clamp(min=1e-300)
    vac_size = ref.live & (ref.amp > 1e3)
    vac_angle = ref.live & (vac_size | ~(angle < 0.1))
    return ch, size, angle, vac_size, vac_angle


def angle_diff(a, b):
    d = (a.double() - b.double()).abs() % (2 * math.pi)
    return torch.minimum(d, 2 * math.pi - d)


def decode_obb_ratios(ref, boxes, scores, levels, min_size, k=(1.0, 1.0, 1.0)):
    """|err| / (k * bound) of a decode result against the fp64 ``ref``: -> dict of the three groups' worst ratios; raises on anything that
    has no bound: dropped slots not all-zero with score -1, levels, finiteness, the exact centre of whole-zero rows, decided keeps."""
    boxes, scores, levels = boxes.detach().double().cpu().reshape(ref.boxes.shape), scores.detach().double().cpu().reshape(-1), levels.detach().double().cpu().reshape(-1)
    ch, size, angle, vac_size, vac_angle = decode_obb_bounds(ref)
    live = ref.live
    assert torch.equal(levels, ref.levels), "levels"
    assert torch.isfinite(boxes).all(), "non-finite box"
    assert not boxes[~live].any() and (scores[~live] == -1).all(), "dropped slot"
    zr = live & ref.zero_row
    assert torch.equal(boxes[zr][:, :3], ref.loc[zr]), "centre of a whole-zero row"
    out = {}
    e = (boxes[:, [0, 1, 2, 5]] - ref.boxes[:, [0, 1, 2, 5]]).abs()
    out["centre_height"] = _ratio(e[live], ch[live] * k[0]).max().item()
    sel = live & ~vac_size
    e = (boxes[:, 3:5] - ref.boxes[:, 3:5]).abs()
    out["size"] = _ratio(e[sel], size[sel, None].expand(-1, 2) * k[1]).max().item()
    sel = live & ~vac_angle
    out["angle"] = _ratio(angle_diff(boxes[sel, 6], ref.boxes[sel, 6]), angle[sel] * k[2]).max().item()
    # keep: decided where every size is further from min_size than its bound (the height's is Mz's)
    dist = torch.stack([(ref.boxes[:, 3] - min_size).abs() - 2 * size, (ref.boxes[:, 4] - min_size).abs() - 2 * size,
                        (ref.boxes[:, 5] - min_size).abs() - 2 * ch[:, 3]], 1).amin(1)
    decided = live & ~vac_size & (dist > 0)
    want = ref.scores
    kept = decided & (want >= 0)
    assert (scores[decided & (want < 0)] == -1).all(), "a row below min_size was kept"
    out["score"] = _ratio((scores[kept] - want[kept]).abs(), 2 * U * want[kept] + ETA).max().item() if kept.any() else 0.0
    und = live & ~decided
    assert ((scores[und] == -1) | ((scores[und] - ref.sqrt_in[und]).abs() <= 2 * U + ETA)).all(), "undecided row's score"
    out["vacuous"] = (vac_angle.sum().item() / max(int(live.sum()), 1))
    out["decided"] = int(decided.sum())
    return out
