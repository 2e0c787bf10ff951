"""float64 references of the RPN proposal / target kernels of csrc/postproc.hip (with csrc/geometry.cuh): the anchor table, the AABB and
midpoint-offset coders (decode_boxes / encode_boxes / coder_pairs), obb_to_aabb, head_flatten / head_unflatten, filter_candidates,
select_kept, match_anchors and rpn_sampled_loss; the same expressions in torch fp32 on the CPU (``dt=F32``: what the allowance k is
measured on), per-element bounds and decided masks, the seeded case families shared by tests/test_rpn_bounds_host.py (no GPU) and
tests/test_gpu_rpn_kernels.py, and the mutations the bounds have to catch.  Every evaluation runs on the fp32 input values the kernel
receives; constants are the kernel's fp32 constants (log 2000, |log(16/1000)|, the truncated pi 3.141592, the 1e-7 guard).

Allowances for the device functions (u = 2^-24): expf, logf, log1pf 2 ulp = 4u relative (fcos_ref); sinf, cosf 2 ulp = 4u absolute
(roi_ref); sqrtf 2u relative (fcos_ref); the division one rounding, counted as 2u; fmodf is exact; atan2f has no allowance in the older references and gets
the OpenCL full-profile limit of 6 ulp = 12u |angle|.  Every sum, difference and product is one rounding u |result| (the unit is
built with -ffp-contract=off).  Every bound holds an absolute floor ETA = 2^-126.

Bounds, first order through the kernel's intermediates, magnitudes from float64 (anchors a, deltas d, w = a_hi - a_lo):
    AABB decode      out = pc -+ half, pc = d w + c, half = exp(min(d, log 2000)) w / 2:
                     u (|out| + |pc| + 2 |d w| + |c| + |w| / 2) + 6u half
    AABB encode      centre (gc - ac) / aw: u (|gc - ac| + |ac| + |gc| + (aw + |gw|) / 2) / aw + 3u |out|;  size log(gw / aw): 4u + 4u |out|
    midpoint decode  g = pc + pw d: e_g = u |g| + 2u |pw d| + u |pc|;  s = pw exp(dd): e_s = 6u s.  A polygon point is centre + offset; its
                     POSITION RELATIVE TO THE CENTRE carries e_c = u |point| + u |offset| + e_offset (the centre's own error moves the four
                     points together: it enters x, y but not the angle or the sides), then the diagonal normalisation: diag = |offset|:
                     e_diag = (|cx| e_cx + |cy| e_cy) / diag + 3u diag (squares and sum 2u, halved by the root, + 2u),
                     scale sc = max diag / diag: e_sc = sc (e_md / md + e_diag / diag + 2u),
                     normalised point: e_r = sc e_c + |c| e_sc + u |c sc| + u |point|.
                     angle th = atan2(-(p1 - p0).y, (p1 - p0).x + 1e-7): the points' positional error divided by |p1 - p0| (guard
                     included): e_th = (e_r(p0) + e_r(p1) + 2u |p1 - p0|_1) / |p1 - p0| + 12u |th|.
                     The normalised polygon is a rectangle aligned with th; measured in a frame rotated by delta its side w reads
                     w cos(delta) + h sin(delta), so e_w = 2 max e_q + u w + w (1 - cos delta) + h sin delta, delta = min(e_th, pi / 2),
                     e_q = position relative to the mean (e_r + max e_r + 3u max |point| + u |q|, both coordinates) + 6u (|qx| + |qy|)
                     for the rotation (products, sum, 4u of cosf / sinf).  Centre: max e_r + e_g + 3u max |point|.
                     Angle after regular_obb: e_th + 6u pi (three roundings at <= 2 pi).  z, depth: e_g, e_s.
    midpoint encode  half extents bx = |w/2 cos| + |h/2 sin|: e_b = 3u (|w| + |h|) + u bx;  hbb corner: u |corner| + e_b;  gx: u |gx| +
                     u (|hx1| + |hx2|) / 2 + e_b;  gw: u gw + u (|hx1| + |hx2|) + 2 e_b;  vertices: e_v = 3u (|w| + |h|) + 2u (|c| + (|w| + |h|) / 2).
                     centre deltas (gx - pc) / pw: (e_gx + u |pc| + u |gx - pc|) / pw + 3u |out|;  log sizes: e_gw / gw + 4u + 4u |out|;
                     offsets (ga - gx) / gw: (e_v + e_gx + u |ga - gx|) / gw + |out| e_gw / gw + 3u |out|.
    obb_to_aabb      e_b + u |out| (z: u |out|)
    filter scores    sigmoid 1 / (1 + exp(-l)): 8u score (exp 4u, sum u, quotient u, rounded up as in fcos_ref)
    sampled loss     dL/dlogit = (sigmoid - y) / n: (8u sigmoid + u |sigmoid - y|) / n + 3u |g|;  dL/ddelta: 5u |g|;
                     BCE term max(x, 0) - x y + log1p(exp(-|x|)): 2u |max(x,0) - x y| + 4u e + 4u log1p + 2u |term|;  smooth-L1 term:
                     5u |term| + u |d| min(|d| / beta, 1);  each loss: sum of its term bounds + depth u sum |term| + 2u |loss|,
                     depth = ceil(terms / 256) + 10 (per-thread strided adds, six shuffle steps, four wave partials).
                     Both branches of smooth-L1 agree at |d| = beta in value and slope, so no element is undecided.
    anchors, head_flatten / head_unflatten, filter boxes / levels / counts / order, select_kept, match_anchors: equality.

Decided masks (undecided elements are skipped and their share asserted: at most 1 % in a random family, none in a constructed one):
    conditioning     an element whose bound exceeds 1e-3 of the box's largest side is undecided
    decode swap      |w - h| <= e_w + e_h: the swap and the pi / 2 shift may differ (sides and angle undecided)
    encode offsets   a vertex with ||y - ymin| - 0.1| (or x, xmax) within 2 e_v of zero
    angle            compared on the circle of period kPiRef: a wrap is not an error
The degenerate family (da -> +0.5 with db -> -0.5, where p0 and p1 coincide and atan2 sees its 1e-7 guard, and the mirror, where the
polygon collapses onto its diagonal) holds x, y, z, depth and the LARGER planar side (bound max(e_w, e_h), no swap decision needed) to
their bounds; the smaller side and the angle are reported undecided, exempt from the cap.  On the exactly degenerate rows p0 == p1 in
every arithmetic, th = atan2f(-0, 1e-7) = -0, and the angle is exactly 0 (wide) or -kHalfPiRef: asserted as an equality, which is what
catches pi for kPiRef (the two constants move the angle by 3.3e-7, below the three roundings of the wrap everywhere else).

match_anchors: the IoU uses + - x / min max only, so the reference is an op-for-op numpy float32 evaluation and labels / matched are
equal with no undecided element; the host test ties it to oracle.boxes.match on the oracle's IoU matrix and to float64 on an
integer-coordinate family.  A GT entirely outside the grid has maximum 0 and every unpadded anchor attains it: they all turn positive
(the reference's documented outcome), asserted as such.

r = worst |err| / bound of the torch fp32 CPU evaluation (host test, printed with -s); the assertion is |err| <= k bound, k = max(1,
min(2, 4 r)).  Measured r and the worst device ratio per family: RESULTS at the end of this docstring.

Mutations (host test; share of decided elements beyond 2 x bound, or a broken equality): clip (log 2000 <-> |log(16/1000)|),
offset_clamp (+-1 for +-0.5), pi (equality on the exactly degenerate rows), ge (w >= h on exact-tie rows: equality of the fp32
evaluation), thr (0.1 -> 0.01), pairing (fix_obb_clip swapped), min_gt (> for >=), beyond_count, tie_high, last_dup, no_low_quality,
inv_npos (1 / npos), no_beta (smooth-L1 without / beta).

RESULTS: r of the torch fp32 CPU evaluation (host test) | worst |err| / (k bound) of the kernels on an MI355X (GPU test), per family
    aabb decode random / clamp                         0.514 / 0.498        | 0.257 / 0.250
    aabb encode random                                 0.469                | 0.250
    midpoint decode random / clamp / theta / square    0.499 / 0.530 / 0.197 / 0.474   | 0.250 / 0.265 / 0.197 / 0.250   (no undecided element)
    midpoint decode degenerate: x y z depth            0.505                | 0.253
                                larger side            0.046                | 0.046 on the 58 % of the rows where its bound is below 1e-3 side
                                undecided: smaller side and angle on 38 % of the rows (the exactly and nearly degenerate ones); a
                                min_size = 1e-3 cut falls differently from float64 on 2 of 2048 rows (float64 sides 5.5e-3 and 8.1e-3,
                                fp32 and device 8.2e-4 and 9.4e-4): recorded in DESIGN.md
    midpoint encode random / theta                     0.534 / 0.581        | 0.267 / 0.280
    round trip (decode of encode)                      0.130                | 0.200 (0.181 against the ground truth itself)
    obb_to_aabb                                        1.000 (z: one rounding, half an ulp is the bound)   | 0.500
    filter scores                                      below 0.25           | 0.173 (every family, both widths); all else equal
    sampled loss dlogit / ddelta / bce / smooth-L1     <= 0.325 / 0.362 / 0.061 / 0.062   | <= 0.250 / 0.250 / 0.061 / 0.083
    anchors (both tables), head_flatten / head_unflatten, filter boxes / levels / counts, select_kept, match_anchors: equal.
    A scratch build with |log(16/1000)| off by 0.01 and select_kept ties broken by the higher index fails midpoint decode [clamp] and
    select_kept [n16384_random, all_equal, tied_boundary, zero_scores] for both widths, and nothing else.
Mutation shares (host test): clip 33 % of the AABB elements, 22 % of the midpoint rows; offset_clamp 16 % of the rows; thr 17 % of the
rows; inv_npos and no_beta 100 % of the affected gradients; pi, ge (686 exact-tie rows), pairing, min_gt, beyond_count, tie_high,
last_dup, no_low_quality break an equality.
"""
import math
import types

import numpy as np
import torch

from fcos_ref import ETA, F32, F64, U, allowance, check, check_equal, ratio  # noqa: F401  (re-exported for the two test files)

f32 = np.float32
LOG2000 = float(f32(7.6009024595420822))
LIM = float(f32(4.1351665567423561))
PI_REF = float(f32(3.141592))
HALF_PI_REF = float(f32(3.141592 / 2))
PI_TRUE32 = float(f32(math.pi))
GUARD = float(f32(1e-7))
COND = 1e-3


def NS(**kw):
    return types.SimpleNamespace(**kw)


def undecided_share(decided):
    return 0.0 if decided.numel() == 0 else 1.0 - decided.double().mean().item()


def angle_diff(a, b, period=PI_REF):
    return torch.remainder(a.double() - b.double() + period / 2, period) - period / 2


# ======================================================================================================================
# anchors
# ======================================================================================================================
SMALL = NS(mesh=(96, 32, 32), grids=((12, 8, 4), (6, 4, 2), (3, 2, 1)))               # strides (8,4,8), (16,8,16), (32,16,32); 5694 anchors
BIG = NS(mesh=(2048, 2048, 1024), grids=((1024, 1024, 512), (512, 512, 256), (256, 256, 128)))


def pyramid(spec):
    from oracle import anchors as OA
    grids = [tuple(g) for g in spec.grids]
    strides = [tuple(spec.mesh[i] // g[i] for i in range(3)) for g in grids]
    base = [OA.base_anchors(s).numpy().astype(np.int64) for s in OA.SIZES[:len(grids)]]
    A = base[0].shape[0]
    counts = [g[0] * g[1] * g[2] * A for g in grids]
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + c)
    return NS(mesh=spec.mesh, grids=grids, strides=strides, base=base, A=A, counts=counts, offsets=offsets, total=offsets[-1])


def anchor_cells(p, sel):
    """(level, ix, iy, iz, a) of the flat indices ``sel`` (python ints / int64), in integers."""
    sel = np.asarray(sel, dtype=np.int64)
    lev = np.searchsorted(np.asarray(p.offsets[1:], dtype=np.int64), sel, side="right")
    local = sel - np.asarray(p.offsets, dtype=np.int64)[lev]
    g = np.asarray(p.grids, dtype=np.int64)[lev]
    a = local % p.A
    cell = local // p.A
    iz = cell % g[:, 2]
    iy = (cell // g[:, 2]) % g[:, 1]
    ix = cell // (g[:, 2] * g[:, 1])
    return lev, ix, iy, iz, a


def anchors_ref(p, sel=None):
    """The closed form in integers (every anchor coordinate is an integer: rounded base + index * stride) -> float32 [K,6]."""
    sel = np.arange(p.total, dtype=np.int64) if sel is None else np.asarray(sel, dtype=np.int64)
    lev, ix, iy, iz, a = anchor_cells(p, sel)
    st = np.asarray(p.strides, dtype=np.int64)[lev]
    base = np.stack(p.base)[lev, a]
    sh = np.stack([ix, iy, iz], 1) * st
    return torch.from_numpy((np.concatenate([sh, sh], 1) + base).astype(np.float32))


def big_table_sel(p):
    """First / last anchor of each level, both sides of each level boundary and of 2^31 and 2^32."""
    pts = set()
    for l in range(len(p.grids)):
        pts.update((p.offsets[l], p.offsets[l + 1] - 1, p.offsets[l] + 1))
        if l:
            pts.add(p.offsets[l] - 1)
    for b in (1 << 31, 1 << 32):
        pts.update((b - 1, b, b + 1))
    pts.update((12, 13, p.A * 512 - 1, p.A * 512, p.A * 512 * 1024, p.total - 14))
    return sorted(v for v in pts if 0 <= v < p.total)


# ======================================================================================================================
# coders
# ======================================================================================================================
def aabb_decode(d, an, dt=F64, mut=None, bound=False):
    d, an = d.to(dt), an.to(dt)
    clip = LIM if mut == "clip" else LOG2000
    w = an[:, 3:] - an[:, :3]
    c = an[:, :3] + 0.5 * w
    dw = d[:, :3] * w
    pc = dw + c
    half = 0.5 * (torch.exp(d[:, 3:].clamp(max=clip)) * w)
    out = torch.cat([pc - half, pc + half], 1)
    if not bound:
        return out
    b = U * (pc.abs() + 2 * dw.abs() + c.abs() + 0.5 * w.abs()) + 6 * U * half
    return out, U * out.abs() + torch.cat([b, b], 1) + ETA


def aabb_encode(gt, an, dt=F64, bound=False):
    gt, an = gt.to(dt), an.to(dt)
    aw = an[:, 3:] - an[:, :3]
    ac = an[:, :3] + 0.5 * aw
    gw = gt[:, 3:] - gt[:, :3]
    gc = gt[:, :3] + 0.5 * gw
    oc, ol = (gc - ac) / aw, torch.log(gw / aw)
    out = torch.cat([oc, ol], 1)
    if not bound:
        return out
    bc = U * ((gc - ac).abs() + ac.abs() + gc.abs() + 0.5 * (aw + gw.abs())) / aw + 3 * U * oc.abs()
    return out, torch.cat([bc, 4 * U + 4 * U * ol.abs()], 1) + ETA


def _pymod(a, b):
    r = torch.fmod(a, b)
    return torch.where((r != 0) & (r < 0), r + b, r)


def mid_decode(d, an, dt=F64, mut=None, bound=False):
    """delta_sp2bbox + rectpoly2obb + regular_obb in the kernel's operation order.  With ``bound``: (out, bound [K,7], info)."""
    d, an = d.to(dt), an.to(dt)
    lim = LOG2000 if mut == "clip" else LIM
    off = 1.0 if mut == "offset_clamp" else 0.5
    pi, hp = (PI_TRUE32, PI_TRUE32 / 2) if mut == "pi" else (PI_REF, HALF_PI_REF)
    pc = (an[:, :3] + an[:, 3:]) * 0.5
    pw = an[:, 3:] - an[:, :3]
    s = pw * torch.exp(d[:, 3:6].clamp(-lim, lim))
    g = pc + pw * d[:, :3]
    da, db = d[:, 6].clamp(-off, off), d[:, 7].clamp(-off, off)
    gx, gy, gw, gh = g[:, 0], g[:, 1], s[:, 0], s[:, 1]
    x1, y1, x2, y2 = gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5
    ga, ga_, gb, gb_ = gx + da * gw, gx - da * gw, gy + db * gh, gy - db * gh
    px, py = torch.stack([ga, x2, ga_, x1], 1), torch.stack([y1, gb, y2, gb_], 1)
    cx, cy = px - gx[:, None], py - gy[:, None]
    diag = torch.sqrt(cx * cx + cy * cy)
    md = diag.max(1).values
    sc = md[:, None] / diag
    qx_, qy_ = cx * sc, cy * sc
    px2, py2 = qx_ + gx[:, None], qy_ + gy[:, None]
    dx, dy = px2[:, 1] - px2[:, 0] + GUARD, -(py2[:, 1] - py2[:, 0])
    th = torch.atan2(dy, dx)
    cs, sn = torch.cos(th), torch.sin(th)
    mx = (((px2[:, 0] + px2[:, 1]) + px2[:, 2]) + px2[:, 3]) / 4
    my = (((py2[:, 0] + py2[:, 1]) + py2[:, 2]) + py2[:, 3]) / 4
    qx, qy = px2 - mx[:, None], py2 - my[:, None]
    rx = qx * cs[:, None] + qy * (-sn[:, None])
    ry = qx * sn[:, None] + qy * cs[:, None]
    w = rx.max(1).values - rx.min(1).values
    h = ry.max(1).values - ry.min(1).values
    wide = (w >= h) if mut == "ge" else (w > h)
    tr = torch.where(wide, th, th + hp)
    tr = _pymod(tr + hp, torch.tensor(pi, dtype=dt)) - hp
    out = torch.stack([mx, my, g[:, 2], torch.where(wide, w, h), torch.where(wide, h, w), s[:, 2], tr], 1)
    if not bound:
        return out
    e_s = 6 * U * s
    e_g = U * g.abs() + 2 * U * (pw * d[:, :3]).abs() + U * pc.abs()
    e_gw, e_gh = e_s[:, 0], e_s[:, 1]
    e_ox = torch.stack([da.abs() * e_gw + U * (da * gw).abs(), 0.5 * e_gw, da.abs() * e_gw + U * (da * gw).abs(), 0.5 * e_gw], 1)
    e_oy = torch.stack([0.5 * e_gh, db.abs() * e_gh + U * (db * gh).abs(), 0.5 * e_gh, db.abs() * e_gh + U * (db * gh).abs()], 1)
    e_cx = U * px.abs() + U * cx.abs() + e_ox
    e_cy = U * py.abs() + U * cy.abs() + e_oy
    e_diag = (cx.abs() * e_cx + cy.abs() * e_cy) / diag + 3 * U * diag
    e_md = e_diag.max(1).values
    e_sc = sc * (e_md[:, None] / md[:, None] + e_diag / diag + 2 * U)
    e_rx = sc * e_cx + cx.abs() * e_sc + U * qx_.abs() + U * px2.abs()
    e_ry = sc * e_cy + cy.abs() * e_sc + U * qy_.abs() + U * py2.abs()
    r = torch.hypot(dx, dy)
    e_th = (e_rx[:, 0] + e_rx[:, 1] + e_ry[:, 0] + e_ry[:, 1] + 2 * U * (dx.abs() + dy.abs())) / r + 12 * U * th.abs() + ETA
    Mx, My = px2.abs().max(1).values, py2.abs().max(1).values
    e_qx = e_rx + (e_rx.max(1).values + 3 * U * Mx)[:, None] + U * qx.abs()
    e_qy = e_ry + (e_ry.max(1).values + 3 * U * My)[:, None] + U * qy.abs()
    e_q = (e_qx + e_qy + 6 * U * (qx.abs() + qy.abs())).max(1).values
    delta = e_th.clamp(max=math.pi / 2)
    e_w = 2 * e_q + U * w + w * (1 - torch.cos(delta)) + h * torch.sin(delta)
    e_h = 2 * e_q + U * h + h * (1 - torch.cos(delta)) + w * torch.sin(delta)
    e_x = e_rx.max(1).values + e_g[:, 0] + 3 * U * Mx
    e_y = e_ry.max(1).values + e_g[:, 1] + 3 * U * My
    e_tr = e_th + 6 * U * math.pi
    bnd = torch.stack([e_x, e_y, e_g[:, 2], torch.where(wide, e_w, e_h), torch.where(wide, e_h, e_w), e_s[:, 2], e_tr], 1) + ETA
    side = torch.stack([w, h, s[:, 2]], 1).max(1).values
    swap_ok = (w - h).abs() > e_w + e_h
    decided = bnd <= COND * side[:, None]
    decided[:, 3] &= swap_ok
    decided[:, 4] &= swap_ok
    decided[:, 6] &= swap_ok
    larger = NS(bound=torch.maximum(e_w, e_h) + ETA, value=torch.maximum(w, h))
    return out, bnd, NS(decided=decided, side=side, w=w, h=h, wide=wide, larger=larger, th=th, swap_ok=swap_ok)


def mid_encode(gt, an, dt=F64, mut=None, bound=False):
    """bbox2delta_sp in the kernel's operation order."""
    gt, an = gt.to(dt), an.to(dt)
    thr = 0.01 if mut == "thr" else 0.1
    cx, cy, w, h, t = gt[:, 0], gt[:, 1], gt[:, 3], gt[:, 4], gt[:, 6]
    cs, sn = torch.cos(t), torch.sin(t)
    bx = (w / 2 * cs).abs() + (h / 2 * sn).abs()
    by = (w / 2 * sn).abs() + (h / 2 * cs).abs()
    hx1, hy1, hx2, hy2 = cx - bx, cy - by, cx + bx, cy + by
    gx, gy, gw, gh = (hx1 + hx2) * 0.5, (hy1 + hy2) * 0.5, hx2 - hx1, hy2 - hy1
    v1x, v1y, v2x, v2y = w / 2 * cs, -w / 2 * sn, -h / 2 * sn, -h / 2 * cs
    xs = torch.stack([cx + v1x + v2x, cx + v1x - v2x, cx - v1x - v2x, cx - v1x + v2x], 1)
    ys = torch.stack([cy + v1y + v2y, cy + v1y - v2y, cy - v1y - v2y, cy - v1y + v2y], 1)
    ymin, xmax = ys.min(1).values, xs.max(1).values
    far = torch.full_like(xs, -1000.0)
    ga = torch.where((ys - ymin[:, None]).abs() > thr, far, xs).max(1).values
    gb = torch.where((xs - xmax[:, None]).abs() > thr, far, ys).max(1).values
    pc = (an[:, :3] + an[:, 3:]) * 0.5
    pw = an[:, 3:] - an[:, :3]
    out = torch.stack([(gx - pc[:, 0]) / pw[:, 0], (gy - pc[:, 1]) / pw[:, 1], (gt[:, 2] - pc[:, 2]) / pw[:, 2],
                       torch.log(gw / pw[:, 0]), torch.log(gh / pw[:, 1]), torch.log(gt[:, 5] / pw[:, 2]),
                       (ga - gx) / gw, (gb - gy) / gh], 1)
    if not bound:
        return out
    wh = w.abs() + h.abs()

    def centre(c, b, h1, h2, gc, gs, p, ps, vs, gsel, o_c, o_l, o_o):
        e_b = 3 * U * wh + U * b
        e_gc = U * gc.abs() + U * (h1.abs() + h2.abs()) / 2 + e_b
        e_gs = U * gs + U * (h1.abs() + h2.abs()) + 2 * e_b
        e_v = 3 * U * wh + 2 * U * (c.abs() + wh / 2)
        b_c = (e_gc + U * p.abs() + U * (gc - p).abs()) / ps + 3 * U * o_c.abs()
        b_l = e_gs / gs + 4 * U + 4 * U * o_l.abs()
        b_o = (e_v + e_gc + U * (gsel - gc).abs()) / gs + o_o.abs() * e_gs / gs + 3 * U * o_o.abs()
        return b_c, b_l, b_o, e_v
    bcx, blx, box_, evx = centre(cx, bx, hx1, hx2, gx, gw, pc[:, 0], pw[:, 0], xs, ga, out[:, 0], out[:, 3], out[:, 6])
    bcy, bly, boy, evy = centre(cy, by, hy1, hy2, gy, gh, pc[:, 1], pw[:, 1], ys, gb, out[:, 1], out[:, 4], out[:, 7])
    bcz = (U * pc[:, 2].abs() + U * (gt[:, 2] - pc[:, 2]).abs()) / pw[:, 2] + 3 * U * out[:, 2].abs()
    blz = 4 * U + 4 * U * out[:, 5].abs()
    bnd = torch.stack([bcx, bcy, bcz, blx, bly, blz, box_, boy], 1) + ETA
    decided = torch.ones_like(bnd, dtype=torch.bool)
    # the x offset selects on y (vertex error evy) and the y offset on x
    decided[:, 6] = (((ys - ymin[:, None]).abs() - 0.1).abs() > 2 * evy[:, None] + U).all(1)
    decided[:, 7] = (((xs - xmax[:, None]).abs() - 0.1).abs() > 2 * evx[:, None] + U).all(1)
    return out, bnd, NS(decided=decided)


def obb_to_aabb(o, dt=F64, bound=False):
    o = o.to(dt)
    cs, sn = torch.cos(o[:, 6]), torch.sin(o[:, 6])
    bx = (o[:, 3] / 2 * cs).abs() + (o[:, 4] / 2 * sn).abs()
    by = (o[:, 3] / 2 * sn).abs() + (o[:, 4] / 2 * cs).abs()
    bz = o[:, 5] / 2
    out = torch.stack([o[:, 0] - bx, o[:, 1] - by, o[:, 2] - bz, o[:, 0] + bx, o[:, 1] + by, o[:, 2] + bz], 1)
    if not bound:
        return out
    wh = o[:, 3].abs() + o[:, 4].abs()
    e = torch.stack([3 * U * wh + U * bx, 3 * U * wh + U * by, torch.zeros_like(bz)], 1)
    return out, U * out.abs() + torch.cat([e, e], 1) + ETA


def decode_jacobian_bound(d, an, e_d):
    """|d out / d deltas| e_d per output column of the float64 midpoint decode (autograd): how an error of the encoded deltas shows in the
    decoded box (round trip)."""
    d = d.double().clone().requires_grad_(True)
    out = mid_decode(d, an, F64)
    cols = []
    for k in range(7):
        (gk,) = torch.autograd.grad(out[:, k].sum(), d, retain_graph=True)
        cols.append((gk.abs() * e_d).sum(1))
    return torch.stack(cols, 1)


# ---- coder families ---------------------------------------------------------------------------------------------------
CODER_ROWS = 2048
_EPS = (2.0 ** -10, 0.25)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sel(p, k, seed):
    return torch.randperm(p.total, generator=_gen(seed))[:k].sort().values


def _mid_deltas(k, seed, offs=0.45):
    g = _gen(seed)
    d = torch.cat([torch.randn(k, 6, generator=g) * 0.5, (torch.rand(k, 2, generator=g) * 2 - 1) * offs], 1)
    return d.float()


def _nudge(v, up):
    return float(np.nextafter(f32(v), f32(np.inf if up else -np.inf)))


def decode_family(name, coder):
    """-> NS(sel int64 [K], deltas f32 [K,dw], anchors f32 [K,6], cap, constructed).  Every family lives on the SMALL pyramid."""
    p = pyramid(SMALL)
    k = CODER_ROWS
    if coder == 0:
        seed = {"random": 11, "clamp": 12}[name]
        sel = _sel(p, k, seed)
        d = (torch.randn(k, 6, generator=_gen(seed + 100)) * 0.5).float()
        if name == "clamp":          # one size clamp per row: log 2000 +- eps, exactly on it, and one step on either side
            vals = [LOG2000 + e for e in _EPS] + [LOG2000 - e for e in _EPS] + [LOG2000, _nudge(LOG2000, True), _nudge(LOG2000, False)]
            for i in range(k):
                d[i, 3 + i % 3] = vals[(i // 3) % len(vals)]
    else:
        seed = {"random": 21, "clamp": 22, "square": 23, "degenerate": 24, "theta": 25}[name]
        sel = _sel(p, k, seed)
        d = _mid_deltas(k, seed + 100)
        if name == "clamp":
            sizes = [s * (LIM + t) for s in (1, -1) for t in (_EPS[0], -_EPS[0], _EPS[1], -_EPS[1], 0.0)]
            offs = [s * (0.5 + t) for s in (1, -1) for t in (_EPS[0], -_EPS[0], _EPS[1], -_EPS[1], 0.0)]
            for i in range(k):
                j = i % 5
                if j < 3:
                    d[i, 3 + j] = sizes[(i // 5) % len(sizes)]
                    if j < 2:        # the other planar size stays unclamped but within e of it: a needle's short side is undecided by conditioning
                        d[i, 4 - j] = math.copysign(LIM - 1.0 - 0.3 * (i % 7) / 7, sizes[(i // 5) % len(sizes)])
                else:
                    d[i, 3 + j] = offs[(i // 5) % len(offs)]
        elif name == "square":       # w ~ h from both sides at a decided distance: equal planar sizes, offsets db = da + t
            an = anchors_ref(p, sel.numpy())
            pw = (an[:, 3:] - an[:, :3]).double()
            t = torch.tensor([3e-3, -3e-3, 1e-2, -1e-2, 0.05, -0.05])[torch.arange(k) % 6]
            d[:, 3] = 0.3
            d[:, 4] = (0.3 + torch.log(pw[:, 0] / pw[:, 1])).float()
            a = (torch.rand(k, generator=_gen(seed + 1)) * 0.6 - 0.3)
            d[:, 6] = a.float()
            d[:, 7] = (a + t).float()
        elif name == "theta":        # decoded angles near 0, +-pi/2 and the wrap: the encoded deltas of boxes at those angles
            an = anchors_ref(p, sel.numpy())
            pc, pw = (an[:, :3] + an[:, 3:]) / 2, an[:, 3:] - an[:, :3]
            w = pw[:, 0] * (1.0 + torch.rand(k, generator=_gen(seed + 1)))
            t = torch.tensor([0.04, -0.04, 0.1, -0.1, HALF_PI_REF - 0.04, -HALF_PI_REF + 0.04, HALF_PI_REF - 0.1, -HALF_PI_REF + 0.1])[torch.arange(k) % 8]
            gt = torch.cat([pc, w[:, None], (w * (0.5 + 0.4 * torch.rand(k, generator=_gen(seed + 2))))[:, None], pw[:, 2:3], t[:, None]], 1).float()
            d = mid_encode(gt, an, F64).float()
        elif name == "degenerate":   # da -> +0.5 with db -> -0.5 (p0 -> p1), and the mirror (the polygon collapses onto its diagonal)
            e = torch.tensor([0.0, 2.0 ** -20, 2.0 ** -16, 2.0 ** -12, 2.0 ** -8, 2.0 ** -6, -0.25, -2.0 ** -10])[torch.arange(k) % 8]
            sgn = torch.where((torch.arange(k) // 8) % 2 == 0, 1.0, -1.0)
            d[:, 6] = (sgn * (0.5 - e)).float()
            d[:, 7] = (-sgn * (0.5 - e)).float()
    an = anchors_ref(p, sel.numpy())
    return NS(name=name, coder=coder, sel=sel, deltas=d.contiguous(), anchors=an, cap=0.01 if name == "random" else 0.0,
              pyramid=p)


def gt_family(name):
    """Ground-truth OBBs [K,7] (w > h, theta in [-pi/2, pi/2)) next to their anchors.  'random': any angle; 'theta': near 0, +-pi/2 and
    the wrap; 'roundtrip': angles at which one vertex is selected per offset, so decode(encode(gt)) returns gt."""
    p = pyramid(SMALL)
    k = CODER_ROWS
    seed = {"random": 31, "theta": 32, "roundtrip": 33}[name]
    g = _gen(seed)
    sel = _sel(p, k, seed)
    an = anchors_ref(p, sel.numpy())
    pc, pw = (an[:, :3] + an[:, 3:]) / 2, an[:, 3:] - an[:, :3]
    ctr = pc + (torch.rand(k, 3, generator=g) - 0.5) * pw
    w = pw[:, 0] * (0.6 + torch.rand(k, generator=g))
    h = w * ((0.5 if name == "roundtrip" else 0.3) + 0.4 * torch.rand(k, generator=g))
    dz = pw[:, 2] * (0.5 + torch.rand(k, generator=g))
    if name == "random":
        t = (torch.rand(k, generator=g) - 0.5) * 3.1
    elif name == "theta":
        base = torch.tensor([0.0, 1e-4, -1e-4, 0.02, -0.02, HALF_PI_REF - 1e-4, -HALF_PI_REF + 1e-4, HALF_PI_REF - 0.02, -HALF_PI_REF + 0.02,
                             -HALF_PI_REF, 0.3, -0.3, 0.003, -0.003, HALF_PI_REF - 0.003, -HALF_PI_REF + 0.003])
        t = base[torch.arange(k) % base.numel()]
    else:
        t = (0.1 + torch.rand(k, generator=g) * (HALF_PI_REF - 0.2)) * torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0)
    gt = torch.cat([ctr, w[:, None], h[:, None], dz[:, None], t[:, None]], 1).float().contiguous()
    return NS(name=name, sel=sel, gt=gt, anchors=an, cap=0.01 if name == "random" else 0.0, pyramid=p)


def gt6_family():
    p = pyramid(SMALL)
    k = CODER_ROWS
    g = _gen(41)
    sel = _sel(p, k, 41)
    an = anchors_ref(p, sel.numpy())
    pc, pw = (an[:, :3] + an[:, 3:]) / 2, an[:, 3:] - an[:, :3]
    ctr = pc + (torch.rand(k, 3, generator=g) - 0.5) * pw
    half = pw * (0.2 + torch.rand(k, 3, generator=g))
    gt = torch.cat([ctr - half, ctr + half], 1).float().contiguous()
    return NS(name="random", sel=sel, gt=gt, anchors=an, cap=0.0, pyramid=p)


def scatter_deltas(fam):
    """The family's rows placed into a dense [T, dw] delta buffer (what decode_boxes indexes by the flat anchor number)."""
    full = torch.zeros(fam.pyramid.total, fam.deltas.shape[1])
    full[fam.sel] = fam.deltas
    return full


# ======================================================================================================================
# head_flatten / head_unflatten
# ======================================================================================================================
HEAD_CASES = [(1, 13, 6, 0), (1, 13, 8, 11), (37, 13, 6, 11), (37, 13, 8, 0), (300, 13, 8, 11), (18000, 13, 8, 0)]      # cells, A, dw, pad


def head_case(cells, A, dw, pad, seed=0):
    g = _gen(seed + cells)
    ld = A * (1 + dw) + pad
    head = torch.randn(cells, ld, generator=g)
    return NS(cells=cells, A=A, dw=dw, ld=ld, head=head, logits=torch.randn(cells * A, generator=g),
              deltas=torch.randn(cells * A, dw, generator=g), scale2=torch.tensor([0.37, 5.0]))


def head_flatten_ref(c):
    """Index-by-index scatter: column k < A of a cell is the logit of anchor k; column A + a dw + j is delta j of anchor a."""
    head = c.head.numpy()
    logits = np.empty(c.cells * c.A, np.float32)
    deltas = np.empty((c.cells * c.A, c.dw), np.float32)
    for a in range(c.A):
        logits[a::c.A] = head[:, a]
        for j in range(c.dw):
            deltas[a::c.A, j] = head[:, c.A + a * c.dw + j]
    return torch.from_numpy(logits), torch.from_numpy(deltas)


def head_unflatten_ref(c, scaled, bf16):
    s0, s1 = (c.scale2[0], c.scale2[1]) if scaled else (torch.tensor(1.0), torch.tensor(1.0))
    out = torch.zeros(c.cells, c.ld)
    lg, dl = c.logits.reshape(c.cells, c.A), c.deltas.reshape(c.cells, c.A, c.dw)
    for a in range(c.A):
        out[:, a] = lg[:, a] * s0                                       # fp32 product, one rounding
        for j in range(c.dw):
            out[:, c.A + a * c.dw + j] = dl[:, a, j] * s1
    return out.to(torch.bfloat16) if bf16 else out                     # torch's cast is round-to-nearest-even


# ======================================================================================================================
# filter_candidates
# ======================================================================================================================
FILTER_MAX = 16384
MIN_SIZE = 2.0 ** -10            # dyadic: extents built from it compare exactly
GRID = (96.0, 32.0, 32.0)


def sigmoid_bound(logits):
    s = torch.sigmoid(logits.double())
    return s, 8 * U * s + ETA


def filter_ref(boxes, logits, levels, valid, grid, min_size, thresh, fix, mut=None):
    """clip_to_grid -> big_enough -> score threshold on numpy rows; returns (boxes f32 [m,w], score f64 [m], levels, source rows)."""
    b = boxes.numpy()
    W = b.shape[1]
    live = np.nonzero(valid.numpy())[0]
    bl = b[live]
    if W == 6:
        hi = np.asarray(grid, np.float32)
        cl = np.concatenate([np.minimum(np.maximum(bl[:, :3], f32(0)), hi), np.minimum(np.maximum(bl[:, 3:], f32(0)), hi)], 1)
        src_box = np.arange(live.size)
    else:
        with np.errstate(invalid="ignore"):
            ok = np.ones(live.size, bool)
            for ax in range(3):
                ok &= (bl[:, ax] >= 0) & (bl[:, ax] <= f32(grid[ax]))
        src_box = np.nonzero(ok)[0]
        cl = bl[src_box]
    own = bool(fix) != (mut == "pairing")
    pair = src_box if own else np.arange(src_box.size)                 # quirk B3: surviving box p takes the score / level of live candidate p
    ext = (cl[:, 3:6] - cl[:, 0:3]) if W == 6 else cl[:, 3:6]
    big = (ext > f32(min_size)).all(1) if mut == "min_gt" else (ext >= f32(min_size)).all(1)
    score = torch.sigmoid(logits.double()).numpy()[live[pair]]
    keep = big & (score >= float(f32(thresh)))
    rows = live[pair][keep]
    return NS(boxes=torch.from_numpy(cl[keep]), scores=torch.from_numpy(score[keep]), levels=levels[rows].clone(), rows=rows,
              count=int(keep.sum()))


FILTER_NAMES = ("n1", "n15", "n16", "n17", "n1000", "n16384", "holes", "all_invalid", "last_only", "edges", "min_size", "thresh", "none")


def filter_case(name, W):
    """-> NS(boxes, logits, levels, valid, thresh).  Logits lie on a 0.25 grid so a threshold between two sigmoid values decides exactly."""
    n = {"n1": 1, "n15": 15, "n16": 16, "n17": 17, "n1000": 1000, "n16384": 16384}.get(name, 1000)
    g = _gen(50 + n + W)
    size = torch.tensor(GRID)
    if W == 6:
        lo = torch.rand(n, 3, generator=g) * size * 1.2 - 0.1 * size
        boxes = torch.cat([lo, lo + torch.rand(n, 3, generator=g) * 20], 1)
    else:
        boxes = torch.cat([torch.rand(n, 3, generator=g) * size * 1.2 - 0.1 * size, torch.rand(n, 3, generator=g) * 20 + 0.5,
                           (torch.rand(n, 1, generator=g) - 0.5) * 3], 1)
    logits = torch.randint(-16, 17, (n,), generator=g).float() * 0.25
    levels = torch.sort(torch.randint(0, 4, (n,), generator=g)).values.to(torch.int32)
    valid = torch.ones(n, dtype=torch.uint8)
    thresh = 0.0
    if name == "holes":
        valid = (torch.rand(n, generator=g) < 0.6).to(torch.uint8)
    elif name == "all_invalid":
        valid.zero_()
    elif name == "last_only":
        valid.zero_()
        valid[-1] = 1
        boxes[-1] = torch.tensor([10., 10., 10., 20., 20., 20.] if W == 6 else [10., 10., 10., 5., 5., 5., 0.3])
    elif name == "edges":
        up = [_nudge(s, True) for s in GRID]
        tiny = -float(np.nextafter(f32(0), f32(1)))
        for i in range(n):
            ax, kind = i % 3, (i // 3) % 6
            if W == 7:      # centre exactly on 0 / on the grid size (kept), one step outside (dropped), NaN (dropped)
                boxes[i, ax] = [0.0, GRID[ax], tiny, up[ax], float("nan"), -0.0][kind]
            else:           # corners on both sides of the clamp
                boxes[i, ax] = [0.0, -3.0, tiny, 5.0, 0.5, 1.0][kind]
                boxes[i, ax + 3] = [GRID[ax], GRID[ax] + 4.0, up[ax], GRID[ax] - 1.0, GRID[ax], 40.0 * GRID[ax]][kind]
    elif name == "min_size":
        below = float(np.nextafter(f32(MIN_SIZE), f32(0)))
        for i in range(n):
            ax, e = i % 3, [MIN_SIZE, below, 2 * MIN_SIZE, 0.0][(i // 3) % 4]
            if W == 7:
                boxes[i, :3] = torch.tensor([8.0, 8.0, 8.0])
                boxes[i, 3 + ax] = e
            else:           # lo = 8 (ulp 2^-20 there): lo + e is exact for e = MIN_SIZE, 2 MIN_SIZE, 0; the 'below' rows use lo = 0
                lo_ = 0.0 if e == below else 8.0
                boxes[i, ax], boxes[i, ax + 3] = lo_, lo_ + e
    elif name == "thresh":
        thresh = 0.5 * (float(torch.sigmoid(torch.tensor(0.25, dtype=F64))) + float(torch.sigmoid(torch.tensor(0.5, dtype=F64))))
    elif name == "none":
        thresh = 0.99
    return NS(name=name, boxes=boxes.float().contiguous(), logits=logits, levels=levels, valid=valid, thresh=thresh, n=n)


# ======================================================================================================================
# select_kept
# ======================================================================================================================
def select_ref(boxes, scores, levels, keep, count, post, mut=None):
    n = boxes.shape[0]
    cnt = n if (count is None or mut == "beyond_count") else min(int(count), n)
    idx = [i for i in range(cnt) if keep[i]]
    s = scores.numpy()
    idx.sort(key=(lambda i: (-s[i], -i)) if mut == "tie_high" else (lambda i: (-s[i], i)))
    m = min(len(idx), post)
    ob = torch.zeros(post, boxes.shape[1])
    os_ = torch.zeros(post)
    ol = torch.full((post,), -1.0)
    top = torch.tensor(idx[:m], dtype=torch.long)
    ob[:m], os_[:m], ol[:m] = boxes[top], scores[top], levels[top].float()
    return ob, os_, ol, m


SELECT_NAMES = ("n1", "n2", "n1000_random", "n16384_random", "count_short", "kept0", "kept1", "post-1", "post", "post+1", "all_kept", "all_equal",
                "tied_boundary", "zero_scores")


def select_case(name, W):
    n = {"n1": 1, "n2": 2, "n16384_random": 16384}.get(name, 1000)
    post = {"n1": 1, "n2": 3, "n16384_random": 2500}.get(name, 100)
    g = _gen(60 + n + W + len(name))
    boxes = torch.randn(n, W, generator=g)
    scores = torch.rand(n, generator=g)
    levels = torch.randint(0, 4, (n,), generator=g).to(torch.int32)
    keep = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
    count = n

    def exactly(k):
        keep.zero_()
        keep[torch.randperm(n, generator=g)[:k]] = 1
    if name in ("n1", "n2"):
        keep.fill_(1)
    elif name == "count_short":
        count = 600
        keep[600:] = 1           # flags beyond count must be ignored
        scores[600:] = 2.0       # ... although they would win
    elif name == "kept0":
        exactly(0)
    elif name == "kept1":
        exactly(1)
    elif name == "post-1":
        exactly(post - 1)
    elif name == "post":
        exactly(post)
    elif name == "post+1":
        exactly(post + 1)
    elif name == "all_kept":
        keep.fill_(1)
    elif name == "all_equal":
        scores.fill_(0.25)
    elif name == "tied_boundary":          # ~post/2 rows above, then a run of ties that spans the post boundary
        keep.fill_(1)
        scores = torch.where(torch.arange(n) % 4 == 0, torch.tensor(0.5), scores * 0.4)
        scores[torch.randperm(n, generator=g)[:post // 2]] = 0.9
    elif name == "zero_scores":
        scores[torch.randperm(n, generator=g)[:n // 2]] = 0.0
        keep.fill_(1)
        post = 900
    return NS(name=name, boxes=boxes, scores=scores, levels=levels, keep=keep, count=count, post=post, n=n)


# ======================================================================================================================
# match_anchors
# ======================================================================================================================
MAX_GT = 1024
FG, BG = 0.35, 0.2


def iou_f32(gt, an):
    """[G,6] x [T,6] -> [G,T], op for op geo::iou3d_aabb(gt, anchor) in numpy float32 (+ - x / min max: correctly rounded everywhere)."""
    a, b = gt.numpy().astype(np.float32)[:, None, :], an.numpy().astype(np.float32)[None, :, :]
    va = (a[..., 3] - a[..., 0]) * (a[..., 4] - a[..., 1]) * (a[..., 5] - a[..., 2])
    vb = (b[..., 3] - b[..., 0]) * (b[..., 4] - b[..., 1]) * (b[..., 5] - b[..., 2])
    e = [np.maximum(np.minimum(a[..., k + 3], b[..., k + 3]) - np.maximum(a[..., k], b[..., k]), f32(0)) for k in range(3)]
    inter = e[0] * e[1] * e[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (va + vb - inter)


def padding_ref(p, ori):
    """True where the anchor lies in the padding: its cell index is not below ceil(ori / stride) on some axis (fp32, as the kernel)."""
    lev, ix, iy, iz, _ = anchor_cells(p, np.arange(p.total))
    st = np.asarray(p.strides, np.float32)[lev]
    lim = np.ceil(np.asarray(ori, np.float32)[None, :] / st).astype(np.int64)
    return ~((ix < lim[:, 0]) & (iy < lim[:, 1]) & (iz < lim[:, 2]))


def match_ref(q, fg, bg, padded=None, mut=None):
    """Matcher on a quality matrix q [G,T] (float32 or float64 numpy): the first maximum per anchor, thresholds, then the low-quality
    rule q == max over the anchors of its GT row.  -> labels f32 [T], matched int32 [T] (clamped at 0)."""
    q = q.copy()
    if padded is not None:
        q[:, padded] = -1.0
    if mut == "last_dup":
        besti = q.shape[0] - 1 - np.argmax(q[::-1], axis=0)
    else:
        besti = np.argmax(q, axis=0)                                   # numpy: the first maximum
    best = q[besti, np.arange(q.shape[1])]
    idx = besti.copy()
    idx[best < q.dtype.type(bg)] = -1
    idx[(best >= q.dtype.type(bg)) & (best < q.dtype.type(fg))] = -2
    if mut != "no_low_quality":
        attains = (q == q.max(axis=1, keepdims=True)).any(axis=0)
        idx[attains] = besti[attains]
    lab = np.where(idx >= 0, 1.0, np.where(idx == -1, 0.0, -1.0)).astype(np.float32)
    if padded is not None:
        lab[padded] = -1.0
    return torch.from_numpy(lab), torch.from_numpy(np.maximum(idx, 0).astype(np.int32))


MATCH_NAMES = ("g1", "g2", "g1024", "duplicate", "equal_anchor", "outside", "low_quality", "ori")


def match_case(name):
    """-> NS(gt f32 [G,6], ori or None) on the SMALL pyramid."""
    p = pyramid(SMALL)
    g = _gen(70 + len(name))
    size = torch.tensor(GRID)

    def rand_gt(k):
        c = torch.rand(k, 3, generator=g) * size
        half = 1.5 + torch.rand(k, 3, generator=g) * 7
        return torch.cat([c - half, c + half], 1).float()
    an = anchors_ref(p)
    ori = None
    if name == "g1":
        gt = rand_gt(1)
    elif name == "g2":
        gt = rand_gt(2)
    elif name == "g1024":
        gt = rand_gt(1024)
    elif name == "duplicate":
        gt = rand_gt(6)
        gt[4] = gt[1]                        # the first of two identical boxes wins
    elif name == "equal_anchor":
        gt = rand_gt(3)
        gt[1] = an[13 * 101 + 4]             # IoU exactly 1
    elif name == "outside":
        gt = rand_gt(3)
        gt[2] = torch.tensor([500., 500., 500., 520., 520., 520.])
    elif name == "low_quality":              # a 5.5-cube centred in the 8-cube anchor of cell (5, 3, 2): best IoU 5.5^3 / 512 = 0.325, between bg and fg
        gt = rand_gt(2)
        gt[1] = torch.tensor([37.25, 9.25, 13.25, 42.75, 14.75, 18.75])
    elif name == "ori":
        gt = rand_gt(5)
        ori = (70.0, 27.0, 21.0)             # no multiple of the strides (8,4,8), (16,8,16), (32,16,32)
    return NS(name=name, gt=gt.contiguous(), ori=ori, pyramid=p, anchors=an)


def match_expect(c, mut=None):
    q = iou_f32(c.gt, c.anchors)
    padded = padding_ref(c.pyramid, c.ori) if c.ori is not None else None
    return match_ref(q, f32(FG), f32(BG), padded, mut), q


# ======================================================================================================================
# rpn_sampled_loss
# ======================================================================================================================
LOSS_ROWS = 2000
BETA = float(f32(1.0 / 9.0))
LOSS_COUNTS = ((0, 5), (5, 0), (1, 0), (100, 156), (128, 129), (300, 400))


def loss_case(npos, nneg, dw, seed=0):
    g = _gen(80 + npos * 7 + nneg + dw + seed)
    logits = torch.randn(LOSS_ROWS, generator=g) * 3
    deltas = torch.randn(LOSS_ROWS, dw, generator=g)
    perm = torch.randperm(LOSS_ROWS, generator=g)
    pos, neg = perm[:npos].sort().values, perm[npos:npos + nneg].sort().values
    targets = torch.randn(npos, dw, generator=g) * 0.3
    special = torch.tensor([0.0, 20.0, -20.0, 100.0, -100.0, 1e-30, -1e-30, 88.0, -88.0, 104.0, -104.0])
    both = torch.cat([pos, neg])
    k = min(both.numel(), special.numel())
    logits[both[torch.randperm(both.numel(), generator=g)[:k]]] = special[:k]
    if npos:             # residuals of exactly 0, +-beta, beta (1 +- 2^-20): target 0 so that d = delta exactly
        res = torch.tensor([0.0, BETA, -BETA, BETA * (1 + 2.0 ** -20), BETA * (1 - 2.0 ** -20), -BETA * (1 + 2.0 ** -20),
                            -BETA * (1 - 2.0 ** -20), 3.0])
        m = min(dw, res.numel())
        for j in range(min(npos, 4)):
            targets[j, :m] = 0.0
            deltas[pos[j], :m] = res.roll(j)[:m]
    return NS(logits=logits, deltas=deltas, targets=targets.contiguous(), pos=pos, neg=neg, dw=dw, npos=npos, nneg=nneg)


def loss_eval(c, dt=F64, mut=None):
    """-> NS(bce, reg, g_logits [M], g_deltas [M,dw]) and, in float64, their bounds."""
    x = torch.cat([c.logits[c.pos], c.logits[c.neg]]).to(dt)
    y = torch.cat([torch.ones(c.npos), torch.zeros(c.nneg)]).to(dt)
    ns = c.npos + c.nneg
    inv = torch.tensor(1.0, dtype=dt) / (c.npos if mut == "inv_npos" else ns)
    e = torch.exp(-x.abs())
    lg = torch.log1p(e)
    lin = x.clamp(min=0) - x * y
    term = lin + lg
    sig = 1.0 / (1.0 + torch.exp(-x))
    gl = (sig - y) * inv
    d = (c.deltas[c.pos].to(dt) - c.targets.to(dt)).reshape(-1)
    ad = d.abs()
    beta = torch.tensor(BETA, dtype=dt)
    quad = 0.5 * d * d if mut == "no_beta" else 0.5 * d * d / beta
    rterm = torch.where(ad < beta, quad, ad - 0.5 * beta)
    gd = torch.where(ad < beta, d if mut == "no_beta" else d / beta, torch.sign(d)) * inv
    g_logits = torch.zeros(LOSS_ROWS, dtype=dt)
    g_logits[torch.cat([c.pos, c.neg])] = gl
    g_deltas = torch.zeros(LOSS_ROWS, c.dw, dtype=dt)
    g_deltas[c.pos] = gd.reshape(c.npos, c.dw)
    out = NS(bce=term.sum() * inv, reg=rterm.sum() * inv, g_logits=g_logits, g_deltas=g_deltas)
    if dt != F64:
        return out
    b_gl = (8 * U * sig + U * (sig - y).abs()) * inv + 3 * U * gl.abs() + ETA
    out.b_logits = torch.zeros(LOSS_ROWS, dtype=F64)
    out.b_logits[torch.cat([c.pos, c.neg])] = b_gl
    out.b_deltas = torch.zeros(LOSS_ROWS, c.dw, dtype=F64)
    out.b_deltas[c.pos] = (5 * U * gd.abs() + ETA).reshape(c.npos, c.dw)
    t_b = 2 * U * lin.abs() + 4 * U * e + 4 * U * lg + 2 * U * term.abs()
    out.b_bce = (t_b.sum() + (math.ceil(ns / 256) + 10) * U * term.abs().sum()) * inv + 2 * U * out.bce.abs() + ETA
    r_b = 5 * U * rterm.abs() + U * ad * (ad / beta).clamp(max=1.0)
    out.b_reg = (r_b.sum() + (math.ceil(max(d.numel(), 1) / 256) + 10) * U * rterm.abs().sum()) * inv + 2 * U * out.reg.abs() + ETA
    return out
