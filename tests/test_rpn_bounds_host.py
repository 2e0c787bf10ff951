"""Host side of tests/test_gpu_rpn_kernels.py (no GPU): the references of tests/rpn_ref.py are anchored to the oracle (oracle/coders.py,
oracle/anchors.py, oracle/boxes.py, torch's own losses) in fp32; their per-element bounds are shown to be satisfiable (the torch fp32
evaluation of the kernels' expressions stays inside every bound: its worst |err| / bound r is printed per family, run with -s) and sharp
(every mutation of rpn_ref lands outside 2 x bound on a stated share of the decided elements, or breaks an equality); the share of
undecided elements is held to its cap on every family: 1 % for the random ones, none for the constructed ones."""
import numpy as np
import pytest
import torch

import rpn_ref as R

F32, F64 = torch.float32, torch.float64


def share_outside(got, want, bound, decided, k=2.0):
    err = (got.double() - want).abs()[decided]
    return (err > k * bound[decided]).double().mean().item()


def report(what, got32, want, bound, decided, cap):
    r = R.ratio(got32[decided], want[decided], bound[decided])
    und = R.undecided_share(decided)
    print(f"{what}: r = {r:.3f}, undecided {100 * und:.4f} % (cap {100 * cap:g} %)")
    assert r <= 1.0, (what, r)
    assert und <= cap, (what, und)
    return r


# ======================================================================================================================
# anchors
# ======================================================================================================================
def test_small_pyramid_equals_the_oracle():
    from oracle import anchors as OA
    p = R.pyramid(R.SMALL)
    assert p.total == 5694 and p.total % 256 != 0 and len({s for st in p.strides for s in st}) > 1
    want = torch.cat(OA.all_anchors(R.SMALL.mesh, p.grids))
    assert torch.equal(R.anchors_ref(p), want)
    sel = np.array([0, 12, 13, p.offsets[1] - 1, p.offsets[1], p.offsets[2], p.total - 1])
    assert torch.equal(R.anchors_ref(p, sel), want[sel])


def test_big_table_levels_start_above_2_31_and_2_32():
    p = R.pyramid(R.BIG)
    assert p.offsets[1] > 1 << 32 and p.offsets[2] > p.offsets[1] and p.total > 1 << 32 and p.offsets[1] > 1 << 31
    sel = R.big_table_sel(p)
    assert {(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, p.offsets[1] - 1, p.offsets[1], p.offsets[2] - 1, p.offsets[2], p.total - 1} <= set(sel)
    lev, ix, iy, iz, a = R.anchor_cells(p, sel)
    for s, l, x, y, z, k in zip(sel, lev, ix, iy, iz, a):             # the closed form inverts: flat = first + ((x gy + y) gz + z) A + a
        g = p.grids[l]
        assert p.offsets[l] + ((int(x) * g[1] + int(y)) * g[2] + int(z)) * p.A + int(k) == s and 0 <= x < g[0]
    an = R.anchors_ref(p, sel)
    assert an.abs().max() < 2 ** 24                                     # every coordinate is an integer fp32 holds exactly


# ======================================================================================================================
# coders: oracle anchoring, r, undecided shares
# ======================================================================================================================
@pytest.mark.parametrize("name", ["random", "clamp"])
def test_aabb_decode(name):
    from oracle import coders as OC
    f = R.decode_family(name, 0)
    want, bound = R.aabb_decode(f.deltas, f.anchors, F64, bound=True)
    got = R.aabb_decode(f.deltas, f.anchors, F32)
    dec = torch.ones_like(bound, dtype=torch.bool)
    report(f"aabb decode {name}", got, want, bound, dec, f.cap)
    assert ((OC.aabb_decode(f.deltas, f.anchors).double() - want).abs() <= 2 * bound).all()


def test_aabb_encode():
    from oracle import coders as OC
    f = R.gt6_family()
    want, bound = R.aabb_encode(f.gt, f.anchors, F64, bound=True)
    dec = torch.ones_like(bound, dtype=torch.bool)
    report("aabb encode random", R.aabb_encode(f.gt, f.anchors, F32), want, bound, dec, f.cap)
    assert ((OC.aabb_encode(f.gt, f.anchors).double() - want).abs() <= 2 * bound).all()


def mid_err(got, want):
    err = (got.double() - want).abs()
    err[:, 6] = R.angle_diff(got[:, 6], want[:, 6]).abs()
    return err


@pytest.mark.parametrize("name", ["random", "clamp", "theta", "square"])
def test_midpoint_decode(name):
    from oracle import coders as OC
    f = R.decode_family(name, 1)
    want, bound, info = R.mid_decode(f.deltas, f.anchors, F64, bound=True)
    got = R.mid_decode(f.deltas, f.anchors, F32)
    assert torch.isfinite(got).all()
    err, dec = mid_err(got, want), info.decided
    r = (err[dec] / bound[dec]).max().item()
    und = R.undecided_share(dec)
    print(f"midpoint decode {name}: r = {r:.3f}, undecided {100 * und:.4f} % (cap {100 * f.cap:g} %), "
          f"|w - h| < 1e-3 on {100 * ((info.w - info.h).abs() < 1e-3).double().mean().item():.4f} % of the rows")
    assert r <= 1.0 and und <= f.cap, (r, und)
    assert (mid_err(OC.midpoint_decode(f.deltas, f.anchors), want)[dec] <= 2 * bound[dec]).all()
    if name == "square":     # both orders of w and h are present, decided
        assert info.swap_ok.all() and 0.2 < info.wide.double().mean().item() < 0.8


def test_midpoint_decode_degenerate_family():
    """x, y, z, depth and the larger planar side stay inside their bounds; the smaller side and the angle are reported.  Also the share
    of rows whose survival of a min_size = 1e-3 cut depends on rounding (smaller side within its bound of the cut)."""
    f = R.decode_family("degenerate", 1)
    want, bound, info = R.mid_decode(f.deltas, f.anchors, F64, bound=True)
    got = R.mid_decode(f.deltas, f.anchors, F32)
    assert torch.isfinite(got).all() and torch.isfinite(want).all()
    cols = [0, 1, 2, 5]
    r = (mid_err(got, want)[:, cols] / bound[:, cols]).max().item()
    large = torch.maximum(got[:, 3], got[:, 4]).double()
    ok = info.larger.bound <= R.COND * info.side
    rl = ((large - info.larger.value).abs()[ok] / info.larger.bound[ok]).max().item()
    und = R.undecided_share(info.decided[:, [3, 4, 6]])
    small = torch.minimum(want[:, 3], want[:, 4])
    sb = torch.maximum(bound[:, 3], bound[:, 4])
    near = ((small - 1e-3).abs() <= sb)
    print(f"midpoint decode degenerate: r(x y z depth) = {r:.3f}, r(larger side) = {rl:.3f} on {100 * ok.double().mean().item():.1f} % of the rows; "
          f"smaller side / angle undecided on {100 * und:.1f} % of their elements; smaller side within its bound of 1e-3 on "
          f"{100 * near.double().mean().item():.1f} % of the rows (sides {small[near].min().item() if near.any() else 0:.2e} .. "
          f"{small[near].max().item() if near.any() else 0:.2e}, fp32 evaluation {torch.minimum(got[:, 3], got[:, 4])[near].min().item() if near.any() else 0:.2e} .. "
          f"{torch.minimum(got[:, 3], got[:, 4])[near].max().item() if near.any() else 0:.2e})")
    s32 = torch.minimum(got[:, 3], got[:, 4]).double()
    flip = (s32 >= 1e-3) != (small >= 1e-3)
    print(f"    min_size = 1e-3 decided differently by the fp32 and the float64 evaluation on {100 * flip.double().mean().item():.1f} % of the rows"
          + (f" (float64 sides {small[flip].min().item():.2e} .. {small[flip].max().item():.2e}, fp32 {s32[flip].min().item():.2e} .. "
             f"{s32[flip].max().item():.2e})" if flip.any() else ""))
    assert r <= 1.0 and rl <= 1.0 and ok.double().mean().item() > 0.5
    # exactly degenerate rows (da = +0.5, db = -0.5): p0 == p1 in any arithmetic, th = -0, the angle is exactly 0 or -kHalfPiRef
    ex = (f.deltas[:, 6] == 0.5) & (f.deltas[:, 7] == -0.5)
    assert ex.sum() >= 64
    exact = got[ex, 6]
    assert set(exact.tolist()) <= {0.0, -R.HALF_PI_REF} and len(set(exact.tolist())) == 2


@pytest.mark.parametrize("name", ["random", "theta"])
def test_midpoint_encode(name):
    from oracle import coders as OC
    f = R.gt_family(name)
    want, bound, info = R.mid_encode(f.gt, f.anchors, F64, bound=True)
    got = R.mid_encode(f.gt, f.anchors, F32)
    report(f"midpoint encode {name}", got, want, bound, info.decided, f.cap)
    d = info.decided
    assert ((OC.midpoint_encode(f.gt, f.anchors).double() - want).abs()[d] <= 2 * bound[d]).all()


def roundtrip(f):
    enc, b_enc, ie = R.mid_encode(f.gt, f.anchors, F64, bound=True)
    want, b_dec, info = R.mid_decode(enc, f.anchors, F64, bound=True)
    bound = b_dec + R.decode_jacobian_bound(enc, f.anchors, b_enc)
    return want, bound, info.decided & ie.decided.all(1)[:, None]


def test_round_trip_returns_the_ground_truth():
    f = R.gt_family("roundtrip")
    want, bound, dec = roundtrip(f)
    assert R.undecided_share(dec) <= f.cap
    back = mid_err(want, f.gt.double())
    assert back.max() < 1e-6          # the 1e-7 guard and the truncated pi are all that separates them
    got = R.mid_decode(R.mid_encode(f.gt, f.anchors, F32), f.anchors, F32)
    r = (mid_err(got, want)[dec] / bound[dec]).max().item()
    print(f"round trip: r = {r:.3f}")
    assert r <= 1.0


def test_obb_to_aabb():
    from oracle import coders as OC
    f = R.gt_family("random")
    want, bound = R.obb_to_aabb(f.gt, F64, bound=True)
    dec = torch.ones_like(bound, dtype=torch.bool)
    report("obb_to_aabb", R.obb_to_aabb(f.gt, F32), want, bound, dec, 0.0)
    assert ((OC.obb3d_to_hbb(f.gt)[:, [0, 1, 2, 3, 4, 5]].double() - want[:, [0, 1, 2, 3, 4, 5]]).abs() <= 2 * bound).all()


# ======================================================================================================================
# coder mutations
# ======================================================================================================================
def test_mutation_clip_constants():
    f = R.decode_family("clamp", 0)
    want, bound = R.aabb_decode(f.deltas, f.anchors, F64, bound=True)
    s = share_outside(R.aabb_decode(f.deltas, f.anchors, F32, mut="clip"), want, bound, torch.ones_like(bound, dtype=torch.bool))
    f8 = R.decode_family("clamp", 1)
    want8, bound8, info = R.mid_decode(f8.deltas, f8.anchors, F64, bound=True)
    got8 = R.mid_decode(f8.deltas, f8.anchors, F32, mut="clip")
    s8 = ((mid_err(got8, want8) > 2 * bound8) & info.decided).any(1).double().mean().item()
    print(f"mutation clip: aabb {100 * s:.1f} % of the elements, midpoint {100 * s8:.1f} % of the rows beyond 2 x bound")
    assert s > 0.25 and s8 > 0.05


def test_mutation_offset_clamp():
    f = R.decode_family("clamp", 1)
    want, bound, info = R.mid_decode(f.deltas, f.anchors, F64, bound=True)
    got = R.mid_decode(f.deltas, f.anchors, F32, mut="offset_clamp")
    s = ((mid_err(got, want) > 2 * bound) & info.decided).any(1).double().mean().item()
    print(f"mutation offset_clamp: {100 * s:.1f} % of the rows beyond 2 x bound")
    assert s > 0.05


def test_mutation_pi_breaks_the_exact_rows():
    f = R.decode_family("degenerate", 1)
    ex = (f.deltas[:, 6] == 0.5) & (f.deltas[:, 7] == -0.5)
    got = R.mid_decode(f.deltas[ex], f.anchors[ex], F32)[:, 6]
    mut = R.mid_decode(f.deltas[ex], f.anchors[ex], F32, mut="pi")[:, 6]
    tall = got != 0
    assert tall.any() and (got[tall] == -R.HALF_PI_REF).all() and (mut[tall] != got[tall]).all() and (mut[~tall] == 0).all()
    print(f"mutation pi: equality broken on {int(tall.sum())} exactly degenerate rows ({mut[tall][0].item():.8f} for {got[tall][0].item():.8f})")


def test_mutation_ge_on_exact_ties():
    """Rows with w == h exactly in fp32 (a square outline with da == db): `w >= h` keeps th where the reference adds pi / 2."""
    f = R.decode_family("square", 1)
    d = f.deltas.clone()
    d[:, 7] = d[:, 6]
    got, mut = R.mid_decode(d, f.anchors, F32), R.mid_decode(d, f.anchors, F32, mut="ge")
    tie = got[:, 3] == got[:, 4]
    moved = R.angle_diff(got[:, 6], mut[:, 6]).abs() > 1.0
    print(f"mutation ge: {int(tie.sum())} exact-tie rows, angle moved by pi / 2 on {int(moved.sum())}")
    assert tie.sum() >= 8 and torch.equal(moved, tie)


def test_mutation_vertex_threshold():
    f = R.gt_family("theta")
    want, bound, info = R.mid_encode(f.gt, f.anchors, F64, bound=True)
    got = R.mid_encode(f.gt, f.anchors, F32, mut="thr")
    s = (((got.double() - want).abs() > 2 * bound) & info.decided).any(1).double().mean().item()
    print(f"mutation thr: {100 * s:.1f} % of the rows beyond 2 x bound")
    assert s > 0.1


# ======================================================================================================================
# head flatten
# ======================================================================================================================
def test_head_scatter_is_the_reshape():
    c = R.head_case(37, 13, 8, 11)
    lg, dl = R.head_flatten_ref(c)
    assert torch.equal(lg, c.head[:, :13].reshape(-1)) and torch.equal(dl, c.head[:, 13:13 * 9].reshape(-1, 8))
    back = R.head_unflatten_ref(R.NS(**{**vars(c), "logits": lg, "deltas": dl}), False, False)
    assert torch.equal(back[:, :13 * 9], c.head[:, :13 * 9]) and not back[:, 13 * 9:].any()
    assert any(cells * A * (1 + dw) > 8192 * 256 for cells, A, dw, _ in R.HEAD_CASES)


# ======================================================================================================================
# filter / select
# ======================================================================================================================
@pytest.mark.parametrize("W", [6, 7])
@pytest.mark.parametrize("name", R.FILTER_NAMES)
def test_filter_reference_is_the_oracle_chain(name, W):
    from oracle import boxes as OB
    c = R.filter_case(name, W)
    ref = R.filter_ref(c.boxes, c.logits, c.levels, c.valid, R.GRID, R.MIN_SIZE, c.thresh, False)
    live = c.valid.bool()
    b, s, l = c.boxes[live], torch.sigmoid(c.logits.double())[live], c.levels[live]
    b = OB.clip_to_grid(b, R.GRID)
    s, l = s[:b.shape[0]], l[:b.shape[0]]                                # quirk B3: scores and levels keep their slots
    k = OB.big_enough(b, R.MIN_SIZE)
    b, s, l = b[k], s[k], l[k]
    k = torch.where(s >= float(np.float32(c.thresh)))[0]
    assert ref.count == k.numel() and torch.equal(ref.boxes.view(torch.int32), b[k].view(torch.int32))
    assert torch.equal(ref.scores, s[k]) and torch.equal(ref.levels, l[k])
    sc = torch.sigmoid(c.logits.double())
    assert ((sc - float(np.float32(c.thresh))).abs() > 16 * R.U).all(), "a score within its bound of the threshold"
    if name == "none":
        assert ref.count == 0
    if name in ("edges", "min_size"):
        assert 0 < ref.count < int(c.valid.sum())


@pytest.mark.parametrize("mut", ["pairing", "min_gt"])
def test_filter_mutations(mut):
    name = {"pairing": "n1000", "min_gt": "min_size"}[mut]
    for W in ((7,) if mut == "pairing" else (6, 7)):
        c = R.filter_case(name, W)
        a = R.filter_ref(c.boxes, c.logits, c.levels, c.valid, R.GRID, R.MIN_SIZE, c.thresh, False)
        b = R.filter_ref(c.boxes, c.logits, c.levels, c.valid, R.GRID, R.MIN_SIZE, c.thresh, False, mut=mut)
        print(f"mutation {mut} (width {W}): count {a.count} -> {b.count}, rows equal: {np.array_equal(a.rows, b.rows)}")
        assert not np.array_equal(a.rows, b.rows)


@pytest.mark.parametrize("name", R.SELECT_NAMES)
def test_select_reference(name):
    c = R.select_case(name, 7)
    ob, os_, ol, m = R.select_ref(c.boxes, c.scores, c.levels, c.keep, c.count, c.post)
    kept = int(c.keep[:c.count].sum())
    assert m == min(kept, c.post)
    order = torch.sort(torch.where(c.keep[:c.count].bool(), c.scores[:c.count], torch.tensor(-1.0)), descending=True, stable=True).indices[:m]
    assert torch.equal(ob[:m], c.boxes[order]) and not ob[m:].any() and (ol[m:] == -1).all()
    want_kept = {"kept0": 0, "kept1": 1, "post-1": c.post - 1, "post": c.post, "post+1": c.post + 1, "all_kept": c.n}.get(name)
    assert want_kept is None or kept == want_kept
    if name == "tied_boundary":
        assert os_[c.post - 1] == os_[c.post // 2 + 3] == 0.5 and (c.scores == 0.5).sum() > c.post


def test_select_mutations():
    c = R.select_case("count_short", 6)
    assert not torch.equal(R.select_ref(c.boxes, c.scores, c.levels, c.keep, c.count, c.post)[0],
                           R.select_ref(c.boxes, c.scores, c.levels, c.keep, c.count, c.post, mut="beyond_count")[0])
    print("mutation beyond_count: rows differ")
    for name in ("all_equal", "tied_boundary"):
        c = R.select_case(name, 6)
        assert not torch.equal(R.select_ref(c.boxes, c.scores, c.levels, c.keep, c.count, c.post)[0],
                               R.select_ref(c.boxes, c.scores, c.levels, c.keep, c.count, c.post, mut="tie_high")[0])
    print("mutation tie_high: rows differ")


# ======================================================================================================================
# matcher
# ======================================================================================================================
@pytest.mark.parametrize("name", R.MATCH_NAMES)
def test_match_reference_is_the_oracle_matcher(name):
    from oracle import boxes as OB
    c = R.match_case(name)
    (lab, matched), q = R.match_expect(c)
    oq = OB.aabb_iou_matrix(c.gt, c.anchors)
    assert torch.equal(torch.from_numpy(q).view(torch.int32), oq.view(torch.int32)), "the fp32 IoU is the oracle's, bit for bit"
    pad = None
    if c.ori is not None:
        from oracle import anchors as OA
        pad = OA.padding_masks(R.SMALL.mesh, c.pyramid.grids, [c.ori])[0]
        assert torch.equal(~pad, torch.from_numpy(R.padding_ref(c.pyramid, c.ori))) and 0 < int((~pad).sum()) < pad.numel()
        oq[:, ~pad] = -1.0
    idx = OB.match(oq, float(np.float32(R.FG)), float(np.float32(R.BG)), True)
    olab = (idx >= 0).float()
    olab[idx == -2] = -1.0
    if pad is not None:
        olab[~pad] = -1.0
    assert torch.equal(lab, olab) and torch.equal(matched.long(), idx.clamp(min=0))
    if name == "equal_anchor":
        assert q[1].max() == 1.0 and lab[13 * 101 + 4] == 1 and matched[13 * 101 + 4] == 1
    if name == "outside":        # the GT's maximum is 0 and every anchor attains it: the reference turns every anchor positive
        assert q[2].max() == 0 and (lab == 1).all()
    if name == "low_quality":
        assert R.BG < q[1].max() < R.FG and abs(q[1].max() - 5.5 ** 3 / 512) < 1e-6 and ((matched == 1) & (lab == 1)).sum() >= 1
    if name == "duplicate":
        assert not (matched == 4).any() and (matched == 1).any()


def test_match_fp32_agrees_with_float64_on_integer_boxes():
    c = R.match_case("g1024")
    gt = c.gt.round()
    gt[:, 3:] = torch.maximum(gt[:, 3:], gt[:, :3] + 1)
    q32 = R.iou_f32(gt, c.anchors)
    a, b = gt.double().numpy()[:, None, :], c.anchors.double().numpy()[None, :, :]
    e = [np.maximum(np.minimum(a[..., k + 3], b[..., k + 3]) - np.maximum(a[..., k], b[..., k]), 0) for k in range(3)]
    inter = e[0] * e[1] * e[2]
    q64 = inter / (np.prod(a[..., 3:] - a[..., :3], -1) + np.prod(b[..., 3:] - b[..., :3], -1) - inter)
    l32, m32 = R.match_ref(q32, np.float32(R.FG), np.float32(R.BG))
    l64, m64 = R.match_ref(q64, R.FG, R.BG)
    assert torch.equal(l32, l64) and torch.equal(m32, m64) and len(set(l32.tolist())) == 3


@pytest.mark.parametrize("mut,name", [("last_dup", "duplicate"), ("no_low_quality", "low_quality")])
def test_match_mutations(mut, name):
    c = R.match_case(name)
    (lab, matched), _ = R.match_expect(c)
    (lab2, matched2), _ = R.match_expect(c, mut)
    diff = int((lab != lab2).sum() + (matched != matched2).sum())
    print(f"mutation {mut}: {diff} labels / indices differ")
    assert diff > 0


# ======================================================================================================================
# sampled loss
# ======================================================================================================================
@pytest.mark.parametrize("dw", [6, 8])
@pytest.mark.parametrize("npos,nneg", R.LOSS_COUNTS)
def test_loss_reference_and_r(npos, nneg, dw):
    import torch.nn.functional as Fn
    c = R.loss_case(npos, nneg, dw)
    ref, got = R.loss_eval(c, F64), R.loss_eval(c, F32)
    lg, dl = c.logits.double().requires_grad_(True), c.deltas.double().requires_grad_(True)
    both = torch.cat([c.pos, c.neg])
    y = torch.cat([torch.ones(npos), torch.zeros(nneg)]).double()
    o = Fn.binary_cross_entropy_with_logits(lg[both], y)
    rr = Fn.smooth_l1_loss(dl[c.pos], c.targets.double(), beta=R.BETA, reduction="sum") / both.numel()
    (o + rr).backward()
    assert torch.allclose(ref.bce, o.detach(), rtol=1e-12, atol=1e-300) and torch.allclose(ref.reg, rr.detach(), rtol=1e-12, atol=1e-300)
    assert torch.allclose(ref.g_logits, lg.grad, rtol=1e-10, atol=1e-60) and torch.allclose(ref.g_deltas, dl.grad, rtol=1e-12, atol=0)
    r = [R.ratio(got.g_logits, ref.g_logits, ref.b_logits), R.ratio(got.g_deltas, ref.g_deltas, ref.b_deltas),
         R.ratio(got.bce, ref.bce, ref.b_bce), R.ratio(got.reg, ref.reg, ref.b_reg)]
    print(f"sampled loss ({npos}, {nneg}) dw {dw}: r = dlogit {r[0]:.3f}, ddelta {r[1]:.3f}, bce {r[2]:.3f}, reg {r[3]:.3f}")
    assert max(r) <= 1.0
    outside = torch.ones(R.LOSS_ROWS, dtype=torch.bool)
    outside[both] = False
    assert not ref.g_logits[outside].any() and not ref.b_logits[outside].any() and not ref.b_deltas[~torch.isin(torch.arange(R.LOSS_ROWS), c.pos)].any()


@pytest.mark.parametrize("mut", ["inv_npos", "no_beta"])
def test_loss_mutations(mut):
    c = R.loss_case(100, 156, 8)
    ref, got = R.loss_eval(c, F64), R.loss_eval(c, F32, mut)
    live = ref.b_deltas > R.ETA
    if mut == "no_beta":       # only the quadratic branch divides by beta
        quad = torch.zeros_like(live)
        quad[c.pos] = ((c.deltas[c.pos] - c.targets).abs() < R.BETA) & ((c.deltas[c.pos] - c.targets) != 0)
        live &= quad
    s = ((got.g_deltas.double() - ref.g_deltas).abs()[live] > 2 * ref.b_deltas[live]).double().mean().item()
    sl = (got.reg.double() - ref.reg).abs().item() / ref.b_reg.item()
    print(f"mutation {mut}: {100 * s:.1f} % of the {int(live.sum())} affected delta gradients beyond 2 x bound, regression loss at {sl:.3g} x bound")
    assert s > 0.9 and sl > 2
