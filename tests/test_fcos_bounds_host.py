"""Host side of tests/test_gpu_fcos_kernels.py (no GPU): the float64 references of tests/fcos_ref.py are anchored to oracle/fcos.py (pinned
to the reference implementation by the goldens), and their per-element bounds are shown on the CPU to be satisfiable (a torch fp32
evaluation of each kernel's expressions stays inside, its worst |err| / bound r is printed: run with -s) and sharp (one mutation per kernel
lands outside its bound or breaks an equality).  The fixture self-checks are here too: every decision boundary of the targets family is
hit by a location, no OBB corner lies near the 0.1 thresholds, no sigmoid lies near the score threshold, and the share of vacuous OBB
decode rows stays under its caps (0 % regular, 30 % degenerate)."""
import pytest
import torch

import fcos_ref as R

F32, F64 = torch.float32, torch.float64


# ======================================================================================================================
# focal
# ======================================================================================================================
def test_focal_formula_equals_autograd_of_the_oracle():
    from oracle import fcos as OF
    logits, labels = R.focal_case(4001)
    keep = labels >= 0
    x = logits.double()[keep].requires_grad_()
    t = (labels[keep] > 0).double()
    loss = OF.focal_loss_sum(x, t)
    (g,) = torch.autograd.grad(loss, x)
    ref = R.focal_ref(logits, labels)
    assert abs(loss.item() - ref.sum) <= 1e-12 * abs(ref.sum)
    assert (g - ref.grad[keep]).abs().max().item() <= 1e-12 * ref.grad.abs().max().item()
    mid = x.detach().abs() <= 6          # away from the oracle's own cancellation in 1 - p
    assert ((g - ref.grad[keep]).abs()[mid] <= 1e-11 * ref.grad[keep].abs()[mid]).all()
    # softplus written out: F.softplus switches to the identity above its threshold of 20
    v = torch.tensor([20.5], dtype=F64)
    assert abs((torch.nn.functional.softplus(v) - R._softplus(v)).item()) > 1e-9


@pytest.mark.parametrize("count", R.FOCAL_COUNTS)
def test_focal_bounds_hold_for_torch_fp32_and_catch_mutations(count):
    logits, labels = R.focal_case(count)
    ref = R.focal_ref(logits, labels)
    term, grad = R.focal_eval(logits, labels)
    r_t, r_g = R.ratio(term, ref.term, ref.term_bound), R.ratio(grad, ref.grad, ref.grad_bound)
    r_s = abs(term.sum().item() - ref.sum) / ref.sum_bound if ref.sum_bound else 0.0
    print(f"focal {count}: torch fp32 r term {r_t:.3f} gradient {r_g:.3f} sum {r_s:.4f}")
    assert r_t <= 1.0 and r_g <= 1.0 and r_s <= 1.0
    for lab in (1, 0):
        sel = labels == lab
        if sel.any():
            print(f"   label {lab}: term {R.ratio(term[sel], ref.term[sel], ref.term_bound[sel]):.3f}"
                  f" gradient {R.ratio(grad[sel], ref.grad[sel], ref.grad_bound[sel]):.3f}")
    if count < 255:
        return
    for mut in ("swap_alpha", "drop2"):
        mt, mg = R.focal_eval(logits, labels, mutate=mut)
        for lab in (1, 0):
            sel = (labels == lab) & (logits.abs() < 8)          # beyond, one of p, q is below u and the mutated factor with it
            m = R._ratio((mg.double() - ref.grad)[sel].abs(), 2 * ref.grad_bound[sel])
            print(f"   {mut} label {lab}: gradient err/bound median {m.median().item():.3g} min {m.min().item():.3g}")
            assert m.median().item() > 100
        with pytest.raises(AssertionError):
            R.check(mg, ref.grad, ref.grad_bound, 2.0, mut)
        if mut == "swap_alpha":
            assert abs(mt.sum().item() - ref.sum) > 2 * ref.sum_bound


def test_focal_all_ignored_is_exactly_zero():
    logits, labels = R.focal_case(257, "ignored")
    ref = R.focal_ref(logits, labels)
    assert ref.sum == 0 and not ref.grad.any() and ref.sum_bound == 0 and not ref.grad_bound.any()


# ======================================================================================================================
# head epilogue
# ======================================================================================================================
HEAD_VARIANTS = [(sc, st, cr, nr, D) for sc, st in zip(R.HEAD_SCALES, R.HEAD_STRIDES) for cr in (0, 1) for nr in (1, 0) for D in (6, 8)]


@pytest.mark.parametrize("sc,stride,ctr_on_reg,norm_reg,D", HEAD_VARIANTS)
def test_head_bounds_hold_for_torch_fp32(sc, stride, ctr_on_reg, norm_reg, D):
    rows, wrows = 257, 64
    cls_out, box_out, dl, dr, dc = R.head_case(rows, wrows, D)
    f64 = R.head_fwd_eval(cls_out.double(), box_out.double(), sc, stride, norm_reg, D, ctr_on_reg)
    f32 = R.head_fwd_eval(cls_out, box_out, sc, stride, norm_reg, D, ctr_on_reg)
    b64 = R.head_bwd_eval(box_out.double(), sc, stride, norm_reg, D, ctr_on_reg, dl, dr, dc)
    b32 = R.head_bwd_eval(box_out, sc, stride, norm_reg, D, ctr_on_reg, dl, dr, dc)
    assert torch.equal(f32[0], cls_out[:, 0]) and torch.equal(f32[2], box_out[:, D] if ctr_on_reg else cls_out[:, 1])
    r_s = abs(b32[2].sum().item() - b64[2].sum().item()) / R.head_scale_bound(b64[2], norm_reg, rows, D)
    if norm_reg:
        # the fp32 evaluation differs from fp64 only by roundings: the reference of this branch IS the fp32 evaluation (equality on the GPU)
        big = (box_out[:, :D].abs() > 1e-30) | (box_out[:, :D] == 0)       # (a product that underflows has its own sign of zero and mask)
        assert R.ratio(f32[1][big], f64[1][big], 2 * R.U * f64[1][big].abs() + R.ETA) <= 1.0
        assert R.ratio(b32[1][:, :D][big], b64[1][:, :D][big], 2 * R.U * b64[1][:, :D][big].abs() + R.ETA) <= 1.0
        # raw * sc that underflows to zero has a zero gradient, as torch's ReLU gives
        x = box_out[:, :6].clone().requires_grad_()
        (torch.relu(x * sc) * stride).backward(dr[:, :6])
        assert torch.equal(x.grad, b32[1][:, :6])
        print(f"head norm_reg sc={sc}: d_scale r {r_s:.4f}")
    else:
        r_f, r_b = R.ratio(f32[1], f64[1], 4 * R.U * f64[1].abs() + R.ETA), R.ratio(b32[1], b64[1], 4 * R.U * b64[1].abs() + R.ETA)
        print(f"head expf sc={sc}: torch fp32 r forward {r_f:.3f} d_box {r_b:.3f} d_scale {r_s:.4f}")
        assert r_f <= 1.0 and r_b <= 1.0
    assert r_s <= 1.0
    # padded columns are zero
    keep = torch.zeros(wrows, dtype=torch.bool)
    keep[:D + (1 if ctr_on_reg else 0)] = True
    assert not b32[1][:, ~keep].any() and not b32[0][:, 2:].any()


def test_head_relu_mask_on_raw_breaks_equality():
    cls_out, box_out, dl, dr, dc = R.head_case(257, 64, 6)
    good = R.head_bwd_eval(box_out, -0.5, 32.0, 1, 6, 1, dl, dr, dc)
    bad = R.head_bwd_eval(box_out, -0.5, 32.0, 1, 6, 1, dl, dr, dc, mutate="mask_raw")
    assert not torch.equal(good[1], bad[1])
    with pytest.raises(AssertionError):
        R.check_equal(bad[1], good[1], "mask on raw")


# ======================================================================================================================
# GT summary and targets
# ======================================================================================================================
def test_obb_summary_fixture_and_bounds():
    from oracle import fcos as OF
    gt = R.OBB_SUMMARY_GTS
    assert R.summary_threshold_distance(gt) >= 0.05
    want, bound = R.summary_ref(gt)
    a32, al32, be32 = OF.obb_summary(gt)
    got = torch.cat([a32, al32[:, None], be32[:, None]], 1)
    r_box, r_ab = R.ratio(got[:, :6], want[:, :6], bound[:, :6]), R.ratio(got[:, 6:], want[:, 6:], bound[:, 6:])
    print(f"obb summary: torch fp32 r footprint {r_box:.3f} alpha/beta {r_ab:.3f}")
    assert r_box <= 1.0 and r_ab <= 1.0
    zero = gt[:, 6] == 0        # angle exactly 0: the footprint is the box
    assert torch.equal(want[zero][:, 6:], torch.tensor([[0.5, -0.5]], dtype=F64).expand(int(zero.sum()), 2))
    swapped = got.clone()
    swapped[:, 6:] = got[:, [7, 6]]
    assert R.ratio(swapped[:, 6:], want[:, 6:], 2 * bound[:, 6:]) > 1e3


def _oracle_aux(geom, targets, radius, norm_reg, use_obb):
    from oracle import fcos as OF
    model = OF.FCOS(None, None, strides=geom.strides, use_obb=use_obb, center_sampling_radius=radius, norm_reg_targets=norm_reg,
                    iou_loss_type="smooth_l1")
    D = 8 if use_obb else 6
    locs = [l.float() for l in geom.locations]
    cls = [torch.zeros(geom.n, 1, *d) for d in geom.dims]
    reg = [torch.ones(geom.n, D, *d) for d in geom.dims]
    masks = OF.padding_masks(locs, geom.ori)
    return model.losses(locs, cls, reg, cls, [t.float() for t in targets], masks)[3]


@pytest.mark.parametrize("use_obb", [False, True])
@pytest.mark.parametrize("radius,norm_reg", [(1.5, True), (0, False)])
def test_flat_targets_equal_the_oracle_loss_path(radius, norm_reg, use_obb):
    """aux['labels'] / aux['reg_targets'] of oracle FCOS.losses (float32, masked to the un-padded locations) equal the float64 flat-order
    wrapper: the order is right, and on quarter-grid coordinates fp32 and fp64 agree exactly."""
    geom, targets = R.targets_case()
    if use_obb:
        targets = [R.as_obb(t) for t in targets]
    labels, regs = R.targets_ref(geom, targets, radius, norm_reg, use_obb)
    aux = _oracle_aux(geom, targets, radius, norm_reg, use_obb)
    keep = labels >= 0
    assert torch.equal(keep, geom.valid())
    assert torch.equal(labels[keep].double(), aux["labels"].double())
    assert torch.equal(regs[keep], aux["reg_targets"].double())


@pytest.mark.parametrize("radius", [1.5, 0])
def test_targets_fixture_hits_every_boundary_and_catches_mutations(radius):
    geom, targets = R.targets_case()
    hit = R.targets_boundaries(geom, targets, radius)
    print(radius, hit)
    assert all(hit.values()), {k: v for k, v in hit.items() if not v}
    labels, regs = R.targets_ref(geom, targets, radius, True, False)
    assert (labels > 0).any() and (labels == 0).any() and (labels < 0).any()
    for mut in ("lo_strict",) + (("inside_ge",) if radius > 0 else ()):
        l2, r2 = R.targets_ref(geom, targets, radius, True, False, mutate=mut)
        print(f"   {mut}: {int((l2 != labels).sum())} labels, {int((r2 != regs).any(1).sum())} target rows differ")
        assert not torch.equal(l2, labels) or not torch.equal(r2, regs)
    # equal volumes: the first GT (lower index) is returned
    g, flat_loc, s = targets[1].double(), geom.flat_locations(), torch.tensor(geom.strides, dtype=F64)[geom.flat_levels()]
    both = [i for i in torch.nonzero((labels > 0) & (geom.flat_scenes() == 1))[:, 0].tolist() if _cared_both(geom, flat_loc[i], g, i, radius)]
    assert both, "no location admits both equal-volume GTs"
    for i in both:
        assert torch.equal(regs[i, :3] * s[i], flat_loc[i] - g[3, :3]), "the tie did not go to the first GT"


def _cared_both(geom, p, g, i, radius):
    """Both equal-volume GTs (3, 4) are admissible at location i (inside the region and within the level's size of interest)."""
    lvl = int(geom.flat_levels()[i])
    s = geom.strides[lvl]
    lo, hi = [[-1, 16], [16, 32], [32, 64], [64, 1e8]][lvl]
    ok = True
    for k in (3, 4):
        d = torch.cat([p - g[k, :3], g[k, 3:] - p])
        if radius > 0:
            c = (g[k, :3] + g[k, 3:]) / 2
            a, b = torch.maximum(c - s * radius, g[k, :3]), torch.minimum(c + s * radius, g[k, 3:])
            inside = torch.cat([p - a, b - p]).min() > 0
        else:
            inside = d.min() > 0
        ok = ok and bool(inside) and lo <= d.max().item() <= hi
    return ok


@pytest.mark.parametrize("radius,norm_reg", [(1.5, True), (0, False)])
def test_rotated_targets_margins_and_bounds(radius, norm_reg):
    """Rotated GTs: no footprint corner near the 0.1 thresholds, nearly every location decided by a margin of 1e-3, and on those the
    oracle's fp32 evaluation gives the float64 labels and stays inside the targets' bound."""
    geom, _ = R.targets_case()
    assert min(R.summary_threshold_distance(t) for t in R.OBB_TARGET_GTS) >= 0.05
    labels, regs, margin, bound = R.rotated_targets_ref(geom, R.OBB_TARGET_GTS, radius, norm_reg)
    l32, r32 = R.targets_ref(geom, R.OBB_TARGET_GTS, radius, norm_reg, True, dtype=F32)
    dec = (margin > R.DECISION_MARGIN) & (labels >= 0)
    assert dec.sum() >= 0.95 * (labels >= 0).sum() and (labels[dec] > 0).sum() > 50
    assert torch.equal(l32[dec], labels[dec])
    r = R.ratio(r32[dec], regs[dec], bound[dec])
    print(f"rotated targets radius={radius}: {int(dec.sum())} of {int((labels >= 0).sum())} decided, torch fp32 r {r:.3f}")
    assert r <= 1.0


def test_targets_without_gt_in_one_scene():
    geom, targets = R.targets_case(empty_second=True)
    labels, regs = R.targets_ref(geom, targets, 1.5, True, False)
    sc = geom.flat_scenes()
    assert not (labels[sc == 1] > 0).any() and not regs[sc == 1].any() and (labels[sc == 0] > 0).any()


# ======================================================================================================================
# scores
# ======================================================================================================================
def test_scores_bounds_and_threshold_distance():
    geom, logits, ctr = R.scores_case()
    want, bound, dist = R.scores_ref(geom, logits, ctr, R.SCORE_THRESH)
    assert dist > 1.0, dist
    assert logits.abs().max() <= 87 and ctr.abs().max() <= 87
    got = R.scores_eval32(geom, logits, ctr, R.SCORE_THRESH)
    assert torch.equal(got < 0, want < 0)
    r = R.ratio(got, want, bound)
    print(f"scores: torch fp32 r {r:.3f}; {int((want >= 0).sum())} candidates of {geom.total}, {int((~geom.valid()).sum())} padded")
    assert r <= 1.0 and (want >= 0).any() and (~geom.valid()).any()
    # mutation: the centerness sigmoid dropped
    one = torch.ones((), dtype=F32)
    bad = torch.where(got >= 0, one / (one + torch.exp(-logits)), -one)
    assert R.ratio(bad, want, 2 * bound) > 1e3


# ======================================================================================================================
# decode
# ======================================================================================================================
def test_decode_aabb_fp32_equals_fp64_and_catches_mutations():
    geom, idx, score, reg, D, ms = R.decode_case("aabb")
    ref = R.decode_ref(geom, idx, score, reg, D, ms)
    f32 = R.decode_ref(geom, idx, score, reg, D, ms, dtype=F32)
    assert torch.equal(f32.boxes.double(), ref.boxes) and torch.equal(f32.scores < 0, ref.scores < 0)
    kept = ref.scores >= 0
    r = R.ratio(f32.scores[kept], ref.scores[kept], 2 * R.U * ref.scores[kept] + R.ETA)
    print(f"decode aabb: torch fp32 r sqrt(score) {r:.3f}; live {int(ref.live.sum())}, kept {int(kept.sum())} of {ref.live.numel()}")
    assert r <= 1.0
    ext = ref.boxes[:, 3:] - ref.boxes[:, :3]
    assert (ref.live & (ext == ms).any(1) & (ext >= ms).all(1)).any(), "no extent exactly equal to min_size"
    assert (ref.live & ~ref.keep).any() and (~ref.live).any()
    bad = R.decode_ref(geom, idx, score, reg, D, ms, mutate="gt_min")
    assert not torch.equal(bad.scores < 0, ref.scores < 0)
    bad = R.decode_ref(geom, idx, score, reg, D, ms, mutate="swap_seg")
    assert not torch.equal(bad.levels, ref.levels) and not torch.equal(bad.boxes, ref.boxes)


@pytest.mark.parametrize("kind,cap", [("obb_regular", 0.0), ("obb_degenerate", 0.30)])
def test_decode_obb_bounds_hold_for_torch_fp32_and_catch_mutations(kind, cap):
    geom, idx, score, reg, D, ms = R.decode_case(kind)
    ref = R.decode_ref(geom, idx, score, reg, D, ms)
    f32 = R.decode_ref(geom, idx, score, reg, D, ms, dtype=F32)
    out = R.decode_obb_ratios(ref, f32.boxes, f32.scores, f32.levels, ms)
    print(f"decode {kind}: torch fp32 r {({k: round(v, 3) for k, v in out.items()})}; live {int(ref.live.sum())}")
    assert max(out["centre_height"], out["size"], out["angle"], out["score"]) <= 1.0
    assert out["vacuous"] <= cap, out["vacuous"]
    if kind == "obb_degenerate":
        assert (ref.live & ref.zero_row).any()
        assert (ref.live & (reg[_flat(geom, idx)][:, 6:].abs().amax(1) > 0.5)).any()        # the clamp acts
        bad = R.decode_ref(geom, idx, score, reg, D, ms, dtype=F32, mutate="no_eps")
        with pytest.raises(AssertionError):
            R.decode_obb_ratios(ref, bad.boxes, bad.scores, bad.levels, ms)
    bad = R.decode_ref(geom, idx, score, reg, D, ms, dtype=F32, mutate="swap_seg")
    with pytest.raises(AssertionError):
        o = R.decode_obb_ratios(ref, bad.boxes, bad.scores, bad.levels, ms, k=(2.0, 2.0, 2.0))
        assert max(o["centre_height"], o["size"]) <= 1.0


def _flat(geom, idx):
    segs, k = idx.shape
    seg = torch.arange(segs * k) // k
    level, scene = seg // geom.n, seg % geom.n
    return torch.tensor(geom.off[:-1])[level] + scene * torch.tensor(geom.counts)[level] + idx.reshape(-1).long().clamp(min=0)
