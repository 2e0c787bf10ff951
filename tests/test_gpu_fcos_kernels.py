"""GPU: the seven FCOS kernels of csrc/fcos.hip that tests/test_gpu_fcos.py reaches only through whole networks - head epilogue forward /
backward, GT summary, target assignment, focal loss, candidate scores, candidate decode - called directly through ops.FocalLossFn,
ops.FcosHeadOutFn, ops.fcos_gt_summary, ops.fcos_targets, ops.fcos_scores and ops.fcos_decode against the float64 references of
tests/fcos_ref.py: every element of every output inside its own derived bound, or equal where the arithmetic is exact.  The bounds, their
derivation and the input families are in fcos_ref's docstring; tests/test_fcos_bounds_host.py shows on the CPU that they are satisfiable
and sharp.  No tolerance here is a bare constant: each is an equality, a bound of fcos_ref times the allowance k = max(1, min(2, 4 r))
measured on torch's fp32 CPU evaluation of the same case (never on the kernel), or max(4 x the oracle's own fp32-versus-fp64 error,
8u x the tensor's scale) for the torch-op parts of the composed loss.  Every check prints its max |err| / bound (run with -s).

Launch branches: counts 1 / 255 / 256 / 257 (one workgroup that is its own last ticket holder, several workgroups) and the second trip of
every capped grid-stride loop (focal and head backward 1024 x 256 + 77, head forward 8192 x 256 + 300, targets 81^3 > 2048 x 256,
scores 129 x 128 x 128 > 8192 x 256).  The decode kernel's cap lies beyond the post-processor's k * L <= 16384 and is left out."""
import pytest
import torch

import fcos_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


def _ids(prefix):
    return lambda v: f"{prefix}{v}" + ("-second_trip" if isinstance(v, int) and v > 1024 * 256 else "")


# ======================================================================================================================
# focal loss
# ======================================================================================================================
def _focal_run(logits, labels, dev, upstream=None):
    from nerf_rpn_amd import ops
    x = logits.to(dev)
    if upstream is not None:
        x.requires_grad_()
    loss = ops.FocalLossFn.apply(x, labels.to(dev), 0.25)
    grad = None
    if upstream is not None:
        (grad,) = torch.autograd.grad(loss, x, torch.tensor(upstream, device=dev))
    torch.cuda.synchronize()
    return loss.detach(), grad


@pytest.mark.parametrize("count", R.FOCAL_COUNTS, ids=_ids("n"))
def test_focal_matches_fp64(count, dev):
    """Loss sum and d loss / d logit of every element, through both autograd paths: with requires_grad (the gradient scaled by an upstream
    factor of 0.5, an exact scaling) and without (null dlogits); the ordered sum is the same bits in both and run to run."""
    logits, labels = R.focal_case(count)
    ref = R.focal_ref(logits, labels)
    t32, g32 = R.focal_eval(logits, labels)
    k_g = R.allowance(R.ratio(g32, ref.grad, ref.grad_bound))
    k_s = R.allowance(abs(t32.sum().item() - ref.sum) / ref.sum_bound)
    loss, grad = _focal_run(logits, labels, dev, upstream=0.5)
    loss2, none = _focal_run(logits, labels, dev)
    assert none is None and torch.equal(loss, loss2), (loss.item(), loss2.item())
    R.check(loss, torch.tensor(ref.sum, dtype=F64), ref.sum_bound, k_s, f"focal {count} sum")
    R.check(grad, 0.5 * ref.grad, 0.5 * ref.grad_bound, k_g, f"focal {count} gradient")
    assert not grad[(labels < 0).to(dev)].any(), "ignored locations carry a gradient"


@pytest.mark.parametrize("kind", ["ignored", "negative"])
def test_focal_uniform_labels(kind, dev):
    logits, labels = R.focal_case(257, kind)
    ref = R.focal_ref(logits, labels)
    loss, grad = _focal_run(logits, labels, dev, upstream=0.5)
    if kind == "ignored":
        assert loss.item() == 0.0 and not grad.any()
        return
    t32, g32 = R.focal_eval(logits, labels)
    R.check(loss, torch.tensor(ref.sum, dtype=F64), ref.sum_bound, R.allowance(abs(t32.sum().item() - ref.sum) / ref.sum_bound), "focal negative sum")
    R.check(grad, 0.5 * ref.grad, 0.5 * ref.grad_bound, R.allowance(R.ratio(g32, ref.grad, ref.grad_bound)), "focal negative gradient")


# ======================================================================================================================
# head epilogue
# ======================================================================================================================
def _head_run(case, sc, stride, norm_reg, D, ctr_on_reg, dev, sink_prefill=None):
    """-> (logits, reg, ctr), (d_cls_out, d_box_out, d_scale) on the device; with ``sink_prefill`` the Scale gradient goes to an arena slot
    and the slot is returned in its place."""
    from nerf_rpn_amd import ops
    cls_out, box_out, dl, dr, dc = case
    co, bo = cls_out.to(dev).requires_grad_(), box_out.to(dev).requires_grad_()
    scale = torch.tensor([sc], device=dev, requires_grad=True)
    slot = None
    if sink_prefill is not None:
        slot = sink_prefill.clone()
        scale._nrpn_sink = ops.GradSink(slot, lambda: None)
    try:
        outs = ops.FcosHeadOutFn.apply(co, bo, scale, stride, norm_reg, D, ctr_on_reg)
        grads = torch.autograd.grad(list(outs), [co, bo, scale], [dl.to(dev), dr.to(dev), dc.to(dev)], allow_unused=True)
        torch.cuda.synchronize()
    finally:
        if slot is not None:
            del scale._nrpn_sink
    if slot is not None:
        assert grads[2] is None
        return outs, (grads[0], grads[1], slot)
    return outs, grads


def _head_check(case, sc, stride, norm_reg, D, ctr_on_reg, dev, what):
    cls_out, box_out, dl, dr, dc = case
    rows = cls_out.shape[0]
    f32 = R.head_fwd_eval(cls_out, box_out, sc, stride, norm_reg, D, ctr_on_reg)
    b32 = R.head_bwd_eval(box_out, sc, stride, norm_reg, D, ctr_on_reg, dl, dr, dc)
    terms64 = R.head_bwd_eval(box_out.double(), sc, stride, norm_reg, D, ctr_on_reg, dl, dr, dc)[2]
    outs, grads = _head_run(case, sc, stride, norm_reg, D, ctr_on_reg, dev)
    R.check_equal(outs[0], f32[0], what + " logits")
    R.check_equal(outs[2], f32[2], what + " centerness")
    R.check_equal(grads[0], b32[0], what + " d_cls_out")
    if norm_reg:
        R.check_equal(outs[1], f32[1], what + " reg")
        R.check_equal(grads[1], b32[1], what + " d_box_out")
    else:
        f64 = R.head_fwd_eval(cls_out.double(), box_out.double(), sc, stride, norm_reg, D, ctr_on_reg)[1]
        b64 = R.head_bwd_eval(box_out.double(), sc, stride, norm_reg, D, ctr_on_reg, dl, dr, dc)[1]
        tf, tb = 4 * R.U * f64.abs() + R.ETA, 4 * R.U * b64[:, :D].abs() + R.ETA
        R.check(outs[1], f64, tf, R.allowance(R.ratio(f32[1], f64, tf)), what + " reg (expf)")
        R.check(grads[1][:, :D], b64[:, :D], tb, R.allowance(R.ratio(b32[1][:, :D], b64[:, :D], tb)), what + " d_box_out (expf)")
        R.check_equal(grads[1][:, D:], b32[1][:, D:], what + " d_box_out padded columns")
    bound = R.head_scale_bound(terms64, norm_reg, rows, D)
    want = terms64.sum()
    k = R.allowance(abs(b32[2].sum().item() - want.item()) / bound)
    R.check(grads[2], want.reshape(1), bound, k, what + " d_scale")
    return grads[2]


@pytest.mark.parametrize("norm_reg", [1, 0], ids=["norm_reg", "expf"])
@pytest.mark.parametrize("D", [6, 8])
@pytest.mark.parametrize("rows", R.HEAD_BWD_COUNTS, ids=_ids("rows"))
def test_head_epilogue_matches_reference(rows, D, norm_reg, dev):
    """Forward and backward on the real tile (wrows = 64): the norm_reg branch equal to torch's fp32 evaluation in the kernel's order,
    the expf branch within 4u of fp64; d_cls_out / d_box_out zero in every padded column; d_scale within the ordered-sum bound."""
    case = R.head_case(rows, 64, D)
    combos = list(zip(R.HEAD_SCALES, R.HEAD_STRIDES))
    variants = [(sc, st, cr) for sc, st in combos for cr in (0, 1)] if rows < 1024 else [(combos[2 - norm_reg] + (norm_reg,))]
    for sc, stride, ctr_on_reg in variants:
        _head_check(case, sc, stride, norm_reg, D, ctr_on_reg, dev, f"head rows={rows} D={D} norm={norm_reg} sc={sc} ctr_on_reg={ctr_on_reg}")


@pytest.mark.parametrize("norm_reg", [1, 0], ids=["norm_reg", "expf"])
def test_head_epilogue_forward_second_trip(norm_reg, dev):
    """8192 x 256 + 300 rows (the forward grid is capped at 8192 blocks), wrows = 9, D = 8."""
    from nerf_rpn_amd import ops
    rows, wrows, D, sc, stride = R.HEAD_FWD_BIG, 9, 8, 1.25, 4.0
    cls_out, box_out = R.head_case(rows, wrows, D, grads=False)
    f32 = R.head_fwd_eval(cls_out, box_out, sc, stride, norm_reg, D, 1)
    with torch.no_grad():
        outs = ops.FcosHeadOutFn.apply(cls_out.to(dev), box_out.to(dev), torch.tensor([sc], device=dev), stride, norm_reg, D, 1)
    torch.cuda.synchronize()
    R.check_equal(outs[0], f32[0], "head forward big logits")
    R.check_equal(outs[2], f32[2], "head forward big centerness")
    if norm_reg:
        R.check_equal(outs[1], f32[1], "head forward big reg")
    else:
        f64 = R.head_fwd_eval(cls_out.double(), box_out.double(), sc, stride, norm_reg, D, 1)[1]
        tol = 4 * R.U * f64.abs() + R.ETA
        R.check(outs[1], f64, tol, R.allowance(R.ratio(f32[1], f64, tol)), "head forward big reg (expf)")


@pytest.mark.parametrize("norm_reg", [1, 0], ids=["norm_reg", "expf"])
def test_head_scale_gradient_is_ordered_and_reaches_the_arena_slot(norm_reg, dev):
    """d_scale of the second-trip case is the same bits run to run (ordered workgroup partials), and with the Scale parameter bound to an
    arena slot the slot receives prefill + the same d_scale while autograd gets nothing."""
    rows, D, sc, stride = R.HEAD_BWD_COUNTS[-1], 8, 0.8, 4.0
    case = R.head_case(rows, 64, D)
    _, a = _head_run(case, sc, stride, norm_reg, D, 1, dev)
    _, b = _head_run(case, sc, stride, norm_reg, D, 1, dev)
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
    pre = torch.tensor([3.25], device=dev)
    _, c = _head_run(case, sc, stride, norm_reg, D, 1, dev, sink_prefill=pre)
    assert torch.equal(c[2], pre + a[2]), (c[2].item(), pre.item(), a[2].item())
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


# ======================================================================================================================
# GT summary and targets
# ======================================================================================================================
def test_gt_summary_matches_fp64(dev):
    from nerf_rpn_amd import ops
    from oracle import fcos as OF
    aabb = R.targets_case()[1][0]
    R.check_equal(ops.fcos_gt_summary(aabb.to(dev)), R.summary_ref(aabb)[0], "summary aabb")
    gt = R.OBB_SUMMARY_GTS
    want, bound = R.summary_ref(gt)
    a32, al32, be32 = OF.obb_summary(gt)
    t32 = torch.cat([a32, al32[:, None], be32[:, None]], 1)
    got = ops.fcos_gt_summary(gt.to(dev))
    R.check(got[:, :6], want[:, :6], bound[:, :6], R.allowance(R.ratio(t32[:, :6], want[:, :6], bound[:, :6])), "summary obb footprint")
    R.check(got[:, 6:], want[:, 6:], bound[:, 6:], R.allowance(R.ratio(t32[:, 6:], want[:, 6:], bound[:, 6:])), "summary obb alpha / beta")
    zero = gt[:, 6] == 0
    R.check_equal(got[zero], want[zero], "summary obb at angle exactly 0")


def _targets_run(geom, targets, radius, norm_reg, D, dev):
    from nerf_rpn_amd import ops
    g = ops.FcosGeometry(geom.n, geom.dims, geom.strides)
    labels, reg_t, npos = ops.fcos_targets(g, [t.to(dev) for t in targets], geom.ori, radius, norm_reg, D, dev)
    torch.cuda.synchronize()
    return labels, reg_t, npos


@pytest.mark.parametrize("D", [6, 8], ids=["aabb", "obb"])
@pytest.mark.parametrize("norm_reg", [1, 0], ids=["norm_reg1", "norm_reg0"])
@pytest.mark.parametrize("radius", [1.5, 0], ids=["radius1.5", "radius0"])
@pytest.mark.parametrize("empty_second", [False, True], ids=["both_gt", "one_scene_without_gt"])
def test_targets_equal_fp64(empty_second, radius, norm_reg, D, dev):
    """Labels AND regression targets of every location equal the float64 oracle: the fixture's coordinates are multiples of 0.25, and it
    sits on every decision boundary (host test): region faces, size-of-interest limits, equal volumes, x == ori."""
    geom, targets = R.targets_case(empty_second)
    if D == 8:
        targets = [R.as_obb(t) for t in targets]
    want_l, want_r = R.targets_ref(geom, targets, radius, bool(norm_reg), D == 8)
    labels, reg_t, npos = _targets_run(geom, targets, radius, norm_reg, D, dev)
    R.check_equal(labels, want_l, "labels")
    R.check_equal(reg_t, want_r, "reg_targets")
    assert int(npos.item()) == int((want_l > 0).sum())


@pytest.mark.parametrize("radius,norm_reg", [(1.5, 1), (0, 0)], ids=["radius1.5-norm_reg1", "radius0-norm_reg0"])
def test_targets_of_rotated_gts(radius, norm_reg, dev):
    """Rotated GTs (angles +-0.3, +-0.8, 1.2): the label of every location whose decision quantities lie further than 1e-3 from their
    thresholds, and on those the targets within the summary's bound."""
    geom, _ = R.targets_case()
    want_l, want_r, margin, bound = R.rotated_targets_ref(geom, R.OBB_TARGET_GTS, radius, bool(norm_reg))
    _, r32 = R.targets_ref(geom, R.OBB_TARGET_GTS, radius, bool(norm_reg), True, dtype=F32)
    labels, reg_t, npos = _targets_run(geom, R.OBB_TARGET_GTS, radius, norm_reg, 8, dev)
    dec = (margin > R.DECISION_MARGIN) & (want_l >= 0)
    R.check_equal(labels.cpu()[dec], want_l[dec], "rotated labels")
    R.check_equal(labels.cpu() < 0, want_l < 0, "rotated padding")
    R.check(reg_t.cpu()[dec], want_r[dec], bound[dec], R.allowance(R.ratio(r32[dec], want_r[dec], bound[dec])), "rotated reg_targets")
    assert int(npos.item()) == int((labels > 0).sum().item())


def test_targets_second_trip(dev):
    """81^3 locations on one level (more than 2048 x 256): labels, targets and the positive count."""
    geom, targets = R.targets_big_case()
    want_l, want_r = R.targets_ref(geom, targets, 1.5, True, False)
    labels, reg_t, npos = _targets_run(geom, targets, 1.5, 1, 6, dev)
    R.check_equal(labels, want_l, "labels 81^3")
    R.check_equal(reg_t, want_r, "reg_targets 81^3")
    assert int((want_l > 0).sum()) > 0 and int(npos.item()) == int((labels > 0).sum().item()) == int((want_l > 0).sum())


# ======================================================================================================================
# scores
# ======================================================================================================================
@pytest.mark.parametrize("big", [False, True], ids=["levels_scenes_padding", "second_trip"])
def test_scores_match_fp64(big, dev):
    from nerf_rpn_amd import ops
    geom, logits, ctr = R.scores_case(big)
    want, bound, dist = R.scores_ref(geom, logits, ctr, R.SCORE_THRESH)
    assert dist > 1.0
    got = ops.fcos_scores(ops.FcosGeometry(geom.n, geom.dims, geom.strides), logits.to(dev), ctr.to(dev), geom.ori, R.SCORE_THRESH)
    torch.cuda.synchronize()
    R.check_equal(got.cpu() < 0, want < 0, "candidate mask")
    R.check_equal(got.cpu()[want < 0], want[want < 0], "non-candidates are -1")
    k = R.allowance(R.ratio(R.scores_eval32(geom, logits, ctr, R.SCORE_THRESH), want, bound))
    R.check(got, want, bound, k, f"scores big={big}")


def test_scores_stay_finite_beyond_the_exp_range(dev):
    from nerf_rpn_amd import ops
    logits, ctr = torch.tensor([100.0, -100.0, 100.0, -100.0]), torch.tensor([100.0, 100.0, -100.0, -100.0])
    got = ops.fcos_scores(ops.FcosGeometry(1, [(2, 2, 1)], [4]), logits.to(dev), ctr.to(dev), None, R.SCORE_THRESH).cpu()
    assert torch.isfinite(got).all() and ((got == -1) | ((got >= 0) & (got <= 1))).all(), got


# ======================================================================================================================
# decode
# ======================================================================================================================
def _decode_run(geom, idx, score, reg, D, min_size, dev):
    from nerf_rpn_amd import ops
    out = ops.fcos_decode(ops.FcosGeometry(geom.n, geom.dims, geom.strides), idx.to(dev), score.to(dev), reg.to(dev), geom.ori, D, min_size)
    torch.cuda.synchronize()
    return out


def test_decode_aabb_equals_fp64(dev):
    """Quarter-grid distances: the clipped box equals the float64 clip, the keep rule `>= min_size` is exact (extents exactly min_size
    included), dropped slots are all-zero with score -1, levels exact."""
    geom, idx, score, reg, D, ms = R.decode_case("aabb")
    ref = R.decode_ref(geom, idx, score, reg, D, ms)
    f32 = R.decode_ref(geom, idx, score, reg, D, ms, dtype=F32)
    boxes, scores, levels = _decode_run(geom, idx, score, reg, D, ms, dev)
    R.check_equal(boxes, ref.boxes, "decode aabb boxes")
    R.check_equal(levels, ref.levels, "decode aabb levels")
    R.check_equal(scores.cpu() < 0, ref.scores < 0, "decode aabb keep")
    tol = torch.where(ref.scores >= 0, 2 * R.U * ref.scores + R.ETA, torch.zeros_like(ref.scores))
    R.check(scores, ref.scores, tol, R.allowance(R.ratio(f32.scores, ref.scores, tol)), "decode aabb sqrt(score)")


@pytest.mark.parametrize("kind", ["obb_regular", "obb_degenerate"])
def test_decode_obb_matches_fp64(kind, dev):
    geom, idx, score, reg, D, ms = R.decode_case(kind)
    ref = R.decode_ref(geom, idx, score, reg, D, ms)
    f32 = R.decode_ref(geom, idx, score, reg, D, ms, dtype=F32)
    r32 = R.decode_obb_ratios(ref, f32.boxes, f32.scores, f32.levels, ms)
    k = tuple(R.allowance(r32[n]) for n in ("centre_height", "size", "angle"))
    out = R.decode_obb_ratios(ref, *_decode_run(geom, idx, score, reg, D, ms, dev), ms, k=k)
    print(f"decode {kind}: max err/bound {({n: round(v, 3) for n, v in out.items()})} (k = {k})")
    assert out["centre_height"] <= 1.0 and out["size"] <= 1.0 and out["angle"] <= 1.0, out
    assert out["score"] <= R.allowance(r32["score"]), out


# ======================================================================================================================
# argument guards
# ======================================================================================================================
def test_argument_guards_return_errors(dev):
    from nerf_rpn_amd import lib, ops
    z = lambda *s: torch.zeros(*s, device=dev)      # noqa: E731
    one = torch.ones(1, device=dev)
    with pytest.raises(lib.NrpnError):              # reg_dim 7
        ops.FcosHeadOutFn.apply(z(4, 64), z(4, 64), one, 1.0, 1, 7, 1)
    with pytest.raises(lib.NrpnError):              # wrows <= reg_dim
        ops.FcosHeadOutFn.apply(z(4, 8), z(4, 8), one, 1.0, 1, 8, 1)
    geom = ops.FcosGeometry(2, [(3, 2, 2), (2, 1, 1)], [4, 8])
    sizes = [(12, 8, 8), (10, 8, 6)]
    with pytest.raises(lib.NrpnError):              # count != levels * n * seg_len
        ops.fcos_decode(geom, torch.zeros(3, 5, dtype=torch.int32, device=dev), z(3, 5), z(geom.total, 6), sizes, 6, 0.0)
    with pytest.raises(lib.NrpnError):              # reg_dim 7
        ops.fcos_decode(geom, torch.zeros(4, 5, dtype=torch.int32, device=dev), z(4, 5), z(geom.total, 7), sizes, 7, 0.0)
    many = ops.FcosGeometry(65, [(1, 1, 1)], [4])
    with pytest.raises(lib.NrpnError):              # 65 scenes
        ops.fcos_scores(many, z(many.total), z(many.total), None, 0.05)
    deep = ops.FcosGeometry(1, [(1, 1, 1)] * 9, [4] * 9)
    with pytest.raises(lib.NrpnError):              # 9 levels
        ops.fcos_scores(deep, z(deep.total), z(deep.total), None, 0.05)
    with pytest.raises(lib.NrpnError):
        ops.fcos_targets(deep, [z(1, 6)], None, 1.5, 1, 6, dev)
    torch.cuda.synchronize()


# ======================================================================================================================
# the loss composition, without a backbone
# ======================================================================================================================
LOSS_DIMS, LOSS_STRIDES, LOSS_SIZES = [(16, 14, 12), (8, 7, 6), (4, 4, 3)], (4, 8, 16), [(64, 56, 48), (46, 44, 34)]
LOSS_GTS = [torch.tensor([[10.0, 10.0, 10.0, 30.0, 28.0, 26.0], [8.0, 8.0, 4.0, 56.0, 52.0, 44.0], [34.0, 30.0, 20.0, 60.0, 50.0, 46.0]]),
            torch.tensor([[6.0, 6.0, 6.0, 40.0, 36.0, 30.0], [20.0, 22.0, 12.0, 36.0, 34.0, 26.0]])]


def _oracle_losses(geom, use_obb, kind, logits, reg, ctr, targets, dtype):
    """oracle FCOS.losses on the flat tensors reshaped into its per-level [N, C, W, L, H] lists -> losses and gradients on the flat order."""
    from oracle import fcos as OF
    D = 8 if use_obb else 6
    model = OF.FCOS(None, None, strides=geom.strides, use_obb=use_obb, center_sampling_radius=1.5, iou_loss_type=kind, norm_reg_targets=True)
    lf, rf, cf = (t.to(dtype).clone().requires_grad_() for t in (logits, reg, ctr))
    cls, regs, ctrs = [], [], []
    for l, d in enumerate(geom.dims):
        a, b = geom.off[l], geom.off[l + 1]
        cls.append(lf[a:b].reshape(geom.n, *d, 1).permute(0, 4, 1, 2, 3))
        regs.append(rf[a:b].reshape(geom.n, *d, D).permute(0, 4, 1, 2, 3))
        ctrs.append(cf[a:b].reshape(geom.n, *d, 1).permute(0, 4, 1, 2, 3))
    locs = [p.to(dtype) for p in geom.locations]
    losses = model.losses(locs, cls, regs, ctrs, [t.to(dtype) for t in targets], OF.padding_masks(locs, geom.ori))
    grads = [torch.autograd.grad(lo, x)[0] for lo, x in zip(losses[:3], (lf, rf, cf))]
    return [lo.detach() for lo in losses[:3]], grads, losses[3]


@pytest.mark.parametrize("use_obb,kind", [(False, "iou"), (False, "linear_iou"), (False, "giou"), (False, "smooth_l1"), (True, "smooth_l1")],
                         ids=["aabb-iou", "aabb-linear_iou", "aabb-giou", "aabb-smooth_l1", "obb-smooth_l1"])
def test_loss_composition_matches_oracle_fp64(use_obb, kind, dev):
    """FCOSLossComputation.__call__ on hand-made head outputs (two scenes of different size, three levels) against oracle FCOS.losses in
    float64: the three losses and their gradients with respect to logits, regressions and centerness.  The classification part carries
    the focal bound divided by the positive count; the regression and centerness parts are torch ops on the positive locations and get
    max(4 x the oracle's own fp32-versus-fp64 error on the same inputs, 8u x the tensor's scale)."""
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model.fcos.loss import FCOSLossComputation
    geom = R.Geometry(2, LOSS_DIMS, LOSS_STRIDES, LOSS_SIZES)
    D = 8 if use_obb else 6
    targets = [R.as_obb(t) for t in LOSS_GTS] if use_obb else LOSS_GTS
    g = torch.Generator().manual_seed(5000 + D)
    logits, ctr = torch.randn(geom.total, generator=g) * 2.0, torch.randn(geom.total, generator=g)
    reg = torch.randn(geom.total, D, generator=g).abs() * 3.0 + 0.1
    if use_obb:
        reg[:, 6:] = torch.rand(geom.total, 2, generator=g) - 0.5
    l64, g64, aux = _oracle_losses(geom, use_obb, kind, logits, reg, ctr, targets, F64)
    l32, g32, _ = _oracle_losses(geom, use_obb, kind, logits, reg, ctr, targets, F32)
    valid = geom.valid()
    npos = float(aux["pos"].numel())
    assert npos > 20

    lg, rg, cg = (t.to(dev).requires_grad_() for t in (logits, reg, ctr))
    crit = FCOSLossComputation(list(LOSS_STRIDES), 1.5, kind, True, 1, use_obb, False)
    losses = crit(ops.FcosGeometry(geom.n, geom.dims, geom.strides), lg, rg, cg, [t.to(dev) for t in targets], geom.ori)
    grads = [torch.autograd.grad(lo, x)[0] for lo, x in zip(losses, (lg, rg, cg))]
    torch.cuda.synchronize()
    labels = crit.last_aux["labels"].cpu()
    R.check_equal(labels[valid], aux["labels"].to(torch.int8), "composed labels")
    assert (labels[~valid] == -1).all()

    # classification: the focal kernel; the division by the positive count and the upstream factor 1 / npos add 2u
    ref = R.focal_ref(logits, labels)
    t32, f32g = R.focal_eval(logits, labels)
    k_s = R.allowance(abs(t32.sum().item() - ref.sum) / ref.sum_bound)
    k_g = R.allowance(R.ratio(f32g, ref.grad, ref.grad_bound))
    assert abs(ref.sum / npos - l64[0].item()) <= 1e-12 * abs(l64[0].item())
    R.check(losses[0], l64[0], ref.sum_bound / npos + 2 * R.U * abs(l64[0].item()), k_s, f"{kind} loss_cls")
    gl = torch.zeros(geom.total, dtype=F64)
    gl[valid] = g64[0][valid]
    R.check(grads[0], gl, ref.grad_bound / npos + 2 * R.U * gl.abs(), k_g, f"{kind} d loss_cls / d logits")
    # regression and centerness: torch ops
    for i, name in ((1, "loss_reg"), (2, "loss_centerness")):
        tol = max(4.0 * abs(l32[i].item() - l64[i].item()), 8 * R.U * abs(l64[i].item()))
        R.check(losses[i], l64[i], tol, 1.0, f"{kind} {name}")
        scale = g64[i].abs().max().item()
        tol = max(4.0 * (g32[i].double() - g64[i]).abs().max().item(), 8 * R.U * scale)
        R.check(grads[i], g64[i], tol, 1.0, f"{kind} d {name}")
        assert not grads[i].cpu()[~valid].any()
