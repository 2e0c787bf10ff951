"""GPU: the second-stage pooling kernels -- csrc/roialign.hip through ops.roi_align_rotated_3d_fwd / _bwd and csrc/roipool.hip through
ops.RoiPoolFn.apply -- against the float64 references of tests/roi_ref.py: every decided element of every output and gradient inside its
own derived bound (times the allowance k = max(1, min(2, 4 r)), r measured on torch's fp32 CPU evaluation of the same case, never on the
kernel), or equal where the arithmetic is exact.  fp32 and bf16 maps (bf16 RoIAlign backward and bf16 'interpolation' included), the
families of roi_ref (random, exact, right angles, offset, ties, stacked, gradient scale, bad batch index, empty, resize edges), the caps on
undecided elements, two runs bit-equal, and non-finite upstream gradients: what autograd would leave non-finite never comes out finite.
The bounds and their derivation are in roi_ref's docstring; tests/test_roi_bounds_host.py shows on the CPU that they are satisfiable and
sharp.  Every check prints its worst |err| / bound (run with -s).  The float64 work runs on the CPU and is cached per module."""
import pytest
import torch

import roi_ref as R

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
ALIGN = R.align_cases()
POOL = {kind: R.pool_cases(kind) for kind in ("aabb", "pooling", "interpolation")}
DTYPES = [F32, BF16]
_ids = {F32: "fp32", BF16: "bf16"}
_cache = {}


def _same_bits(a, b):
    """Bit-equality of two runs (torch.equal would call a NaN different from itself)."""
    if a is None or b is None:
        return a is None and b is None
    view = torch.int32 if a.dtype == F32 else torch.int16
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _q(t, dtype):
    return R.bf16_round(t) if dtype == BF16 else t


# ======================================================================================================================
# rotated RoIAlign
# ======================================================================================================================
def align_ref(name, dtype, top_scale=1.0):
    key = ("align", name, dtype, top_scale)
    if key not in _cache:
        c = ALIGN[name]()
        feat, top = _q(c.feat, dtype), _q(c.top * top_scale, dtype)
        _cache[key] = (c, feat, top, R.align_case(feat, c.rois, c.scale, c.pooled, c.sampling, top, bf16=dtype == BF16, exact=c.exact))
    return _cache[key]


def align_run(c, feat, top, dtype, dev):
    from nerf_rpn_amd import ops
    f, t, rois = feat.to(dev).to(dtype), top.to(dev).to(dtype), c.rois.to(dev)
    out = ops.roi_align_rotated_3d_fwd(f, rois, c.scale, c.pooled, c.sampling)
    grads = [ops.roi_align_rotated_3d_bwd(t, rois, tuple(f.shape), c.scale, c.pooled, c.sampling) for _ in range(2)]
    torch.cuda.synchronize()
    assert out.dtype == dtype and grads[0].dtype == dtype
    assert _same_bits(grads[0], grads[1]), "two runs of the backward differ"
    C = feat.shape[-1]
    return out.float().cpu().reshape(c.rois.shape[0], -1, C), grads[0].float().cpu().reshape(-1, C)


def align_check(c, o, out, grad, what):
    d = o.out_decided[..., None].expand_as(o.out)
    assert R.undecided_share(o.out_decided) <= c.cap and R.undecided_share(o.grad_decided) <= c.cap
    k_o = R.allowance(R.ratio(o.out32[d], o.out[d], o.out_bound[d]))
    k_g = R.allowance(R.ratio(o.grad32[o.grad_decided], o.grad[o.grad_decided], o.grad_bound[o.grad_decided]))
    R.check(out[d], o.out[d], o.out_bound[d], k_o, what + " forward")
    R.check(grad[o.grad_decided], o.grad[o.grad_decided], o.grad_bound[o.grad_decided], k_g, what + " backward")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
@pytest.mark.parametrize("name", list(ALIGN))
def test_roialign_matches_fp64(name, dtype, dev):
    c, feat, top, o = align_ref(name, dtype)
    out, grad = align_run(c, feat, top, dtype, dev)
    align_check(c, o, out, grad, f"roialign {name} {_ids[dtype]}")
    if c.exact and dtype == F32:
        R.check_equal(out, o.out.float(), f"roialign {name} forward")
        R.check_equal(grad, o.grad.float(), f"roialign {name} backward")
    if name == "bad-batch":
        assert (~o.geo.good).sum() == 3 and not out[~o.geo.good].any(), "a RoI with a bad batch index must pool to exact zeros"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
@pytest.mark.parametrize("scale", [1e-9, 1e3])
def test_roialign_gradient_scale(scale, dtype, dev):
    """grad_out x 1e-9: contributions near and below 2^-45 (those vanish, the bound holds 2^-45 for each); x 1e3: far from the clamp."""
    c, feat, top, o = align_ref("random-c4", dtype, scale)
    out, grad = align_run(c, feat, top, dtype, dev)
    align_check(c, o, out, grad, f"roialign grad_out x {scale:g} {_ids[dtype]}")
    if scale == 1e-9:        # single contributions top w / count of the valid samples: some are below 2^-45 and vanish, others are well above
        g = o.geo
        t = top.reshape(-1, top.shape[-1])[g.roi * g.nbins + g.bin].double().abs()
        contrib = (t[:, None, :] * g.w[:, :, None] / g.count[g.roi][:, None, None])[g.valid]
        assert ((contrib > 0) & (contrib < 2.0 ** -45)).any() and (contrib > 2.0 ** -40).any()


def test_roialign_one_contribution_lands_on_the_clamp(dev):
    """One RoI of one voxel on an integer centre: a single sample, a single tap of weight 1, count 1.  grad_out = +-1e7 is clamped to
    +-2^18 (the documented clamp of one contribution), every other element is what it was."""
    from nerf_rpn_amd import ops
    rois = torch.tensor([[0, 3.0, 3.0, 2.0, 1.0, 1.0, 1.0, 0.0], [1, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0]])
    top = torch.tensor([[1e7, -1e7, 3.0, 2.0 ** 18], [-4.0, 5.0, 1e7, -1e7]]).reshape(2, 1, 1, 1, 4)
    ref = R.align_case(torch.zeros(2, 7, 6, 5, 4), rois, 1.0, (1, 1, 1), 0, top, exact=True)
    grad = ops.roi_align_rotated_3d_bwd(top.to(dev), rois.to(dev), (2, 7, 6, 5, 4), 1.0, (1, 1, 1), 0).cpu()
    R.check_equal(grad.reshape(-1, 4), ref.grad.float(), "roialign clamp")
    assert grad[0, 3, 3, 2].tolist() == [2.0 ** 18, -2.0 ** 18, 3.0, 2.0 ** 18] and grad[1, 2, 1, 1].tolist() == [-4.0, 5.0, 2.0 ** 18, -2.0 ** 18]
    assert grad.count_nonzero().item() == 8


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
def test_roialign_without_rois(dtype, dev):
    from nerf_rpn_amd import ops
    feat = torch.randn(2, 7, 6, 5, 12, device=dev).to(dtype)
    out = ops.roi_align_rotated_3d_fwd(feat, torch.zeros(0, 8, device=dev), 1.0, (2, 3, 2), 0)
    grad = ops.roi_align_rotated_3d_bwd(torch.zeros(0, 2, 3, 2, 12, device=dev, dtype=dtype), torch.zeros(0, 8, device=dev), (2, 7, 6, 5, 12), 1.0, (2, 3, 2), 0)
    assert tuple(out.shape) == (0, 2, 3, 2, 12) and tuple(grad.shape) == (2, 7, 6, 5, 12) and grad.dtype == dtype and not grad.any()


def finite_allowance(g32, ref_grad, ref_bound, decided):
    """k = max(1, min(2, 4 r)) with r of the torch fp32 evaluation over the elements that are finite in it and in the reference."""
    m = decided & torch.isfinite(ref_grad) & torch.isfinite(g32.double())
    return R.allowance(R.ratio(g32[m], ref_grad[m], ref_bound[m]))


def nonfinite_check(ref_grad, ref_bound, decided, got, k, what):
    """Wherever the reference's gradient is not finite the kernel's is not; wherever the kernel's is finite it is within its bound."""
    bad_ref, fin = ~torch.isfinite(ref_grad), torch.isfinite(got)
    assert bad_ref.any(), what + ": the fixture produced no non-finite gradient"
    leaked = bad_ref & fin
    print(f"{what}: reference non-finite at {int(bad_ref.sum())} elements, kernel finite at {int(leaked.sum())} of them "
          f"(kernel finite at {int(fin.sum())} of {fin.numel()})")
    assert not leaked.any(), (what, "a non-finite contribution came out finite", got[leaked][:4].tolist())
    m = fin & decided
    if m.any():
        R.check(got[m], ref_grad[m], ref_bound[m], k, what + " finite part")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
@pytest.mark.parametrize("poison", ["nan", "inf", "-inf", "inf-at-zero-weight"])
def test_roialign_nonfinite_upstream_gradient(poison, dtype, dev):
    """NaN / +-Inf in grad_out only (no address depends on it).  'inf-at-zero-weight': +Inf on a bin of the exact family whose samples sit
    on integers, where seven of the eight taps have weight 0: inf * 0 is NaN for autograd."""
    name = "exact" if poison == "inf-at-zero-weight" else "random-c4"
    c = ALIGN[name]()
    feat, top = _q(c.feat, dtype), _q(c.top, dtype).clone()
    value = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf"), "inf-at-zero-weight": float("inf")}[poison]
    top[0, 0, 0, 0, 1] = value
    top[5, 1, 2, 1, 2] = value
    o = R.align_case(feat, c.rois, c.scale, c.pooled, c.sampling, top, bf16=dtype == BF16, exact=c.exact)
    _, grad = align_run(c, feat, top, dtype, dev)
    decided = o.grad_decided[:, None].expand_as(o.grad)
    k = finite_allowance(o.grad32, o.grad, o.grad_bound, decided)
    nonfinite_check(o.grad, o.grad_bound, decided, grad.double(), k, f"roialign {poison} {_ids[dtype]}")


# ======================================================================================================================
# ROIPool without the op
# ======================================================================================================================
def pool_ref(kind, name, dtype, dout_scale=1.0):
    key = ("pool", kind, name, dtype, dout_scale)
    if key not in _cache:
        c = POOL[kind][name]()
        feats, dout = [_q(f, dtype) for f in c.feats], c.dout * dout_scale
        args = (kind, feats, c.meta, c.level_of, c.scales, c.out_size)
        _cache[key] = (c, feats, dout, R.pool_eval(*args, F64, dout, bf16=dtype == BF16, exact=c.exact),
                       R.pool_eval(*args, F32, dout, bf16=dtype == BF16, exact=c.exact))
    return _cache[key]


def pool_run(c, feats, dout, dtype, dev, need_grad=None):
    from nerf_rpn_amd import ops
    need_grad = [True] * len(feats) if need_grad is None else need_grad
    runs = []
    for _ in range(2):
        leaves = [f.to(dev).to(dtype).requires_grad_(ng) for f, ng in zip(feats, need_grad)]
        out = ops.RoiPoolFn.apply(c.kind, c.meta.to(dev), c.level_of.to(dev), c.scales, c.out_size, *[f.permute(3, 0, 1, 2) for f in leaves])
        out.backward(dout.permute(0, 4, 1, 2, 3).to(dev))
        torch.cuda.synchronize()
        assert out.dtype == F32 and all(f.grad is None or f.grad.dtype == dtype for f in leaves)
        runs.append((out.detach().permute(0, 2, 3, 4, 1).cpu(), [None if f.grad is None else f.grad.float().cpu() for f in leaves]))
    assert torch.equal(runs[0][0], runs[1][0]), "two runs of the forward differ"
    assert all(_same_bits(a, b) for a, b in zip(runs[0][1], runs[1][1])), "two runs of the backward differ"
    return runs[0]


def pool_check(c, o, e, out, grads, what, bf16=False):
    d = o.out_decided[..., None].expand_as(o.out)
    assert R.undecided_share(o.out_decided) <= c.cap and all(R.undecided_share(m) <= R.grad_cap(c, bf16) for m in o.grad_decided)
    if c.kind == "aabb":
        R.check_equal(out, o.out.float(), what + " forward")
    else:
        R.check(out[d], o.out[d], o.out_bound[d], R.allowance(R.ratio(e.out[d], o.out[d], o.out_bound[d])), what + " forward")
    for l, (g, w, b, m, g32) in enumerate(zip(grads, o.grads, o.grad_bounds, o.grad_decided, e.grads)):
        if g is None:
            continue
        R.check(g[m], w[m], b[m], R.allowance(R.ratio(g32[m], w[m], b[m])), what + f" gradient of level {l}")


# every family in both types.  ('pooling', 'offset', bf16): the forward is checked in full and the decided part of the gradient; the cap on
# undecided gradient voxels is waived for that fixture alone (roi_ref.pool_cases says why)
POOL_RUNS = [(kind, name, dtype) for kind in POOL for name in POOL[kind] for dtype in DTYPES]


@pytest.mark.parametrize("kind,name,dtype", POOL_RUNS, ids=lambda v: _ids.get(v, v))
def test_roipool_matches_fp64(kind, name, dtype, dev):
    c, feats, dout, o, e = pool_ref(kind, name, dtype)
    out, grads = pool_run(c, feats, dout, dtype, dev)
    what = f"roipool {kind} {name} {_ids[dtype]}"
    pool_check(c, o, e, out, grads, what, dtype == BF16)
    if (kind, name, dtype) == ("pooling", "offset", BF16):
        assert o.out_decided.all() and any(m.any() for m in o.grad_decided)
    if c.exact:                       # ties included: the value, the argmax and the voxel that receives the gradient are exact
        R.check_equal(out, o.out.float(), what + " forward")
        if dtype == F32:
            for l, (g, w) in enumerate(zip(grads, o.grads)):
                R.check_equal(g, w.float(), what + f" gradient of level {l}")
    if name == "ties-negative":
        assert (out == 0).any(), "no window in which the padding zero wins"
    if name == "unused-level":
        assert not grads[1].any(), "a level that no RoI uses must receive exact zeros"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
@pytest.mark.parametrize("kind", list(POOL))
@pytest.mark.parametrize("scale", [1e-9, 1e3])
def test_roipool_gradient_scale(scale, kind, dtype, dev):
    c, feats, dout, o, e = pool_ref(kind, "random-c3", dtype, scale)
    out, grads = pool_run(c, feats, dout, dtype, dev)
    pool_check(c, o, e, out, grads, f"roipool {kind} grad_out x {scale:g} {_ids[dtype]}", dtype == BF16)


def test_roipool_one_contribution_lands_on_the_clamp(dev):
    """'aabb' hands the whole of dout to one voxel: +-1e7 arrives as +-2^18 (the rotated kinds split a gradient over eight corners,
    which coincide at an integer point: eight clamped contributions to one voxel are beyond the documented range of the sum, 2^19)."""
    c, feats, dout, o, e = pool_ref("aabb", "exact", F32, 1.0)
    big = dout.clone()
    big[0, 0, 0, 0, 0], big[3, 1, 1, 1, 1] = 1e7, -1e7
    ref = R.pool_eval("aabb", feats, c.meta, c.level_of, c.scales, c.out_size, F64, big, exact=True)
    out, grads = pool_run(c, feats, big, F32, dev)
    for l, (g, w) in enumerate(zip(grads, ref.grads)):
        R.check_equal(g, w.float(), f"roipool aabb clamp, level {l}")
    assert (ref.grads[0] > 2.0 ** 17).any() and (ref.grads[1] < -2.0 ** 17).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
@pytest.mark.parametrize("kind", list(POOL))
def test_roipool_empty_and_frozen_levels(kind, dtype, dev):
    """R = 0: the gradient is exact zeros of the map's shape; a level that does not require grad gets none and the other is unchanged."""
    from nerf_rpn_amd import ops
    c, feats, dout, o, e = pool_ref(kind, "random-c3", dtype)
    leaves = [f.to(dev).to(dtype).requires_grad_() for f in feats]
    meta = c.meta[:0].to(dev)
    out = ops.RoiPoolFn.apply(kind, meta, c.level_of[:0].to(dev), c.scales, c.out_size, *[f.permute(3, 0, 1, 2) for f in leaves])
    assert tuple(out.shape) == (0, 3, *c.out_size)
    out.backward(torch.zeros_like(out))
    assert all(f.grad is not None and f.grad.shape == f.shape and f.grad.dtype == dtype and not f.grad.any() for f in leaves)
    out, grads = pool_run(c, feats, dout, dtype, dev, need_grad=[True, False])
    assert grads[1] is None
    pool_check(c, o, e, out, grads, f"roipool {kind} frozen level 1 {_ids[dtype]}", dtype == BF16)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids.get)
@pytest.mark.parametrize("kind", list(POOL))
@pytest.mark.parametrize("poison", ["nan", "inf", "-inf"])
def test_roipool_nonfinite_upstream_gradient(poison, kind, dtype, dev):
    """NaN / +-Inf in the upstream gradient only.  'interpolation' on the exact family multiplies +-Inf by resize weights that are 0
    (inf * 0); the rotated kinds also hold grid points outside the map, whose blend the reference multiplies by its 0 mask."""
    name = "exact" if kind == "interpolation" else "random-c3"
    c, feats, dout, o, e = pool_ref(kind, name, dtype)
    bad = dout.clone()
    value = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf")}[poison]
    bad[0, 0, 0, 0, 0], bad[1, 0, 0, 0, 1], bad[6, -1, -1, -1, 2], bad[7, 0, 1, 0, 0] = value, value, value, value
    ref = R.pool_eval(kind, feats, c.meta, c.level_of, c.scales, c.out_size, F64, bad, bf16=dtype == BF16, exact=c.exact)
    e32 = R.pool_eval(kind, feats, c.meta, c.level_of, c.scales, c.out_size, F32, bad, bf16=dtype == BF16, exact=c.exact)
    out, grads = pool_run(c, feats, bad, dtype, dev)
    hit = False
    for l, (g, w, b, m, g32) in enumerate(zip(grads, ref.grads, ref.grad_bounds, ref.grad_decided, e32.grads)):
        k = finite_allowance(g32, w, b, m)
        if torch.isfinite(w).all():
            R.check(g[m], w[m], b[m], k, f"roipool {kind} {poison} {_ids[dtype]} level {l} (no non-finite contribution)")
            continue
        hit = True
        nonfinite_check(w, b, m, g.double(), k, f"roipool {kind} {poison} {_ids[dtype]} level {l}")
    assert hit
