"""GPU: the proposal / target kernels of csrc/postproc.hip -- anchors, decode_boxes / encode_boxes / coder_pairs (both coders), obb_to_aabb,
head_flatten / head_unflatten, filter_candidates, select_kept, match_anchors, rpn_sampled_loss -- against the references of
tests/rpn_ref.py: every decided element inside its own derived bound times the allowance k = max(1, min(2, 4 r)) (r measured on torch's
fp32 CPU evaluation of the same case, never on the kernel), or equal where the arithmetic is exact.  The bounds, the decided masks and the
families are described in rpn_ref's docstring; tests/test_rpn_bounds_host.py shows on the CPU that they are satisfiable and sharp.  Every
check prints its worst |err| / (k bound) (run with -s) and, when it fails, the inputs of the offending row."""
import pytest
import torch

import rpn_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def hold(what, err, bound, dec, k, *inputs):
    """err <= k bound on every decided element; prints the worst ratio, and the inputs of the offending row when it fails."""
    m = torch.where(dec, err / (k * bound), torch.zeros_like(err))
    m = torch.where(torch.isfinite(m), m, torch.full_like(m, float("inf")))
    worst = m.max().item() if m.numel() else 0.0
    print(f"{what}: max err / (k bound) = {worst:.3f} (k = {k:.2f}, {int(dec.sum())} of {dec.numel()} elements decided)")
    if not worst <= 1.0:
        row = int(m.reshape(m.shape[0], -1).max(1).values.argmax())
        raise AssertionError((what, "worst ratio", worst, "bad elements", int((m > 1).sum()), "row", row, "ratios", m[row].tolist(),
                              "inputs", [t[row].tolist() for t in inputs]))
    return worst


def k_of(err32, bound, dec):
    return R.allowance((err32[dec] / bound[dec]).max().item() if dec.any() else 0.0)


def mid_err(got, want):
    err = (got.double() - want).abs()
    err[:, 6] = R.angle_diff(got[:, 6], want[:, 6]).abs()
    return err


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def table(p, dev):
    from nerf_rpn_amd import ops
    return cached(("table", p.mesh), lambda: ops.AnchorTable(p.mesh, p.grids, ops.ANCHOR_SIZES[:len(p.grids)], ops.ASPECT_RATIOS[:len(p.grids)], device=dev))


# ======================================================================================================================
# anchors
# ======================================================================================================================
def test_anchors_small_non_cubic_pyramid(dev):
    from nerf_rpn_amd import ops
    p = R.pyramid(R.SMALL)
    tab = table(p, dev)
    assert tab.total == p.total and tab.strides == p.strides
    want = R.anchors_ref(p)
    R.check_equal(ops.anchors(tab), want, "anchors, whole table")
    sel = torch.tensor([0, 12, 13, p.offsets[1] - 1, p.offsets[1], p.offsets[2] - 1, p.offsets[2], p.total - 1, 255, 256, 257])
    R.check_equal(ops.anchors(tab, sel.to(dev)), want[sel], "anchors, selected")


def test_anchors_level_offsets_beyond_32_bits(dev):
    """Levels that start above 2^31 and 2^32 (the lo / hi words of the table), queried through sel only."""
    from nerf_rpn_amd import ops
    p = R.pyramid(R.BIG)
    tab = table(p, dev)
    assert tab.total == p.total > 1 << 32 and tab.offsets == p.offsets
    sel = R.big_table_sel(p)
    got = ops.anchors(tab, torch.tensor(sel, dtype=torch.int64, device=dev))
    R.check_equal(got, R.anchors_ref(p, sel), "anchors beyond 2^32")
    # the coders read the same cell: zero deltas decode every selected anchor to itself (exp(0) = 1, integer coordinates)
    s = torch.tensor([v for v in sel if v < 1 << 23], dtype=torch.int64)      # the delta buffer is indexed by the flat anchor number
    assert 6 <= s.numel() and int(s.max()) > 1 << 22
    deltas = torch.zeros(int(s.max()) + 1, 6)
    R.check_equal(ops.decode_boxes(tab, deltas.to(dev), s.to(dev), 0), R.anchors_ref(p, s.numpy()), "decode at the first anchors of the big table")
    # ... and an anchor encodes to exact zeros against itself, at every selected index (gt is indexed by row, the anchor by sel)
    enc = ops.encode_boxes(tab, R.anchors_ref(p, sel).to(dev), torch.tensor(sel, dtype=torch.int64, device=dev), 0)
    R.check_equal(enc, torch.zeros(len(sel), 6), "encode of each selected anchor against itself")


# ======================================================================================================================
# coders
# ======================================================================================================================
def run_decode(f, dev):
    """The four entry points agree bit for bit: decode_boxes through the table with sel, with sel = None, and coder_pairs."""
    from nerf_rpn_amd import ops
    tab = table(f.pyramid, dev)
    full = R.scatter_deltas(f).to(dev)
    sel = f.sel.to(dev)
    via_tab = ops.decode_boxes(tab, full, sel, f.coder)
    pairs = ops.coder_pairs(full[sel], ops.anchors(tab, sel), f.coder, False)
    assert torch.equal(bits(via_tab), bits(pairs)), "decode_boxes(tab, deltas, sel) != coder_pairs(deltas[sel], anchors(tab, sel))"
    everything = ops.decode_boxes(tab, full, None, f.coder)
    assert torch.equal(bits(everything), bits(ops.decode_boxes(tab, full, torch.arange(f.pyramid.total, device=dev), f.coder))), "sel = None"
    assert torch.equal(bits(everything[sel]), bits(via_tab))
    holes = sel.clone()
    holes[::3] = -1
    z = ops.decode_boxes(tab, full, holes, f.coder)
    assert not z[::3].any() and torch.equal(bits(z[1::3]), bits(via_tab[1::3])), "rows with sel < 0 decode to exact zeros"
    return via_tab.cpu()


@pytest.mark.parametrize("name", ["random", "clamp"])
def test_aabb_decode(name, dev):
    f = R.decode_family(name, 0)
    want, bound = cached(("d6", name), lambda: R.aabb_decode(f.deltas, f.anchors, F64, bound=True))
    dec = torch.ones_like(bound, dtype=torch.bool)
    k = k_of((R.aabb_decode(f.deltas, f.anchors, F32).double() - want).abs(), bound, dec)
    hold(f"aabb decode {name}", (run_decode(f, dev).double() - want).abs(), bound, dec, k, f.deltas, f.anchors)


@pytest.mark.parametrize("name", ["random", "clamp", "theta", "square"])
def test_midpoint_decode(name, dev):
    f = R.decode_family(name, 1)
    want, bound, info = cached(("d8", name), lambda: R.mid_decode(f.deltas, f.anchors, F64, bound=True))
    assert R.undecided_share(info.decided) <= f.cap
    k = k_of(mid_err(R.mid_decode(f.deltas, f.anchors, F32), want), bound, info.decided)
    got = run_decode(f, dev)
    assert torch.isfinite(got).all()
    hold(f"midpoint decode {name}", mid_err(got, want), bound, info.decided, k, f.deltas, f.anchors)


def test_midpoint_decode_degenerate(dev):
    """da -> +0.5 with db -> -0.5 and the mirror: finite outputs; x, y, z, depth and the larger planar side inside their bounds; on the
    exactly degenerate rows the angle is exactly 0 (wide) or -kHalfPiRef."""
    f = R.decode_family("degenerate", 1)
    want, bound, info = cached(("d8", "degenerate"), lambda: R.mid_decode(f.deltas, f.anchors, F64, bound=True))
    got32 = R.mid_decode(f.deltas, f.anchors, F32)
    got = run_decode(f, dev)
    assert torch.isfinite(got).all()
    cols = [0, 1, 2, 5]
    dec = torch.ones(got.shape[0], 4, dtype=torch.bool)
    hold("midpoint decode degenerate, x y z depth", mid_err(got, want)[:, cols], bound[:, cols], dec,
         k_of(mid_err(got32, want)[:, cols], bound[:, cols], dec), f.deltas, f.anchors)
    ok = (info.larger.bound <= R.COND * info.side)[:, None]
    e32 = (torch.maximum(got32[:, 3], got32[:, 4]).double() - info.larger.value).abs()[:, None]
    e = (torch.maximum(got[:, 3], got[:, 4]).double() - info.larger.value).abs()[:, None]
    hold("midpoint decode degenerate, larger side", e, info.larger.bound[:, None], ok, k_of(e32, info.larger.bound[:, None], ok), f.deltas, f.anchors)
    print(f"    undecided: larger side {100 * R.undecided_share(ok):.1f} %, smaller side and angle {100 * R.undecided_share(info.decided[:, [4, 6]]):.1f} %")
    small, s64 = torch.minimum(got[:, 3], got[:, 4]).double(), torch.minimum(want[:, 3], want[:, 4])
    flip = (small >= 1e-3) != (s64 >= 1e-3)
    print(f"    a min_size = 1e-3 cut decides {int(flip.sum())} of {flip.numel()} rows differently from float64"
          + (f" (float64 sides {s64[flip].min().item():.2e} .. {s64[flip].max().item():.2e}, device {small[flip].min().item():.2e} .. "
             f"{small[flip].max().item():.2e})" if flip.any() else ""))
    ex = (f.deltas[:, 6] == 0.5) & (f.deltas[:, 7] == -0.5) & ((info.w - info.h).abs() > 1e-3 * info.side)
    assert ex.sum() >= 32
    expect = torch.where(info.w[ex] > info.h[ex], 0.0, -R.HALF_PI_REF).float()
    R.check_equal(got[ex, 6], expect, "angle of the exactly degenerate rows")


def run_encode(gt, sel, p, coder, dev):
    from nerf_rpn_amd import ops
    tab = table(p, dev)
    g, s = gt.to(dev), sel.to(dev)
    via_tab = ops.encode_boxes(tab, g, s, coder)
    pairs = ops.coder_pairs(g, ops.anchors(tab, s), coder, True)
    assert torch.equal(bits(via_tab), bits(pairs)), "encode_boxes(tab, gt, sel) != coder_pairs(gt, anchors(tab, sel))"
    head = min(gt.shape[0], p.total)
    assert torch.equal(bits(ops.encode_boxes(tab, g[:head], None, coder)), bits(ops.encode_boxes(tab, g[:head], torch.arange(head, device=dev), coder)))
    return via_tab.cpu()


def test_aabb_encode(dev):
    f = R.gt6_family()
    want, bound = R.aabb_encode(f.gt, f.anchors, F64, bound=True)
    dec = torch.ones_like(bound, dtype=torch.bool)
    k = k_of((R.aabb_encode(f.gt, f.anchors, F32).double() - want).abs(), bound, dec)
    hold("aabb encode", (run_encode(f.gt, f.sel, f.pyramid, 0, dev).double() - want).abs(), bound, dec, k, f.gt, f.anchors)


@pytest.mark.parametrize("name", ["random", "theta"])
def test_midpoint_encode(name, dev):
    f = R.gt_family(name)
    want, bound, info = R.mid_encode(f.gt, f.anchors, F64, bound=True)
    assert R.undecided_share(info.decided) <= f.cap
    k = k_of((R.mid_encode(f.gt, f.anchors, F32).double() - want).abs(), bound, info.decided)
    got = run_encode(f.gt, f.sel, f.pyramid, 1, dev)
    hold(f"midpoint encode {name}", (got.double() - want).abs(), bound, info.decided, k, f.gt, f.anchors)


def test_round_trip(dev):
    """decode(encode(gt)) on the device against the float64 round trip, held to the decode bound plus the encode bound carried through
    the decode's Jacobian."""
    from nerf_rpn_amd import ops
    f = R.gt_family("roundtrip")
    enc, b_enc, ie = R.mid_encode(f.gt, f.anchors, F64, bound=True)
    want, b_dec, info = R.mid_decode(enc, f.anchors, F64, bound=True)
    bound = b_dec + R.decode_jacobian_bound(enc, f.anchors, b_enc)
    dec = info.decided & ie.decided.all(1)[:, None]
    assert R.undecided_share(dec) <= f.cap
    k = k_of(mid_err(R.mid_decode(R.mid_encode(f.gt, f.anchors, F32), f.anchors, F32), want), bound, dec)
    an = f.anchors.to(dev)
    got = ops.coder_pairs(ops.coder_pairs(f.gt.to(dev), an, 1, True), an, 1, False).cpu()
    hold("round trip", mid_err(got, want), bound, dec, k, f.gt, f.anchors)
    hold("round trip against the ground truth itself", mid_err(got, f.gt.double()), bound + 1e-6, dec, k, f.gt, f.anchors)


def test_obb_to_aabb(dev):
    from nerf_rpn_amd import ops
    for name in ("random", "theta"):
        f = R.gt_family(name)
        want, bound = R.obb_to_aabb(f.gt, F64, bound=True)
        dec = torch.ones_like(bound, dtype=torch.bool)
        k = k_of((R.obb_to_aabb(f.gt, F32).double() - want).abs(), bound, dec)
        hold(f"obb_to_aabb {name}", (ops.obb_to_aabb(f.gt.to(dev)).cpu().double() - want).abs(), bound, dec, k, f.gt)


# ======================================================================================================================
# head_flatten / head_unflatten
# ======================================================================================================================
@pytest.mark.parametrize("cells,A,dw,pad", R.HEAD_CASES)
def test_head_flatten_and_unflatten(cells, A, dw, pad, dev):
    from nerf_rpn_amd import lib, ops
    c = R.head_case(cells, A, dw, pad)
    st = ops._s()
    head = c.head.to(dev)
    logits = torch.full((cells * A,), float("nan"), device=dev)
    deltas = torch.full((cells * A, dw), float("nan"), device=dev)
    lib.call("head_flatten_f32", head.data_ptr(), cells, c.ld, A, dw, logits.data_ptr(), deltas.data_ptr(), st)
    wl, wd = R.head_flatten_ref(c)
    assert torch.equal(bits(logits.cpu()), bits(wl)) and torch.equal(bits(deltas.cpu()), bits(wd)), "head_flatten"
    gl, gd, sc = c.logits.to(dev), c.deltas.to(dev), c.scale2.to(dev)
    for bf16 in (False, True):
        for scaled in (False, True):
            out = torch.full((cells, c.ld), float("nan"), dtype=torch.bfloat16 if bf16 else F32, device=dev)
            lib.call("head_unflatten", gl.data_ptr(), gd.data_ptr(), cells, c.ld, A, dw, sc.data_ptr() if scaled else 0, out.data_ptr(),
                     lib.BF16 if bf16 else lib.F32, st)
            want = R.head_unflatten_ref(c, scaled, bf16)
            assert torch.equal(bits(out.cpu()), bits(want)), ("head_unflatten", bf16, scaled)
            assert not out[:, A * (1 + dw):].any(), "padding columns"
    print(f"head_flatten / head_unflatten cells {cells} dw {dw} ld {c.ld}: equal")


# ======================================================================================================================
# filter_candidates
# ======================================================================================================================
@pytest.mark.parametrize("W", [6, 7])
@pytest.mark.parametrize("name", R.FILTER_NAMES)
def test_filter_candidates(name, W, dev):
    from nerf_rpn_amd import ops
    c = R.filter_case(name, W)
    s32 = torch.sigmoid(c.logits)
    s64, sb = R.sigmoid_bound(c.logits)
    k = R.allowance(R.ratio(s32, s64, sb))
    for fix in (False, True):
        ref = R.filter_ref(c.boxes, c.logits, c.levels, c.valid, R.GRID, R.MIN_SIZE, c.thresh, fix)
        ob, os_, ol, cnt = ops.filter_candidates(c.boxes.to(dev), c.logits.to(dev), c.levels.to(dev), c.valid.to(dev), R.GRID, R.MIN_SIZE,
                                                 c.thresh, fix)
        m = int(cnt.item())
        assert m == ref.count, (name, W, fix, m, ref.count)
        R.check_equal(ol[:m], ref.levels, f"filter {name} w{W} fix={fix} levels")
        assert torch.equal(bits(ob[:m].cpu()), bits(ref.boxes)), (name, W, fix, "boxes are copied or clamped: bit-equal")
        _, b = R.sigmoid_bound(c.logits[torch.from_numpy(ref.rows)])
        R.check(os_[:m], ref.scores, b, k, f"filter {name} w{W} fix={fix} scores ({m} of {c.n} rows)")


def test_filter_refuses_more_than_16384(dev):
    from nerf_rpn_amd import lib, ops
    n = R.FILTER_MAX + 1
    with pytest.raises(lib.NrpnError):
        ops.filter_candidates(torch.zeros(n, 7, device=dev), torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                              torch.ones(n, dtype=torch.uint8, device=dev), R.GRID, R.MIN_SIZE, 0.0)


# ======================================================================================================================
# select_kept
# ======================================================================================================================
@pytest.mark.parametrize("W", [6, 7])
@pytest.mark.parametrize("name", R.SELECT_NAMES)
def test_select_kept(name, W, dev):
    from nerf_rpn_amd import ops
    c = R.select_case(name, W)
    wb, ws, wl, m = R.select_ref(c.boxes, c.scores, c.levels, c.keep, c.count, c.post)
    for count in ([None] if c.count == c.n else []) + [torch.tensor([c.count], dtype=torch.int32, device=dev)]:
        ob, os_, ol, oc = ops.select_kept(c.boxes.to(dev), c.scores.to(dev), c.levels.to(dev), c.keep.to(dev), count, c.post)
        assert int(oc.item()) == m, (name, int(oc.item()), m)
        assert torch.equal(bits(ob.cpu()), bits(wb)) and torch.equal(bits(os_.cpu()), bits(ws)) and torch.equal(bits(ol.cpu()), bits(wl)), name
    print(f"select_kept {name} w{W}: {m} of {c.post} rows, equal")


# ======================================================================================================================
# match_anchors
# ======================================================================================================================
@pytest.mark.parametrize("name", R.MATCH_NAMES)
def test_match_anchors(name, dev):
    from nerf_rpn_amd import ops
    c = R.match_case(name)
    (lab, matched), _ = cached(("match", name), lambda: R.match_expect(c))
    got_l, got_m = ops.match_anchors(table(c.pyramid, dev), c.gt.to(dev), R.FG, R.BG, c.ori)
    R.check_equal(got_l, lab, f"match {name} labels")
    R.check_equal(got_m, matched, f"match {name} matched")
    if name == "outside":
        assert (got_l == 1).all()


def test_match_refuses_more_than_1024_boxes(dev):
    from nerf_rpn_amd import lib, ops
    p = R.pyramid(R.SMALL)
    gt = torch.tensor([[1., 1., 1., 9., 9., 9.]]).repeat(R.MAX_GT + 1, 1)
    with pytest.raises(lib.NrpnError):
        ops.match_anchors(table(p, dev), gt.to(dev), R.FG, R.BG)


# ======================================================================================================================
# rpn_sampled_loss
# ======================================================================================================================
@pytest.mark.parametrize("dw", [6, 8])
@pytest.mark.parametrize("npos,nneg", R.LOSS_COUNTS)
def test_sampled_loss(npos, nneg, dw, dev):
    from nerf_rpn_amd import ops
    c = R.loss_case(npos, nneg, dw)
    ref, e32 = R.loss_eval(c, F64), R.loss_eval(c, F32)
    lg, dl = c.logits.to(dev).requires_grad_(True), c.deltas.to(dev).requires_grad_(True)
    o, r = ops.SampledLossFn.apply(lg, dl, c.targets.to(dev), c.pos.to(dev), c.neg.to(dev), R.BETA)
    (o + r).backward()
    what = f"sampled loss ({npos}, {nneg}) dw {dw}"
    R.check(lg.grad, ref.g_logits, ref.b_logits, R.allowance(R.ratio(e32.g_logits, ref.g_logits, ref.b_logits)), what + " dlogits")
    R.check(dl.grad, ref.g_deltas, ref.b_deltas, R.allowance(R.ratio(e32.g_deltas, ref.g_deltas, ref.b_deltas)), what + " ddeltas")
    R.check(o.detach(), ref.bce, ref.b_bce, R.allowance(R.ratio(e32.bce, ref.bce, ref.b_bce)), what + " bce")
    R.check(r.detach(), ref.reg, ref.b_reg, R.allowance(R.ratio(e32.reg, ref.reg, ref.b_reg)), what + " smooth-L1")
    outside = torch.ones(R.LOSS_ROWS, dtype=torch.bool)
    outside[torch.cat([c.pos, c.neg])] = False
    no_pos = torch.ones(R.LOSS_ROWS, dtype=torch.bool)
    no_pos[c.pos] = False
    assert not lg.grad.cpu()[outside].any() and not dl.grad.cpu()[no_pos].any(), "rows outside the sample must stay exactly zero"
    assert torch.isfinite(lg.grad).all() and torch.isfinite(dl.grad).all()
