"""GPU: the row-list conv kernels of the cone head (nrpn_conv3d_fwd_rows, nrpn_conv3d_wgrad_rows) on the exactly summable families of
tests/conv_ref.py.  They share the dense kernels' MFMA loop and none of their addressing: rows are gathered by voxel id, the in-bounds
taps come from a 27-bit word of the list, outputs and the ReLU mask are scattered by voxel id, and the K-slice / tail-split plan is their
own (rows_plan).  Every sum is an fp32 number in any order, so every launch must EQUAL the float64 reference of conv_ref (ROW_CASES): fp32
outputs bit for bit, bf16 outputs its single round-to-nearest-even rounding.

Every test first asserts the plan its case is there for (conv_ref.ROW_PLANS, the same table the host test checks without a GPU).  Inputs
hold NaN wherever a correct kernel does not read: x on the voxels no in-bounds tap of a listed row reaches, dy and the ReLU mask off the
list; outputs start as a sentinel that every row off the list must keep.  Every launch runs twice and must repeat its bits."""
import numpy as np
import pytest
import torch

import conv_ref as cr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SENTINEL = 3.140625           # a bf16 number no output of the families equals on a whole row
NAN = float("nan")

FWD = [(m, l) for m, l, fwd, _ in cr.ROW_CASES if fwd]
WGRAD = [(m, l) for m, l, _, wg in cr.ROW_CASES if wg]
_PLANS = {}


def _dtype(m):
    return BF if m.kind == "i8" else F32


def _code(dtype):
    from nerf_rpn_amd import lib
    return lib.BF16 if dtype == BF else lib.F32


def _list(lname, dev):
    """(ops.ConePlan, k) holding list ``lname``.  The cone lists come from the real cone_build on the sample of conv_ref.cone_sample and must
    equal conv_ref's own derivation; the others are written in the device format by conv_ref.tap_words."""
    from nerf_rpn_amd import ops
    rl = cr.row_list(lname)
    if lname.startswith("cone"):
        if "cone" not in _PLANS:
            from test_gpu_cone import A, _plan
            assert A == cr.CONE_ANCHORS
            plan = _plan(cr.CONE_GRIDS, cr.CONE_SCENES, 2, *cr.cone_sample(), dev)
            lists = plan.lists.cpu().numpy().view(np.uint32)
            for k in range(3):
                want = cr.row_list(f"cone{k}")
                assert plan.counts[k] == want.n
                np.testing.assert_array_equal(lists[k, :want.n], want.words)
            _PLANS["cone"] = plan
        return _PLANS["cone"], int(lname[4:])
    if lname not in _PLANS:
        plan = ops.ConePlan(rl.segs, 1, 0, dev)
        assert plan.total == rl.total and plan.segs == rl.segs
        plan.lists[0, :rl.n] = torch.from_numpy(rl.words.view(np.int32)).to(dev)
        plan.counts = [rl.n]
        _PLANS[lname] = plan
    return _PLANS[lname], 0


def _fwd_plan(n, cin, cout, ksize, dtype):
    from nerf_rpn_amd import lib
    return cr.rows_plan_class(lib.query("conv3d_fwd_rows_workspace_bytes", n, cin, cout, ksize, _code(dtype)), n, cout)


def _poisoned(t, keep, dtype, dev):
    """f64 [total, C] -> device tensor of ``dtype`` with NaN on the rows outside the bool mask ``keep``."""
    t = t.clone()
    t[torch.from_numpy(~keep)] = NAN
    return t.to(dtype).to(dev)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _launch(what, ids, ev, want, x, wp, bias, plan, k, cin, cout, ksize, flags, odt, mask=None):
    """One row-list launch into a sentinel-filled output, twice: the evaluated rows equal ``want`` (f64, as stored), the rows off the list keep
    the sentinel's bits, and the second run repeats the first bit for bit."""
    from nerf_rpn_amd import ops
    dev = x.device
    outs = []
    for _ in range(2):
        y = torch.full((plan.total, cout), SENTINEL, dtype=odt, device=dev)
        ops.conv_rows_fwd(x, wp, bias, y, plan, k, cin, cout, cout, ksize, flags, mask)
        outs.append(y)
    y = outs[0]
    got = y[torch.from_numpy(ids[ev]).to(dev)].double().cpu()
    assert torch.equal(got, want), f"{what}: {cr.first_diff(got, want)}"
    off = torch.ones(plan.total, dtype=torch.bool, device=dev)
    off[torch.from_numpy(ids).to(dev)] = False
    sent = _bits(torch.full((1,), SENTINEL, dtype=odt, device=dev))
    assert bool((_bits(y)[off] == sent).all()), f"{what}: a row off the list was written"
    assert not bool((_bits(y)[~off] == sent).all(1).any()), f"{what}: a listed row was not written"
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{what}: two runs differ"


def _switches(name, lname):
    """[(knob, value, forward plan)] the case runs under; the first entry is the plan the case is there for."""
    want = cr.ROW_PLANS.get(f"{name}-{lname}", (("ksplit",), ("ksplit",)))[0]
    if want[0] == "tail":
        return [("set_rows_tail_split", 1, want), ("set_rows_tail_split", 0, ("unsliced",))]      # off: two plain rounds of the chip
    if lname == "r30":
        return [("set_rows_big_tile", 1, want), ("set_rows_big_tile", 0, want)]
    return [(None, 0, want)]


def test_head_widths_are_the_models():
    """The 1x1x1 cases run at the packed widths ConeHeadFn uses as rows_total: asked of the model, not guessed."""
    from nerf_rpn_amd.model import RPNHead
    assert {RPNHead(128, a, 1, rotate=r).head_rows for a in (13, 15) for r in (False, True)} == set(cr.HEAD_WIDTHS)


@pytest.mark.parametrize("name,lname", FWD, ids=[f"{m}-{l}" for m, l in FWD])
def test_forward_and_dgrad_equal_fp64(name, lname, dev):
    from nerf_rpn_amd import lib, ops
    m, rl = cr.get(name), cr.row_list(lname)
    dt = _dtype(m)
    plan, k = _list(lname, dev)
    ids, ev, vox = rl.ids, rl.ev, rl.vox()
    listed, reads = rl.listed(), rl.reads(m.k)
    x = _poisoned(m.x, reads, dt, dev)
    wp, wpd = ops.PackedWeight().get([m.w.float().to(dev)], dt, m.cout, True, m.cin)
    bias = m.bias.float().to(dev)
    mask = _poisoned(m.gy, listed, dt, dev)                      # indexed by voxel id; NaN off the list
    acc = m.acc(vox)
    relu = lib.CONV_RELU
    # (epilogue, bias, flags, mask, output types, reference)
    variants = [("plain", None, 0, None, [dt], acc),
                ("bias+relu", bias, relu, None, [dt] + ([F32] if dt == BF else []), cr.epilogue(acc, m.bias, relu=True)),
                ("bias", bias, 0, None, [F32] if dt == BF else [], acc + m.bias),
                ("bias+mask", bias, 0, mask, [dt], cr.epilogue(acc, m.bias, mask=m.gy[vox]))]
    legal_dgrad = (m.cout * (2 if dt == BF else 4)) % 128 == 0
    dplan = cr.ROW_PLANS.get(f"{name}-{lname}", (("ksplit",), ("ksplit",)))[1]
    gy = rl.gy(m)
    dacc = cr.conv_dx(gy, m.w, m.geom, vox) if legal_dgrad else None
    try:
        for knob, val, want in _switches(name, lname):
            if knob:
                lib.call(knob, val)
            got = _fwd_plan(rl.n, m.cin, m.cout, m.k, dt)
            assert got[:len(want)] == want, (name, lname, knob, val, got)
            if lname == "r30":       # the size query does not know the 256x256 form: its conditions (rows_plan) are asserted here
                assert -(-rl.n // 256) * (-(-m.cout // 256)) >= 96 and m.cout >= 256 and dt == BF
            for vn, b, flags, msk, odts, ref in variants:
                for odt in odts:
                    _launch(f"{name} {lname} [{knob}={val}] forward {vn} -> {odt}", ids, ev, cr.store(ref, odt), x, wp, b, plan, k, m.cin, m.cout, m.k,
                            flags, odt, msk)
            if not legal_dgrad:
                continue
            got = _fwd_plan(rl.n, m.cout, m.cin, m.k, dt)
            assert knob == "set_rows_tail_split" and val == 0 or got[:len(dplan)] == dplan, (name, lname, "dgrad", got)
            g = _poisoned(gy, reads, dt, dev)                   # dense gradient; NaN where no tap of the list reads
            for odt in [dt] + ([F32] if dt == BF else []):
                _launch(f"{name} {lname} [{knob}={val}] dgrad -> {odt}", ids, ev, cr.store(dacc, odt), g, wpd, None, plan, k, m.cout, m.cin, m.k, 0, odt)
            saved = _poisoned(m.x, listed, dt, dev)              # the saved activation as the ReLU mask, NaN off the list
            _launch(f"{name} {lname} [{knob}={val}] dgrad with the ReLU mask", ids, ev, cr.store(cr.epilogue(dacc, mask=m.x[vox]), dt), g, wpd, None,
                    plan, k, m.cout, m.cin, m.k, 0, dt, saved)
    finally:
        lib.call("set_rows_big_tile", 0)
        lib.call("set_rows_tail_split", 1)


@pytest.mark.parametrize("name", ["cone_c64_96", "cone_c128_264", "cone_k1_c128_256"])
def test_dgrad_as_the_cone_head_runs_it(name, dev):
    """ConeHeadFn._backward: the gradient is nonzero on S_k only and the input gradient is taken on S_{k+1} with the saved activation as the
    ReLU mask (1x1x1: on S_0 itself).  gy holds NaN on every voxel that no tap of S_{k+1} reads, the mask holds NaN off S_{k+1}.  Cout 96 and
    264 are no legal Cin of the bf16 kernels (row bytes no multiple of 128): those members run as their own dgrad, Cin -> Cin."""
    from nerf_rpn_amd import ops
    m = cr.get(name)
    dt = _dtype(m)
    g = torch.Generator().manual_seed(m.cin)
    w = cr._ints(g, (m.cin, m.cin, m.k, m.k, m.k), -4, 4) if m.cout in (96, 264) else m.w
    cout = w.shape[0]
    gy_all = m.gy if w is m.w else cr._ints(g, (m.geom.m_in, cout), -8, 8)
    _, wpd = ops.PackedWeight().get([w.float().to(dev)], dt, cout, True, m.cin)
    for k in ((0,) if m.k == 1 else (0, 1)):
        src, dst = cr.row_list(f"cone{k}"), cr.row_list(f"cone{k if m.k == 1 else k + 1}")
        plan, kd = _list(dst.name, dev)
        got = _fwd_plan(dst.n, cout, m.cin, m.k, dt)
        assert got[0] == ("unsliced" if m.k == 1 else "ksplit"), got
        gy = torch.zeros_like(gy_all)
        gy[src.ids] = gy_all[src.ids]
        assert (gy[src.ids] != 0).any() and (~dst.reads(m.k)).sum() > 0
        want = cr.epilogue(cr.conv_dx(gy, w, m.geom, dst.ids), mask=m.x[dst.ids])
        _launch(f"{name} dgrad S{k} -> S{kd}", dst.ids, dst.ev, cr.store(want, dt), _poisoned(gy, dst.reads(m.k), dt, dev), wpd, None, plan, kd, cout,
                m.cin, m.k, 0, dt, _poisoned(m.x, dst.listed(), dt, dev))


def _sink(t):
    from nerf_rpn_amd import ops
    return ops.GradSink(t, lambda: None)


@pytest.mark.parametrize("name,lname", WGRAD, ids=[f"{m}-{l}" for m, l in WGRAD])
def test_weight_and_bias_gradient_equal_fp64(name, lname, dev):
    """ops.conv_rows_wgrad (bf16x3 members: conv_rows_wgrad_x3) on one slice (ragged and cone lists), 2 and 4 slices (2100 rows, bf16 and fp32) and
    in the 256x256 form on 5 slices (5200 rows, Cin = Cout = 256).  dy is NaN off the list, x where no tap of the list reads.  A second call
    adds into gradient slots that already hold integers in [-8, 8] (times the family's unit): reference + previous."""
    from nerf_rpn_amd import lib, ops
    m, rl = cr.get(name), cr.row_list(lname)
    dt = _dtype(m)
    plan, k = _list(lname, dev)
    a = (1, rl.n, 1, 1, m.cin, m.cout, m.cout, m.k, lib.BF16 if m.kind in ("i8", "x3") else lib.F32)
    slices, big = lib.query("conv3d_wgrad_slices", *a), lib.query("conv3d_wgrad_plan", *a)
    assert big == (1 if lname == "r18" else 0) and slices >= (5 if lname == "r18" else 2 if lname == "w2100" else 1), (slices, big)
    gy = rl.gy(m)
    x = _poisoned(m.x, rl.reads(m.k), dt, dev)
    w = torch.nn.Parameter(m.w.float().to(dev))
    b = torch.nn.Parameter(m.bias.float().to(dev))
    if m.kind == "x3":
        # the bias gradient of this form is the fp32 column sum of dy over ALL voxels: its contract is dy == 0 off the list
        zero = torch.zeros_like(gy)
        zero[rl.ids] = gy[rl.ids]
        dy = zero.to(dt).to(dev)
        run = ops.conv_rows_wgrad_x3
        dw, lolo = cr.x3_terms(m.x, gy, lambda p, q: cr.conv_dw(p, q, m.geom, rl.ids)[0])
        db = gy[rl.ids].sum(0)
    else:
        dy = _poisoned(gy, rl.listed(), dt, dev)
        run = ops.conv_rows_wgrad
        dw, db = cr.conv_dw(m.x, gy, m.geom, rl.ids)
    first = run(x, dy, [w], [b], m.cout, m.k, plan, k)
    for what, got, want in (("dW", first[0], dw), ("db", first[1], db)):
        got = got.double().cpu()
        assert torch.equal(got, want), f"{name} {lname} {what}: {cr.first_diff(got, want)}"
    again = run(x, dy, [w], [b], m.cout, m.k, plan, k)
    assert torch.equal(_bits(first[0]), _bits(again[0])) and torch.equal(_bits(first[1]), _bits(again[1])), "two runs differ"
    g = torch.Generator().manual_seed(7)
    pw, pb = cr._ints(g, tuple(m.w.shape), -8, 8) * m.unit, cr._ints(g, (m.cout,), -8, 8) * m.unit      # (x3: sums in units of 2^9)
    sw, sb = _sink(pw.float().to(dev)), _sink(pb.float().to(dev))
    res = run(x, dy, [w], [b], m.cout, m.k, plan, k, ([sw], [sb]))
    assert res[0] is None and res[1] is None
    for what, got, want in (("dW", sw.slot, dw + pw), ("db", sb.slot, db + pb)):
        got = got.double().cpu()
        assert torch.equal(got, want), f"{name} {lname} accumulated {what}: {cr.first_diff(got, want)}"
    if m.kind == "x3":      # the dropped lo lo term is not in the result: the host test prints its share
        got = first[0].double().cpu()
        assert (lolo != 0).double().mean().item() > 0.3 and (got != dw + lolo)[lolo != 0].all()
