"""GPU: the conv3d kernels on the exactly summable families of tests/conv_ref.py.  Every product and every partial sum is an fp32 number in any
order and any K split, so each kernel -- whatever its tile, MFMA order, slice count or epilogue staging -- must EQUAL the float64 reference:
fp32 outputs bit for bit, bf16 outputs its single round-to-nearest-even rounding.  Every test asserts through the plan queries that its
shape runs the kernel it names.

Plans measured from the library (they differ from a reading of the plan functions in three places): the (2, (7,6,5)) and (1, (9,8,7)) grids are
too small for an unsliced launch -- conv_ksplit takes every 3x3x3 shape below 128 tiles, whatever tile is forced -- so the unsliced 128-row
kernels run on (2, (24,20,17)) (16320 rows = 127 tiles + 64 rows), the 256-row kernels on (1, (24,20,17)) (8160 rows = 31 tiles + 224) and,
for the partial column tile, on (1, (20,17,16)) (5440 rows; Cout 264 on 8160 rows would enter the conv_big_split window); the small grids
stay as K-sliced cases.  The bf16 weight gradient needs >= 2048 rows for two slices: (2, (12,10,9)) = 2160 rows, and the Cin = 128 pair form of the
256x256 weight-gradient kernel is selected from 10240 rows on: (1, (24,22,20))."""
import pytest
import torch
from torch import nn

import conv_ref as cr

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


def _eq(got, want, what):
    got = got.detach().double().cpu().reshape(want.shape)
    assert torch.equal(got, want), f"{what}: {cr.first_diff(got, want)}"


def _x5(m, t2d, dev, dtype, out=False):
    if m.ragged:
        return t2d.to(dtype).view(1, -1, 1, 1, t2d.shape[1]).to(dev)
    return m.nchw(t2d, out=out).to(dtype).contiguous().to(dev)


def _code(dtype):
    from nerf_rpn_amd import lib
    return lib.BF16 if dtype == BF else lib.F32


def _plan(m, dtype, tile, pairing, swap=False):
    """(plan, workspace bytes, statistics rows) of the forward (swap: the dgrad, Cout -> Cin) launch of member m."""
    from nerf_rpn_amd import lib
    o = lib.ConvOpts(tile=tile, halo_pairing=pairing)
    ci, co = (m.cout, m.cin) if swap else (m.cin, m.cout)
    a = (m.n, *m.grid, ci, co, m.k, _code(dtype), o.ptr())
    return (lib.query("conv3d_fwd_plan_ex", *a), lib.query("conv3d_fwd_workspace_bytes_ex", *a), lib.query("conv3d_fwd_stats_rows_ex", *a))


T128, TWS, T256, TW4, THALO = 128, 256, 512, 1024, 2048       # lib.TILE_*
# (member, dtype, tile, halo pairing, forward plan, dgrad plan or None where Cout is no legal Cin, K-sliced forward)
FWD = [
    ("gG2_c32_64", BF, T128, 0, 0, 0, False),          # 128-row tile, 64-byte K-step (Cin 32), 64-column tile; dgrad: 128-byte K-step
    ("gG2_c64_96", BF, T128, 0, 0, 0, False),          # 128-row tile, 128-byte K-step, partial 128-column tile
    ("gG2_f32_c16_32", F32, T128, 0, 0, 0, False),     # fp32, 64-byte K-step
    ("gG2_f32_c32_64", F32, T128, 0, 0, 0, False),     # fp32, 128-byte K-step
    ("g765_c32_64", BF, T128, 0, 3, 3, True),          # 420 rows = 3 tiles + 36: 128-row tile on K slices
    ("g765_c64_96", BF, T128, 0, 3, 3, True),
    ("g765_f32_c16_32", F32, T128, 0, 3, 3, True),
    ("g765_f32_c32_64", F32, T128, 0, 3, 3, True),
    ("g555_c128_256", BF, T128, 0, 3, 3, True),        # 5^3 pyramid level: conv_ksplit
    ("g987_c64_256", BF, T256, 0, 3, 3, True),         # 504 rows: too few tiles for the 256-row kernels, K-sliced 128-row tile instead
    ("g987_c64_264", BF, TW4, 0, 3, None, True),       # the same with a partial column tile
    ("gG1_c64_256", BF, T256, 0, 1, 3, False),         # 256x256, 8 waves: 31 tiles + 224 rows
    ("gG1_c64_256", BF, TW4, 0, 5, 3, False),          # 256x256, 4 waves
    ("gG1_c64_256", BF, TWS, 0, 4, 3, False),          # wave-specialised 256x128
    ("gG1_c256_256", BF, T256, 0, 1, 1, False),        # dgrad on the 256x256 tile as well
    ("gG1_c256_256", BF, TW4, 0, 5, 5, False),
    ("gH1_c64_264", BF, T256, 0, 1, None, False),      # partial 256-column tile
    ("gH1_c64_264", BF, TW4, 0, 5, None, False),
    ("g59a_c96_256", BF, THALO, 0, 7, 3, False),       # halo form, partial 4x8x8 blocks in every axis, two scenes
    ("g59a_c256_256", BF, THALO, 0, 7, 7, False),      # dgrad in the halo form as well (Cin 256: default pairing = across chunks)
    ("g59a_c128_264", BF, THALO, 1, 7, None, False),   # taps paired across chunk boundaries
    ("g59a_c128_264", BF, THALO, 2, 7, None, False),
    ("gk20_c128_512", BF, T256, 0, 2, 3, True),        # 50 tiles of 256x256 on K slices (conv_big_split)
    ("gk20_c128_512", BF, TW4, 0, 6, 3, True),
    ("g443_k1_c128_256", BF, 0, 0, 0, 0, False),       # 1x1x1
    ("g443_k1_c32_64", BF, 0, 0, 0, 0, False),
]


_SUMS = {}


def _sums(m):
    """(forward accumulator, dgrad accumulator) of member m, computed once and shared by the cases that force different tiles on it."""
    if m.name not in _SUMS:
        _SUMS[m.name] = (m.acc(), cr.conv_dx(m.gy, m.w, m.geom))
    return _SUMS[m.name]


def _variants(m, dtype, out_dtype, plan):
    """(name, kwargs of _conv_fwd, kwargs of cr.epilogue) of every epilogue the kernel of ``plan`` takes with this output type."""
    v = [("plain", dict(bias=None, flags=0), dict()),
         ("bias+relu", dict(bias=m.bias, flags=2), dict(bias=m.bias, relu=True)),
         ("scale+shift+relu", dict(bias=m.shift, flags=2, scale=m.scale), dict(bias=m.shift, scale=m.scale, relu=True))]
    if out_dtype == dtype:                        # the ReLU mask needs outputs in the input type
        v.append(("bias+mask", dict(bias=m.bias, flags=0, mask=m.gy), dict(bias=m.bias, mask=m.gy)))
    return v


@pytest.mark.parametrize("name,dtype,tile,pairing,pf,pd,sliced", FWD, ids=[f"{c[0]}-{'bf16' if c[1] == BF else 'f32'}-t{c[2]}p{c[3]}" for c in FWD])
def test_forward_and_dgrad_equal_fp64(name, dtype, tile, pairing, pf, pd, sliced, dev):
    from nerf_rpn_amd import ops
    m = cr.get(name)
    plan, wsb, _ = _plan(m, dtype, tile, pairing)
    assert plan == pf and (wsb > 0) == sliced, (plan, wsb)
    x = _x5(m, m.x, dev, dtype)
    wp, wpd = ops.PackedWeight().get([m.w.float().to(dev)], dtype, m.cout, True)
    acc = _sums(m)[0]
    f = lambda t: None if t is None else t.float().to(dev)
    for out_dtype in ([dtype] if dtype == F32 else [BF, F32]):
        for vn, kw, ep in _variants(m, dtype, out_dtype, plan):
            mask = _x5(m, kw["mask"], dev, dtype, out=True) if "mask" in kw else None
            y = ops._conv_fwd(x, wp, f(kw["bias"]), m.cout, m.cout, m.k, kw["flags"], out_dtype, mask=mask, scale=f(kw.get("scale")), tile=tile,
                              halo_pairing=pairing)
            assert y.dtype == out_dtype
            _eq(y, cr.store(cr.epilogue(acc, **ep), out_dtype), f"{name} forward {vn} -> {out_dtype}")
    if pd is None:
        return
    assert _plan(m, dtype, tile, pairing, swap=True)[0] == pd
    gy = _x5(m, m.gy, dev, dtype, out=True)
    dacc = _sums(m)[1]
    for out_dtype in ([dtype] if dtype == F32 else [BF, F32]):
        dx = ops._conv_fwd(gy, wpd, None, m.cin, m.cin, m.k, 0, out_dtype, tile=tile, halo_pairing=pairing)
        _eq(dx, cr.store(dacc, out_dtype), f"{name} dgrad -> {out_dtype}")
    dx = ops._conv_fwd(gy, wpd, None, m.cin, m.cin, m.k, 0, dtype, mask=x, tile=tile, halo_pairing=pairing)      # dx = 0 where the saved activation <= 0
    _eq(dx, cr.store(cr.epilogue(dacc, mask=m.x), dtype), f"{name} dgrad with the ReLU mask")


def test_tail_split_rows_equal_fp64(dev):
    """323 tiles of 256 rows = one round of the chip + 67: the last 67 M tiles run on 3 K slices (conv_tail_split).  The reference is evaluated
    on every row from tile0 * 256 on and on 512 seeded rows of the first round."""
    from nerf_rpn_amd import ops
    m = cr.get("gtail_c64_256")
    plan, wsb, _ = _plan(m, BF, 0, 0)
    M = m.geom.m_out
    tile0 = 256
    assert plan == 1 and wsb == 3 * (M - tile0 * 256) * m.cout * 4, (plan, wsb)          # the split is active: 3 slices of the tail rows
    g = torch.Generator().manual_seed(5)
    rows = torch.cat([torch.randperm(tile0 * 256, generator=g)[:512].sort().values, torch.arange(tile0 * 256, M)]).numpy()
    acc = m.acc(rows)
    x = _x5(m, m.x, dev, BF)
    wp, _ = ops.PackedWeight().get([m.w.float().to(dev)], BF, m.cout, False)
    for vn, kw, ep in _variants(m, BF, BF, plan):
        mask = _x5(m, kw["mask"], dev, BF, out=True) if "mask" in kw else None
        if "mask" in ep:
            ep = dict(ep, mask=m.gy[rows])
        y = ops._conv_fwd(x, wp, None if kw["bias"] is None else kw["bias"].float().to(dev), m.cout, m.cout, 3, kw["flags"], BF, mask=mask,
                          scale=kw["scale"].float().to(dev) if "scale" in kw else None)
        _eq(y.reshape(-1, m.cout)[torch.from_numpy(rows).to(dev)], cr.store(cr.epilogue(acc, **ep), BF), f"tail split forward {vn}")


# (member, tile, pairing, plan, rows per statistics partial; "halo": two partials per 4 x 8 x 8 block, one per pair of x-planes)
STATS = [("st_gG2_c64_96", T128, 0, 0, 64), ("st_gG1_c64_256", T256, 0, 1, 128), ("st_gG1_c64_256", TW4, 0, 5, 128),
         ("st_g59a_c96_256", THALO, 0, 7, "halo"), ("st_g59a_c128_264", THALO, 1, 7, "halo"), ("st_g59a_c128_264", THALO, 2, 7, "halo")]


@pytest.mark.parametrize("name,tile,pairing,pf,group", STATS, ids=[f"{c[0]}-t{c[1]}p{c[2]}" for c in STATS])
def test_fused_statistics_equal_the_sums_of_the_stored_outputs(name, tile, pairing, pf, group, dev):
    from nerf_rpn_amd import ops
    m = cr.get(name)
    plan, _, rows = _plan(m, BF, tile, pairing)
    assert plan == pf and rows > 0
    x = _x5(m, m.x, dev, BF)
    wp, _ = ops.PackedWeight().get([m.w.float().to(dev)], BF, m.cout, False)
    st = {}
    y = ops._conv_fwd(x, wp, m.bias.float().to(dev), m.cout, m.cout, 3, 0, BF, stats=st, tile=tile, halo_pairing=pairing)
    want = cr.store(m.pre(), BF)
    _eq(y, want, f"{name} forward with statistics")
    part = st["partials"].double().cpu()
    assert tuple(part.shape) == (rows, 2, m.cout)
    assert torch.equal(part[:, 0].sum(0), want.sum(0)), cr.first_diff(part[:, 0].sum(0), want.sum(0))
    assert torch.equal(part[:, 1].sum(0), (want * want).sum(0)), cr.first_diff(part[:, 1].sum(0), (want * want).sum(0))
    if group == "halo":         # conv_halo.hip: partial row = block * 2 + wave row; voxels outside the grid count as 0
        ref = cr.halo_partials(want, m.n, m.grid)
    else:                       # partial p = `group` consecutive rows (conv3d.hip: store_col_stats row index = tile * groups per tile + wave row)
        ref = cr.stats_partials(want, group, rows)
    assert torch.equal(part, ref), cr.first_diff(part, ref)


def _module(m, dev, requires_grad=True):
    conv = nn.Conv3d(m.cin, m.cout, m.k, stride=m.stride, padding=m.k // 2).to(dev)
    with torch.no_grad():
        conv.weight.copy_(m.w.float())
        conv.bias.copy_(m.bias.float())
    return conv.requires_grad_(requires_grad)


def _backward(m, dev, dtype, relu, x3=False, segs=None):
    """conv(+ReLU) and its whole backward through hip_nn.conv3d -> the same dict as Member.reference."""
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model import hip_nn
    conv = _module(m, dev)
    x = _x5(m, m.x, dev, dtype).requires_grad_(m.k != 7)
    ops.SPLIT3[0] = x3
    try:
        y = hip_nn.conv3d(conv, x, relu=relu, segs=segs)
        y.backward(_x5(m, m.gy, dev, dtype, out=True))
        torch.cuda.synchronize()
    finally:
        ops.SPLIT3[0] = False
    return dict(y=y.detach(), dx=x.grad, dw=conv.weight.grad, db=conv.bias.grad)


def _check(got, ref, what):
    for k in ("y", "dx", "dw", "db"):
        if ref.get(k) is not None and got.get(k) is not None:
            _eq(got[k], ref[k], f"{what} {k}")


# (member, dtype, wgrad plan); every case is asserted to run on at least 2 voxel slices
WGRAD = [("gw2_c32_64", BF, 0), ("gw2_c64_128", BF, 0), ("gw2_f32_c32_64", F32, 0), ("gw_c256_512", BF, 1), ("gw_c128_256", BF, 1), ("gw2_k1_c64_96", BF, 0)]


@pytest.mark.parametrize("name,dtype,pw", WGRAD, ids=[c[0] for c in WGRAD])
def test_weight_and_bias_gradient_equal_fp64(name, dtype, pw, dev):
    """128x128 kernel (fp32, bf16 in both fetch modes, two taps per workgroup on and off), 256x256 kernel (Cin >= 256 and the Cin = 128 pair
    form), ksize 1; always >= 2 voxel slices, so the slice sum and the bias partials are on the path."""
    from nerf_rpn_amd import lib
    m = cr.get(name)
    a = (m.n, *m.grid, m.cin, m.cout, m.cout, m.k, _code(dtype))
    assert lib.query("conv3d_wgrad_plan", *a) == pw and lib.query("conv3d_wgrad_slices", *a) >= 2
    ref = m.reference(True, dtype)
    switches = [("set_wgrad_pack2", 1)]
    if pw == 0 and m.k == 3:
        switches.append(("set_wgrad_pack2", 0))
        if dtype == BF:
            switches.append(("set_wgrad_transpose_read", 0))
    for knob, val in switches:
        lib.call(knob, val)
        try:
            _check(_backward(m, dev, dtype, True), ref, f"{name} [{knob}={val}]")
        finally:
            lib.call(knob, 1)


@pytest.mark.parametrize("name,tile,plan", [("gG1_c256_256", T256, 1), ("gG1_c256_256", TW4, 5), ("g59a_c256_256", THALO, 7)])
def test_autograd_path_with_a_forced_tile(name, tile, plan, dev):
    """conv + ReLU and its whole backward through hip_nn.conv3d with ops.CONV_TILE forcing the tile of the forward AND of the dgrad inside
    autograd (ReLU backward, dgrad, wgrad, bias gradient chained as in training)."""
    from nerf_rpn_amd import ops
    m = cr.get(name)
    assert _plan(m, BF, tile, 0)[0] == plan and _plan(m, BF, tile, 0, swap=True)[0] == plan
    old = ops.CONV_TILE[0]
    ops.CONV_TILE[0] = tile
    try:
        got = _backward(m, dev, BF, True)
    finally:
        ops.CONV_TILE[0] = old
    _check(got, m.reference(True, BF), f"{name} tile {tile}")


@pytest.mark.parametrize("name,dtype", [("rag_c64_128", BF), ("rag_f32_c64_128", F32)])
def test_ragged_list_equals_the_ragged_reference(name, dtype, dev):
    """Grids [(6,5,4), (3,3,2), (9,2,1), (1,1,1)] x 2 scenes laid end to end: forward, dgrad, wgrad and bias gradient in ONE launch each, against
    the reference's own ragged evaluation (segment boundaries and the batch boundary are zero padding)."""
    m = cr.get(name)
    _check(_backward(m, dev, dtype, True, segs=m.geom.segs), m.reference(True, dtype), name)


STEM = [("stem_s1_9_8_7", BF, 0), ("stem_s2_16_14_13", BF, 0), ("stem_s2_18_15_12", BF, 1), ("stem_s2_34_26_20", BF, 1),
        ("stem_f32_s1_9_8_7", F32, 0), ("stem_f32_s2_16_14_13", F32, 0), ("stem_f32_s2_18_15_12", F32, 0)]


@pytest.mark.parametrize("name,dtype,halo", STEM, ids=[c[0] for c in STEM])
def test_stem_equals_fp64(name, dtype, halo, dev):
    """7x7x7, Cin 4 -> 64, two scenes: forward, weight gradient (even Z at stride 2: the z-row kernel), bias gradient, and the folded
    scale / shift (+ ReLU) forward; bf16 with an even Z runs the halo forward, and the im2col form with ops.STEM_HALO off."""
    from nerf_rpn_amd import lib, ops
    from nerf_rpn_amd.model import hip_nn
    m = cr.get(name)
    assert lib.query("stem_halo_supported", m.grid[2], 64, m.stride, _code(dtype)) == halo
    ref = m.reference(False, dtype)
    fold = cr.store(cr.epilogue(m.acc(), m.shift, m.scale, relu=True), dtype)
    for halo_on in ([True, False] if halo else [True]):
        ops.STEM_HALO[0] = halo_on
        try:
            _check(_backward(m, dev, dtype, False), ref, f"{name} [halo={halo_on}]")
            with torch.no_grad():
                y = hip_nn.conv3d(_module(m, dev), _x5(m, m.x, dev, dtype), relu=True, affine=(m.scale.float().to(dev), m.shift.float().to(dev)))
            _eq(y, fold, f"{name} folded scale/shift [halo={halo_on}]")
        finally:
            ops.STEM_HALO[0] = True


@pytest.mark.parametrize("name", ["x3_g555_c128_256", "x3_g765_c64_96"])
def test_bf16x3_mode_equals_the_split_evaluation(name, dev):
    """fp32 operands of 10-11 significant bits (512 h + l).  With ops.SPLIT3 raised, y, dx, dw, db equal sum(hi hi + hi lo + lo hi) and
    therefore differ from the full product wherever the dropped lo lo term is not zero."""
    m = cr.get(name)
    ref = m.reference(True, F32, x3=True)
    got = _backward(m, dev, F32, True, x3=True)
    _check(got, ref, f"{name} bf16x3")
    for k, lolo in (("dx", ref["dx_lolo"]), ("dw", ref["dw_lolo"])):
        g = got[k].double().cpu().reshape(lolo.shape)
        assert (lolo != 0).double().mean().item() > 0.3 and (g != ref[k] + lolo)[lolo != 0].all(), k
    pre_full = ref["pre"] + ref["y_lolo"]
    sel = (ref["y_lolo"] != 0) & (ref["pre"] > 0) & (pre_full > 0)
    assert sel.double().mean().item() > 0.2 and (got["y"].double().cpu().reshape(pre_full.shape) != pre_full)[sel].all()


@pytest.mark.parametrize("rows,c", [(524291, 64), (4099, 64), (1001, 96)])
def test_bf16x3_bias_column_sum_equals_fp64(rows, c, dev):
    """The bias gradient of the bf16x3 mode = ops.column_sum_f32 of dy: the slab pass with its fp64 finish (>= 2^25 elements), the column-sum
    kernel below that and for widths the slab pass does not take (96).  Integers in [-8, 8]: sum|a| <= 8 rows < 2^24."""
    from nerf_rpn_amd import ops
    t = torch.randint(-8, 9, (rows, c), generator=torch.Generator().manual_seed(rows), dtype=torch.int32).float()
    want = t.double().sum(0)
    got = ops.column_sum_f32(t.to(dev))
    _eq(got, want, f"column sum {rows} x {c}")
    acc = torch.ones(c, device=dev)
    _eq(ops.column_sum_f32(t.to(dev), out=acc, accumulate=True), want + 1, f"column sum {rows} x {c}, accumulated")


@pytest.mark.parametrize("name", ["g765_f32_c32_64"])
def test_bf16x3_mode_off_is_the_plain_fp32_evaluation(name, dev):
    """The same entry points with the mode off run the fp32 kernels: equal to the full float64 product (f32 family: operands beyond 2^8, so a
    path that split or rounded them would not be)."""
    m = cr.get(name)
    _check(_backward(m, dev, F32, True, x3=False), m.reference(True, F32), name)


def test_ragged_bf16x3_follows_grad_mode(dev):
    """Under torch.no_grad() with ops.SPLIT3 raised, a ragged conv whose weights require gradients runs the split operands: its output equals
    the split evaluation and therefore differs from the fp32 one (the decision used to be taken from ctx.needs_input_grad, which mirrors
    requires_grad even under no_grad: every eval-mode ragged conv silently ran the fp32 kernels).  With gradients required, the launch has to
    stay on the fp32 kernels -- the split dgrad / wgrad know no segments: output and all gradients equal the fp32 evaluation."""
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model import hip_nn
    m = cr.get("rag_x3_c64_128")
    ref = m.reference(True, F32, x3=True)
    conv = _module(m, dev)                         # trainable weights, as in a model switched to eval()
    assert conv.weight.requires_grad
    ops.SPLIT3[0] = True
    try:
        with torch.no_grad():
            y = hip_nn.conv3d(conv, _x5(m, m.x, dev, F32), relu=True, segs=m.geom.segs)
        f = cr.get("rag_f32_c64_128")
        got = _backward(f, dev, F32, True, x3=True, segs=f.geom.segs)
    finally:
        ops.SPLIT3[0] = False
    _eq(y, ref["y"], "ragged bf16x3 forward under no_grad")
    full = (ref["pre"] + ref["y_lolo"]).clamp_min(0)
    sel = (ref["y_lolo"] != 0) & (ref["pre"] > 0) & (full > 0)
    assert sel.double().mean().item() > 0.2 and (y.double().cpu().reshape(full.shape) != full)[sel].all()
    _check(got, f.reference(True, F32), "differentiated ragged conv under SPLIT3 (fp32 kernels)")
