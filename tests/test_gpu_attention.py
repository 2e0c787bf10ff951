"""GPU: the shifted-window attention kernels of csrc/swin.hip (fp32 VALU, bf16 VALU, bf16 MFMA; forward, backward, the table and
padded-token reductions) called directly through ops.WindowAttnFn - no Linears around them - against the float64 reference of
tests/attention_ref.py, every element of every output (out, dqkv, dtable, dbias_pad) inside its own derived bound; nothing is normalised by
a tensor maximum.  The bounds and their derivation are in attention_ref's docstring; tests/test_attention_bounds_host.py shows on the CPU
that they are satisfiable (an emulation of the MFMA rounding points passes) and sharp (a transposed relative-position bias fails by 4x to
1e6x).  The reference runs on the values the kernel read: bf16 cases use bf16-representable qkv, dout AND qkv bias (the MFMA kernels stage
padded tokens as bf16, the VALU kernels keep the fp32 bias; on a representable bias both read the same numbers).

The allowance k of the fp32 term is measured per case and output on torch's fp32 CPU evaluation, never on the kernel (k = max(1, min(2,
4 r_torch))).  r_torch as measured on the CPU (host module, and this module's cases): normal 0.02-0.12, peaked 0.2-0.5 (Lambda up to 137),
offset_v up to 0.93 (dq, where dP - rowdot cancels), selector 0.02-0.14.  Every check prints its max |err| / bound (run with -s).

Also here: the small Swin pieces (GeluFn, ScaleAddFn, PatchMergeFn, ops.patchify) against float64 / exact gathers in fp32 and bf16, at a
small odd shape and beyond one grid stride of their loops (8192 blocks x 256 lanes x 4 elements = 8.4 M)."""
import pytest
import torch
import torch.nn.functional as F

import attention_ref as AR

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
INDEX = AR.relative_position_index()


# ======================================================================================================================
# running one kernel family
# ======================================================================================================================
def _run(kernel, qkv, bias, table, dout, heads, shift, dev, index=None):
    """ops.WindowAttnFn forward + backward on one kernel family -> (out, dqkv, dtable, dbias_pad or None), all on the device."""
    from nerf_rpn_amd import lib, ops
    dtype = F32 if kernel == "f32" else BF16
    idx = (INDEX if index is None else index).to(torch.int32).to(dev)
    lib.call("set_window_attn_mfma", 0 if kernel == "bf16_valu" else 1)
    try:
        q = qkv.to(dev).to(dtype).requires_grad_()
        t = table.to(dev).requires_grad_()
        b = bias.to(dev).requires_grad_() if bias is not None else None
        out = ops.WindowAttnFn.apply(q, b, t, idx, heads, shift > 0)
        assert out.dtype == dtype
        grads = torch.autograd.grad(out, [q, t] + ([b] if b is not None else []), dout.to(dev).to(dtype), allow_unused=True)
        torch.cuda.synchronize()
    finally:
        lib.call("set_window_attn_mfma", 1)
    return out.detach(), grads[0], grads[1], (grads[2] if b is not None else None)


def _reference(family, shape, heads, shift, seed, with_bias, bf16):
    """Inputs of a case, their fp64 reference and the allowance k per output (from torch's fp32 CPU evaluation of the same inputs)."""
    qkv, bias, table, dout = AR.make_case(family, shape, heads, seed, with_bias=with_bias, bf16=bf16)
    ref = AR.attn_core_ref(qkv.double(), None if bias is None else bias.double(), table.double(), INDEX, heads, shift, dout=dout.double())
    r32 = AR.torch32_ratios(ref, AR.attn_core_explicit(qkv, bias, table, INDEX, heads, shift, dout))
    return (qkv, bias, table, dout), ref, {n: AR.allowance(v) for n, v in r32.items()}, r32


def _check_outputs(ref, ks, kernel, got, what):
    out, dqkv, dtable, dpad = got
    c = out.shape[-1]
    AR.check(ref, "out", kernel, out, ks["out"], what)
    AR.check(ref, "dqkv", kernel, dqkv, ks["dqkv"], what)
    AR.check(ref, "dtable", kernel, dtable, ks["dtable"], what)
    if ref.dbias_pad is None:
        assert dpad is None
    elif not any(ref.frame.pad):              # no padded token: the kernels hand back no bias gradient at all, the reference's is zero
        assert dpad is None and not ref.dbias_pad.any()
    else:
        assert dpad is not None and dpad.shape == (3 * c,)
        assert torch.equal(dpad[:c], torch.zeros_like(dpad[:c])), "the q third of dbias_pad must be exactly zero"
        AR.check(ref, "dbias_pad", kernel, dpad, ks["dbias_pad"], what)


def _case(family, shape, heads, shift, kernels, dev, seed, biases=(False, True)):
    for with_bias in biases:
        for bf16 in (False, True):
            todo = [k for k in kernels if (k != "f32") == bf16]
            if not todo:
                continue
            inputs, ref, ks, r32 = _reference(family, shape, heads, shift, seed, with_bias, bf16)
            what = f"{family} {shape} heads={heads} shift={shift} bias={with_bias}"
            print(what, "bf16" if bf16 else "fp32", "values: torch fp32 / T32", {n: round(v, 3) for n, v in r32.items()})
            for kernel in todo:
                _check_outputs(ref, ks, kernel, _run(kernel, *inputs, heads, shift, dev), what)


# ======================================================================================================================
# geometries
# ======================================================================================================================
# every axis situation, mixed per axis: shorter than a window / exactly one window (never shifted) / several windows; n = 1, 2, 3
AXIS_GEOMS = [(1, 1, 1, 1, 3), (2, 3, 2, 2, 24), (1, 4, 4, 4, 3), (1, 8, 4, 4, 6), (1, 4, 9, 3, 12), (2, 5, 4, 3, 12), (1, 10, 7, 6, 6),
              (3, 13, 6, 5, 3)]
# window counts around the steps of attn_table_reduce_kernel / attn_pad_reduce_kernel (16 window lanes, a four-way unrolled trip of 64
# windows entered at >= 49, twice at >= 113): (n, X, Y, Z, heads, windows)
COUNT_GEOMS = [(1, 12, 19, 3, 3, 15), (2, 8, 7, 8, 3, 16), (1, 67, 4, 4, 3, 17), (3, 16, 8, 7, 3, 48), (1, 28, 27, 4, 6, 49),
               (1, 16, 16, 16, 3, 64), (1, 20, 49, 4, 3, 65), (1, 450, 4, 3, 3, 113), (2, 20, 52, 3, 3, 130)]
# Swin stages of the 160^3 scene and one stage of the benchmark scene (padded 52 x 52 x 36, 1521 windows); the two largest run one kernel
# path each (the fp64 reference of 1000+ windows is what costs the time, not the kernels)
STAGE_GEOMS = [((1, 40, 40, 40, 3), ("bf16_mfma",)), ((1, 20, 20, 20, 6), AR.KERNELS), ((1, 10, 10, 10, 12), AR.KERNELS),
               ((1, 5, 5, 5, 24), AR.KERNELS), ((1, 50, 50, 33, 3), ("f32",))]


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("geom", AXIS_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_attention_axis_situations(geom, shift, dev):
    *shape, heads = geom
    _case("normal", tuple(shape), heads, shift, AR.KERNELS, dev, seed=100 + sum(geom) + shift)


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("geom", COUNT_GEOMS, ids=lambda g: f"{g[5]}windows")
def test_attention_window_counts(geom, shift, dev):
    *shape, heads, windows = geom
    assert AR.Frame(tuple(shape), shift).windows == windows
    _case("normal", tuple(shape), heads, shift, AR.KERNELS, dev, seed=200 + windows + shift)


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("geom,kernels", STAGE_GEOMS, ids=lambda g: "x".join(map(str, g)) if isinstance(g[0], int) else None)
def test_attention_stage_shapes(geom, kernels, shift, dev):
    *shape, heads = geom
    _case("normal", tuple(shape), heads, shift, kernels, dev, seed=300 + sum(geom) + shift)


# every family on a padded + shifted grid (24 windows, n = 2) and on an unpadded one
FAMILY_GEOMS = [((2, 10, 7, 6), 6, 2), ((2, 8, 8, 8), 3, 0), ((2, 8, 8, 8), 3, 2)]


@pytest.mark.parametrize("shape,heads,shift", FAMILY_GEOMS)
@pytest.mark.parametrize("family", AR.FAMILIES)
def test_attention_input_families(family, shape, heads, shift, dev):
    _case(family, shape, heads, shift, AR.KERNELS, dev, seed=400 + AR.FAMILIES.index(family), biases=(True,))


@pytest.mark.parametrize("shape,shift", [((2, 8, 8, 8), 0), ((2, 8, 8, 8), 2), ((1, 8, 4, 4), 2), ((2, 5, 4, 3), 2), ((1, 10, 7, 6), 0)])
@pytest.mark.parametrize("kernel", AR.KERNELS)
def test_uniform_family_closed_form(kernel, shape, shift, dev):
    """q = 0 and a zero table: every output token carries the mean of (x, y, z, 1, b) over its window-and-region set (the mean coordinate
    of its window where nothing is shifted or padded), computed by index arithmetic without the reference.  The sets have 8 .. 64 members
    (powers of two) and the values are small integers, so every kernel's fp32 arithmetic is exact; bf16 stores round that exact value."""
    heads = 3
    qkv, _, table, dout = AR.make_case("uniform", shape, heads, 13, with_bias=False, bf16=kernel != "f32")
    out = _run(kernel, qkv, None, table, dout, heads, shift, dev)[0].float().cpu()
    want = AR.uniform_closed_form(shape, shift).float()
    if kernel != "f32":
        want = AR.bf16_round(want)
    for h in range(heads):
        got = out[..., h * AR.HD:h * AR.HD + 5]
        assert torch.equal(got, want), (h, (got - want).abs().max().item())


# ======================================================================================================================
# further properties
# ======================================================================================================================
@pytest.mark.parametrize("kernel", AR.KERNELS)
def test_attention_two_runs_bit_identical(kernel, dev):
    """Padded + shifted, 130 windows (two unrolled trips of the table reduction), n = 2: out, dqkv, dtable, dbias_pad are the same bits
    run to run (per-unit partials summed in a fixed order; no floating-point atomics across workgroups)."""
    shape, heads, shift = (2, 20, 52, 3), 3, 2
    inputs = AR.make_case("normal", shape, heads, 77, with_bias=True, bf16=kernel != "f32")
    a = _run(kernel, *inputs, heads, shift, dev)
    b = _run(kernel, *inputs, heads, shift, dev)
    assert a[3] is not None
    for name, x, y in zip(AR.NAMES, a, b):
        assert torch.equal(x, y), (name, (x.float() - y.float()).abs().max().item())


@pytest.mark.parametrize("kernel", ["f32", "bf16_mfma"])
@pytest.mark.parametrize("shape", [(2, 8, 8, 8), (2, 10, 7, 6)], ids=["unpadded", "padded"])
def test_attention_gradients_through_arena_slots(shape, kernel, dev):
    """dtable (and, on a padded grid, dbias_pad) delivered into prefilled GradSink slots - contiguous (the table reduction adds in place
    where there is no padding) and strided - equal prefill + the gradients the same call hands back without slots, bit for bit, and
    prefill + the fp64 gradient within the sum bound of test_gpu_norms."""
    from nerf_rpn_amd import ops
    from test_gpu_norms import _check_slots, _prefills, _sinks
    heads, shift = 3, 2
    bf16 = kernel != "f32"
    qkv, bias, table, dout = AR.make_case("normal", shape, heads, 55, with_bias=True, bf16=bf16)
    ref = AR.attn_core_ref(qkv.double(), bias.double(), table.double(), INDEX, heads, shift, dout=dout.double())
    _, _, dtable, dpad = _run(kernel, qkv, bias, table, dout, heads, shift, dev)
    padded = any(ref.frame.pad)
    assert (dpad is not None) == padded
    dtype = BF16 if bf16 else F32
    tp, bp = table.to(dev).requires_grad_(), bias.to(dev).requires_grad_()
    pre = _prefills([(343, heads), (3 * heads * AR.HD,)], 57, dev)
    for direct in (True, False):
        slots = _sinks([tp, bp], pre, direct)
        try:
            q = qkv.to(dev).to(dtype).requires_grad_()
            out = ops.WindowAttnFn.apply(q, bp, tp, INDEX.to(torch.int32).to(dev), heads, True)
            out.backward(dout.to(dev).to(dtype))
            ops.wgrad_stream_join()
            torch.cuda.synchronize()
        finally:
            del tp._nrpn_sink, bp._nrpn_sink
        assert tp.grad is None and bp.grad is None
        assert torch.equal(slots[0], pre[0] + dtable), ("table slot", direct)
        assert torch.equal(slots[1], pre[1].reshape(-1) + dpad if padded else pre[1].reshape(-1)), ("bias slot", direct)
        _check_slots(slots[:1], pre[:1], [ref.dtable], [ref.terms["dtable"]], f"attention table direct={direct}")


def test_index_guard_rejects_permuted_relative_position_index(dev):
    """The MFMA kernels compute the relative-position index arithmetically and ignore the tensor: a module whose buffer differs from the
    reference's 4x4x4 formula must be refused before any kernel runs."""
    from nerf_rpn_amd.model.feature_extractor import ShiftedWindowAttention
    att = ShiftedWindowAttention(96, [4, 4, 4], [0, 0, 0], 3)
    assert torch.equal(att.relative_position_index, INDEX)
    good = att.to(dev)._index32()
    assert good.dtype == torch.int32 and torch.equal(good.cpu().long(), INDEX)
    bad = ShiftedWindowAttention(96, [4, 4, 4], [0, 0, 0], 3)
    bad.relative_position_index.copy_(INDEX.view(64, 64).t().reshape(-1))      # the transposed convention
    with pytest.raises(NotImplementedError):
        bad.to(dev)._index32()
    with pytest.raises(NotImplementedError):
        bad(torch.randn(1, 4, 4, 4, 96, device=dev))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_channel_count_guard(dtype, dev):
    """C != heads * 32 is an error from the library, not a launch."""
    from nerf_rpn_amd import lib, ops
    qkv = torch.randn(1, 4, 4, 4, 3 * 64, device=dev).to(dtype)
    table = torch.zeros(343, 3, device=dev)
    with pytest.raises(lib.NrpnError, match="must equal heads"):
        ops.WindowAttnFn.apply(qkv, None, table, INDEX.to(torch.int32).to(dev), 3, False)
    torch.cuda.synchronize()


# ======================================================================================================================
# the small pieces: GELU, residual join, patch merging, patch embedding gather
# ======================================================================================================================
EPS32 = 2.0 ** -24
SMALL, BIG = (3, 5, 7, 12), (1, 24, 24, 40, 384)          # 1260 elements; 8.85 M > one grid stride (8192 x 256 x 4 = 8.39 M)


def _ulp_bf16(ref):
    _, e = torch.frexp(ref)
    return torch.where(ref != 0, torch.ldexp(torch.ones_like(ref), e - 8), torch.zeros_like(ref))


def _within(got, ref, tol, what):
    m = AR._ratio((got.double().cpu() - ref).abs(), tol)
    worst = m.max().item()
    print(f"{what}: max err/bound = {worst:.3f}")
    assert worst <= 1.0, (what, int((m > 1).sum()), worst, int(m.reshape(-1).argmax()))


def _gelu64(x):
    cdf = 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) * (2.0 * torch.pi) ** -0.5


@pytest.mark.parametrize("shape", [SMALL, BIG], ids=["small", "big"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gelu_matches_fp64(dtype, shape, dev):
    """1 + erf cancels for negative x, so the natural bound is absolute: c * 2^-24 * (1 + |x|) forward, times |dy| backward, c = max(4, 4 x
    the same ratio of torch's fp32 CPU F.gelu on these inputs), printed by the test; bf16 adds
    one ulp of the reference for the store."""
    from nerf_rpn_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*shape, generator=g) * 3
    special = torch.tensor([0.0, 1e-30, 0.5, 3.0, 6.0, 12.0, 40.0])
    x.view(-1)[:14] = torch.cat([special, -special])
    dy = torch.randn(*shape, generator=g)
    x, dy = x.to(dtype), dy.to(dtype)
    x64, dy64 = x.double(), dy.double()
    y64, d64 = _gelu64(x64)
    base_f, base_b = EPS32 * (1.0 + x64.abs()), EPS32 * (1.0 + x64.abs()) * dy64.abs()
    xt = x.float().requires_grad_()
    yt = F.gelu(xt)
    (gt,) = torch.autograd.grad(yt, xt, dy.float())
    c_f = max(4.0, 4.0 * AR._ratio((yt.detach().double() - y64).abs(), base_f).max().item())
    c_b = max(4.0, 4.0 * AR._ratio((gt.double() - d64 * dy64).abs(), base_b).max().item())
    print("gelu c forward / backward:", c_f, c_b)
    xg = x.to(dev).requires_grad_()
    y = ops.GeluFn.apply(xg)
    (gx,) = torch.autograd.grad(y, xg, dy.to(dev))
    assert y.dtype == dtype and gx.dtype == dtype
    extra = (lambda r: _ulp_bf16(r)) if dtype == BF16 else (lambda r: 0.0)
    _within(y, y64, c_f * base_f + extra(y64), f"gelu {dtype} {shape}")
    _within(gx, d64 * dy64, c_b * base_b + extra(d64 * dy64), f"gelu backward {dtype} {shape}")


@pytest.mark.parametrize("shape", [(3, 5, 3, 7, 4), (3, 24, 24, 40, 128)], ids=["small", "big"])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_scale_add_matches_fp64(dtype, scaled, shape, dev):
    """y = a + s[n] b is one fused multiply-add: |err| <= 2^-24 (|a| + |s b|) in fp32, plus one bf16 ulp of the fp64 value for the bf16
    store; the gradients (dy, s[n] dy) are exact."""
    from nerf_rpn_amd import ops
    g = torch.Generator().manual_seed(4)
    a, b, dy = (torch.randn(*shape, generator=g).to(dtype) for _ in range(3))
    sc = torch.tensor([0.0, 1.25, 2.0]) if scaled else None
    s5 = sc.view(3, 1, 1, 1, 1) if scaled else torch.ones(1)
    ag, bg = a.to(dev).requires_grad_(), b.to(dev).requires_grad_()
    y = ops.ScaleAddFn.apply(ag, bg, sc.to(dev) if scaled else None)
    ga, gb = torch.autograd.grad(y, (ag, bg), dy.to(dev))
    ref = a.double() + s5.double() * b.double()
    tol = EPS32 * (a.double().abs() + (s5.double() * b.double()).abs()) + (_ulp_bf16(ref) if dtype == BF16 else 0.0)
    _within(y, ref, tol, f"scale_add {dtype} scaled={scaled} {shape}")
    assert torch.equal(ga.cpu(), dy) and torch.equal(gb.cpu(), (s5 * dy.float()).to(dtype))


@pytest.mark.parametrize("shape", [(2, 5, 4, 3, 8), (1, 47, 45, 33, 128)], ids=["small", "big"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_patch_merge_is_an_exact_gather(dtype, shape, dev):
    from nerf_rpn_amd import ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(*shape, generator=g).to(dtype)
    xp = F.pad(x, (0, 0, 0, shape[3] % 2, 0, shape[2] % 2, 0, shape[1] % 2)).requires_grad_()
    yr = torch.cat([xp[:, i::2, j::2, k::2] for k in (0, 1) for j in (0, 1) for i in (0, 1)], -1)
    dy = torch.randn(yr.shape, generator=g).to(dtype)
    (rx,) = torch.autograd.grad(yr, xp, dy)
    xg = x.to(dev).requires_grad_()
    y = ops.PatchMergeFn.apply(xg)
    (gx,) = torch.autograd.grad(y, xg, dy.to(dev))
    assert torch.equal(y.cpu(), yr.detach()) and torch.equal(gx.cpu(), rx[:, :shape[1], :shape[2], :shape[3]])


@pytest.mark.parametrize("shape,patch", [((2, 21, 16, 12), 4), ((1, 7, 5, 9), 2), ((1, 160, 160, 96), 4)], ids=["small", "odd", "big"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_patchify_is_an_exact_gather(dtype, shape, patch, dev):
    from nerf_rpn_amd import ops
    n, gx, gy, gz = shape
    x = torch.randn(*shape, 4, generator=torch.Generator().manual_seed(6)).to(dtype)
    ox, oy, oz, p = gx // patch, gy // patch, gz // patch, patch
    yr = x[:, :ox * p, :oy * p, :oz * p].reshape(n, ox, p, oy, p, oz, p, 4).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(n, ox, oy, oz, 4 * p ** 3)
    assert torch.equal(ops.patchify(x.to(dev), patch).cpu(), yr)
