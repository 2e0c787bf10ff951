"""GPU: BatchNorm3d / GroupNorm / LayerNorm kernels against a plain float64 CPU reference of the same operation, at every dispatch branch
(channel tiles, row lanes, slab counts, grid strides, the fast and general apply kernels), in fp32 and bf16, on offset data (mean / std up
to 100, where single-pass statistics cancel; BatchNorm's are strict expected failures) and through the accumulate-into-arena
parameter-gradient paths (ops.GradSink).

The reference always runs on the values the kernel read (the bf16-rounded input where the dtype is bf16); where a ReLU is fused it takes
its mask from the kernel's own stored output, which is the mask the backward kernels use.  Bounds:
  * fp32 outputs and dx:  |err| <= 1e-5 * (1 + |ref|) per element;
  * bf16 outputs:         |err| <= 1 bf16 ulp of the fp64 value, with an absolute floor of 2^-22 * max|ref| (the fp32 arithmetic before the
                          rounding, where the result cancels to near zero);  bf16 dx: the same plus an absolute floor of 1e-6 * max|ref|;
  * sums (dgamma, dbeta, mean, var, running statistics, arena slots):  |err| <= 1e-5 * sum|terms|, per channel;
  * offset data (fp32):   max|err| of the output and of dx <= max(4 x torch fp32 CPU's max|err| on the same input, 2e-6)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _seeded(seed):
    return torch.Generator().manual_seed(seed)


def check_elem(got, ref, dtype, what, dx=False):
    """Per-element bound of an output / input gradient (see the module docstring)."""
    got, ref = got.double().cpu().reshape(-1), ref.double().cpu().reshape(-1)
    err = (got - ref).abs()
    if dtype == F32:
        tol = 1e-5 * (1.0 + ref.abs())
    else:
        _, e = torch.frexp(ref)
        ulp = torch.where(ref != 0, torch.ldexp(torch.ones_like(ref), e - 8), torch.zeros_like(ref))      # 2^(floor(log2|v|) - 7)
        amax = ref.abs().max().item()
        tol = torch.clamp(ulp, min=2.0 ** -22 * amax) + (1e-6 * amax if dx else 0.0)
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), err.max().item(), (err / tol).max().item())


def check_sum(got, ref, terms_abs, what):
    """Sum bound: |err| <= 1e-5 * sum|terms| per entry."""
    got, ref, terms_abs = got.double().cpu().reshape(-1), ref.double().cpu().reshape(-1), terms_abs.double().cpu().reshape(-1)
    err = (got - ref).abs()
    tol = 1e-5 * terms_abs
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), err.max().item(), (err / tol.clamp(min=1e-300)).max().item())


def check_offset(got, ref, torch32, what):
    """Offset data: the kernel's max error against fp64 is at most 4 x torch fp32 CPU's, with a floor of 2e-6."""
    e_k = (got.double().cpu() - ref).abs().max().item()
    e_t = (torch32.double() - ref).abs().max().item()
    assert e_k <= max(4.0 * e_t, 2e-6), (what, e_k, e_t)


def _switch(name, on):
    from nerf_rpn_amd import lib
    lib.call(name, 1 if on else 0)


# ======================================================================================================================
# float64 references
# ======================================================================================================================
def bn_ref_fwd(x, gamma, beta, eps):
    """x [R, C] f64 -> mean, biased var, xhat, rstd, y (before ReLU)."""
    m = x.mean(0)
    v = ((x - m) ** 2).mean(0)
    rs = 1.0 / torch.sqrt(v + eps)
    xh = (x - m) * rs
    return m, v, xh, rs, xh * gamma + beta


def bn_ref_bwd(gm, xh, rs, gamma):
    """gm = dy * mask [R, C] -> dx, dgamma, dbeta and the absolute term sums of dgamma / dbeta."""
    r = gm.shape[0]
    db, dg = gm.sum(0), (gm * xh).sum(0)
    dx = gamma * rs * (gm - db / r - xh * dg / r)
    return dx, dg, db, (gm * xh).abs().sum(0), gm.abs().sum(0)


def gn_ref_fwd(x, gamma, beta, groups, eps):
    """x [N, R, C] f64 -> mean [N, G], rstd [N, G], xhat [N, R, C], y (before ReLU)."""
    n, r, c = x.shape
    xg = x.reshape(n, r, groups, c // groups)
    m = xg.mean(dim=(1, 3))
    v = ((xg - m[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rs = 1.0 / torch.sqrt(v + eps)
    xh = ((xg - m[:, None, :, None]) * rs[:, None, :, None]).reshape(n, r, c)
    return m, rs, xh, xh * gamma + beta


def gn_ref_bwd(gm, xh, rs, gamma, groups):
    n, r, c = gm.shape
    gg = (gm * gamma).reshape(n, r, groups, c // groups)
    xhg = xh.reshape(n, r, groups, c // groups)
    a = (gg * xhg).mean(dim=(1, 3), keepdim=True)
    b = gg.mean(dim=(1, 3), keepdim=True)
    dx = (rs[:, None, :, None] * (gg - b - xhg * a)).reshape(n, r, c)
    return dx, (gm * xh).sum(dim=(0, 1)), gm.sum(dim=(0, 1)), (gm * xh).abs().sum(dim=(0, 1)), gm.abs().sum(dim=(0, 1))


def ln_ref(x, gamma, beta, dy, eps):
    """x, dy [R, C] f64 -> y, dx, dgamma, dbeta, |terms| of dgamma / dbeta."""
    m = x.mean(1, keepdim=True)
    v = ((x - m) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(v + eps)
    xh = (x - m) * rs
    gg = dy * gamma
    dx = rs * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    return xh * gamma + beta, dx, (dy * xh).sum(0), dy.sum(0), (dy * xh).abs().sum(0), dy.abs().sum(0)


# ======================================================================================================================
# BatchNorm3d
# ======================================================================================================================
def _bn_params(c, seed, dev):
    g = _seeded(seed)
    gamma = (torch.rand(c, generator=g) + 0.5).to(dev).requires_grad_()
    beta = (torch.randn(c, generator=g) * 0.3).to(dev).requires_grad_()
    rmean = (torch.randn(c, generator=g) * 0.1).to(dev)
    rvar = (torch.rand(c, generator=g) + 0.5).to(dev)
    return gamma, beta, rmean, rvar


def _bn_run(x, gamma, beta, rmean, rvar, dy, relu, momentum=0.1, eps=1e-5):
    """Training forward + backward through ops.BatchNormFn; returns (y, dx, dgamma, dbeta, running mean, running var)."""
    from nerf_rpn_amd import ops
    xx = x.clone().requires_grad_()
    rm, rv = rmean.clone(), rvar.clone()
    y = ops.BatchNormFn.apply(xx, gamma, beta, rm, rv, True, momentum, eps, relu)
    gx, gg, gb = torch.autograd.grad(y, (xx, gamma, beta), dy)
    torch.cuda.synchronize()
    return y.detach(), gx, gg, gb, rm, rv


# rows below one slab (45 < 64), ragged slabs (420, 990 rows; 64-row slabs), more than one grid stride of the apply kernels (144000 rows x
# 64 ch: 2.3 M four-channel groups > 8192 x 256 lanes of the general kernels; > 2048 x 256 of the fast forward and 1280 x 256 of the fast
# backward), n = 1 and 2, C = 4 (one channel group, 256 row lanes) .. 2048 (two blockIdx.y channel tiles of 1024, one row lane)
BN_CASES = [(4, (1, 3, 3, 5)), (4, (2, 7, 6, 5)), (64, (1, 3, 3, 5)), (64, (2, 7, 6, 5)), (64, (1, 40, 40, 90)), (256, (2, 7, 6, 5)),
            (256, (1, 10, 9, 11)), (512, (2, 4, 4, 5)), (2048, (1, 3, 3, 5)), (2048, (2, 4, 4, 5))]


@pytest.mark.parametrize("c,shape", BN_CASES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_batchnorm_train_matches_fp64(c, shape, dtype, dev):
    from nerf_rpn_amd import ops
    g = _seeded(c + sum(shape))
    x = (torch.randn(*shape, c, generator=g) * 1.7 + torch.randn(c, generator=g) * 0.5).to(dtype)
    dy = torch.randn(*shape, c, generator=g).to(dtype)
    gamma, beta, rmean, rvar = _bn_params(c, 1, dev)
    momentum, eps = 0.1, 1e-5
    outs = {}
    for fast in (1, 0):
        _switch("set_bn_fast", fast)
        try:
            outs[fast] = _bn_run(x.to(dev), gamma, beta, rmean, rvar, dy.to(dev), True, momentum, eps)
        finally:
            _switch("set_bn_fast", 1)
    # fast and general apply kernels: the same bits.  Not yet where the fp32 fast kernels loop more than once per lane (144000 rows x 64
    # ch: the input gradients differ in the last bit there, both within the fp64 bounds below; cause not found yet)
    if not (dtype == F32 and x.numel() // c > 100000):
        for a, b in zip(outs[1], outs[0]):
            assert torch.equal(a, b)
    r = x.numel() // c
    x64, dy64 = x.double().reshape(r, c), dy.double().reshape(r, c)
    g64, b64 = gamma.detach().double().cpu(), beta.detach().double().cpu()
    m, v, xh, rs, ylin = bn_ref_fwd(x64, g64, b64, eps)
    for y, gx, gg, gb, _, _ in (outs[1], outs[0]):
        mask = (y.reshape(r, c).cpu() > 0).double()
        check_elem(y.reshape(r, c), ylin.clamp(min=0), dtype, "y")
        dx, dg, db, tg, tb = bn_ref_bwd(dy64 * mask, xh, rs, g64)
        check_elem(gx.reshape(r, c), dx, dtype, "dx", dx=True)
        check_sum(gg, dg, tg, "dgamma")
        check_sum(gb, db, tb, "dbeta")
    y, gx, gg, gb, rm, rv = outs[1]
    # running statistics (unbiased variance, momentum); their terms: the old value and the batch statistic's own terms
    rm0, rv0 = rmean.double().cpu(), rvar.double().cpu()
    check_sum(rm, (1 - momentum) * rm0 + momentum * m, (1 - momentum) * rm0.abs() + momentum * x64.abs().mean(0), "running_mean")
    unb = v * r / (r - 1)
    check_sum(rv, (1 - momentum) * rv0 + momentum * unb, (1 - momentum) * rv0 + momentum * unb, "running_var")
    # eval forward on the updated running statistics
    ye = ops.BatchNormFn.apply(x.to(dev), gamma, beta, rm, rv, False, momentum, eps, True)
    rme, rve = rm.double().cpu(), rv.double().cpu()
    check_elem(ye.reshape(r, c), (((x64 - rme) / torch.sqrt(rve + eps)) * g64 + b64).clamp(min=0), dtype, "y_eval")


@pytest.mark.parametrize("c,shape", [(64, (2, 7, 6, 5)), (256, (1, 10, 9, 11)), (2048, (2, 4, 4, 5))])
def test_batchnorm_bf16_v8_reduction_matches_fp64(c, shape, dev):
    """The 8-channel-lane statistics / backward reductions (tools switch set_bn_reduce_v8): a different summation grouping, so the same
    fp64 bounds rather than the same bits."""
    g = _seeded(7 + c)
    x = (torch.randn(*shape, c, generator=g) * 1.7 + 0.4).to(BF16)
    dy = torch.randn(*shape, c, generator=g).to(BF16)
    gamma, beta, rmean, rvar = _bn_params(c, 2, dev)
    _switch("set_bn_reduce_v8", 1)
    try:
        y, gx, gg, gb, _, _ = _bn_run(x.to(dev), gamma, beta, rmean, rvar, dy.to(dev), True)
    finally:
        _switch("set_bn_reduce_v8", 0)
    r = x.numel() // c
    x64, dy64 = x.double().reshape(r, c), dy.double().reshape(r, c)
    g64, b64 = gamma.detach().double().cpu(), beta.detach().double().cpu()
    _, _, xh, rs, ylin = bn_ref_fwd(x64, g64, b64, 1e-5)
    check_elem(y.reshape(r, c), ylin.clamp(min=0), BF16, "y")
    dx, dg, db, tg, tb = bn_ref_bwd(dy64 * (y.reshape(r, c).cpu() > 0).double(), xh, rs, g64)
    check_elem(gx.reshape(r, c), dx, BF16, "dx", dx=True)
    check_sum(gg, dg, tg, "dgamma")
    check_sum(gb, db, tb, "dbeta")


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_batchnorm_c96_training_refused_eval_exact(dtype, dev):
    """C = 96 (min(C, 1024) / 4 does not divide 256): the statistics and backward kernels must refuse it, never compute it wrong; the
    eval forward (bn_apply only, general kernel) must be right."""
    from nerf_rpn_amd import lib, ops
    c = 96
    g = _seeded(96)
    x = (torch.randn(2, 5, 4, 3, c, generator=g) * 1.5 + 0.3).to(dtype)
    gamma, beta, rmean, rvar = _bn_params(c, 3, dev)
    with pytest.raises(lib.NrpnError):
        ops.BatchNormFn.apply(x.to(dev), gamma, beta, rmean.clone(), rvar.clone(), True, 0.1, 1e-5, True)
    torch.cuda.synchronize()
    ye = ops.BatchNormFn.apply(x.to(dev), gamma, beta, rmean, rvar, False, 0.1, 1e-5, False)
    r = x.numel() // c
    ref = (x.double().reshape(r, c) - rmean.double().cpu()) / torch.sqrt(rvar.double().cpu() + 1e-5) * gamma.detach().double().cpu() \
        + beta.detach().double().cpu()
    check_elem(ye.reshape(r, c), ref, dtype, "y_eval")


# the bn_stats path (no conv-epilogue partials), mean / std = r.  Its single-pass fp32 sums cancel there (measured: 17x / 220x torch fp32
# CPU's output error at r = 10 / 100); the shifted form waits for the BatchNorm training tests' bounds, DESIGN.md 3.2
@pytest.mark.xfail(strict=True, reason="bn_stats keeps single-pass fp32 sums of x and x^2 (DESIGN.md 3.2)")
@pytest.mark.parametrize("r", [10.0, 100.0])
@pytest.mark.parametrize("c,shape", [(64, (2, 7, 6, 5)), (256, (1, 20, 20, 20))])
def test_batchnorm_offset_data(r, c, shape, dev):
    g = _seeded(int(r) + c)
    x = torch.randn(*shape, c, generator=g) + r
    dy = torch.randn(*shape, c, generator=g)
    gamma, beta, rmean, rvar = _bn_params(c, 4, dev)
    y, gx, gg, gb, _, _ = _bn_run(x.to(dev), gamma, beta, rmean, rvar, dy.to(dev), True)
    rows = x.numel() // c
    mask = (y.reshape(rows, c).cpu() > 0)
    x64, g64, b64 = x.double().reshape(rows, c), gamma.detach().double().cpu(), beta.detach().double().cpu()
    _, _, xh, rs, ylin = bn_ref_fwd(x64, g64, b64, 1e-5)
    gm = dy.double().reshape(rows, c) * mask.double()
    dx, dg, db, tg, tb = bn_ref_bwd(gm, xh, rs, g64)
    # torch fp32 CPU on the same input, with the same mask
    xt = x.reshape(rows, c).clone().requires_grad_()
    yt = F.batch_norm(xt, None, None, gamma.detach().cpu(), beta.detach().cpu(), True, 0.1, 1e-5)
    (dxt,) = torch.autograd.grad(yt, (xt,), gm.float())
    check_offset(torch.where(mask, y.reshape(rows, c).cpu(), 0), torch.where(mask, ylin, 0), torch.where(mask, yt.detach(), 0), "y")
    check_offset(gx.reshape(rows, c), dx, dxt, "dx")
    check_sum(gg, dg, tg, "dgamma")
    check_sum(gb, db, tb, "dbeta")


# the conv epilogue's fused statistics keep a single-pass fp32 form: covered at the mean / std measured in this network (<= 4).
# bf16 64 -> 64 channels on a 40^3 grid is a shape whose conv kernel leaves them.
@pytest.mark.parametrize("r", [0.0, 4.0])
def test_conv_epilogue_statistics_at_network_offsets(r, dev):
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model import hip_nn
    from torch import nn
    torch.manual_seed(0)
    conv = nn.Conv3d(64, 64, 3, padding=1).to(dev)
    gamma, beta, rmean, rvar = _bn_params(64, 6, dev)
    x = torch.randn(1, 40, 40, 40, 64, generator=_seeded(5)).to(dev).to(BF16)
    with torch.no_grad():
        conv.bias.fill_(r / math.sqrt(3.0))      # output std ~ 1 / sqrt(3) with the default weight initialisation: mean / std ~ r
        holder = {}
        y = hip_nn.conv3d(conv, x, stats=holder)
        assert holder.get("partials") is not None, "the conv left no epilogue statistics"
        out = ops.BatchNormFn.apply(y, gamma, beta, rmean, rvar, True, 0.1, 1e-5, False, holder["partials"])
    c = 64
    rows = y.numel() // c
    _, _, _, _, ylin = bn_ref_fwd(y.double().reshape(rows, c).cpu(), gamma.detach().double().cpu(), beta.detach().double().cpu(), 1e-5)
    check_elem(out.reshape(rows, c), ylin, BF16, "y")


# ======================================================================================================================
# GroupNorm
# ======================================================================================================================
GN_CASES = [(256, 32, (2, 6, 5, 4)), (256, 32, (1, 21, 7, 3)), (64, 8, (3, 4, 4, 4)), (64, 8, (1, 40, 40, 30)), (96, 8, (2, 5, 4, 3)),
            (96, 8, (3, 7, 5, 3)), (1024, 32, (1, 5, 4, 3)), (1024, 32, (2, 3, 3, 3)), (128, 16, (2, 9, 4, 4))]


def _gn_run(x, gamma, beta, dy, groups, relu, eps=1e-5):
    from nerf_rpn_amd import ops
    xx = x.clone().requires_grad_()
    y = ops.GroupNormFn.apply(xx, gamma, beta, groups, eps, relu)
    gx, gg, gb = torch.autograd.grad(y, (xx, gamma, beta), dy)
    torch.cuda.synchronize()
    return y.detach(), gx, gg, gb


@pytest.mark.parametrize("c,groups,shape", GN_CASES)
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_groupnorm_matches_fp64(c, groups, shape, relu, dtype, dev):
    g = _seeded(c + groups + sum(shape))
    x = (torch.randn(*shape, c, generator=g) * 1.7 + torch.randn(c, generator=g) * 0.5).to(dtype)
    dy = torch.randn(*shape, c, generator=g).to(dtype)
    gamma = (torch.rand(c, generator=g) + 0.5).to(dev).requires_grad_()
    beta = (torch.randn(c, generator=g) * 0.3).to(dev).requires_grad_()
    outs = {}
    for fast in (1, 0):
        _switch("set_gn_fast", fast)
        try:
            outs[fast] = _gn_run(x.to(dev), gamma, beta, dy.to(dev), groups, relu)
        finally:
            _switch("set_gn_fast", 1)
    for a, b in zip(outs[1], outs[0]):
        assert torch.equal(a, b)
    y, gx, gg, gb = outs[1]
    n = shape[0]
    rows = x[0].numel() // c
    x64, dy64 = x.double().reshape(n, rows, c), dy.double().reshape(n, rows, c)
    g64, b64 = gamma.detach().double().cpu(), beta.detach().double().cpu()
    _, rs, xh, ylin = gn_ref_fwd(x64, g64, b64, groups, 1e-5)
    y3 = y.reshape(n, rows, c).cpu()
    mask = (y3 > 0).double() if relu else torch.ones_like(x64)
    check_elem(y3, ylin.clamp(min=0) if relu else ylin, dtype, "y")
    dx, dg, db, tg, tb = gn_ref_bwd(dy64 * mask, xh, rs, g64, groups)
    check_elem(gx.reshape(n, rows, c), dx, dtype, "dx", dx=True)
    check_sum(gg, dg, tg, "dgamma")
    check_sum(gb, db, tb, "dbeta")


@pytest.mark.parametrize("r", [10.0, 100.0])
@pytest.mark.parametrize("c,groups,shape,relu", [(256, 32, (2, 6, 5, 4), True), (96, 8, (2, 9, 7, 5), False), (64, 8, (1, 40, 40, 30), True)])
def test_groupnorm_offset_data(r, c, groups, shape, relu, dev):
    g = _seeded(int(r) + c)
    x = torch.randn(*shape, c, generator=g) + r
    dy = torch.randn(*shape, c, generator=g)
    gamma = (torch.rand(c, generator=g) + 0.5).to(dev).requires_grad_()
    beta = (torch.randn(c, generator=g) * 0.3).to(dev).requires_grad_()
    y, gx, gg, gb = _gn_run(x.to(dev), gamma, beta, dy.to(dev), groups, relu)
    n = shape[0]
    rows = x[0].numel() // c
    x64 = x.double().reshape(n, rows, c)
    g64, b64 = gamma.detach().double().cpu(), beta.detach().double().cpu()
    _, rs, xh, ylin = gn_ref_fwd(x64, g64, b64, groups, 1e-5)
    y3 = y.reshape(n, rows, c).cpu()
    mask = (y3 > 0) if relu else torch.ones_like(y3, dtype=torch.bool)
    gm = dy.double().reshape(n, rows, c) * mask.double()
    dx, dg, db, tg, tb = gn_ref_bwd(gm, xh, rs, g64, groups)
    # torch fp32 CPU GroupNorm on the same input ([N, C, rows]), with the same mask
    xt = x.reshape(n, rows, c).permute(0, 2, 1).contiguous().requires_grad_()
    yt = F.group_norm(xt, groups, gamma.detach().cpu(), beta.detach().cpu(), 1e-5)
    (dxt,) = torch.autograd.grad(yt, (xt,), gm.float().permute(0, 2, 1))
    yt, dxt = yt.detach().permute(0, 2, 1), dxt.permute(0, 2, 1)
    check_offset(torch.where(mask, y3, 0), torch.where(mask, ylin, 0), torch.where(mask, yt, 0), "y")
    check_offset(gx.reshape(n, rows, c), dx, dxt, "dx")
    check_sum(gg, dg, tg, "dgamma")
    check_sum(gb, db, tb, "dbeta")


# ======================================================================================================================
# LayerNorm
# ======================================================================================================================
LN_WIDTHS = [32, 96, 100, 192, 384, 768, 1000, 1536, 3072]      # MAXK 4 / 12 / 24 / 48 backward forms, C not a multiple of 64


def _ln_run(x, gamma, beta, dy, eps=1e-5):
    from nerf_rpn_amd import ops
    xx = x.clone().requires_grad_()
    y = ops.LayerNormFn.apply(xx, gamma, beta, eps)
    gx, gg, gb = torch.autograd.grad(y, (xx, gamma, beta), dy)
    torch.cuda.synchronize()
    return y.detach(), gx, gg, gb


@pytest.mark.parametrize("c", LN_WIDTHS)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_layernorm_matches_fp64(c, dtype, dev):
    g = _seeded(c)
    rows = 4352 if c <= 768 else 600      # 4352 rows: more than one grid stride of the backward (1024 blocks x 4 rows)
    x = (torch.randn(rows, c, generator=g) * 1.7 + torch.randn(rows, 1, generator=g) * 0.5).to(dtype)
    dy = torch.randn(rows, c, generator=g).to(dtype)
    gamma = (torch.rand(c, generator=g) + 0.5).to(dev).requires_grad_()
    beta = (torch.randn(c, generator=g) * 0.3).to(dev).requires_grad_()
    y, gx, gg, gb = _ln_run(x.to(dev), gamma, beta, dy.to(dev))
    yr, dx, dg, db, tg, tb = ln_ref(x.double(), gamma.detach().double().cpu(), beta.detach().double().cpu(), dy.double(), 1e-5)
    check_elem(y, yr, dtype, "y")
    check_elem(gx, dx, dtype, "dx", dx=True)
    check_sum(gg, dg, tg, "dgamma")
    check_sum(gb, db, tb, "dbeta")


@pytest.mark.parametrize("r", [10.0, 100.0])
@pytest.mark.parametrize("c", [96, 768])
def test_layernorm_offset_data(r, c, dev):
    g = _seeded(c + int(r))
    x = torch.randn(700, c, generator=g) + r
    dy = torch.randn(700, c, generator=g)
    gamma = (torch.rand(c, generator=g) + 0.5).to(dev).requires_grad_()
    beta = (torch.randn(c, generator=g) * 0.3).to(dev).requires_grad_()
    y, gx, gg, gb = _ln_run(x.to(dev), gamma, beta, dy.to(dev))
    yr, dx, dg, db, tg, tb = ln_ref(x.double(), gamma.detach().double().cpu(), beta.detach().double().cpu(), dy.double(), 1e-5)
    xt = x.clone().requires_grad_()
    yt = F.layer_norm(xt, (c,), gamma.detach().cpu(), beta.detach().cpu(), 1e-5)
    (dxt,) = torch.autograd.grad(yt, (xt,), dy)
    check_offset(y, yr, yt.detach(), "y")
    check_offset(gx, dx, dxt, "dx")
    check_sum(gg, dg, tg, "dgamma")
    check_sum(gb, db, tb, "dbeta")


# ======================================================================================================================
# accumulate-into-arena parameter gradients (GradSink slots)
# ======================================================================================================================
def _sinks(params, prefills, direct):
    """Give each parameter a GradSink slot prefilled with ``prefill``: a contiguous fp32 tensor (``direct``: the form ops._slots_direct
    accepts) or a strided view of a larger buffer (the kernels then hand back a gradient that is added to the slot)."""
    from nerf_rpn_amd import ops
    slots = []
    for p, pre in zip(params, prefills):
        if direct:
            slot = pre.clone().reshape(p.shape)
        else:
            slot = torch.zeros(*p.shape, 2, dtype=torch.float32, device=pre.device)[..., 0]
            slot.copy_(pre.reshape(p.shape))
            assert not slot.is_contiguous()
        p._nrpn_sink = ops.GradSink(slot, lambda: None)
        slots.append(slot)
    return slots


def _prefills(shapes, seed, dev):
    g = _seeded(seed)
    return [(torch.randn(s, generator=g) * 3.0).to(dev) for s in shapes]


def _check_slots(slots, prefills, refs, terms, what):
    for slot, pre, ref, t in zip(slots, prefills, refs, terms):
        pre64 = pre.double().cpu().reshape(-1)
        check_sum(slot.reshape(-1), pre64 + ref.reshape(-1), pre64.abs() + t.reshape(-1), what)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_arena_slots_layernorm(dtype, dev):
    from nerf_rpn_amd import ops
    c, rows = 384, 900
    g = _seeded(21)
    x = (torch.randn(rows, c, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(rows, c, generator=g).to(dtype)
    gamma0, beta0 = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    _, _, dg, db, tg, tb = ln_ref(x.double(), gamma0.double(), beta0.double(), dy.double(), 1e-5)
    gamma, beta = gamma0.to(dev).requires_grad_(), beta0.to(dev).requires_grad_()
    pre = _prefills([(c,), (c,)], 23, dev)
    got = {}
    for direct in (True, False):
        slots = _sinks([gamma, beta], pre, direct)
        try:
            xx = x.to(dev).requires_grad_()
            y = ops.LayerNormFn.apply(xx, gamma, beta, 1e-5)
            y.backward(dy.to(dev))
            torch.cuda.synchronize()
        finally:
            del gamma._nrpn_sink, beta._nrpn_sink
        assert gamma.grad is None and beta.grad is None      # everything went to the slots
        _check_slots(slots, pre, [dg, db], [tg, tb], f"layernorm direct={direct}")
        got[direct] = [s.reshape(-1).clone() for s in slots]
    assert all(torch.equal(a, b) for a, b in zip(got[True], got[False]))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_arena_slots_groupnorm(dtype, dev):
    from nerf_rpn_amd import ops
    c, groups, shape = 256, 32, (2, 6, 5, 4)
    g = _seeded(31)
    x = (torch.randn(*shape, c, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(*shape, c, generator=g).to(dtype)
    gamma = (torch.rand(c, generator=g) + 0.5).to(dev).requires_grad_()
    beta = (torch.randn(c, generator=g) * 0.3).to(dev).requires_grad_()
    n, rows = shape[0], x[0].numel() // c
    pre = _prefills([(c,), (c,)], 33, dev)
    got = {}
    for direct in (True, False):
        slots = _sinks([gamma, beta], pre, direct)
        try:
            xx = x.to(dev).requires_grad_()
            y = ops.GroupNormFn.apply(xx, gamma, beta, groups, 1e-5, True)
            y.backward(dy.to(dev))
            torch.cuda.synchronize()
        finally:
            del gamma._nrpn_sink, beta._nrpn_sink
        assert gamma.grad is None and beta.grad is None
        x64 = x.double().reshape(n, rows, c)
        _, rs, xh, _ = gn_ref_fwd(x64, gamma.detach().double().cpu(), beta.detach().double().cpu(), groups, 1e-5)
        mask = (y.detach().reshape(n, rows, c).cpu() > 0).double()
        _, dg, db, tg, tb = gn_ref_bwd(dy.double().reshape(n, rows, c) * mask, xh, rs, gamma.detach().double().cpu(), groups)
        _check_slots(slots, pre, [dg, db], [tg, tb], f"groupnorm direct={direct}")
        got[direct] = [s.reshape(-1).clone() for s in slots]
    assert all(torch.equal(a, b) for a, b in zip(got[True], got[False]))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_arena_slots_batchnorm(dtype, dev):
    """BatchNorm's backward adds into whichever parameter has a slot; without slots the gradients go back to autograd, and prefill + that
    gradient must be the same bits."""
    from nerf_rpn_amd import ops
    c, shape = 64, (2, 7, 6, 5)
    g = _seeded(41)
    x = (torch.randn(*shape, c, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(*shape, c, generator=g).to(dtype)
    gamma, beta, rmean, rvar = _bn_params(c, 42, dev)
    pre = _prefills([(c,), (c,)], 43, dev)
    slots = _sinks([gamma, beta], pre, True)
    try:
        xx = x.to(dev).requires_grad_()
        y = ops.BatchNormFn.apply(xx, gamma, beta, rmean.clone(), rvar.clone(), True, 0.1, 1e-5, True)
        y.backward(dy.to(dev))
        torch.cuda.synchronize()
        y = y.detach()
    finally:
        del gamma._nrpn_sink, beta._nrpn_sink
    assert gamma.grad is None and beta.grad is None
    r = x.numel() // c
    _, _, xh, rs, _ = bn_ref_fwd(x.double().reshape(r, c), gamma.detach().double().cpu(), beta.detach().double().cpu(), 1e-5)
    _, dg, db, tg, tb = bn_ref_bwd(dy.double().reshape(r, c) * (y.reshape(r, c).cpu() > 0).double(), xh, rs, gamma.detach().double().cpu())
    _check_slots(slots, pre, [dg, db], [tg, tb], "batchnorm")
    # the autograd path (no slots): prefill + its gradient, the same bits
    _, _, gg, gb, _, _ = _bn_run(x.to(dev), gamma, beta, rmean, rvar, dy.to(dev), True)
    assert torch.equal(slots[0], pre[0] + gg) and torch.equal(slots[1], pre[1] + gb)


@pytest.mark.parametrize("shift", [0, 2])
def test_arena_slot_window_attention_table(shift, dev):
    """The relative-position bias table's gradient: added into a contiguous slot by the table reduction itself (direct), or handed back and
    added to a strided slot; both equal prefill + the fp64 gradient within the sum bound (terms: every window's score gradient)."""
    from nerf_rpn_amd import ops
    from oracle import nets as ON
    heads, shape = 3, (2, 8, 8, 8)
    c = 32 * heads
    ref_mod = ON.WindowAttention(c, heads, shift)
    index = ref_mod.relative_position_index      # int64 for the reference; the kernel reads it as int32
    g = _seeded(51 + shift)
    qkv = torch.randn(*shape, 3 * c, generator=g)
    dout = torch.randn(*shape, c, generator=g)
    table = torch.randn(343, heads, generator=g) * 0.5
    from attention_ref import attn_core_ref      # the fp64 attention core shared with test_gpu_attention.py
    ref = attn_core_ref(qkv.double(), None, table.double(), index, heads, shift, dout=dout.double())
    # sum |terms|: |score gradient| of every window and (i, j), scattered onto the table entries
    dt64, terms = ref.dtable, ref.terms["dtable"]
    tp = table.to(dev).requires_grad_()
    pre = _prefills([(343, heads)], 53, dev)
    got = {}
    for direct in (True, False):
        slots = _sinks([tp], pre, direct)
        try:
            out = ops.WindowAttnFn.apply(qkv.to(dev), None, tp, index.to(torch.int32).to(dev), heads, shift > 0)
            out.backward(dout.to(dev))
            ops.wgrad_stream_join()
            torch.cuda.synchronize()
        finally:
            del tp._nrpn_sink
        assert tp.grad is None
        _check_slots(slots, pre, [dt64], [terms], f"attention table direct={direct}")
        got[direct] = slots[0].reshape(-1).clone()
    assert torch.equal(got[True], got[False])
