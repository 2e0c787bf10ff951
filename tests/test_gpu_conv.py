"""GPU parity: conv3d family + BN / pool / upsample / optimiser kernels vs a plain torch fp32 CPU reference of the
same op (fp32 kernels: 1e-4-class tolerances; bf16 kernels: bf16-rounded inputs, fp32 accumulate, 2e-2)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu


def cl(x):
    return x.permute(0, 2, 3, 4, 1).contiguous()


def cf(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12)).item()


CASES = [  # (N, grid, Cin, Cout, k)
    (2, (7, 6, 5), 64, 96, 3), (1, (9, 8, 8), 16, 64, 3), (1, (5, 5, 5), 128, 256, 3), (2, (6, 5, 4), 256, 256, 1),
    (1, (10, 10, 10), 64, 128, 1), (1, (4, 4, 3), 32, 13, 1)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_forward_backward(case, dtype, dev):
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model import hip_nn
    n, grid, cin, cout, k = case
    if dtype == torch.bfloat16 and (cin * 2) % 64:
        pytest.skip("Cin*2 must be a multiple of 64 bytes")
    if (cout * (4 if dtype == torch.float32 else 2)) % 16:
        pytest.skip("wgrad needs 16-byte rows; small heads go through the padded fused-head GEMM")
    torch.manual_seed(0)
    conv = nn.Conv3d(cin, cout, k, padding=k // 2)
    x = torch.randn(n, cin, *grid)
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
        conv.weight.data = conv.weight.data.bfloat16().float()
    xr = x.clone().requires_grad_(True)
    yr = F.relu(conv(xr))
    gy = torch.randn_like(yr)
    if dtype == torch.bfloat16:
        gy = gy.bfloat16().float()
    yr.backward(gy)
    ref = dict(y=yr.detach(), dx=xr.grad, dw=conv.weight.grad.clone(), db=conv.bias.grad.clone())
    conv.zero_grad()
    hconv = nn.Conv3d(cin, cout, k, padding=k // 2).to(dev)
    hconv.load_state_dict(conv.state_dict())
    xh = cl(x).to(dev).to(dtype).requires_grad_(True)
    yh = hip_nn.conv3d(hconv, xh, relu=True)
    yh.backward(cl(gy).to(dev).to(dtype))
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    assert relerr(cf(yh.detach().float().cpu()), ref["y"]) < tol
    assert relerr(cf(xh.grad.float().cpu()), ref["dx"]) < tol
    assert relerr(hconv.weight.grad.cpu(), ref["dw"]) < tol
    assert relerr(hconv.bias.grad.cpu(), ref["db"]) < tol


@pytest.mark.parametrize("tr", [1, 0])
def test_wgrad_bf16_transpose_read_modes(tr, dev):
    """Both bf16 operand-fetch modes (ds_read_b64_tr_b16 and the scalar gather) must give the same weight gradient."""
    from nerf_rpn_amd import lib
    from nerf_rpn_amd.model import hip_nn
    lib.call("set_wgrad_transpose_read", tr)
    try:
        torch.manual_seed(1)
        conv = nn.Conv3d(64, 128, 3, padding=1)
        x = torch.randn(1, 64, 6, 7, 5).bfloat16().float()
        xr = x.clone().requires_grad_(True)
        y = conv(xr)
        gy = torch.randn_like(y).bfloat16().float()
        y.backward(gy)
        h = nn.Conv3d(64, 128, 3, padding=1).to(dev)
        h.load_state_dict(conv.state_dict())
        xh = cl(x).to(dev).bfloat16().requires_grad_(True)
        hip_nn.conv3d(h, xh).backward(cl(gy).to(dev).bfloat16())
        assert relerr(h.weight.grad.cpu(), conv.weight.grad) < 2e-2, f"tr_mode={tr}"
    finally:
        lib.call("set_wgrad_transpose_read", 1)


@pytest.mark.parametrize("stride,grid", [(2, (16, 14, 13)), (1, (9, 8, 7)), (2, (18, 15, 12)), (2, (34, 26, 20))])    # even Z + stride 2: z-row wgrad kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_stem(stride, grid, dtype, dev):
    from nerf_rpn_amd.model import hip_nn
    torch.manual_seed(0)
    conv = nn.Conv3d(4, 64, 7, stride=stride, padding=3)
    x = torch.rand(2, 4, *grid)
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
        conv.weight.data = conv.weight.data.bfloat16().float()
    y = conv(x)
    gy = torch.randn_like(y)
    if dtype == torch.bfloat16:
        gy = gy.bfloat16().float()
    y.backward(gy)
    h = nn.Conv3d(4, 64, 7, stride=stride, padding=3).to(dev)
    h.load_state_dict(conv.state_dict())
    yh = hip_nn.conv3d(h, cl(x).to(dev).to(dtype))
    assert tuple(yh.shape[1:4]) == tuple(y.shape[2:])
    yh.backward(cl(gy).to(dev).to(dtype))
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    assert relerr(cf(yh.detach().float().cpu()), y.detach()) < tol
    assert relerr(h.weight.grad.cpu(), conv.weight.grad) < tol
    assert relerr(h.bias.grad.cpu(), conv.bias.grad) < tol


# (128, small): 16 / 32 channel groups per row (8 bf16 / 4 fp32 channels per lane); (4, ...): one group per row, 8-byte bf16 accesses;
# (64, 70 x 66 x 64): 2.4 M channel groups > one grid stride of the apply kernels (8192 blocks x 256 lanes), several iterations per lane
@pytest.mark.parametrize("c,grid", [(128, (9, 7, 6)), (4, (5, 4, 3)), (64, (70, 66, 64))])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batchnorm_relu(dtype, c, grid, dev):
    from nerf_rpn_amd.model import hip_nn
    torch.manual_seed(0)
    bn = nn.BatchNorm3d(c)
    bn.weight.data.uniform_(0.5, 1.5)
    bn.bias.data.normal_(0, 0.2)
    x = torch.randn(2 if grid[0] < 20 else 1, c, *grid) * 2 + 0.7
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
    xr = x.clone().requires_grad_(True)
    y = F.relu(bn(xr))
    gy = torch.randn_like(y)
    y.backward(gy)
    h = nn.BatchNorm3d(c).to(dev)
    h.load_state_dict({k: v.clone() for k, v in nn.BatchNorm3d(c).state_dict().items()})
    h.weight.data.copy_(bn.weight.data)
    h.bias.data.copy_(bn.bias.data)
    xh = cl(x).to(dev).to(dtype).requires_grad_(True)
    yh = hip_nn.batch_norm(h, xh, True)
    yh.backward(cl(gy).to(dev).to(dtype))
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert relerr(cf(yh.detach().float().cpu()), y.detach()) < tol
    assert relerr(cf(xh.grad.float().cpu()), xr.grad) < (1e-4 if dtype == torch.float32 else 3e-2)
    assert relerr(h.weight.grad.cpu(), bn.weight.grad) < (1e-4 if dtype == torch.float32 else 3e-2)
    assert relerr(h.bias.grad.cpu(), bn.bias.grad) < (1e-4 if dtype == torch.float32 else 3e-2)
    assert torch.allclose(h.running_mean.cpu(), bn.running_mean, atol=1e-5) and torch.allclose(h.running_var.cpu(), bn.running_var, rtol=1e-4)
    assert int(h.num_batches_tracked) == 1
    h.eval(); bn.eval()
    with torch.no_grad():
        ye = hip_nn.batch_norm(h, cl(x).to(dev).to(dtype), False)
        assert relerr(cf(ye.float().cpu()), bn(x)) < tol * 5


@pytest.mark.parametrize("cfg", [(3, 2, 1, False, (16, 15, 13)), (2, 2, 0, True, (9, 8, 5)), (2, 2, 0, True, (10, 10, 10)), (3, 2, 1, False, (7, 8, 9))])
@pytest.mark.parametrize("dtype,ch", [(torch.float32, 64), (torch.bfloat16, 64), (torch.bfloat16, 36)])     # bf16 with C % 8 == 0: 8 channels per lane
def test_maxpool(cfg, dtype, ch, dev):
    from nerf_rpn_amd import ops
    k, s, p, ceil_mode, grid = cfg
    torch.manual_seed(0)
    x = F.relu(torch.randn(2, ch, *grid))      # many exact-zero ties, as after ReLU
    gy_seed = torch.Generator().manual_seed(1)
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
    xr = x.clone().requires_grad_(True)
    y = F.max_pool3d(xr, k, s, p, ceil_mode=ceil_mode)
    gy = torch.randn(y.shape, generator=gy_seed)
    if dtype == torch.bfloat16:
        gy = gy.bfloat16().float()
    y.backward(gy)
    xh = cl(x).to(dev).to(dtype).requires_grad_(True)
    yh = ops.MaxPoolFn.apply(xh, k, s, p, ceil_mode)
    assert torch.equal(cf(yh.detach().float().cpu()), y.detach())
    yh.backward(cl(gy).to(dev).to(dtype))
    # overlapping windows (3/2/1) add up to 8 gradients per voxel: fp32 summation order vs torch's, one bf16 rounding of the sum otherwise
    assert torch.allclose(cf(xh.grad.float().cpu()), xr.grad, atol=1e-5 if dtype == torch.float32 else 3e-2, rtol=0 if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("cfg", [(3, 2, 1, False, (16, 15, 13)), (2, 2, 0, True, (9, 8, 5)), (3, 1, 1, False, (7, 8, 9)), (3, 2, 1, False, (40, 40, 40))])
@pytest.mark.parametrize("dtype,ch", [(torch.float32, 64), (torch.bfloat16, 64), (torch.bfloat16, 36)])
def test_maxpool_fast_index_arithmetic_is_bit_identical(cfg, dtype, ch, dev):
    """Round 6: the pools' multiply-shift index arithmetic (+ compile-time stride in the backward) against the general kernels: outputs,
    argmax codes (through the backward) and input gradients must be the same bits (two scenes, ragged grids, ceil mode, stride 1 and 2)."""
    from nerf_rpn_amd import lib, ops
    k, s, p, ceil_mode, grid = cfg
    torch.manual_seed(0)
    x = F.relu(torch.randn(2, *grid, ch, device=dev)).to(dtype)
    out = []
    for fast in (1, 0):
        lib.call("set_pool_fast", fast)
        try:
            xh = x.clone().requires_grad_(True)
            yh = ops.MaxPoolFn.apply(xh, k, s, p, ceil_mode)
            gy = torch.randn(yh.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).to(dtype)
            yh.backward(gy)
            out.append((yh.detach().clone(), xh.grad.clone()))
        finally:
            lib.call("set_pool_fast", 1)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("sizes", [((10, 10, 10), (5, 5, 5)), ((40, 40, 40), (20, 20, 20)), ((9, 7, 5), (5, 4, 3))])
@pytest.mark.parametrize("dtype,ch", [(torch.float32, 32), (torch.bfloat16, 256), (torch.bfloat16, 36)])
def test_upsample_add_fast_forms_are_bit_identical(sizes, dtype, ch, dev):
    """Round 6: the top-down add with multiply-shift index arithmetic, and the backward of an exact 2x pyramid step as a direct sum of the 8
    children, against the general kernels (which also serve the non-2x case here): same bits, two scenes."""
    from nerf_rpn_amd import lib, ops
    fine_s, coarse_s = sizes
    torch.manual_seed(0)
    fine, coarse = torch.randn(2, *fine_s, ch, device=dev).to(dtype), torch.randn(2, *coarse_s, ch, device=dev).to(dtype)
    gy = torch.randn(2, *fine_s, ch, device=dev).to(dtype)
    out = []
    for fast in (1, 0):
        lib.call("set_pool_fast", fast)
        try:
            f, c = fine.clone().requires_grad_(True), coarse.clone().requires_grad_(True)
            y = ops.UpsampleAddFn.apply(f * 1.0, c)
            y.backward(gy)
            out.append((y.detach().clone(), c.grad.clone()))
        finally:
            lib.call("set_pool_fast", 1)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("sizes", [((10, 10, 10), (5, 5, 5)), ((9, 7, 5), (5, 4, 3)), ((33, 20, 7), (17, 10, 4))])
def test_upsample_add(sizes, dev):
    from nerf_rpn_amd import ops
    fine_s, coarse_s = sizes
    torch.manual_seed(0)
    fine, coarse = torch.randn(2, 32, *fine_s), torch.randn(2, 32, *coarse_s)
    fr, cr = fine.clone().requires_grad_(True), coarse.clone().requires_grad_(True)
    y = fr + F.interpolate(cr, size=fine_s, mode="nearest")
    gy = torch.randn_like(y)
    y.backward(gy)
    fh = cl(fine).to(dev).requires_grad_(True)
    ch = cl(coarse).to(dev).requires_grad_(True)
    yh = ops.UpsampleAddFn.apply(fh * 1.0, ch)
    assert torch.allclose(cf(yh.detach().cpu()), y.detach(), atol=1e-6)
    yh.backward(cl(gy).to(dev))
    assert torch.allclose(cf(ch.grad.cpu()), cr.grad, atol=1e-5) and torch.allclose(cf(fh.grad.cpu()), fr.grad, atol=1e-6)


def test_layout_roundtrip_and_adamw_smoke(dev):
    """The channels-last round trip, and a three-step smoke check of grad_sumsq + adamw_step against torch.optim.AdamW with
    clip_grad_norm_ (10007 elements: the remainder loop and the scalar tail only; no shadow, no zero_grad, grad_scale 1).  What holds the
    optimiser kernels element by element, at every loop and configuration, is tests/test_gpu_optim_kernels.py."""
    from nerf_rpn_amd import ops
    torch.manual_seed(0)
    x = torch.randn(2, 5, 7, 6, 3)
    c = ops.to_channels_last(x.to(dev), torch.float32)
    assert torch.equal(c.cpu(), cl(x)) and torch.equal(ops.to_channels_first(c).cpu(), x)
    assert torch.equal(ops.to_channels_last(x.to(dev), torch.bfloat16).cpu(), cl(x).bfloat16())
    p = torch.randn(10007)
    g = torch.randn(10007) * 3
    ref = nn.Parameter(p.clone())
    opt = torch.optim.AdamW([ref], lr=3e-4, weight_decay=1e-2)
    ph, m, v = p.to(dev), torch.zeros(10007, device=dev), torch.zeros(10007, device=dev)
    from nerf_rpn_amd import lib
    ss = torch.zeros(lib.query("grad_sumsq_floats"), device=dev)
    for step in (1, 2, 3):
        ref.grad = g.clone() * step
        torch.nn.utils.clip_grad_norm_([ref], 0.1)
        opt.step()
        gh = (g * step).to(dev)
        ops.grad_sumsq(gh, ss)
        ops.adamw_step(ph, gh, m, v, ss, 0.1, 3e-4, (0.9, 0.999), 1e-8, 1e-2, step)
    assert torch.allclose(ph.cpu(), ref.detach(), atol=1e-6)


# (case, forward plan, dgrad plan, wgrad plan): nrpn_conv3d_fwd_plan codes 1 = 256x256 tile, 2 = 256x256 tile on K slices, 0 = 128-row tile, 7 = halo form
BIG_CASES = [((1, (40, 40, 40), 256, 256, 3), 7, 7, 1),      # the dominant launch of the bench step itself: halo form (plan 7) for forward AND dgrad, against
                                                           # torch fp32 on the CPU (it used to meet an independent reference only on <= 8000 voxels)
             ((1, (40, 40, 33), 256, 256, 3), 1, 1, 1),
             # 323 tiles of 256 rows = one round of the chip + 67: the last 67 M tiles run on 3 K slices (conv_tail_split), the first 256 whole --
             # the level-0 maps of the reference's eval benchmark shape (200 x 200 x 130), forward and dgrad
             ((1, (50, 50, 33), 256, 256, 3), 1, 1, 1), ((1, (20, 20, 20), 512, 512, 3), 2, 2, 1), ((1, (20, 20, 20), 256, 512, 3), 2, 3, 1),
             ((1, (24, 20, 18), 320, 256, 3), 0, 2, 1), ((2, (40, 30, 30), 128, 256, 1), 1, 0, 0)]


@pytest.mark.parametrize("case,pf,pd,pw", BIG_CASES)
def test_large_tile_kernels_vs_torch_fp32(case, pf, pd, pw, dev):
    """The kernels that dominate the 160^3 step -- conv_igemm_big_kernel (256x256 tile), its K-sliced form for the 20^3 maps and
    conv_wgrad_big_kernel -- against torch fp32 on the CPU with bf16-rounded operands (fp32 accumulation on both sides):
    forward(+bias+ReLU), dgrad, wgrad and the bias gradient.  The plan queries assert each shape really selects those kernels."""
    from nerf_rpn_amd import lib
    from nerf_rpn_amd.model import hip_nn
    n, grid, cin, cout, k = case
    assert lib.query("conv3d_fwd_plan", n, *grid, cin, cout, k, lib.BF16) == pf
    assert lib.query("conv3d_fwd_plan", n, *grid, cout, cin, k, lib.BF16) == pd
    assert lib.query("conv3d_wgrad_plan", n, *grid, cin, cout, cout, k, lib.BF16) == pw
    torch.manual_seed(1)
    conv = nn.Conv3d(cin, cout, k, padding=k // 2)
    conv.weight.data = conv.weight.data.bfloat16().float()
    x = torch.randn(n, cin, *grid).bfloat16().float()
    gy = (torch.randn(n, cout, *grid) * (torch.rand(n, 1, *grid) < 0.3)).bfloat16().float()
    h = nn.Conv3d(cin, cout, k, padding=k // 2).to(dev)
    h.load_state_dict(conv.state_dict())
    xh = cl(x).to(dev).bfloat16().requires_grad_(True)
    yh = hip_nn.conv3d(h, xh, relu=True)
    yh.backward(cl(gy).to(dev).bfloat16())
    # The ReLU mask is taken from the kernel's own output: an output that is zero to fp32 rounding can land on either side in two
    # summation orders, and ONE flipped mask element moves the 320 weight-gradient entries it touches by ~1 % of max|dw| -- that is a
    # property of ReLU at 0, not of the convolution under test.
    xr = x.clone().requires_grad_(True)
    pre = conv(xr)
    mask = (cf(yh.detach().float().cpu()) > 0).float()
    yr = pre * mask
    assert ((pre.detach() > 0).float() != mask).float().mean().item() < 1e-4       # the masks differ on at most a few near-zero outputs
    yr.backward(gy)
    # y / dx are stored in bf16 (2^-9 relative rounding of each element); dw / db are fp32 sums of bf16 products
    for name, a, b, tol in (("y", cf(yh.detach().float().cpu()), yr.detach(), 1e-2), ("dx", cf(xh.grad.float().cpu()), xr.grad, 1e-2),
                            ("dw", h.weight.grad.cpu(), conv.weight.grad, 2e-3), ("db", h.bias.grad.cpu(), conv.bias.grad, 2e-3)):
        assert relerr(a, b) < tol, (case, name, relerr(a, b))
    # elementwise check of the bf16 outputs: every element within 1.5 bf16 ulps of the fp32 result (+ a small absolute floor)
    yy, rr = cf(yh.detach().float().cpu()), yr.detach()
    assert ((yy - rr).abs() <= 1.2e-2 * rr.abs() + 2e-3 * rr.abs().max()).all()


def test_conv_kernels_are_deterministic(dev):
    """Same inputs twice -> bit-identical y, dx, dw, db for every kernel family (K-sliced small grids, 256x256 tiles, wgrad voxel
    slices, bias partials): no fp32 atomics anywhere on the conv path."""
    from nerf_rpn_amd.model import hip_nn
    for (n, grid, cin, cout, k, dtype) in [(1, (5, 5, 5), 256, 256, 3, torch.bfloat16), (1, (10, 10, 10), 512, 512, 3, torch.bfloat16),
                                           (1, (20, 20, 20), 256, 512, 3, torch.bfloat16), (2, (9, 8, 7), 64, 128, 3, torch.float32),
                                           (1, (5, 5, 5), 512, 256, 1, torch.float32), (1, (40, 40, 20), 256, 256, 3, torch.bfloat16)]:
        torch.manual_seed(3)
        conv = nn.Conv3d(cin, cout, k, padding=k // 2).to(dev)
        x = torch.randn(n, *grid, cin, device=dev).to(dtype)
        gy = torch.randn(n, *grid, cout, device=dev).to(dtype)
        outs = []
        for _ in range(2):
            conv.zero_grad()
            xh = x.clone().requires_grad_(True)
            y = hip_nn.conv3d(conv, xh, relu=True)
            y.backward(gy)
            outs.append((y.detach().clone(), xh.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone()))
        for a, b in zip(*outs):
            assert torch.equal(a, b), (grid, cin, cout, k, dtype)
    torch.manual_seed(4)
    st = nn.Conv3d(4, 64, 7, stride=2, padding=3).to(dev)
    x = torch.rand(1, 48, 40, 36, 4, device=dev)
    gy = torch.randn(1, 24, 20, 18, 64, device=dev)
    outs = []
    for _ in range(2):
        st.zero_grad()
        hip_nn.conv3d(st, x).backward(gy)
        outs.append((st.weight.grad.clone(), st.bias.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_grad_sumsq_is_deterministic_and_exact(dev):
    from nerf_rpn_amd import lib, ops
    torch.manual_seed(5)
    for count in (3, 1000, 74_815_925):
        g = torch.randn(count, device=dev) * 1e-3
        a = torch.zeros(lib.query("grad_sumsq_floats"), device=dev)
        b = torch.zeros_like(a)
        ops.grad_sumsq(g, a, 0.5)
        ops.grad_sumsq(g, b, 0.5)
        assert a[0].item() == b[0].item()
        ref = (g.double() * 0.5).pow(2).sum().item()
        assert abs(a[0].item() - ref) <= 2e-6 * ref, (count, a[0].item(), ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("grids,cin,cout", [([(6, 5, 4), (3, 3, 2), (9, 2, 1), (1, 1, 1)], 64, 128), ([(12, 10, 9), (6, 5, 5), (3, 3, 3)], 256, 256),
                                            ([(40, 40, 36), (20, 20, 18), (10, 10, 9), (5, 5, 5)], 256, 256)])
def test_ragged_conv_equals_per_grid_convs(grids, cin, cout, dtype, dev):
    """A weight-sharing 3x3x3 conv over several grids laid end to end in ONE launch (ragged voxel list: per-row grid geometry in the
    implicit-GEMM loaders, segment ids in the wgrad tap masks) == the same conv run grid by grid: forward, dgrad, wgrad, bias."""
    from nerf_rpn_amd.model import hip_nn
    torch.manual_seed(2)
    n = 2 if grids[0][0] < 20 else 1
    conv = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
    feats = [torch.randn(n, *g, cin, device=dev).to(dtype) for g in grids]
    gys = [(torch.randn(n, *g, cout, device=dev) * (torch.rand(n, *g, 1, device=dev) < 0.5)).to(dtype) for g in grids]
    xs = [f.clone().requires_grad_(True) for f in feats]
    ys = [hip_nn.conv3d(conv, x, relu=True) for x in xs]
    torch.autograd.backward(ys, gys)
    ref = ([y.detach().float() for y in ys], [x.grad.float() for x in xs], conv.weight.grad.clone(), conv.bias.grad.clone())
    conv.zero_grad()
    xr = [f.clone().requires_grad_(True) for f in feats]
    rag, segs = hip_nn.ragged_cat(xr)
    assert len(segs) == n * len(grids)
    yr = hip_nn.ragged_split(hip_nn.conv3d(conv, rag, relu=True, segs=segs), feats)
    torch.autograd.backward(yr, gys)
    tol = 1e-5 if dtype == torch.float32 else 2e-2       # bf16: the per-grid launches may run another kernel (halo form) than the ragged one --
    for a, b in zip(yr, ref[0]):                         # another fp32 summation order, then one bf16 rounding
        assert a.shape == b.shape and relerr(a.detach().float().cpu(), b.cpu()) < tol
    for x, b in zip(xr, ref[1]):
        assert relerr(x.grad.float().cpu(), b.cpu()) < tol
    # bf16: where the two paths run different kernels, outputs that round to either side of zero flip their ReLU mask in the backward
    assert relerr(conv.weight.grad.cpu(), ref[2].cpu()) < (1e-5 if dtype == torch.float32 else 2e-2)
    assert relerr(conv.bias.grad.cpu(), ref[3].cpu()) < (1e-5 if dtype == torch.float32 else 2e-2)


def test_ragged_conv_under_bf16x3_keeps_its_gradients(dev):
    """with the bf16x3 mode raised, a DIFFERENTIATED ragged conv must not take the split-operand path (its dgrad / wgrad
    launches know no segments: the ragged list would be read as one dense grid) -- the decision is made from the operands' requires_grad,
    not from grad mode (always off inside autograd.Function.forward).  Gradients must equal the fp32 ragged path's; without autograd the
    ragged forward may use the split operands and must agree with fp32 to the mode's tolerance.  (That the no_grad leg really runs the
    split operands -- the decision follows grad mode, passed in by hip_nn.conv3d -- is proved on exactly summable data by
    test_gpu_conv_exact.py::test_ragged_bf16x3_follows_grad_mode.)"""
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model import hip_nn
    torch.manual_seed(4)
    grids, cin, cout = [(12, 10, 9), (6, 5, 5), (3, 3, 3)], 256, 256
    conv = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
    feats = [torch.randn(1, *g, cin, device=dev) for g in grids]
    gys = [torch.randn(1, *g, cout, device=dev) for g in grids]

    def run():
        conv.zero_grad()
        xr = [f.clone().requires_grad_(True) for f in feats]
        rag, segs = hip_nn.ragged_cat(xr)
        yr = hip_nn.ragged_split(hip_nn.conv3d(conv, rag, relu=True, segs=segs), feats)
        torch.autograd.backward(yr, gys)
        return [y.detach().clone() for y in yr], [x.grad.clone() for x in xr], conv.weight.grad.clone(), conv.bias.grad.clone()
    ref = run()
    ops.SPLIT3[0] = True
    try:
        got = run()
        with torch.no_grad():
            rag, segs = hip_nn.ragged_cat(feats)
            y_ng = hip_nn.ragged_split(hip_nn.conv3d(conv, rag, relu=True, segs=segs), feats)
    finally:
        ops.SPLIT3[0] = False
    for a, b in zip(got[0] + got[1] + [got[2], got[3]], ref[0] + ref[1] + [ref[2], ref[3]]):
        assert torch.equal(a, b)                  # the differentiated ragged conv ran the fp32 kernels: same bits
    for a, b in zip(y_ng, ref[0]):
        assert relerr(a.cpu(), b.cpu()) < 2e-5


@pytest.mark.parametrize("cin,cout,grid,rows_expected", [
    (64, 64, (1, 40, 40, 21), True),       # 128-row kernel, 64-column tiles (four row groups per tile), ragged last tile
    (128, 128, (2, 30, 30, 21), True),     # 128-row kernel, 128-column tiles, two scenes, ragged last tile
    (256, 256, (1, 40, 40, 33), True),     # 256x256 kernel (>= 200 tiles), ragged last tile
    (512, 512, (1, 20, 20, 20), False),    # K-sliced: no fused statistics, the holder stays empty
])
def test_batchnorm_statistics_from_the_conv_epilogue(cin, cout, grid, rows_expected, dev):
    """conv -> BatchNorm3d (training): the conv launch leaves per-row-group (sum, sum of squares) of its STORED bf16 outputs
    (nrpn_conv3d_fwd_stats) and BatchNorm only finishes them.  Output, batch statistics, running statistics and the gradients must
    match the two-kernel statistics pass (nrpn_bn_stats) on the same conv output."""
    from nerf_rpn_amd import lib, ops
    from nerf_rpn_amd.model import hip_nn
    n, gx, gy, gz = grid
    rows = lib.query("conv3d_fwd_stats_rows", n, gx, gy, gz, cin, cout, 3, lib.BF16)
    assert (rows > 0) == rows_expected, rows
    torch.manual_seed(cin + gx)
    conv = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
    bn = nn.BatchNorm3d(cout).to(dev)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.3, 0.3)
        conv.bias.uniform_(-0.5, 0.5)
    x = torch.randn(n, gx, gy, gz, cin, device=dev).bfloat16()
    out = {}
    for fused in (True, False):
        bn.running_mean.zero_()
        bn.running_var.fill_(1.0)
        xi = x.clone().requires_grad_(True)
        holder = {} if fused else None
        y = hip_nn.conv3d(conv, xi, stats=holder)
        assert (fused and rows_expected) == bool(holder)                 # the fused path really ran (or really did not)
        if holder:
            assert tuple(holder["partials"].shape) == (rows, 2, cout)
        z = hip_nn.batch_norm(bn, y, True, stats=holder)
        (z.float() * torch.linspace(0.5, 1.5, cout, device=dev)).sum().backward()
        out[fused] = (y.detach().clone(), z.detach().clone(), bn.running_mean.clone(), bn.running_var.clone(), xi.grad.clone(),
                      conv.weight.grad.clone(), bn.weight.grad.clone())
        conv.zero_grad(); bn.zero_grad()
    assert torch.equal(out[True][0], out[False][0])                       # the conv output itself is unchanged
    for a, b, tol in zip(out[True][2:4], out[False][2:4], (1e-6, 1e-6)):
        assert torch.allclose(a, b, rtol=1e-5, atol=tol), (a - b).abs().max()
    zerr = (out[True][1].float() - out[False][1].float()).abs().max().item()
    assert zerr <= 2 ** -6, zerr                                          # at most one bf16 ulp of an O(1) value where the statistics differ in the last bit
    for a, b in zip(out[True][4:], out[False][4:]):
        scale = b.float().abs().max().item() + 1e-12
        assert (a.float() - b.float()).abs().max().item() <= 2e-2 * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,cout,grid,k", [
    (64, 64, (2, 9, 8, 7), 3),          # 128-row kernel, 64-column tiles
    (128, 256, (1, 12, 10, 9), 3),      # 128-row kernel on K slices (small grid): the fold lives in splitk_epilogue_kernel
    (256, 256, (1, 40, 40, 33), 3),     # 256x256 kernel (bf16) / 128-row kernel (fp32)
    (512, 512, (1, 20, 20, 20), 3),     # 256x256 kernel on K slices (bf16)
    (128, 256, (1, 20, 16, 10), 1),     # 1x1x1 lateral
])
def test_eval_batchnorm_folded_into_the_conv_epilogue(cin, cout, grid, k, dtype, dev):
    """eval mode: conv -> BatchNorm3d -> ReLU runs as ONE launch (per-channel scale + shift + ReLU in the conv epilogue,
    nrpn_conv_opts.scale) and must match torch's conv -> batch_norm(running statistics) -> relu (reference feature_extractor.py:345-358)."""
    from nerf_rpn_amd.model import hip_nn
    n, gx, gy, gz = grid
    torch.manual_seed(cin + gx + k)
    conv = nn.Conv3d(cin, cout, k, padding=k // 2)
    bn = nn.BatchNorm3d(cout)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3); bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5)
        conv.bias.uniform_(-0.5, 0.5)
        conv.weight.mul_(3.0)
    x = torch.randn(n, cin, gx, gy, gz)
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
        conv.weight.data = conv.weight.data.bfloat16().float()
    seq = nn.Sequential(conv, bn, nn.ReLU()).eval()
    with torch.no_grad():
        ref = seq(x)
    hseq = nn.Sequential(nn.Conv3d(cin, cout, k, padding=k // 2), nn.BatchNorm3d(cout), nn.ReLU()).to(dev).eval()
    hseq.load_state_dict(seq.state_dict())
    xh = cl(x).to(dev).to(dtype)
    with torch.no_grad():
        folded = hip_nn.run_modules(hseq, xh)
        hip_nn.FOLD_EVAL_BN = False
        try:
            separate = hip_nn.run_modules(hseq, xh)
        finally:
            hip_nn.FOLD_EVAL_BN = True
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    assert relerr(cf(folded.float().cpu()), ref) < tol
    # the fold rounds once (fp32 affine on the accumulator) where the two-kernel path rounds the conv output to bf16 first: it is at
    # least as close to the fp32 reference as the separate path
    if dtype == torch.bfloat16:
        assert relerr(cf(folded.float().cpu()), ref) <= relerr(cf(separate.float().cpu()), ref) * 1.05 + 1e-4
    # a second forward reuses the cached (scale, shift): no change; an in-place parameter update invalidates the cache
    with torch.no_grad():
        again = hip_nn.run_modules(hseq, xh)
        assert torch.equal(again, folded)
        hseq[1].running_mean.add_(0.25)
        moved = hip_nn.run_modules(hseq, xh)
    assert not torch.equal(moved, folded)


def test_eval_stem_with_folded_batchnorm(dev):
    from nerf_rpn_amd.model import hip_nn
    torch.manual_seed(4)
    for dtype, grid in ((torch.bfloat16, (34, 26, 20)), (torch.float32, (18, 15, 12)), (torch.bfloat16, (17, 15, 13))):      # halo kernel / im2col kernels
        conv, bn = nn.Conv3d(4, 64, 7, stride=2, padding=3), nn.BatchNorm3d(64)
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3); bn.running_mean.normal_(0, 0.2); bn.running_var.uniform_(0.5, 1.5)
        x = torch.rand(2, 4, *grid)
        if dtype == torch.bfloat16:
            x = x.bfloat16().float()
            conv.weight.data = conv.weight.data.bfloat16().float()
        seq = nn.Sequential(conv, bn, nn.ReLU()).eval()
        with torch.no_grad():
            ref = seq(x)
        hseq = nn.Sequential(nn.Conv3d(4, 64, 7, stride=2, padding=3), nn.BatchNorm3d(64), nn.ReLU()).to(dev).eval()
        hseq.load_state_dict(seq.state_dict())
        with torch.no_grad():
            got = hip_nn.run_modules(hseq, cl(x).to(dev).to(dtype))
        assert relerr(cf(got.float().cpu()), ref) < (2e-5 if dtype == torch.float32 else 2e-2), (dtype, grid)


def test_stem_halo_kernel_on_a_multi_tile_grid(dev):
    """bf16 stem forward (halo form: 4x4x16 output blocks, input halo staged once in LDS) on a grid with several tiles per axis and
    ragged last tiles, two scenes; against torch fp32 on bf16-rounded operands and against the im2col kernel it replaces."""
    from nerf_rpn_amd import lib, ops
    from nerf_rpn_amd.model import hip_nn
    torch.manual_seed(9)
    grid = (70, 44, 72)                           # output 35 x 22 x 36: 9 x 6 x 3 tiles, ragged in every axis
    assert lib.query("stem_halo_supported", grid[2], 64, 2, lib.BF16) == 1
    conv = nn.Conv3d(4, 64, 7, stride=2, padding=3)
    conv.weight.data = conv.weight.data.bfloat16().float()
    x = torch.rand(2, 4, *grid).bfloat16().float()
    with torch.no_grad():
        ref = conv(x)
    h = nn.Conv3d(4, 64, 7, stride=2, padding=3).to(dev)
    h.load_state_dict(conv.state_dict())
    xh = cl(x).to(dev).bfloat16()
    with torch.no_grad():
        got = hip_nn.conv3d(h, xh)
        ops.STEM_HALO[0] = False
        try:
            old = hip_nn.conv3d(h, xh)
        finally:
            ops.STEM_HALO[0] = True
    assert relerr(cf(got.float().cpu()), ref) < 1e-2
    assert relerr(got.float().cpu(), old.float().cpu()) < 1e-2


def _conv_case(dev, n, grid, cin, cout, seed=0):
    from nerf_rpn_amd import ops
    torch.manual_seed(seed)
    x = torch.randn(n, *grid, cin, device=dev).bfloat16()
    w = (torch.randn(cout, cin, 3, 3, 3, device=dev) * 0.05)
    wp, _ = ops.PackedWeight().get([w], torch.bfloat16, cout, False)
    bias = torch.randn(cout, device=dev)
    return x, wp, bias


@pytest.mark.parametrize("cin,cout,grid,plan", [(256, 256, (40, 40, 33), 5), (512, 512, (20, 20, 20), 6), (256, 512, (40, 30, 32), 5)])
def test_four_wave_256x256_kernel_is_bit_identical_to_the_eight_wave_kernel(cin, cout, grid, plan, dev):
    """conv_igemm_big4_kernel (4 waves x 128x128, selected per call through nrpn_conv_opts.tile) keeps the per-accumulator MFMA order of
    conv_igemm_big_kernel: outputs, ReLU-masked outputs and the BatchNorm statistics partials must be EQUAL, also on K slices."""
    from nerf_rpn_amd import lib, ops
    x, wp, bias = _conv_case(dev, 1, grid, cin, cout)
    o4 = lib.ConvOpts(tile=lib.TILE_256X256_W4)
    assert lib.query("conv3d_fwd_plan_ex", 1, *grid, cin, cout, 3, lib.BF16, o4.ptr()) == plan
    o8 = lib.ConvOpts(tile=lib.TILE_256X256)
    assert lib.query("conv3d_fwd_plan_ex", 1, *grid, cin, cout, 3, lib.BF16, o8.ptr()) == plan - 4
    scale = torch.rand(cout, device=dev) + 0.5
    mask = torch.randn(1, *grid, cout, device=dev).bfloat16()
    for kw in (dict(), dict(scale=scale), dict(mask=mask)):
        a = ops._conv_fwd(x, wp, bias, cout, cout, 3, lib.CONV_RELU if "mask" not in kw else 0, torch.bfloat16, tile=lib.TILE_256X256, **kw)
        b = ops._conv_fwd(x, wp, bias, cout, cout, 3, lib.CONV_RELU if "mask" not in kw else 0, torch.bfloat16, tile=lib.TILE_256X256_W4, **kw)
        assert torch.equal(a, b), (kw.keys(), (a.float() - b.float()).abs().max().item())
    if plan == 5:
        sa, sb = {}, {}
        ops._conv_fwd(x, wp, bias, cout, cout, 3, 0, torch.bfloat16, stats=sa, tile=lib.TILE_256X256)
        ops._conv_fwd(x, wp, bias, cout, cout, 3, 0, torch.bfloat16, stats=sb, tile=lib.TILE_256X256_W4)
        assert sa["partials"].shape == sb["partials"].shape
        # same values summed over the same 128 rows per partial row, in a different order inside a lane: fp32 rounding only
        assert torch.allclose(sa["partials"], sb["partials"], rtol=1e-5, atol=1e-3)
    f4 = ops._conv_fwd(x, wp, bias, cout, cout, 3, 0, torch.float32, tile=lib.TILE_256X256_W4)
    f8 = ops._conv_fwd(x, wp, bias, cout, cout, 3, 0, torch.float32, tile=lib.TILE_256X256)
    assert torch.equal(f4, f8)


def test_two_threads_with_different_plans_share_no_state(dev):
    """no global state except what the caller passes.  Two host threads launch the same conv on their own streams with
    DIFFERENT per-call plans (nrpn_conv_opts.tile) at the same time, many times; every result must equal the single-threaded one
    of its own plan (the process-wide nrpn_set_* knobs are never touched)."""
    import threading
    from nerf_rpn_amd import lib, ops
    grid, cin, cout = (40, 40, 33), 256, 256
    x, wp, bias = _conv_case(dev, 1, grid, cin, cout, seed=3)
    tiles = [lib.TILE_128, lib.TILE_256X256_W4]
    want = [ops._conv_fwd(x, wp, bias, cout, cout, 3, lib.CONV_RELU, torch.bfloat16, tile=t) for t in tiles]
    opts = [lib.ConvOpts(tile=t) for t in tiles]           # keep the structs alive while the library reads them
    plans = [lib.query("conv3d_fwd_plan_ex", 1, *grid, cin, cout, 3, lib.BF16, o.ptr()) for o in opts]
    assert plans == [0, 5]
    torch.cuda.synchronize()
    errors = []

    def worker(i):
        try:
            st = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(st):
                for _ in range(20):
                    y = ops._conv_fwd(x, wp, bias, cout, cout, 3, lib.CONV_RELU, torch.bfloat16, tile=tiles[i])
                    if not torch.equal(y, want[i]):
                        errors.append((i, "mismatch"))
            st.synchronize()
        except Exception as e:          # noqa: BLE001
            errors.append((i, repr(e)))
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("n,grid,cin,cout", [(1, (40, 40, 40), 256, 256), (1, (37, 42, 29), 128, 256), (2, (12, 16, 19), 384, 512), (1, (9, 8, 8), 128, 264)])
def test_halo_kernel_cross_chunk_tap_pairing_and_fp32_rows(n, grid, cin, cout, dev):
    """Round 5: (a) nrpn_conv_opts.halo_pairing = 1 pairs the taps of the halo kernel across channel-chunk boundaries (54 full K-steps per four
    chunks instead of 4 x 14 with a half-empty one).  Every accumulator still meets the (chunk, tap, channel half) products in the same order,
    so the outputs must be BIT-IDENTICAL to the classic K order -- plain, with scale / mask, and the statistics partials.  (b) the fp32-row
    epilogue (NRPN_CONV_OUT_F32 on the halo form, used by the bf16x3 parity mode): rounded to bf16 it is the bf16 output exactly, and it
    agrees with the 128-row kernel's fp32 rows to fp32 summation-order error."""
    from nerf_rpn_amd import lib, ops
    x, wp, bias = _conv_case(dev, n, grid, cin, cout, seed=cin + grid[0])
    scale = torch.rand(cout, device=dev) + 0.5
    mask = torch.randn(n, *grid, cout, device=dev).bfloat16()
    for kw in (dict(), dict(scale=scale), dict(mask=mask)):
        flags = lib.CONV_RELU if "mask" not in kw else 0
        a = ops._conv_fwd(x, wp, bias, cout, cout, 3, flags, torch.bfloat16, tile=lib.TILE_HALO, halo_pairing=2, **kw)
        b = ops._conv_fwd(x, wp, bias, cout, cout, 3, flags, torch.bfloat16, tile=lib.TILE_HALO, halo_pairing=1, **kw)
        assert torch.equal(a, b), (list(kw), (a.float() - b.float()).abs().max().item())
    sa, sb = {}, {}
    ya = ops._conv_fwd(x, wp, bias, cout, cout, 3, 0, torch.bfloat16, stats=sa, tile=lib.TILE_HALO, halo_pairing=2)
    yb = ops._conv_fwd(x, wp, bias, cout, cout, 3, 0, torch.bfloat16, stats=sb, tile=lib.TILE_HALO, halo_pairing=1)
    assert torch.equal(ya, yb) and torch.equal(sa["partials"], sb["partials"])
    for pairing in (2, 1):
        for kw in (dict(), dict(scale=scale)):
            f = ops._conv_fwd(x, wp, bias, cout, cout, 3, lib.CONV_RELU, torch.float32, tile=lib.TILE_HALO, halo_pairing=pairing, **kw)
            h = ops._conv_fwd(x, wp, bias, cout, cout, 3, lib.CONV_RELU, torch.bfloat16, tile=lib.TILE_HALO, halo_pairing=pairing, **kw)
            assert f.dtype == torch.float32 and torch.equal(f.bfloat16(), h), (pairing, list(kw))
            g = ops._conv_fwd(x, wp, bias, cout, cout, 3, lib.CONV_RELU, torch.float32, tile=lib.TILE_128, **kw)
            assert (f - g).abs().max().item() <= 2e-5 * g.abs().max().item() + 1e-6, (pairing, (f - g).abs().max().item(), g.abs().max().item())


@pytest.mark.parametrize("n,grid,cin,cout", [(1, (40, 40, 40), 256, 256), (1, (37, 42, 29), 256, 256), (2, (12, 16, 19), 128, 512), (1, (9, 8, 8), 64, 264)])
def test_halo_form_of_the_3x3x3_kernel(n, grid, cin, cout, dev):
    """conv_halo_kernel (4 x 8 x 8 voxel blocks, input halo staged once per 32-channel chunk, slot-major LDS tiles; nrpn_conv_opts.tile =
    NRPN_TILE_HALO) against the default kernel of the shape and against torch fp32 on the bf16-rounded operands: exact grids, ragged
    blocks in every axis, two scenes, a Cout that is not a multiple of the 256-column tile; bias / scale / ReLU / ReLU mask /
    BatchNorm statistics partials."""
    from nerf_rpn_amd import lib, ops
    x, wp, bias = _conv_case(dev, n, grid, cin, cout, seed=cin + grid[0])
    oh = lib.ConvOpts(tile=lib.TILE_HALO)
    assert lib.query("conv3d_fwd_plan_ex", n, *grid, cin, cout, 3, lib.BF16, oh.ptr()) == 7
    scale = torch.rand(cout, device=dev) + 0.5
    mask = torch.randn(n, *grid, cout, device=dev).bfloat16()
    for kw in (dict(), dict(scale=scale), dict(mask=mask)):
        flags = lib.CONV_RELU if "mask" not in kw else 0
        a = ops._conv_fwd(x, wp, bias, cout, cout, 3, flags, torch.bfloat16, tile=lib.TILE_128, **kw).float()
        b = ops._conv_fwd(x, wp, bias, cout, cout, 3, flags, torch.bfloat16, tile=lib.TILE_HALO, **kw).float()
        # same products, another summation order (chunk-of-32 outer, tap inner): fp32 rounding, then one bf16 rounding of the result
        assert (a - b).abs().max().item() <= 2 ** -7 * a.abs().max().item(), (kw.keys(), (a - b).abs().max().item(), a.abs().max().item())
        assert (a != b).float().mean().item() < 0.02
    rows = lib.query("conv3d_fwd_stats_rows_ex", n, *grid, cin, cout, 3, lib.BF16, oh.ptr())
    assert rows == 2 * n * -(-grid[0] // 4) * -(-grid[1] // 8) * -(-grid[2] // 8)
    st = {}
    y = ops._conv_fwd(x, wp, bias, cout, cout, 3, 0, torch.bfloat16, stats=st, tile=lib.TILE_HALO).float()
    part = st["partials"]
    assert tuple(part.shape) == (rows, 2, cout)
    flat = y.reshape(-1, cout)
    assert torch.allclose(part[:, 0].sum(0), flat.sum(0), rtol=1e-4, atol=1e-2 * flat.abs().max().item())
    assert torch.allclose(part[:, 1].sum(0), (flat * flat).sum(0), rtol=1e-4, atol=1e-2 * (flat * flat).max().item())
    if grid[0] * grid[1] * grid[2] * n <= 8000:
        w = (torch.randn(cout, cin, 3, 3, 3, device=dev) * 0.05)
        torch.manual_seed(cin + grid[0])
        xx = torch.randn(n, *grid, cin, device=dev).bfloat16()
        ww = (torch.randn(cout, cin, 3, 3, 3, device=dev) * 0.05)
        wpp, _ = ops.PackedWeight().get([ww], torch.bfloat16, cout, False)
        got = ops._conv_fwd(xx, wpp, None, cout, cout, 3, 0, torch.bfloat16, tile=lib.TILE_HALO).float().cpu()
        ref = F.conv3d(cf(xx.float().cpu()), ww.bfloat16().float().cpu(), padding=1)
        assert relerr(cf(got), ref) < 1e-2


def test_split_bf16x3_operands(dev):
    """nrpn_split_bf16x3: hi = bf16(x), lo = bf16(x - hi); hi + lo reproduces x to 2^-16 relative; the interleaved segments and the planes hold
    hi / lo where the pattern bits say."""
    from nerf_rpn_amd import ops
    torch.manual_seed(3)
    x = (torch.randn(5, 7, 64, device=dev) * torch.logspace(-6, 6, 64, device=dev)).contiguous()
    inter, planes = ops.split3(x, 0b100, 3, 0b010)
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    assert inter.shape == (5, 7, 192) and planes.shape == (3, 5, 7, 64)
    assert torch.equal(inter[..., :64], hi) and torch.equal(inter[..., 64:128], hi) and torch.equal(inter[..., 128:], lo)
    assert torch.equal(planes[0], hi) and torch.equal(planes[1], lo) and torch.equal(planes[2], hi)
    rec = hi.double() + lo.double()
    assert ((rec - x.double()).abs() <= 2.0 ** -16 * x.double().abs()).all()
    only_planes = ops.split3(x, None, 2, 0b10)
    assert only_planes[0] is None and torch.equal(only_planes[1][0], hi) and torch.equal(only_planes[1][1], lo)


@pytest.mark.parametrize("n,grid,cin,cout,relu", [(2, (7, 6, 5), 64, 96, True), (1, (5, 5, 5), 128, 256, False), (1, (12, 16, 19), 256, 256, True),
                                                  (1, (20, 20, 20), 256, 512, True)])
def test_bf16x3_conv_is_fp32_grade(n, grid, cin, cout, relu, dev):
    """The bf16x3 mode (ops.SPLIT3) of ConvFn -- forward, input gradient, weight gradient (three planes on the batch axis), bias gradient (fp32
    column sums) -- against torch fp32 on the CPU at the tolerance the exact-fp32 MFMA kernels are held to (test_conv_forward_backward: 2e-5
    of the tensor's maximum; 3e-5 here: the dropped lo*lo term adds 2^-16 per product to the fp32 accumulation error), and against the
    HIP fp32 kernels themselves.  Shapes: 64-column / 128-row tiles, the K-sliced 256x256 tile (20^3), a ragged small grid."""
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model import hip_nn
    torch.manual_seed(cin + cout)
    conv = nn.Conv3d(cin, cout, 3, padding=1)
    x = torch.randn(n, cin, *grid)
    xr = x.clone().requires_grad_(True)
    pre = conv(xr)
    yr = F.relu(pre) if relu else pre
    gy = torch.randn_like(yr)
    if relu:
        # a pre-activation within 1e-5 of zero may come out on the other side of the ReLU in another arithmetic -- ONE such routing flip moves
        # 27 * Cin entries of dx by |gy * w| ~ 1e-2 of the tensor's maximum (first version of this test: 1.5e-2 on dx with y equal to 4e-6).
        # The incoming gradient is therefore zero wherever the ReLU's decision is not safe: the kernels are compared on identical routing.
        gy = gy * (pre.detach().abs() > 1e-3 * pre.detach().abs().max())
    yr.backward(gy)
    ref = dict(y=yr.detach(), dx=xr.grad, dw=conv.weight.grad.clone(), db=conv.bias.grad.clone())
    out = {}
    for mode in (False, True):
        h = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
        h.load_state_dict(conv.state_dict())
        xh = cl(x).to(dev).requires_grad_(True)
        ops.SPLIT3[0] = mode
        try:
            yh = hip_nn.conv3d(h, xh, relu=relu)
            yh.backward(cl(gy).to(dev))
            torch.cuda.synchronize()
        finally:
            ops.SPLIT3[0] = False
        assert yh.dtype == torch.float32 and xh.grad.dtype == torch.float32
        out[mode] = dict(y=cf(yh.detach().cpu()), dx=cf(xh.grad.cpu()), dw=h.weight.grad.cpu(), db=h.bias.grad.cpu())
    for k in ("y", "dx", "dw", "db"):
        e32, e3, e = relerr(out[False][k], ref[k]), relerr(out[True][k], ref[k]), relerr(out[True][k], out[False][k])
        print(f"[bf16x3] {cin}->{cout}@{grid} {k}: fp32 kernel {e32:.2e}, bf16x3 {e3:.2e} vs torch fp32; bf16x3 vs fp32 kernel {e:.2e}")
        assert e3 < 3e-5, (k, e3, e32)
        assert e < 3e-5, (k, e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,grid,cin,cout", [(1, (12, 10, 9), 64, 64), (2, (9, 8, 7), 64, 128), (1, (8, 8, 6), 32, 96), (1, (24, 22, 20), 128, 256),
                                             (2, (20, 16, 17), 128, 320)])
def test_wgrad_two_taps_per_workgroup(n, grid, cin, cout, dtype, dev):
    """conv_wgrad_kernel<..., PACK2> (round 5): dense 3x3x3 layers with Cin <= 64 -- a workgroup owns a PAIR of taps, the B tile holds
    [tap 2t | tap 2t + 1], 14 workgroups per (tile, slice), the 27th tap's partner absent -- and conv_wgrad_big_kernel<false, PACK2> for bf16
    layers with Cin == 128, Cout >= 256 (the two 128-channel B sub-tiles = the two taps of a pair; nrpn_conv3d_wgrad_plan says 256x256).  Weight and bias gradients against torch fp32 on the
    CPU (the tolerance of test_conv_forward_backward) and against the one-tap-per-workgroup form of the same kernel (nrpn_set_wgrad_pack2(0)):
    the same products in another slice grouping."""
    from nerf_rpn_amd import lib
    from nerf_rpn_amd.model import hip_nn
    if dtype == torch.bfloat16 and (cin * 2) % 64:
        pytest.skip("Cin*2 must be a multiple of 64 bytes")
    torch.manual_seed(cin + cout)
    conv = nn.Conv3d(cin, cout, 3, padding=1)
    x = torch.randn(n, cin, *grid)
    if dtype == torch.bfloat16:
        x = x.bfloat16().float()
        conv.weight.data = conv.weight.data.bfloat16().float()
    y = conv(x)
    gy = torch.randn_like(y)
    if dtype == torch.bfloat16:
        gy = gy.bfloat16().float()
    y.backward(gy)
    got = {}
    code = lib.BF16 if dtype == torch.bfloat16 else lib.F32
    if cin == 128:
        assert lib.query("conv3d_wgrad_plan", n, *grid, cin, cout, cout, 3, code) == (1 if dtype == torch.bfloat16 else 0)
    try:
        for on in (1, 0):
            lib.call("set_wgrad_pack2", on)
            h = nn.Conv3d(cin, cout, 3, padding=1).to(dev)
            h.load_state_dict(conv.state_dict())
            hip_nn.conv3d(h, cl(x).to(dev).to(dtype)).backward(cl(gy).to(dev).to(dtype))
            torch.cuda.synchronize()
            got[on] = (h.weight.grad.cpu(), h.bias.grad.cpu())
    finally:
        lib.call("set_wgrad_pack2", 1)
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    for on in (1, 0):
        assert relerr(got[on][0], conv.weight.grad) < tol and relerr(got[on][1], conv.bias.grad) < tol, (on, relerr(got[on][0], conv.weight.grad))
    assert relerr(got[1][0], got[0][0]) < 2e-5 and relerr(got[1][1], got[0][1]) < 2e-5


@pytest.mark.parametrize("sunk", ["weight", "bias"])
def test_conv_with_an_incomplete_set_of_sinks(sunk, dev):
    """ConvFn k3 fp32 on a (1, 6, 5, 4) grid, Cin = Cout = 32, with a GradSink (zero-filled slot) on ONE of its two parameters: that
    gradient lands in the slot and its position in the returned tuple is None, the other one is handed back, both bit-equal to the
    gradients of the same call without sinks -- and no launch leaves the main stream (the side stream is for layers whose gradients ALL
    have sinks)."""
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model import hip_nn
    from step_trace import Recorder
    torch.manual_seed(5)
    conv = nn.Conv3d(32, 32, 3, padding=1).to(dev)
    x = torch.randn(1, 6, 5, 4, 32, device=dev, requires_grad=True)
    dy = torch.randn(1, 6, 5, 4, 32, device=dev)
    assert ops._WGRAD_SIDE["enabled"]

    def grads():
        y = ops.ConvFn.apply(x, hip_nn._pack_of(conv), 32, False, False, 1, conv.weight, conv.bias)
        return torch.autograd.grad(y, [x, conv.weight, conv.bias], dy, allow_unused=True)
    _, gw, gb = grads()
    param = conv.weight if sunk == "weight" else conv.bias
    slot = torch.zeros_like(param, dtype=torch.float32)
    param._nrpn_sink = ops.GradSink(slot, lambda: None)
    try:
        with Recorder(ops) as rec:
            rec.on = True
            _, sw, sb = grads()
        torch.cuda.synchronize()
    finally:
        del param._nrpn_sink
    launches = [e for e in rec.trace if not e[0].startswith("py:")]
    assert any(e[0] == "conv3d_wgrad" for e in launches) and all(e[1][-1] == 0 for e in launches), launches
    if sunk == "weight":
        assert sw is None and torch.equal(slot, gw) and torch.equal(sb, gb)
    else:
        assert sb is None and torch.equal(slot, gb) and torch.equal(sw, gw)
