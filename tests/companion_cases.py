"""The cases behind tests/golden/companion_digests.json: every HBM-bound companion kernel (csrc/elementwise.hip, swin.hip, fcos.hip,
roialign.hip) on the smallest shapes that reach every channel width and index form, digested output by output.

tools/record_companion_digests.py records the digests from a build of the commit BEFORE a change to those kernels;
tests/test_gpu_companion_bits.py reproduces them with the in-tree library.

Shapes.  Two scenes on a (9, 7, 5) grid (odd, no multiple of anything, 630 voxels: three 256-lane blocks), (10, 10, 10) over (5, 5, 5)
where an exact 2x pair is needed.  C = 36 in bf16 and fp32 takes 4 channels per lane (36 % 8 != 0), C = 64 in bf16 takes 8; GroupNorm runs
on C = 32 with 4 groups (8 channels per group: the 8-wide form) and 8 groups (the general form).  The BatchNorm statistics and backward
accept C only when min(C, 1024) / 4 divides 256, which 36 does not: they run on C = 4 (4 per lane in both dtypes) and C = 64, and
bn_apply, which has no such rule, on C = 36 as well.  Two BatchNorm cases are long (BN_LONG): the only path a small shape cannot reach.

Values.  Seeded normal data from numpy's legacy generator (the same stream on every version), post-ReLU where ties decide (pools, ReLU
masks).  A few elements sit exactly on bf16 rounding ties (1 + 2^-8, 1 + 3 * 2^-8, and sums that land there), one is an fp32 denormal,
and the copying / selecting / adding ops (pools, ReLU backward, subsample, residual joins, upsample-add, patch merge) also see one
+inf and one -inf.  The normalisations, GELU and RoIAlign get no infinity: inf - inf and 0 * inf are NaN, and NaN payloads are not part
of what the kernels promise.  No input holds a NaN.

Every case runs under both settings of the pool / BatchNorm fast-path switches (`fast` = 1, 0)."""
import hashlib

import numpy as np
import torch

from nerf_rpn_amd import lib, ops
from nerf_rpn_amd.ops import _dt, _p, _s, call, query

GRID, GRID2, COARSE2 = (9, 7, 5), (10, 10, 10), (5, 5, 5)
WIDTHS = [(36, torch.bfloat16), (36, torch.float32), (64, torch.bfloat16)]
BN_WIDTHS = [(4, torch.bfloat16), (4, torch.float32), (64, torch.bfloat16)]
# rows at which the fast apply kernels' grid-stride loops turn more than twice (their grids stop at 2048 / 1280 blocks of 256 lanes): the
# unrolled loop body and its remainder are code paths the 630-row cases never enter
BN_LONG = [(4, torch.float32, 1_600_000), (64, torch.bfloat16, 200_000)]
TIES = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8))
DENORMAL = 1e-40


def _name(c, dtype):
    return f"c{c}_{'bf16' if dtype == torch.bfloat16 else 'f32'}"


def tensor(seed, shape, dtype, dev, relu=False, inf=False, scale=1.0):
    """Seeded fp32 data with the special values planted at fixed flat positions, then cast to `dtype` (round-to-nearest-even on the host)."""
    a = (np.random.RandomState(seed).standard_normal(int(np.prod(shape))) * scale).astype(np.float32)
    if relu:
        a = np.maximum(a, 0.0)
    n = a.size
    for i, v in enumerate(TIES):
        a[(7 + 13 * i) % n] = abs(v) if relu else v
    a[31 % n] = DENORMAL
    if inf:
        a[43 % n] = np.inf
        a[(n - 5) % n] = 0.0 if relu else -np.inf
        if relu:
            a[59 % n] = -np.inf       # -inf below a ReLU'd neighbourhood: never a maximum unless the window holds nothing else
    return torch.from_numpy(a.reshape(shape)).to(dtype).to(dev)


def digest(t):
    t = t.detach().contiguous().cpu()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def _bn(c, dtype, dev, rows=2 * 9 * 7 * 5):
    x = tensor(1, (rows, c), dtype, dev, scale=2.0)
    dy = tensor(2, (rows, c), dtype, dev)
    gamma = tensor(3, (c,), torch.float32, dev) + 1.5
    beta = tensor(4, (c,), torch.float32, dev) * 0.5
    f32 = dict(dtype=torch.float32, device=dev)
    mean, var = torch.empty(c, **f32), torch.empty(c, **f32)
    rmean, rvar = torch.zeros(c, **f32), torch.ones(c, **f32)
    ws = torch.empty(query("bn_workspace_bytes", rows, c), dtype=torch.uint8, device=dev)
    call("bn_stats", _p(x), rows, c, _dt(x), _p(mean), _p(var), _p(rmean), _p(rvar), 0.1, _p(ws), _s())
    yield "stats", torch.stack([mean, var, rmean, rvar])
    for relu in (0, 1):
        y = torch.empty_like(x)
        call("bn_apply", _p(x), _p(y), rows, c, _dt(x), _p(mean), _p(var), _p(gamma), _p(beta), 1e-5, relu, _s())
        yield f"apply_relu{relu}", y
        for src in (("y", "beta") if relu else ("none",)):      # where the backward takes its ReLU mask from
            dx, dg, db = torch.empty_like(x), torch.empty(c, **f32), torch.empty(c, **f32)
            ag, ab = torch.ones(c, **f32), torch.ones(c, **f32)
            call("bn_backward", _p(x), _p(y) if src == "y" else 0, _p(dy), _p(dx), rows, c, _dt(x), _p(mean), _p(var), _p(gamma),
                 _p(beta) if src == "beta" else 0, 1e-5, relu, _p(dg), _p(db), _p(ag), _p(ab), _p(ws), _s())
            yield f"backward_relu{relu}_mask_{src}", dx
            yield f"backward_relu{relu}_mask_{src}_params", torch.stack([dg, db, ag, ab])


def _bn_apply_only(c, dtype, dev):
    rows = 2 * 9 * 7 * 5
    x = tensor(1, (rows, c), dtype, dev, scale=2.0)
    mean, var = tensor(5, (c,), torch.float32, dev) * 0.1, tensor(6, (c,), torch.float32, dev).abs() + 0.5
    gamma, beta = tensor(3, (c,), torch.float32, dev) + 1.5, tensor(4, (c,), torch.float32, dev) * 0.5
    for relu in (0, 1):
        y = torch.empty_like(x)
        call("bn_apply", _p(x), _p(y), rows, c, _dt(x), _p(mean), _p(var), _p(gamma), _p(beta), 1e-5, relu, _s())
        yield f"apply_relu{relu}", y


def _pool(c, dtype, dev, k, s, p, ceil):
    x = tensor(10, (2,) + GRID + (c,), dtype, dev, relu=True, inf=True)
    o = [query("pool_out_size", g, k, s, p, ceil) for g in GRID]
    y = torch.empty((2, *o, c), dtype=dtype, device=dev)
    arg = torch.empty(y.shape, dtype=torch.int8, device=dev)
    call("maxpool3d_fwd", _p(x), _p(y), _p(arg), 2, *GRID, c, k, s, p, ceil, _dt(x), _s())
    yield "fwd", y
    yield "argmax", arg
    dy = tensor(11, tuple(y.shape), dtype, dev, inf=False)
    dx = torch.empty_like(x)
    call("maxpool3d_bwd", _p(dy), _p(arg), _p(dx), 2, *GRID, c, k, s, p, ceil, _dt(x), _s())
    yield "bwd", dx


def _upsample(c, dtype, dev, fine_shape, coarse_shape):
    fine = tensor(20, (2,) + fine_shape + (c,), dtype, dev, inf=True)
    coarse = tensor(21, (2,) + coarse_shape + (c,), dtype, dev)
    call("upsample_add_fwd", _p(fine), _p(coarse), 2, *fine_shape, *coarse_shape, c, _dt(fine), _s())
    yield "fwd", fine
    d = tensor(22, (2,) + fine_shape + (c,), dtype, dev)
    for acc in (0, 1):
        dc = tensor(23, (2,) + coarse_shape + (c,), dtype, dev)
        call("upsample_add_bwd", _p(d), _p(dc), 2, *fine_shape, *coarse_shape, c, _dt(d), acc, _s())
        yield f"bwd_acc{acc}", dc


def _subsample(c, dtype, dev):
    x = tensor(30, (2,) + GRID + (c,), dtype, dev, inf=True)
    y = ops.SubsampleFn.apply(x, 2)
    yield "fwd", y
    dx = torch.empty_like(x)
    call("subsample3d", _p(y), _p(dx), 2, *GRID, c, 2, 1, _dt(x), _s())
    yield "bwd", dx


def _joins(c, dtype, dev):
    shape = (2,) + GRID + (c,)
    a, b = tensor(40, shape, dtype, dev, inf=True), tensor(41, shape, dtype, dev)
    for i, lo in ((7, 1.0), (20, 1.0 + 2.0 ** -7)):      # bf16 operands whose fp32 sum is a bf16 tie: 1 + 2^-8 (down to even), 1 + 3 * 2^-8 (up)
        a.view(-1)[i], b.view(-1)[i] = lo, 2.0 ** -8
    for relu in (0, 1):
        y = torch.empty_like(a)
        call("add_relu", _p(a), _p(b), _p(y), a.numel(), relu, _dt(a), _s())
        yield f"add_relu{relu}", y
    g = torch.empty_like(a)
    call("relu_backward", _p(a), _p(b), _p(g), a.numel(), _dt(a), _s())
    yield "relu_backward", g
    scale = torch.tensor([0.75, 1.0 / 0.9], dtype=torch.float32, device=dev)
    for sc in (None, scale):
        y = torch.empty_like(a)
        call("scale_add", _p(a), _p(b), _p(sc), _p(y), 2, a[0].numel(), _dt(a), _s())
        yield f"scale_add_{'rows' if sc is not None else 'plain'}", y
    y = torch.empty_like(a)
    call("scale_add", None, _p(b), _p(scale), _p(y), 2, a[0].numel(), _dt(a), _s())
    yield "scale_add_bwd", y


def _gelu(c, dtype, dev):
    x, dy = tensor(50, (2,) + GRID + (c,), dtype, dev, scale=2.0), tensor(51, (2,) + GRID + (c,), dtype, dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    call("gelu", _p(x), None, _p(y), x.numel(), 0, _dt(x), _s())
    call("gelu", _p(x), _p(dy), _p(dx), x.numel(), 1, _dt(x), _s())
    yield "fwd", y
    yield "bwd", dx


def _layernorm(c, dtype, dev):
    x, dy = tensor(60, (2,) + GRID + (c,), dtype, dev, scale=2.0), tensor(61, (2,) + GRID + (c,), dtype, dev)
    gamma, beta = tensor(62, (c,), torch.float32, dev) + 1.5, tensor(63, (c,), torch.float32, dev) * 0.5
    rows = x.numel() // c
    mean, rstd = torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    call("layernorm_fwd", _p(x), _p(y), _p(gamma), _p(beta), _p(mean), _p(rstd), rows, c, 1e-5, _dt(x), _s())
    yield "fwd", y
    yield "fwd_stats", torch.stack([mean, rstd])
    ws = torch.empty(query("layernorm_workspace_bytes", rows, c), dtype=torch.uint8, device=dev)
    dg, db = torch.empty(c, dtype=torch.float32, device=dev), torch.empty(c, dtype=torch.float32, device=dev)
    call("layernorm_bwd", _p(x), _p(dy), _p(dx), _p(gamma), _p(mean), _p(rstd), _p(dg), _p(db), rows, c, _dt(x), 0, _p(ws), _s())
    yield "bwd", dx
    yield "bwd_params", torch.stack([dg, db])


def _groupnorm(dtype, dev, groups, relu):
    c = 32
    x, dy = tensor(70, (2,) + GRID + (c,), dtype, dev, scale=2.0), tensor(71, (2,) + GRID + (c,), dtype, dev)
    gamma, beta = tensor(72, (c,), torch.float32, dev) + 1.5, tensor(73, (c,), torch.float32, dev) * 0.5
    rows = x[0].numel() // c
    f32 = dict(dtype=torch.float32, device=dev)
    mean, rstd = torch.empty(2 * groups, **f32), torch.empty(2 * groups, **f32)
    ws = torch.empty(query("groupnorm_workspace_bytes", 2, c, groups), dtype=torch.uint8, device=dev)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    call("groupnorm_fwd", _p(x), _p(y), _p(gamma), _p(beta), _p(mean), _p(rstd), 2, rows, c, groups, 1e-5, relu, _dt(x), _p(ws), _s())
    yield "fwd", y
    yield "fwd_stats", torch.stack([mean, rstd])
    dg, db = torch.empty(c, **f32), torch.empty(c, **f32)
    call("groupnorm_bwd", _p(x), _p(y), _p(dy), _p(dx), _p(gamma), _p(mean), _p(rstd), _p(dg), _p(db), 2, rows, c, groups, relu, _dt(x), 0,
         _p(ws), _s())
    yield "bwd", dx
    yield "bwd_params", torch.stack([dg, db])


def _patch_merge(c, dtype, dev):
    x = tensor(80, (2,) + GRID + (c,), dtype, dev, inf=True)
    y = ops.PatchMergeFn.apply(x)
    yield "fwd", y
    dx = torch.empty_like(x)
    call("patch_merge", _p(y), _p(dx), 2, *GRID, c, 1, _dt(x), _s())
    yield "bwd", dx


def _roialign(c, dtype, dev):
    feat = tensor(90, (2,) + GRID + (c,), dtype, dev)
    rois = torch.tensor([[0, 4.2, 3.1, 2.4, 5.0, 3.0, 2.5, 0.4], [1, 2.0, 5.5, 1.0, 3.0, 6.0, 4.0, -1.1], [1, 8.5, 0.5, 4.5, 4.0, 2.0, 2.0, 0.0],
                         [0, 4.5, 3.5, 2.5, 9.0, 7.0, 5.0, 1.5707963705062866]], dtype=torch.float32, device=dev)
    out = ops.roi_align_rotated_3d_fwd(feat, rois, 1.0, (3, 2, 2), 2)
    yield "fwd", out
    top = tensor(91, tuple(out.shape), dtype, dev)
    yield "bwd", ops.roi_align_rotated_3d_bwd(top, rois, tuple(feat.shape), 1.0, (3, 2, 2), 2)


def cases():
    """(name, generator function of `dev`), in a fixed order."""
    out = []
    for c, dt in BN_WIDTHS:
        out.append((f"bn_{_name(c, dt)}", lambda dev, c=c, dt=dt: _bn(c, dt, dev)))
    for c, dt, rows in BN_LONG:
        out.append((f"bn_long_{_name(c, dt)}", lambda dev, c=c, dt=dt, rows=rows: _bn(c, dt, dev, rows)))
    for c, dt in WIDTHS:
        n = _name(c, dt)
        out.append((f"bn_apply_{n}", lambda dev, c=c, dt=dt: _bn_apply_only(c, dt, dev)))
        for k, s, p, ceil in ((3, 2, 1, 0), (2, 2, 0, 1), (3, 1, 1, 0)):
            out.append((f"maxpool_{k}{s}{p}_{n}", lambda dev, c=c, dt=dt, a=(k, s, p, ceil): _pool(c, dt, dev, *a)))
        out.append((f"upsample_x2_{n}", lambda dev, c=c, dt=dt: _upsample(c, dt, dev, GRID2, COARSE2)))
        out.append((f"upsample_ragged_{n}", lambda dev, c=c, dt=dt: _upsample(c, dt, dev, GRID, (5, 4, 3))))
        out.append((f"subsample_{n}", lambda dev, c=c, dt=dt: _subsample(c, dt, dev)))
        out.append((f"joins_{n}", lambda dev, c=c, dt=dt: _joins(c, dt, dev)))
        out.append((f"gelu_{n}", lambda dev, c=c, dt=dt: _gelu(c, dt, dev)))
        out.append((f"layernorm_{n}", lambda dev, c=c, dt=dt: _layernorm(c, dt, dev)))
        out.append((f"patch_merge_{n}", lambda dev, c=c, dt=dt: _patch_merge(c, dt, dev)))
        out.append((f"roialign_{n}", lambda dev, c=c, dt=dt: _roialign(c, dt, dev)))
    for dt in (torch.bfloat16, torch.float32):
        for groups in (4, 8):
            for relu in (0, 1):
                out.append((f"groupnorm_g{groups}_relu{relu}_{_name(32, dt)}", lambda dev, dt=dt, g=groups, r=relu: _groupnorm(dt, dev, g, r)))
    return out


def run_case(fn, dev, fast):
    """{output name: sha256} of one case under one setting of the pool / BatchNorm fast-path switches (restored afterwards)."""
    try:
        lib.call("set_pool_fast", fast)
        lib.call("set_bn_fast", fast)
        got = {name: digest(t) for name, t in fn(dev)}
    finally:
        lib.call("set_pool_fast", 1)
        lib.call("set_bn_fast", 1)
    return got


def run_all(dev):
    return {f"{name}/fast{fast}": run_case(fn, dev, fast) for name, fn in cases() for fast in (1, 0)}
