"""GPU: the "copy / select / add" companions of csrc/elementwise.hip, called through their C entry points (and once each through the
autograd wrappers MaxPoolFn, UpsampleAddFn, SubsampleFn, AddReluFn), against the float64 / integer references of tests/pyramid_ref.py.
Every assertion is a bit equality, or -- the multi-term backwards on "rounding" data only -- the per-element bound derived in
pyramid_ref's docstring times the allowance k = max(1, min(2, 4 r)), r measured on torch's fp32 CPU evaluation of the same case (never
on the kernel).  Each bounded check prints k and its max |err| / (k bound) (run with -s).  tests/test_pyramid_ref_host.py shows on the
CPU that the references are right and that a 0-padded pool, "last maximum wins", the integer-floor index rule and the mask y >= 0 each
mismatch on this data.  Every output buffer is followed by a guard of sentinels that must survive; the pool and upsample cases run under
nrpn_set_pool_fast(1) and (0), restored to 1 in a finally.

Types and widths (pyramid_ref.WIDTHS): fp32 C = 4, 12 and bf16 C = 36 (4 channels per lane), bf16 C = 8, 64 (8 per lane); two scenes.

Kernel instantiations and loops reached, per entry point (T, V over the widths above), and the case that reaches them:
  nrpn_maxpool3d_fwd   maxpool_fwd_fast_kernel<K = 2>: (2,2,0,ceil) without, (2,2,1) and (2,1,1,ceil) with the low-side clamp and mask
                       maxpool_fwd_fast_kernel<K = 0>, the k == 3 run of three loads: (3,2,1), (3,1,1)
                       maxpool_fwd_fast_kernel<K = 0>, the generic loop: (4,2,2), (5,3,2,ceil), (1,2,0), (1,1,0)
                       maxpool_fwd_kernel<unsigned>: every configuration with the switch at 0
                       null argmax pointer: MaxPoolFn without requires_grad
  nrpn_maxpool3d_bwd   maxpool_bwd_fast_kernel<2,2>: (2,2,0,ceil), (2,2,1);  <2,0>: (3,2,1), (4,2,2), (1,2,0);  <1,0>: (3,1,1), (2,1,1,ceil), (1,1,0)
                       maxpool_bwd_kernel<unsigned>: (5,3,2,ceil) with the switch at 1 (s = 3 has no fast form), everything at 0
  nrpn_upsample_add_fwd  upsample_add_fwd_fast_kernel and upsample_add_fwd_kernel<unsigned>: all six size pairs, switch 1 / 0
  nrpn_upsample_add_bwd  upsample_add_bwd_x2_kernel: (10,10,10)/(5,5,5) at 1;  upsample_add_bwd_kernel<unsigned>: the other five pairs, and all at 0;
                       accumulate 0 and 1; (46,3,2)/(14,2,1): the fp32 rule is not the integer floor at fine index 23 (candidate window)
  nrpn_subsample3d     subsample_kernel<FWD> and <!FWD>, s = 1, 2, 3 on (9,7,5) and (8,6,4)
  nrpn_add_relu / nrpn_relu_backward   counts 4, 1028 and 4 (8192 * 256 + 5)
  nrpn_ncdhw_to_ndhwc  planes4_to_cl_kernel (C = 4), transpose_kernel<TO_CL> with ragged tiles (C = 5, 33: a second channel tile of one
                       channel; 315 voxels = 9 full tiles + 27) and C = 64, to fp32 and bf16
  nrpn_ndhwc_to_ncdhw  transpose_kernel<!TO_CL> from fp32 and from bf16, the same shapes
  second trip of the grid-stride loops (the grid stops at 8192 blocks x 256 lanes = 2 097 152 lane groups), "exact" data, fp32 C = 4
  (one lane group per voxel), one scene:
      pool forward    2/1/1-ceil on (129,128,128): 130 * 129 * 129 = 2 163 330 groups (fast K = 2 and general<unsigned>)
      pool backward   the same case: 129 * 128 * 128 = 2 113 536 groups (fast <1,0> and general<unsigned>)
      upsample fwd    fine (258,256,256) over coarse (129,128,128): 16 908 288 groups, 9 trips
      x2 upsample bwd the same pair: 2 113 536 coarse groups (and the general kernel with the switch at 0)
      subsample       forward s = 2 of (258,256,256): 2 113 536 groups; backward s = 2 into (129,128,128): 2 113 536 groups
      add_relu, relu_backward   2 097 157 groups
  64-bit index forms (test_64_bit_index_forms): one bf16 C = 8 scene of (1024,512,512) = 2^31 elements, closed-form input built on the
  device: maxpool_fwd_kernel<long long> and maxpool_bwd_kernel<long long> (2/2/0; 2^25 and 2^28 lane groups), upsample_add_fwd_kernel<long long>
  and upsample_add_bwd_kernel<long long> (accumulate 0 and 1) over the (512,256,256) coarse grid.  Measured 0.4 - 0.8 s and 11.4 GiB peak
  device memory of its own on one MI355X: kept.
Left unreached: the second trip of planes4_to_cl_kernel (needs 2 097 153 voxels of a 4-channel scene; its loop body has no index that
depends on the trip), and the fp32 instantiations of the <long long> forms (8 GiB per tensor).  The transposes have no grid-stride loop.

Measured on one MI355X (pytest -s --durations=0, whole file 36 tests in 10 s): add_relu at 8 388 628 elements 1.5 s, maxpool 3/2/1 1.3 s
(the first launch of the process), relu_backward at 8 388 628 1.0 s, second-trip maxpool 1.0 s, second-trip upsample-add 0.5 s + 0.6 s
for the shared tensors, 64-bit forms 0.8 s + 0.2 s setup, every other test <= 0.08 s.
Allowance and worst |err| / bound of the bounded checks (kernel against float64, over both switch settings and all widths):
  maxpool dx        fp32: k = 1.0 - 2.0 (r = 1.0 where a two-term sum attains u sum|t|), bf16: k = 2.0 (r = 0.996);
                    worst |err| / (k bound): 0.499 (3/2/1), 0.498 (3/1/1), 0.500 (2/1/1-ceil), 0.498 (4/2/2), 0.498 (5/3/2-ceil);
                    0.000 for 2/2/0-ceil, 2/2/1, 1/2/0, 1/1/0 (non-overlapping windows: at most one term, equality)
  upsample-add bwd  fp32: k = 1.0 - 2.0, bf16: k = 1.8 - 2.0; worst |err| / (k bound): 0.498 on the 10/5, 9x7x5/5x4x3, 46x3x2/14x2x1,
                    identity and 3x2x2/7x5x3 pairs, 0.472 on 7x5x3/1
  i.e. the kernels sit at |err| / bound = 1.0 unscaled, the half-ulp line of the bf16 store, exactly where torch's fp32 evaluation sits."""
import numpy as np
import pytest
import torch

import pyramid_ref as R

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
GUARD = 64
ARG_SENTINEL = -86
CAP = 8192 * 256                       # lane groups of one trip of a capped grid
NAMES = {F32: "f32", BF16: "bf16"}


def _lib():
    from nerf_rpn_amd import lib
    from nerf_rpn_amd.ops import _dt, _p, _s, call
    return lib, call, _p, _dt, _s


def _put(x64, dtype, dev):
    """Values on the device as the head of a buffer whose last GUARD elements hold the sentinel -> (view, guard)."""
    t = R.to_torch(x64, dtype)
    buf = torch.full((t.numel() + GUARD,), R.SENTINEL, dtype=dtype, device=dev)
    buf[:t.numel()] = t.reshape(-1).to(dev)
    return buf[:t.numel()].view(t.shape), buf[t.numel():]


def _out(shape, dtype, dev):
    """An output buffer full of sentinels with its guard -> (view, guard)."""
    n = int(np.prod(shape))
    fill = ARG_SENTINEL if dtype == torch.int8 else R.SENTINEL
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=dev)
    return buf[:n].view(tuple(shape)), buf[n:]


def _intact(*guards):
    torch.cuda.synchronize()
    return all(bool((g == (ARG_SENTINEL if g.dtype == torch.int8 else R.SENTINEL)).all()) for g in guards)


def _bounded(got, ref, mag, cnt, t32, dtype, what):
    """|got - ref| <= k * sum_bound, k from torch's fp32 evaluation ``t32`` of the same case."""
    tol = R.t64(R.sum_bound(cnt, mag, ref, dtype))
    k = R.allowance(R.ratio(R.t64(t32), R.t64(ref), tol))
    return R.check(got, R.t64(ref), tol, k, what)


class _pool_fast:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        _lib()[0].call("set_pool_fast", self.on)

    def __exit__(self, *exc):
        _lib()[0].call("set_pool_fast", 1)


# ======================================================================================================================
# max pool
# ======================================================================================================================
def pool_dispatch(k, s, fast, elements=0):
    """The instantiations nrpn_maxpool3d_fwd / _bwd launch (their dispatch, restated) -> (forward, backward)."""
    if elements >= 2 ** 31:
        return "fwd general<long long>", "bwd general<long long>"
    fwd = ("fwd fast K=2" if k == 2 else "fwd fast K=0, k==3 run" if k == 3 else "fwd fast K=0, generic loop") if fast else "fwd general<unsigned>"
    bwd = ("bwd fast <2,2>" if (s, k) == (2, 2) else "bwd fast <2,0>" if s == 2 else "bwd fast <1,0>") if fast and s in (1, 2) else "bwd general<unsigned>"
    return fwd, bwd


def test_pool_cases_reach_every_instantiation():
    reached = {}
    for k, s, p, ceil in R.POOL_CONFIGS:
        for fast in (1, 0):
            for name in pool_dispatch(k, s, fast):
                reached.setdefault(name, []).append((k, s, p, ceil, fast))
    for name, cases in sorted(reached.items()):
        print(name, "<-", cases)
    assert set(reached) == {"fwd fast K=2", "fwd fast K=0, k==3 run", "fwd fast K=0, generic loop", "fwd general<unsigned>", "bwd fast <2,2>",
                            "bwd fast <2,0>", "bwd fast <1,0>", "bwd general<unsigned>"}
    assert (5, 3, 2, 1, 1) in reached["bwd general<unsigned>"]          # the general backward with s = 3 while the switch is on
    assert {(2, 2, 1, 0, 1), (2, 1, 1, 1, 1)} <= set(reached["fwd fast K=2"])      # the 2-wide window with left padding


def _pool_launch(x, dy, grid, c, cfg, dev):
    lib, call, _p, _dt, _s = _lib()
    k, s, p, ceil = cfg
    o = [lib.query("pool_out_size", g, k, s, p, ceil) for g in grid]
    y, gy = _out((2, *o, c), x.dtype, dev)
    arg, ga = _out((2, *o, c), torch.int8, dev)
    call("maxpool3d_fwd", _p(x), _p(y), _p(arg), 2, *grid, c, k, s, p, ceil, _dt(x), _s())
    dx, gd = _out(x.shape, x.dtype, dev)
    if dy is not None:
        call("maxpool3d_bwd", _p(dy), _p(arg), _p(dx), 2, *grid, c, k, s, p, ceil, _dt(x), _s())
    return y, arg, dx, (gy, ga, gd)


@pytest.mark.parametrize("cfg", R.POOL_CONFIGS, ids=["%d%d%d%s" % (k, s, p, "c" if c else "") for k, s, p, c in R.POOL_CONFIGS])
def test_maxpool_matches_reference(cfg, dev):
    """y and the argmax code bit-equal on both data classes; dx bit-equal on "exact" data, inside its bound on "rounding" data."""
    k, s, p, ceil = cfg
    worst = 0.0
    for grid in R.POOL_GRIDS:
        for c, dtype in R.WIDTHS:
            for kind in ("exact", "rounding"):
                x = R.data(kind, 10, (2,) + grid + (c,), dtype, inf=True, mean=R.POOL_MEAN)
                ref = R.maxpool_ref(x, k, s, p, ceil)
                dy = R.data(kind, 11, ref.y.shape, dtype)
                acc, mag, cnt = ref.dx(dy)
                t32 = R.maxpool_dx_torch32(x, dy, k, s, p, ceil, dtype) if kind == "rounding" else None
                xd, gx = _put(x, dtype, dev)
                dyd, gdy = _put(dy, dtype, dev)
                for fast in (1, 0):
                    what = f"maxpool {cfg} {grid} c{c} {NAMES[dtype]} {kind} fast{fast} [{' | '.join(pool_dispatch(k, s, fast))}]"
                    with _pool_fast(fast):
                        y, arg, dx, guards = _pool_launch(xd, dyd, grid, c, cfg, dev)
                    assert _intact(gx, gdy, *guards), (what, "a guard was written")
                    assert tuple(y.shape[1:4]) == ref.o, (what, "output grid", tuple(y.shape), ref.o)
                    R.check_equal(y, ref.y, what + " y")
                    R.check_equal(arg, ref.code, what + " argmax")
                    if kind == "exact":
                        R.check_equal(dx, R.round_to(dtype)(acc), what + " dx")
                    else:
                        worst = max(worst, _bounded(dx, acc, mag, cnt, t32, dtype, what + " dx"))
                        one = cnt <= 1                                  # nothing was added there: equality
                        assert torch.equal(R.bits(dx)[torch.from_numpy(one)], R.bits(R.to_torch(acc, dtype))[torch.from_numpy(one)]), (what, "single-term dx")
    print(f"maxpool {cfg}: worst dx |err| / (k bound) {worst:.3f}")


def test_maxpool_wrapper(dev):
    """MaxPoolFn: forward + backward through autograd, and without requires_grad (a null argmax pointer)."""
    from nerf_rpn_amd import ops
    grid, c, dtype, cfg = (9, 7, 5), 36, BF16, (3, 2, 1, 0)
    x = R.data("exact", 10, (2,) + grid + (c,), dtype)
    ref = R.maxpool_ref(x, *cfg)
    dy = R.data("exact", 11, ref.y.shape, dtype)
    xd = R.to_torch(x, dtype).to(dev)
    plain = ops.MaxPoolFn.apply(xd, 3, 2, 1, False)
    R.check_equal(plain, ref.y, "MaxPoolFn without requires_grad")
    xg = xd.clone().requires_grad_(True)
    y = ops.MaxPoolFn.apply(xg, 3, 2, 1, False)
    y.backward(R.to_torch(dy, dtype).to(dev))
    R.check_equal(y, ref.y, "MaxPoolFn y")
    R.check_equal(xg.grad, R.round_to(dtype)(ref.dx(dy)[0]), "MaxPoolFn dx")


# ======================================================================================================================
# upsample-add
# ======================================================================================================================
def upsample_dispatch(fine, coarse, fast):
    x2 = all(f == 2 * c for f, c in zip(fine, coarse))
    return "fwd fast" if fast else "fwd general<unsigned>", "bwd x2" if fast and x2 else "bwd general<unsigned>"


@pytest.mark.parametrize("fine,coarse", R.UPSAMPLE_PAIRS, ids=["%dx%dx%d_over_%dx%dx%d" % (f + c) for f, c in R.UPSAMPLE_PAIRS])
def test_upsample_add_matches_reference(fine, coarse, dev):
    """Forward bit-equal to round(fine + coarse[src]); backward with accumulate 0 and 1 (over a prefilled dcoarse) bit-equal on "exact"
    data, inside its bound on "rounding" data."""
    lib, call, _p, _dt, _s = _lib()
    worst = 0.0
    for c, dtype in R.WIDTHS:
        for kind in ("exact", "rounding"):
            f = R.data(kind, 20, (2,) + fine + (c,), dtype, inf=True)
            co = R.data(kind, 21, (2,) + coarse + (c,), dtype)
            d = R.data(kind, 22, f.shape, dtype)
            pre = R.data(kind, 23, co.shape, dtype)
            if f.size >= 18 and fine == coarse:
                R.plant_pairs(f, co, dtype)
            want = R.round_to(dtype)(R.upsample_add_ref(f, co))
            refs = {0: R.upsample_add_bwd_ref(d, co.shape), 1: R.upsample_add_bwd_ref(d, co.shape, pre)}
            t32 = {a: R.upsample_bwd_torch32(d, co.shape, pre if a else None, dtype) for a in (0, 1)} if kind == "rounding" else None
            cod, gco = _put(co, dtype, dev)
            dd, gdd = _put(d, dtype, dev)
            for fast in (1, 0):
                what = f"upsample_add {fine}/{coarse} c{c} {NAMES[dtype]} {kind} fast{fast} [{' | '.join(upsample_dispatch(fine, coarse, fast))}]"
                with _pool_fast(fast):
                    fd, gf = _put(f, dtype, dev)
                    call("upsample_add_fwd", _p(fd), _p(cod), 2, *fine, *coarse, c, _dt(fd), _s())
                    assert _intact(gf, gco), (what, "a guard was written")
                    R.check_equal(fd, want, what + " fwd")
                    R.check_equal(cod, co, what + " coarse untouched")
                    for accumulate in (0, 1):
                        dc, gdc = _put(pre, dtype, dev) if accumulate else _out(co.shape, dtype, dev)
                        call("upsample_add_bwd", _p(dd), _p(dc), 2, *fine, *coarse, c, _dt(dd), accumulate, _s())
                        assert _intact(gdd, gdc), (what, "a guard was written")
                        acc, mag, cnt = refs[accumulate]
                        if kind == "exact":
                            R.check_equal(dc, R.round_to(dtype)(acc), f"{what} bwd acc{accumulate}")
                        else:
                            worst = max(worst, _bounded(dc, acc, mag, cnt, t32[accumulate], dtype, f"{what} bwd acc{accumulate}"))
    print(f"upsample_add {fine}/{coarse}: worst bwd |err| / (k bound) {worst:.3f}")


def test_upsample_add_wrapper_is_in_place(dev):
    """UpsampleAddFn mutates and returns ``fine``; the gradient of fine is d itself, that of coarse the reference."""
    from nerf_rpn_amd import ops
    fine, coarse, c, dtype = (9, 7, 5), (5, 4, 3), 12, F32
    f, co, d = (R.data("exact", 20 + i, (2,) + g + (c,), dtype) for i, g in enumerate((fine, coarse, fine)))
    leaf = R.to_torch(f, dtype).to(dev).requires_grad_(True)
    cd = R.to_torch(co, dtype).to(dev).requires_grad_(True)
    work = leaf * 1.0
    ptr = work.data_ptr()
    out = ops.UpsampleAddFn.apply(work, cd)
    assert out.data_ptr() == ptr and out.shape == work.shape, "fine is not returned in place"
    R.check_equal(work, R.round_to(dtype)(R.upsample_add_ref(f, co)), "UpsampleAddFn fine, mutated")
    out.backward(R.to_torch(d, dtype).to(dev))
    R.check_equal(leaf.grad, d, "UpsampleAddFn d(fine) is d")
    R.check_equal(cd.grad, R.round_to(dtype)(R.upsample_add_bwd_ref(d, co.shape)[0]), "UpsampleAddFn d(coarse)")


# ======================================================================================================================
# subsample
# ======================================================================================================================
@pytest.mark.parametrize("s", (1, 2, 3))
def test_subsample_matches_reference(s, dev):
    """Forward a pure selection; the backward writes dy at the multiples of s and +0 over every other element of a sentinel-filled dst."""
    lib, call, _p, _dt, _s = _lib()
    from nerf_rpn_amd import ops
    for grid in R.SUBSAMPLE_GRIDS:
        for c, dtype in R.WIDTHS:
            x = R.data("rounding", 30, (2,) + grid + (c,), dtype, inf=True)
            want = R.subsample_ref(x, s)
            dy = R.data("rounding", 31, want.shape, dtype, inf=True)
            what = f"subsample s{s} {grid} c{c} {NAMES[dtype]}"
            xd, gx = _put(x, dtype, dev)
            y, gy = _out(want.shape, dtype, dev)
            call("subsample3d", _p(xd), _p(y), 2, *grid, c, s, 0, _dt(xd), _s())
            dyd, gdy = _put(dy, dtype, dev)
            dx, gdx = _out(x.shape, dtype, dev)
            call("subsample3d", _p(dyd), _p(dx), 2, *grid, c, s, 1, _dt(xd), _s())
            assert _intact(gx, gy, gdy, gdx), (what, "a guard was written")
            R.check_equal(y, want, what + " fwd")
            R.check_equal(dx, R.subsample_bwd_ref(dy, x.shape, s), what + " bwd")
    xg = R.to_torch(x, dtype).to(dev).requires_grad_(True)
    yw = ops.SubsampleFn.apply(xg, s)
    yw.backward(R.to_torch(dy, dtype).to(dev))
    R.check_equal(yw, want, f"SubsampleFn s{s} y")
    R.check_equal(xg.grad, R.subsample_bwd_ref(dy, x.shape, s), f"SubsampleFn s{s} dx")


# ======================================================================================================================
# residual join, ReLU backward
# ======================================================================================================================
JOIN_COUNTS = (4, 1028, 4 * (CAP + 5))          # one lane; five blocks, the last ragged; 2 097 157 lane groups: the second trip of the capped grid


def _join_case(count, dtype):
    n = max(count, 20)                                       # the named positions need 18 elements; the kernel sees the first `count`
    a, b = R.data("rounding", 40, (n,), dtype, inf=True), R.data("rounding", 41, (n,), dtype)
    R.plant_pairs(a, b, dtype)
    return a, b


@pytest.mark.parametrize("count", JOIN_COUNTS)
def test_add_relu_matches_reference(count, dev):
    lib, call, _p, _dt, _s = _lib()
    for dtype in (F32, BF16):
        a, b = _join_case(count, dtype)
        ad, ga = _put(a, dtype, dev)
        bd, gb = _put(b, dtype, dev)
        for relu in (0, 1):
            what = f"add_relu n{count} {NAMES[dtype]} relu{relu}"
            y, gy = _out((a.size,), dtype, dev)
            call("add_relu", _p(ad), _p(bd), _p(y), count, relu, _dt(ad), _s())
            assert _intact(ga, gb, gy), (what, "a guard was written")
            want = R.add_relu_ref(a, b, relu, dtype)
            want[count:] = R.SENTINEL                        # beyond the count nothing is written
            R.check_equal(y, want, what)
            if count >= 18:
                got = R.bits(y)
                for name in R.PAIRS:
                    i = R.PAIRS[name]
                    assert got[i] == R.bits(R.to_torch(want[i:i + 1], dtype))[0], (what, name, y[i].item(), want[i])
                assert got[R.PAIRS["cancel"]] == 0, (what, "a + (-a) is +0.0")
                assert (got[R.PAIRS["neg_zero"]] == 0) == bool(relu), (what, "-0.0 + -0.0 is -0.0, +0.0 after relu")
                assert y[R.PAIRS["denormal"]].item() > 0, (what, "the denormal sum was flushed")


@pytest.mark.parametrize("count", JOIN_COUNTS)
def test_relu_backward_matches_reference(count, dev):
    lib, call, _p, _dt, _s = _lib()
    for dtype in (F32, BF16):
        n = max(count, 20)
        y = R.plant_mask(R.data("rounding", 42, (n,), dtype, inf=True), dtype)
        dy = R.data("rounding", 43, (n,), dtype)
        dy[[R.MASKS[m] for m in R.MASKS]] = 2.5
        what = f"relu_backward n{count} {NAMES[dtype]}"
        yd, gy = _put(y, dtype, dev)
        dyd, gdy = _put(dy, dtype, dev)
        dx, gdx = _out((n,), dtype, dev)
        call("relu_backward", _p(yd), _p(dyd), _p(dx), count, _dt(yd), _s())
        assert _intact(gy, gdy, gdx), (what, "a guard was written")
        want = R.relu_backward_ref(y, dy)
        want[count:] = R.SENTINEL
        R.check_equal(dx, want, what)
        if count >= 18:
            got = dx.cpu().double()
            assert [got[R.MASKS[m]].item() for m in ("neg_zero", "pos_zero", "denormal", "negative", "positive")] == [0.0, 0.0, 2.5, 0.0, 2.5], what
            assert R.bits(dx)[R.MASKS["neg_zero"]] == 0, (what, "the masked gradient is +0.0")


def test_add_relu_wrapper(dev):
    from nerf_rpn_amd import ops
    dtype = BF16
    a, b = _join_case(2 * 315 * 36, dtype)
    dy = R.data("rounding", 44, a.shape, dtype)
    for relu in (True, False):
        ad, bd = (R.to_torch(t, dtype).to(dev).requires_grad_(True) for t in (a, b))
        y = ops.AddReluFn.apply(ad, bd, relu)
        y.backward(R.to_torch(dy, dtype).to(dev))
        want = R.add_relu_ref(a, b, int(relu), dtype)
        R.check_equal(y, want, f"AddReluFn relu={relu} y")
        g = R.relu_backward_ref(want, dy) if relu else dy
        R.check_equal(ad.grad, g, f"AddReluFn relu={relu} da")
        R.check_equal(bd.grad, g, f"AddReluFn relu={relu} db")


# ======================================================================================================================
# layouts
# ======================================================================================================================
@pytest.mark.parametrize("c", (4, 5, 33, 64))
def test_layouts_match_reference(c, dev):
    """[2][C][315] fp32 -> [2][315][C] fp32 / bf16 and back from both: the permutation and one round-to-nearest-even."""
    lib, call, _p, _dt, _s = _lib()
    n, vox = 2, 315
    x = R.rounding(50, (n, c, vox), F32, inf=True)
    src, gs = _put(x, F32, dev)
    for dtype in (F32, BF16):
        what = f"layout c{c} {NAMES[dtype]}"
        cl, gcl = _out((n, vox, c), dtype, dev)
        call("ncdhw_to_ndhwc", _p(src), _p(cl), n, c, vox, _dt(cl), _s())
        assert _intact(gs, gcl), (what, "a guard was written")
        want = R.to_channels_last_ref(x, dtype)
        R.check_equal(cl, want, what + " ncdhw_to_ndhwc")
        back, gb = _out((n, c, vox), F32, dev)
        call("ndhwc_to_ncdhw", _p(cl), _p(back), n, c, vox, _dt(cl), _s())
        assert _intact(gcl, gb), (what, "a guard was written")
        R.check_equal(back, R.to_channels_first_ref(want), what + " ndhwc_to_ncdhw")


# ======================================================================================================================
# second trip of the grid-stride loops
# ======================================================================================================================
BIG_COARSE, BIG_FINE = (129, 128, 128), (258, 256, 256)


def _eighths(seed, shape):
    """"exact" data as int8 numerators (value = numerator / 8), generated fast."""
    return np.random.RandomState(seed).randint(-64, 65, size=shape, dtype=np.int8)


def _dev_f32(i8, dev):
    return torch.from_numpy(i8).to(dev).to(F32) / 8.0


def _same(got, want, what):
    """Bit equality on the device of two fp32 tensors; a failure names the first flat index and its trip of the capped grid."""
    a, b = got.reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32)
    if not torch.equal(a, b):
        bad = (a != b).nonzero().reshape(-1)
        raise AssertionError((what, "bits differ at", int(bad.numel()), "of", a.numel(), "first flat index", int(bad[0]), "lane group", int(bad[0]) // 4,
                              "trip", int(bad[0]) // 4 // CAP))
    print(f"{what}: bit-equal ({a.numel()} elements)")


def test_second_trip_maxpool(dev):
    """2/1/1-ceil, one scene of (129,128,128) x 4 fp32: 2 163 330 output and 2 113 536 input lane groups, both above 2 097 152."""
    lib, call, _p, _dt, _s = _lib()
    grid, c, cfg = BIG_COARSE, 4, (2, 1, 1, 1)
    k, s, p, ceil = cfg
    x8 = _eighths(60, (1,) + grid + (c,))
    ref = R.maxpool_ref(x8.astype(np.float32), k, s, p, ceil)          # selections are exact in any float type; dx sums in float64
    assert int(np.prod(ref.o)) > CAP and int(np.prod(grid)) > CAP and ref.o == (130, 129, 129)
    dy8 = _eighths(61, ref.y.shape)
    acc = ref.dx(dy8.astype(np.float32) / 8.0)[0]
    xd, dyd = _dev_f32(x8, dev), _dev_f32(dy8, dev)
    want_y, want_arg, want_dx = torch.from_numpy(ref.y).to(dev) / 8.0, torch.from_numpy(ref.code).to(dev), torch.from_numpy(acc).to(dev).to(F32)
    for fast in (1, 0):
        what = f"second trip maxpool fast{fast} [{' | '.join(pool_dispatch(k, s, fast))}]"
        y, gy = _out((1, *ref.o, c), F32, dev)
        arg, ga = _out((1, *ref.o, c), torch.int8, dev)
        dx, gd = _out(xd.shape, F32, dev)
        with _pool_fast(fast):
            call("maxpool3d_fwd", _p(xd), _p(y), _p(arg), 1, *grid, c, k, s, p, ceil, _dt(xd), _s())
            call("maxpool3d_bwd", _p(dyd), _p(arg), _p(dx), 1, *grid, c, k, s, p, ceil, _dt(xd), _s())
        assert _intact(gy, ga, gd), (what, "a guard was written")
        _same(y, want_y, what + " y")
        assert torch.equal(arg, want_arg), (what, "argmax")
        _same(dx, want_dx, what + " dx")


@pytest.fixture(scope="module")
def big_pair(dev):
    """One scene, fine (258,256,256) over coarse (129,128,128), 4 fp32 channels of "exact" data: numerators on the host, values on the device."""
    f8, c8 = _eighths(62, (1,) + BIG_FINE + (4,)), _eighths(63, (1,) + BIG_COARSE + (4,))
    return f8, c8, _dev_f32(f8, dev), _dev_f32(c8, dev)


def test_second_trip_upsample_add(big_pair, dev):
    """16 908 288 fine lane groups (9 trips of the forward), 2 113 536 coarse ones (the x2 backward and, switch at 0, the general one)."""
    lib, call, _p, _dt, _s = _lib()
    f8, c8, fd, cd = big_pair
    assert f8.size // 4 > CAP and c8.size // 4 > CAP
    up = c8.astype(np.int16).repeat(2, axis=1).repeat(2, axis=2).repeat(2, axis=3)               # the exact 2x pair: src = dst // 2
    for a, b in zip(BIG_FINE, BIG_COARSE):
        assert np.array_equal(R.nearest_index(a, b), np.arange(a) // 2)
    want_f = (torch.from_numpy(f8.astype(np.int16) + up).to(dev).to(F32) / 8.0)
    n, fx, fy, fz, c = f8.shape
    sums = f8.reshape(n, fx // 2, 2, fy // 2, 2, fz // 2, 2, c).sum(axis=(2, 4, 6), dtype=np.int32)      # eight children, in integers
    for fast in (1, 0):
        what = f"second trip upsample_add fast{fast} [{' | '.join(upsample_dispatch(BIG_FINE, BIG_COARSE, fast))}]"
        work, gw = _out(fd.shape, F32, dev)
        work.copy_(fd)
        with _pool_fast(fast):
            call("upsample_add_fwd", _p(work), _p(cd), 1, *BIG_FINE, *BIG_COARSE, 4, _dt(work), _s())
            for accumulate in (0, 1):
                dc, gdc = _out(cd.shape, F32, dev)
                if accumulate:
                    dc.copy_(cd)
                call("upsample_add_bwd", _p(fd), _p(dc), 1, *BIG_FINE, *BIG_COARSE, 4, _dt(fd), accumulate, _s())
                assert _intact(gdc), (what, "a guard was written")
                want = torch.from_numpy(sums + (c8 if accumulate else 0)).to(dev).to(F32) / 8.0
                _same(dc, want, f"{what} bwd acc{accumulate}")
        assert _intact(gw), (what, "a guard was written")
        _same(work, want_f, what + " fwd")


def test_second_trip_subsample(big_pair, dev):
    """Forward s = 2 of (258,256,256) and backward s = 2 into (129,128,128): 2 113 536 lane groups each."""
    lib, call, _p, _dt, _s = _lib()
    f8, c8, fd, cd = big_pair
    y, gy = _out(cd.shape, F32, dev)
    call("subsample3d", _p(fd), _p(y), 1, *BIG_FINE, 4, 2, 0, _dt(fd), _s())
    assert _intact(gy)
    _same(y, _dev_f32(np.ascontiguousarray(R.subsample_ref(f8, 2)), dev), "second trip subsample fwd")
    small8 = _eighths(64, (1, 65, 64, 64, 4))
    dx, gdx = _out(cd.shape, F32, dev)
    call("subsample3d", _p(_dev_f32(small8, dev)), _p(dx), 1, *BIG_COARSE, 4, 2, 1, _dt(fd), _s())
    assert _intact(gdx)
    want = np.zeros(c8.shape, np.int8)
    want[:, ::2, ::2, ::2] = small8
    _same(dx, _dev_f32(want, dev), "second trip subsample bwd")


# ======================================================================================================================
# 64-bit index forms
# ======================================================================================================================
BIG64_GRID, BIG64_OUT, BIG64_C, BIG64_SLAB = (1024, 512, 512), (512, 256, 256), 8, 64


def _coords(x0, x1, gy, gz, dev):
    i32 = dict(dtype=torch.int32, device=dev)
    return (torch.arange(x0, x1, **i32).view(-1, 1, 1, 1), torch.arange(gy, **i32).view(1, -1, 1, 1), torch.arange(gz, **i32).view(1, 1, -1, 1),
            torch.arange(BIG64_C, **i32).view(1, 1, 1, -1))


def _hash(wx, wy, wz, ch, a, b, c, m):
    return (wx * a + wy * b + wz * c + ch) % m


def _x_closed(x0, x1, dev):
    """Input planes x0 .. x1 - 1: sign(ch) * ((ix & 1) 4 + (iy & 1) 2 + (iz & 1)) + 8 h(window, ch), sign = +1 on even channels, -1 on odd:
    inside a 2/2/0 window h is constant, so the maximum is 7 + 8 h at offset (1,1,1), code 7, on even channels and 8 h at (0,0,0), code 0, on odd."""
    ix, iy, iz, ch = _coords(x0, x1, *BIG64_GRID[1:], dev)
    return (1 - 2 * (ch & 1)) * ((ix & 1) * 4 + (iy & 1) * 2 + (iz & 1)) + 8 * _hash(ix >> 1, iy >> 1, iz >> 1, ch, 3, 5, 7, 11)


def _out_closed(w0, w1, dev):
    """Output planes w0 .. w1 - 1 -> (y, dy, coarse): the known maxima, and two more integer fields for the gradient and the coarse operand."""
    wx, wy, wz, ch = _coords(w0, w1, *BIG64_OUT[1:], dev)
    return (7 * (1 - (ch & 1)) + 8 * _hash(wx, wy, wz, ch, 3, 5, 7, 11), _hash(wx, wy, wz, ch, 1, 2, 3, 13) - 6, _hash(wx, wy, wz, ch, 2, 1, 5, 9) - 4)


def _up2(t):
    return t.repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2)


def _slab_equal(got, want_int, what, plane):
    want = want_int.to(F32).to(BF16)                               # small integers: exact in fp32, one rounding to bf16
    if not torch.equal(got.view(torch.int16), want.view(torch.int16)):
        bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()[0].tolist()
        raise AssertionError((what, "first mismatch in the slab at plane", plane, "index", bad, "got", got[tuple(bad)].item(), "want", want[tuple(bad)].item()))


def test_64_bit_index_forms(dev):
    """One bf16 C = 8 scene of (1024,512,512): 2^31 input elements, so every launcher takes its <long long> instantiation -- 2/2/0 pool
    forward and backward, upsample-add forward and backward over the (512,256,256) coarse grid.  The input is a closed form built on the
    device in slabs; expected tensors are elementwise torch expressions of the coordinates and strided views, slab by slab."""
    import time
    lib, call, _p, _dt, _s = _lib()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()                           # what earlier tests of the session still hold: not this test's
    t0 = time.time()
    g, o, c = BIG64_GRID, BIG64_OUT, BIG64_C
    assert int(np.prod(g)) * c >= 2 ** 31 and pool_dispatch(2, 2, 1, int(np.prod(g)) * c) == ("fwd general<long long>", "bwd general<long long>")
    slabs = [(x0, x0 + BIG64_SLAB) for x0 in range(0, g[0], BIG64_SLAB)]
    x, gx = _out((1, *g, c), BF16, dev)
    y, gy = _out((1, *o, c), BF16, dev)
    arg, ga = _out((1, *o, c), torch.int8, dev)
    dy, gdy = _out((1, *o, c), BF16, dev)
    co, gco = _out((1, *o, c), BF16, dev)
    dx, gdx = _out((1, *g, c), BF16, dev)
    for x0, x1 in slabs:
        x[0, x0:x1] = _x_closed(x0, x1, dev).to(BF16)
        _, dyi, coi = _out_closed(x0 // 2, x1 // 2, dev)
        dy[0, x0 // 2:x1 // 2], co[0, x0 // 2:x1 // 2] = dyi.to(BF16), coi.to(BF16)
    call("maxpool3d_fwd", _p(x), _p(y), _p(arg), 1, *g, c, 2, 2, 0, 0, _dt(x), _s())
    call("maxpool3d_bwd", _p(dy), _p(arg), _p(dx), 1, *g, c, 2, 2, 0, 0, _dt(x), _s())
    assert _intact(gx, gy, ga, gdy, gdx), "a guard was written"
    codes = torch.tensor([7, 0] * (c // 2), dtype=torch.int8, device=dev)
    assert bool((arg.view(-1, c) == codes).all()), "argmax codes"
    for x0, x1 in slabs:
        yi, dyi, _ = _out_closed(x0 // 2, x1 // 2, dev)
        _slab_equal(y[0, x0 // 2:x1 // 2], yi, "pool forward <long long>", x0 // 2)
        want = torch.zeros((x1 - x0, g[1], g[2], c), dtype=torch.int32, device=dev)
        want[1::2, 1::2, 1::2, 0::2] = dyi[..., 0::2]                 # even channels: the window's (1,1,1) voxel takes the gradient
        want[0::2, 0::2, 0::2, 1::2] = dyi[..., 1::2]                 # odd channels: its (0,0,0) voxel
        _slab_equal(dx[0, x0:x1], want, "pool backward <long long>", x0)
    del dx, gdx, want
    # fine = x, in place; then x (now x + up(co)) is the gradient handed to the backward: each coarse voxel sums its eight children
    call("upsample_add_fwd", _p(x), _p(co), 1, *g, *o, c, _dt(x), _s())
    dc0, g0 = _out((1, *o, c), BF16, dev)
    dc1, g1 = _out((1, *o, c), BF16, dev)
    dc1.copy_(dy)
    call("upsample_add_bwd", _p(x), _p(dc0), 1, *g, *o, c, _dt(x), 0, _s())
    call("upsample_add_bwd", _p(x), _p(dc1), 1, *g, *o, c, _dt(x), 1, _s())
    assert _intact(gx, gco, g0, g1), "a guard was written"
    for x0, x1 in slabs:
        _, dyi, coi = _out_closed(x0 // 2, x1 // 2, dev)
        xi = _x_closed(x0, x1, dev)
        _slab_equal(x[0, x0:x1], xi + _up2(coi), "upsample-add forward <long long>", x0)
        children = (xi.view((x1 - x0) // 2, 2, g[1] // 2, 2, g[2] // 2, 2, c).sum(dim=(1, 3, 5)) + 8 * coi)
        _slab_equal(dc0[0, x0 // 2:x1 // 2], children, "upsample-add backward <long long>", x0 // 2)
        _slab_equal(dc1[0, x0 // 2:x1 // 2], children + dyi, "upsample-add backward <long long>, accumulate", x0 // 2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    print(f"64-bit index forms: {time.time() - t0:.2f} s, peak device memory of this test {peak / 2 ** 30:.2f} GiB")
    assert peak < 16 * 2 ** 30
