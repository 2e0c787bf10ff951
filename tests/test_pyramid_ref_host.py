"""CPU: the references of tests/pyramid_ref.py are right and their bounds satisfiable.  maxpool_ref against torch's float64 max_pool3d
(values, indices mapped to the window code, gradient) on every configuration and grid the GPU test runs; the fp32 index rule against
F.interpolate(mode="nearest") on every size pair up to 64, with the pairs where it is not the integer floor; the gradient references
against autograd in float64; round_to against numpy / torch casts and a double-rounding counterexample; the allowance measured on torch's
fp32 evaluation; and one mutation per reference that has to produce a mismatch on the data the GPU test uses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import pyramid_ref as R

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _ncdhw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 4, 1, 2, 3).contiguous()


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous().numpy()


# ======================================================================================================================
# rounding
# ======================================================================================================================
def test_round_to_is_one_rounding_to_nearest_even():
    rs = np.random.RandomState(1)
    x = np.concatenate([rs.standard_normal(4000) * 10.0 ** rs.randint(-45, 39, 4000), [0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-45, 3.4028235677973366e38,
                        1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 2.0 ** -150, 1.5 * 2.0 ** -150]])
    with np.errstate(over="ignore"):
        want32 = x.astype(np.float32)
    got32 = R.round_to(F32)(x)
    assert np.array_equal(got32.astype(np.float32).view(np.int32), want32.view(np.int32))
    # from fp32 values the cast of torch is one rounding: the same bits
    want16 = torch.from_numpy(want32).to(BF16)
    got16 = R.to_torch(R.round_to(BF16)(want32.astype(np.float64)), BF16)
    assert torch.equal(R.bits(got16), R.bits(want16))
    for v, want in ((1 + 2.0 ** -8, 1.0), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6), (-(1 + 2.0 ** -8), -1.0), (2.0 ** -134, 0.0), (3 * 2.0 ** -134, 2.0 ** -132)):
        assert R.round_to(BF16)(v) == want
    # directly from float64 it is NOT the two-step cast: 1 + 2^-8 + 2^-40 is above the tie, through fp32 it falls on it and goes to even
    v = 1 + 2.0 ** -8 + 2.0 ** -40
    assert R.round_to(BF16)(v) == 1 + 2.0 ** -7 and float(torch.tensor(v, dtype=F64).to(F32).to(BF16)) == 1.0
    assert np.signbit(R.round_to(BF16)(-0.0)) and np.signbit(R.round_to(F32)(-1e-60))


def test_two_term_sums_survive_double_rounding():
    """round_to(bf16)(a + b) in one step equals fp32-add-then-store for bf16 operands (the module docstring's claim), ties included."""
    rs = np.random.RandomState(2)
    a = R.round_to(BF16)(rs.standard_normal(200000) * 2.0 ** rs.randint(-12, 12, 200000))
    b = R.round_to(BF16)(rs.standard_normal(200000) * 2.0 ** rs.randint(-12, 12, 200000))
    R.plant_pairs(a, b, BF16)
    two_step = (R.to_torch(a, F32) + R.to_torch(b, F32)).to(BF16)
    R.check_equal(two_step, R.round_to(BF16)(a + b), "bf16 a + b: one rounding against fp32 add + store")
    a32, b32 = R.rounding(3, (4096,), F32), R.rounding(4, (4096,), F32)
    R.plant_pairs(a32, b32, F32)
    R.check_equal(R.to_torch(a32, F32) + R.to_torch(b32, F32), R.round_to(F32)(a32 + b32), "fp32 a + b")
    want = R.add_relu_ref(a, b, 0, BF16).reshape(-1)
    assert want[R.PAIRS["tie_down"]] == 1.0 and want[R.PAIRS["tie_up"]] == 1 + 2.0 ** -6
    assert want[R.PAIRS["cancel"]] == 0 and not np.signbit(want[R.PAIRS["cancel"]]) and np.signbit(want[R.PAIRS["neg_zero"]])
    assert not np.signbit(R.add_relu_ref(a, b, 1, BF16).reshape(-1)[R.PAIRS["neg_zero"]])
    assert R.add_relu_ref(a, b, 1, BF16).reshape(-1)[R.PAIRS["denormal"]] == 2.0 ** -133


# ======================================================================================================================
# max pool
# ======================================================================================================================
def _torch_pool(x, dy, k, s, p, ceil):
    xt = _ncdhw(x).requires_grad_(True)
    y, idx = Fn.max_pool3d(xt, k, s, p, ceil_mode=bool(ceil), return_indices=True)
    y.backward(_ncdhw(dy))
    gx, gy, gz = x.shape[1:4]
    ix, iy, iz = idx // (gy * gz), (idx // gz) % gy, idx % gz
    o = y.shape[2:]
    w = [torch.arange(q).view([-1 if i == j else 1 for j in range(3)]) * s - p for i, q in enumerate(o)]
    code = ((ix - w[0]) * k + (iy - w[1])) * k + (iz - w[2])
    return _ndhwc(y.detach()), _ndhwc(code), _ndhwc(xt.grad)


@pytest.mark.parametrize("k,s,p,ceil", R.POOL_CONFIGS)
def test_maxpool_ref_matches_torch_float64(k, s, p, ceil):
    for grid in R.POOL_GRIDS:
        for kind, dtype in (("exact", F32), ("rounding", BF16), ("rounding", F32)):
            x = R.data(kind, 10, (2,) + grid + (4,), dtype, inf=True, mean=R.POOL_MEAN)
            ref = R.maxpool_ref(x, k, s, p, ceil)
            dy = R.data(kind, 11, ref.y.shape, dtype)
            y, code, dx = _torch_pool(x, dy, k, s, p, ceil)
            assert ref.y.shape == y.shape, (grid, "output size", ref.y.shape, y.shape)
            assert np.array_equal(ref.y, y) and np.array_equal(ref.code, code), (grid, kind)
            acc, mag, cnt = ref.dx(dy)
            assert np.abs(acc - dx).max() <= 1e-13 * max(1.0, mag.max()), (grid, kind)
            if kind == "exact":
                assert np.array_equal(acc, dx)
            assert cnt.sum() == ref.y.size and cnt.max() <= (-(-k // s)) ** 3
    if (k, s, p) == (3, 1, 1):
        assert cnt.max() >= 4            # multi-term sums exist


def test_maxpool_data_has_negative_windows_and_ties():
    """What the mutations below and the GPU test rely on: all-negative windows at the border, and windows whose maximum occurs twice."""
    x = R.data("rounding", 10, (2, 9, 7, 5, 4), BF16, inf=True, mean=R.POOL_MEAN)
    ref = R.maxpool_ref(x, 3, 2, 1, 0)
    assert (ref.y < 0).sum() > 20 and np.isneginf(x).sum() == 1 and np.isposinf(ref.y).sum() >= 1
    xe = R.data("exact", 10, (2, 9, 7, 5, 4), F32)
    ye = R.maxpool_ref(xe, 3, 2, 1, 0).y
    padded = np.pad(xe, ((0, 0), (1, 1), (1, 1), (1, 1), (0, 0)), constant_values=-np.inf)
    twice = sum((padded[:, a:a + 9:2, b:b + 7:2, d:d + 5:2] == ye) for a in range(3) for b in range(3) for d in range(3))
    assert (twice >= 2).sum() > 10


@pytest.mark.parametrize("mutate,kind", [("zero_pad", "rounding"), ("last_wins", "exact")])
def test_maxpool_mutations_are_seen(mutate, kind):
    hits = 0
    for k, s, p, ceil in R.POOL_CONFIGS:
        if k == 1 or (mutate == "zero_pad" and p == 0 and not ceil):
            continue                      # one-element windows have no order, unpadded floor-mode windows no padding
        x = R.data(kind, 10, (2, 9, 7, 5, 4), BF16, inf=True, mean=R.POOL_MEAN)
        good, bad = R.maxpool_ref(x, k, s, p, ceil), R.maxpool_ref(x, k, s, p, ceil, mutate=mutate)
        differ = int((good.y != bad.y).sum() + (good.code != bad.code).sum())
        print(f"maxpool {mutate} {k}/{s}/{p}/{ceil}: {differ} mismatches")
        assert differ > 0, (mutate, k, s, p, ceil)
        if mutate == "last_wins":
            dy = R.data(kind, 11, good.y.shape, BF16)
            assert (good.dx(dy)[0] != bad.dx(dy)[0]).any()
        hits += 1
    assert hits >= 6


def test_maxpool_bound_holds_for_torch_fp32():
    worst = {}
    for k, s, p, ceil in R.POOL_CONFIGS:
        for grid in R.POOL_GRIDS:
            for c, dtype in ((4, F32), (8, BF16)):
                x = R.data("rounding", 10, (2,) + grid + (c,), dtype, inf=True, mean=R.POOL_MEAN)
                ref = R.maxpool_ref(x, k, s, p, ceil)
                dy = R.data("rounding", 11, ref.y.shape, dtype)
                acc, mag, cnt = ref.dx(dy)
                r = R.ratio(R.t64(R.maxpool_dx_torch32(x, dy, k, s, p, ceil, dtype)), R.t64(acc), R.t64(R.sum_bound(cnt, mag, acc, dtype)))
                worst[dtype] = max(worst.get(dtype, 0.0), r)
                assert r <= 1.0, (k, s, p, ceil, grid, dtype, r)
    print("maxpool dx, torch fp32 evaluation: max |err| / bound", {str(d): round(v, 3) for d, v in worst.items()},
          "allowance", {str(d): R.allowance(v) for d, v in worst.items()})


# ======================================================================================================================
# upsample-add
# ======================================================================================================================
def _torch_nearest(inn, out):
    src = torch.arange(inn, dtype=F32).view(1, 1, inn)       # float32: on float64 tensors torch forms the scale in double
    return Fn.interpolate(src, size=out, mode="nearest").view(-1).long().numpy()


def test_fp32_index_rule_is_torch_nearest():
    differs = []
    for out in range(1, 65):
        for inn in range(1, 65):
            idx = R.nearest_index(out, inn)
            assert np.array_equal(idx, _torch_nearest(inn, out)), (inn, out)
            if inn <= out and not np.array_equal(idx, R.nearest_index(out, inn, "integer")):
                differs.append((inn, out))
    assert differs == sorted(R.FP32_RULE_PAIRS, key=lambda q: (q[1], q[0])), differs
    # the pair the GPU test runs really is such a pair -- and the coarse index it moves is named, so the case cannot stop covering the edge
    a, b = R.nearest_index(46, 14), R.nearest_index(46, 14, "integer")
    moved = np.nonzero(a != b)[0]
    assert moved.tolist() == [23] and a[23] == 6 and b[23] == 7, (moved, a[moved], b[moved])      # 23 * 14 / 46 is 7; (float)14 / 46 is rounded down
    for fine, coarse in R.UPSAMPLE_PAIRS:
        for f, c in zip(fine, coarse):
            assert np.array_equal(R.nearest_index(f, c), _torch_nearest(c, f)), (c, f)


@pytest.mark.parametrize("fine,coarse", R.UPSAMPLE_PAIRS)
def test_upsample_refs_match_autograd_float64(fine, coarse):
    for kind in ("exact", "rounding"):
        f = R.data(kind, 20, (2,) + fine + (4,), F32, inf=True)
        c = R.data(kind, 21, (2,) + coarse + (4,), F32)
        d = R.data(kind, 22, f.shape, F32)
        pre = R.data(kind, 23, c.shape, F32)
        ft, ct = _ncdhw(np.where(np.isfinite(f), f, 0.0)).requires_grad_(True), _ncdhw(c).requires_grad_(True)
        ix, iy, iz = (torch.from_numpy(R.nearest_index(a, b)) for a, b in zip(fine, coarse))      # the rule itself: the test above
        out = ft + ct[:, :, ix][:, :, :, iy][:, :, :, :, iz]
        out.backward(_ncdhw(d))
        finite = np.isfinite(f)
        assert np.array_equal(R.upsample_add_ref(f, c)[finite], _ndhwc(out.detach())[finite])
        assert np.array_equal(_ndhwc(ft.grad), d)
        acc, mag, cnt = R.upsample_add_bwd_ref(d, c.shape)
        assert np.abs(acc - _ndhwc(ct.grad)).max() <= 1e-13 * max(1.0, mag.max())
        assert cnt.sum() == d.size
        acc1, mag1, cnt1 = R.upsample_add_bwd_ref(d, c.shape, pre)
        assert np.abs(acc1 - (_ndhwc(ct.grad) + pre)).max() <= 1e-13 * max(1.0, mag1.max()) and np.array_equal(cnt1, cnt + 1)
        if kind == "exact":
            assert np.array_equal(acc, _ndhwc(ct.grad)) and np.array_equal(acc1, _ndhwc(ct.grad) + pre)
        for dtype in (F32, BF16):
            for p in (None, pre):
                dd, pp = R.round_to(dtype)(d), None if p is None else R.round_to(dtype)(p)
                a, m, n = R.upsample_add_bwd_ref(dd, c.shape, pp)
                r = R.ratio(R.t64(R.upsample_bwd_torch32(dd, c.shape, pp, dtype)), R.t64(a), R.t64(R.sum_bound(n, m, a, dtype)))
                print(f"upsample bwd {fine}/{coarse} {kind} {dtype} acc{int(p is not None)}: torch fp32 |err| / bound {r:.3f} -> k {R.allowance(r):.2f}")
                assert r <= 1.0
    if coarse == (7, 5, 3):
        assert (cnt == 0).sum() > 0          # coarse voxels that receive nothing


def test_integer_floor_rule_is_seen():
    fine, coarse = (46, 3, 2), (14, 2, 1)
    f, c = R.data("exact", 20, (2,) + fine + (4,), F32), R.data("exact", 21, (2,) + coarse + (4,), F32)
    d = R.data("exact", 22, f.shape, F32)
    fwd = int((R.upsample_add_ref(f, c) != R.upsample_add_ref(f, c, "integer")).sum())
    bwd = int((R.upsample_add_bwd_ref(d, c.shape)[0] != R.upsample_add_bwd_ref(d, c.shape, rule="integer")[0]).sum())
    print(f"integer-floor rule on 46/14: {fwd} forward, {bwd} backward mismatches")
    assert fwd > 0 and bwd > 0


# ======================================================================================================================
# subsample, joins, layouts
# ======================================================================================================================
@pytest.mark.parametrize("s", (1, 2, 3))
def test_subsample_refs_match_autograd(s):
    for grid in R.SUBSAMPLE_GRIDS:
        x = R.data("rounding", 30, (2,) + grid + (4,), F32, inf=True)
        xt = torch.from_numpy(np.where(np.isfinite(x), x, 0.0)).requires_grad_(True)
        y = xt[:, ::s, ::s, ::s]
        assert y.shape == R.subsample_ref(x, s).shape == (2,) + tuple((g - 1) // s + 1 for g in grid) + (4,)
        dy = R.data("rounding", 31, tuple(y.shape), F32)
        y.backward(torch.from_numpy(dy))
        assert np.array_equal(R.subsample_bwd_ref(dy, x.shape, s), xt.grad.numpy())


def test_relu_mask_and_its_mutation():
    for dtype in (F32, BF16):
        y = R.plant_mask(R.data("rounding", 40, (1028,), dtype), dtype)
        dy = R.data("rounding", 41, (1028,), dtype)
        dy[[R.MASKS[n] for n in R.MASKS]] = 2.5
        g = R.relu_backward_ref(y, dy)
        assert [g[R.MASKS[n]] for n in ("neg_zero", "pos_zero", "denormal", "negative", "positive")] == [0.0, 0.0, 2.5, 0.0, 2.5]
        yt = torch.from_numpy(y).requires_grad_(True)          # torch's relu gradient is the same mask on a value that is its own relu
        torch.relu(yt).backward(torch.from_numpy(dy))
        assert np.array_equal(g, yt.grad.numpy())
        bad = R.relu_backward_ref(y, dy, mutate="ge")
        print(f"mask y >= 0 ({dtype}): {int((bad != g).sum())} mismatches")
        assert bad[R.MASKS["neg_zero"]] == 2.5 and bad[R.MASKS["pos_zero"]] == 2.5 and (bad != g).sum() >= 2


def test_layout_refs_are_the_permutation():
    x = R.rounding(50, (2, 5, 315), F32, inf=True)
    cl = R.to_channels_last_ref(x, F32)
    assert cl.shape == (2, 315, 5) and np.array_equal(cl, torch.from_numpy(x).permute(0, 2, 1).numpy())
    assert np.array_equal(R.to_channels_first_ref(cl), x)
    want = torch.from_numpy(x).to(F32).permute(0, 2, 1).to(BF16)
    assert torch.equal(R.bits(R.to_torch(R.to_channels_last_ref(x, BF16), BF16)), R.bits(want))
    assert (R.to_channels_last_ref(x, BF16) != cl).sum() > 1000 and R.to_channels_last_ref(x, BF16).reshape(-1)[0] == R.round_to(BF16)(x[0, 0, 0])


def test_exact_data_sums_are_exact():
    e = R.exact(1, (100000,))
    assert np.abs(e).max() == R.EXACT_MAX and np.array_equal(e * 8, np.round(e * 8)) and (e < 0).any()
    # any order of fp32 additions gives the float64 sum: 105 terms (the largest sum of the GPU test) stay far below 2^24 eighths
    t = torch.from_numpy(e[:105 * 900].reshape(900, 105)).to(F32)
    fwd, rev = torch.zeros(900), torch.zeros(900)
    for j in range(105):
        fwd, rev = fwd + t[:, j], rev + t[:, 104 - j]
    assert torch.equal(fwd.double(), t.double().sum(1)) and torch.equal(rev, fwd) and 105 * 64 < 2 ** 24
