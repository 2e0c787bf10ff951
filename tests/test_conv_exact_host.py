"""CPU only: the float64 conv reference of tests/conv_ref.py is anchored against torch's float64 convolution and its autograd (EQUAL), torch's
fp32 CPU convolution reaches the same equality (so an fp32 implementation that is not the code under test can), every family member
satisfies its exactness condition and is not vacuous, and every mutation of the reference breaks equality.  The row-list cases of the cone
head's kernels (conv_ref.ROW_CASES) get the same treatment on their lists: the device list format against the oracle's derivation, exactness
on the listed rows, the data rules, the plan each case must reach (through the size queries, which need no GPU) and the row-list mutations.
``-s`` prints the measured figures that stand in conv_ref's docstring."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr

BF, F32 = torch.bfloat16, torch.float32


def _torch_conv(m, dt, x=None, w=None, gy=None, bias=True):
    """conv (+ autograd) of member m in dtype dt through torch, segment by segment -> acc + bias rows, dx rows, dw, db."""
    x = (m.x if x is None else x).to(dt)
    gy = (m.gy if gy is None else gy).to(dt)
    w = (m.w if w is None else w).to(dt).clone().requires_grad_(True)
    b = (m.bias if bias else torch.zeros_like(m.bias)).to(dt).clone().requires_grad_(True)
    ys, dxs, oi, oo = [], [], 0, 0
    for (X, Y, Z), (OX, OY, OZ) in zip(m.geom.segs, m.geom.osegs):
        xi = x[oi:oi + X * Y * Z].view(1, X, Y, Z, m.cin).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        y = F.conv3d(xi, w, b, stride=m.stride, padding=m.k // 2)
        g = gy[oo:oo + OX * OY * OZ].view(1, OX, OY, OZ, m.cout).permute(0, 4, 1, 2, 3)
        y.backward(g)
        ys.append(y.detach().permute(0, 2, 3, 4, 1).reshape(-1, m.cout))
        dxs.append(xi.grad.permute(0, 2, 3, 4, 1).reshape(-1, m.cin))
        oi, oo = oi + X * Y * Z, oo + OX * OY * OZ
    return torch.cat(ys).double(), torch.cat(dxs).double(), w.grad.double(), b.grad.double()


def _mine(m, geom=None):
    geom = geom or m.geom
    y = cr.conv_acc(m.x, m.w, geom) + m.bias
    dx = cr.conv_acc(m.gy, cr.flip_t(m.w), cr.Geometry(geom.segs, m.k, 1)) if m.stride == 1 else None
    dw, db = cr.conv_dw(m.x, m.gy, geom)
    return y, dx, dw, db


@pytest.mark.parametrize("name", cr.HOST_FULL)
def test_reference_equals_torch_fp64_and_torch_fp32_reaches_equality(name):
    m = cr.get(name)
    mine = _mine(m)
    for dt in (torch.float64, torch.float32):
        if m.kind == "x3" and dt == torch.float32:
            continue        # the full product of two 11-bit operands at K = 27 Cin is no fp32 number: the split terms are checked below
        got = _torch_conv(m, dt)
        for nm, a, b in zip(("y", "dx", "dw", "db"), got, mine):
            if b is None:          # the stem has no input gradient in this model; torch's is still checked against the definition
                b = _stem_dx(m)
            assert torch.equal(a, b), (name, dt, nm, cr.first_diff(a, b))
    if m.kind == "x3":
        xh, xl = cr.split(m.x)
        wh, wl = cr.split(m.w)
        gh, gl = cr.split(m.gy)
        assert ((xl != 0).double().mean() >= 0.5) and ((wl != 0).double().mean() >= 0.5) and ((gl[m.gy[:, 0] != 0] != 0).double().mean() >= 0.5)
        y = dx = dw = 0
        for (xa, wa, ga) in ((xh, wh, gh), (xh, wl, gh), (xl, wh, gl)):      # y: hi hi + hi lo + lo hi; each term through torch fp32
            y = y + _torch_conv(m, torch.float32, x=xa, w=wa, bias=False)[0].float()
        ref = m.reference(False, F32, x3=True)
        assert torch.equal(y.double() + m.bias, ref["pre"]), cr.first_diff(y.double() + m.bias, ref["pre"])
        for (ga, wa) in ((gh, wh), (gh, wl), (gl, wh)):
            dx = dx + _torch_conv(m, torch.float32, gy=ga, w=wa, bias=False)[1].float()
        assert torch.equal(dx.double(), ref["dx"]), cr.first_diff(dx.double(), ref["dx"])
        for (xa, ga) in ((xh, gh), (xl, gh), (xh, gl)):
            dw = dw + _torch_conv(m, torch.float32, x=xa, gy=ga, bias=False)[2].float()
        assert torch.equal(dw.double(), ref["dw"]), cr.first_diff(dw.double(), ref["dw"])


def _stem_dx(m):
    """dx of a strided conv from its definition: scatter gy[v] w[:, :, off] into x[v * s + off]."""
    dx = torch.zeros_like(m.x)
    for t in m.geom.taps():
        idx, ok = m.geom.tap(t)
        dx.index_add_(0, idx[ok], (m.gy @ m.w[:, :, t[0], t[1], t[2]])[ok])
    return dx


def test_row_subset_and_k_slices_are_the_same_sums():
    m = cr.get("g765_c64_96")
    full = m.acc()
    rows = torch.tensor([0, 5, 209, 210, 419]).numpy()
    assert torch.equal(m.acc(rows), full[rows])
    K = 27 * m.cin
    parts = [m.acc(krange=(a, min(K, a + 300))) for a in range(0, K, 300)]
    assert torch.equal(sum(parts), full)


def _exact_figures(m):
    """-> dict of the largest sum|a||b| (in units of the member's lowest product bit) of y, folded y, dx, dw, db."""
    u = m.unit
    x, w, gy = m.x, m.w, m.gy
    if m.kind == "x3":       # kept terms only: |hi||hi| + |hi||lo| + |lo||hi|, hi / lo of the signed operands
        def mag(a, b, fn):
            (ah, al), (bh, bl) = cr.split(a), cr.split(b)
            return fn(ah.abs(), bh.abs()) + fn(ah.abs(), bl.abs()) + fn(al.abs(), bh.abs())
    else:
        mag = lambda a, b, fn: fn(a.abs(), b.abs())
    fig = {"y": (mag(x, w, lambda a, b: cr.conv_acc(a, b, m.geom)) + m.bias.abs()).max().item() / u}
    # acc * scale is exact (a power of two); the lowest bit of acc * scale + shift is scale * u (shift is a multiple of it)
    fig["y_fold"] = (mag(x, w, lambda a, b: cr.conv_acc(a, b, m.geom)) + m.shift.abs() / m.scale).max().item() / u
    if m.k != 7:             # the stem reads the network's input: it has no input gradient
        fig["dx"] = mag(gy, w, lambda a, b: cr.conv_dx(a, b, m.geom)).max().item() / u
    fig["dw"] = mag(x, gy, lambda a, b: cr.conv_dw(a, b, m.geom)[0]).max().item() / u
    fig["db"] = gy.abs().sum(0).max().item()
    return fig


@pytest.mark.parametrize("name", cr.names())
def test_exact_ok(name):
    """sum|a||b| < 2^24 (in units of the lowest product bit) for every element of y, dx, dw, db: measured for the members of HOST_FULL, by
    the rigorous bound K max|a| max|b| for the large ones."""
    m = cr.get(name)
    if name in cr.HOST_FULL:
        fig = _exact_figures(m)
    else:
        K, ax, aw, ag = m.k ** 3 * m.cin, m.x.abs().max().item(), m.w.abs().max().item(), m.gy.abs().max().item()
        rows = int((m.gy.abs().sum(1) != 0).sum())
        fig = {"y": (K * ax * aw + m.bias.abs().max().item()) / m.unit,
               "y_fold": (K * ax * aw + (m.shift.abs() / m.scale).max().item()) / m.unit,
               "dx": m.k ** 3 * m.cout * ag * aw / m.unit, "dw": rows * ax * ag / m.unit, "db": rows * ag}
        if max(fig.values()) >= cr.TWO24:       # the bound is too coarse for this member (f32 family): measure
            fig = _exact_figures(m)
    print(f"[exact_ok] {name:22s} " + " ".join(f"{k}={v:.4g}" for k, v in fig.items()))
    assert max(fig.values()) < cr.TWO24, fig
    for t in (m.x, m.w, m.gy, m.bias, m.shift):
        assert torch.equal(t.float().double(), t)
        if t is not m.shift and m.kind in ("i8", "st"):
            assert torch.equal(t.bfloat16().double(), t)       # the bf16 kernels read these operands unchanged
    if m.kind == "st":
        y = cr.store(m.pre(), BF)
        top = cr.stats_exact_ok(y)            # statistics are a training-mode feature: the folded (eval) epilogue never asks for them
        print(f"[exact_ok] {name:22s} largest sum of 128 y_stored^2 of a channel = {top:.4g}")
        assert top < cr.TWO24


@pytest.mark.parametrize("name", cr.names())
def test_members_are_not_vacuous(name):
    """Every member.  Two conditions cannot hold for the st family and are not asked of it: 128 y^2 < 2^24 keeps |y| below 362, so few of its
    outputs need a bf16 rounding (the i8 members carry the rounding checks, on the same kernels)."""
    m = cr.get(name)
    rows = None
    if m.geom.m_out > 20000:          # the 50 x 50 x 33 member: the rows the GPU test compares are a subset as well
        rows = torch.randperm(m.geom.m_out, generator=torch.Generator().manual_seed(1))[:4096].numpy()
    if m.kind == "x3":
        kept, lolo = cr.x3_terms(m.x, m.w, lambda a, b: cr.conv_acc(a, b, m.geom, rows))
        pre = kept + m.bias
    else:
        pre = m.pre(rows)
    le0, eq0 = (pre <= 0).double().mean().item(), (pre == 0).double().mean().item()
    line = f"[shares] {name:22s} pre<=0 {100 * le0:.1f}% pre==0 {100 * eq0:.3f}%"
    assert le0 >= 0.30 and eq0 > 0
    assert (m.bias != 0).all() and (m.shift != 0).all() and (m.scale != 1).all()
    assert torch.equal(torch.log2(m.scale), torch.log2(m.scale).round())
    if not m.ragged:                 # every face of the grid has nonzero inputs
        v = m.nchw(m.x, out=False)
        for f in (v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1], v[:, :, :, 0], v[:, :, :, -1]):
            assert (f != 0).any()
    else:
        o = 0
        for (X, Y, Z) in m.geom.segs:
            v = m.x[o:o + X * Y * Z].view(X, Y, Z, -1)
            for f in (v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1]):
                assert (f != 0).any()
            o += X * Y * Z
    if m.kind in ("i8", "st"):
        rnd = (cr.store(pre, BF) != pre).double().mean().item()
        up, dn = cr.store(pre, BF, "half_up"), cr.store(pre, BF, "trunc")
        ties = (((pre - dn).abs() == (up - pre).abs()) & (up != dn) & (dn != pre)).double().mean().item()
        line += f" bf16 rounds {100 * rnd:.1f}% ties {100 * ties:.1f}%"
        if m.kind == "i8":
            assert rnd >= 0.25 and ties >= 0.05
        else:
            assert rnd > 0 and ties > 0
    if m.kind == "f32":
        for t in (m.x, m.w, m.gy):
            assert ((t.abs() > 256) & (t.bfloat16().double() != t)).double().mean().item() > 0.005      # a bf16 copy of the operand is another tensor
    if m.kind == "x3":
        for t in (m.x, m.w):
            assert (cr.split(t)[1] != 0).double().mean().item() >= 0.5
        share = (lolo != 0).double().mean().item()
        line += f" lo*lo != 0 on {100 * share:.1f}%"
        assert share >= 0.5
    print(line)


# ----------------------------------------------------------------------------------------------------------------------
# mutations: each must break equality on every member it applies to
# ----------------------------------------------------------------------------------------------------------------------
def _share(a, b):
    return (a != b).double().mean().item()


def _mutations(m):
    """-> {mutation: share of elements changed} for member m."""
    out = {}
    K = m.k ** 3 * m.cin
    acc = m.acc()
    pre = acc + m.bias
    out["bias dropped"] = _share(acc, pre)
    out["bias once per K slice"] = _share(cr.epilogue(acc, m.bias, bias_times=3), pre)
    w1 = m.w.clone()
    w1[:, -1, m.k // 2, 0, m.k - 1] = 0
    out["last channel of one tap dropped"] = _share(m.acc(w=w1), acc)
    if m.cin >= 32:
        out["last K-step (32 channels) dropped"] = _share(m.acc(krange=(0, K - 32)), acc)
    if m.stride == 1 and m.k == 3:
        out["dgrad with unflipped taps"] = _share(cr.conv_dx(m.gy, m.w, m.geom, flipped=False), cr.conv_dx(m.gy, m.w, m.geom))
    if m.k > 1:
        wrapped = m.acc(geom=cr.Geometry(m.geom.segs, m.k, m.stride, wrap=True))
        out["zero padding -> wrap-around"] = _share(wrapped, acc)
        if m.ragged or m.n == 2:                 # the batch boundary is one of the wrapped faces: scene 0's last / scene 1's first row
            last0 = m.geom.osegs[0][0] * m.geom.osegs[0][1] * m.geom.osegs[0][2]
            assert (wrapped[last0 - 1] != acc[last0 - 1]).any() and (wrapped[last0] != acc[last0]).any()
    if m.ragged and m.k > 1:                     # (1x1x1 reads no neighbour: the two are the same sums)
        out["ragged read as one dense grid"] = _share(m.acc(geom=cr.Geometry([(m.geom.m_in, 1, 1)], m.k)), acc)
    if m.geom.m_out % 256:
        y = pre.clone()
        y[m.geom.m_out // 256 * 256:] = 0
        out["last partial 256-row tile unwritten"] = _share(y, pre)
    if m.kind in ("i8", "st"):
        ok = cr.store(pre, BF)
        if m.k > 1:
            out["bf16 store by truncation"] = _share(cr.store(pre, BF, "trunc"), ok)
            out["bf16 store by round-half-up"] = _share(cr.store(pre, BF, "half_up"), ok)
            parts = [cr.store(m.acc(krange=(a, min(K, a + -(-K // 3)))), BF) for a in range(0, K, -(-K // 3))]
            out["K-slice partials rounded to bf16"] = _share(sum(parts) + m.bias, pre)
    fold = m.pre(fold=True)
    out["(acc + shift) * scale"] = _share(cr.epilogue(acc, m.shift, m.scale, swapped=True), fold)
    if m.kind == "st":
        a, b = cr.stats_partials(cr.store(pre, BF), 128), cr.stats_partials(pre, 128)
        out["statistics from the accumulator"] = _share(a.sum(0), b.sum(0))
    if m.kind == "x3":
        r = m.reference(False, F32, x3=True)
        out["lo*lo included"] = _share(r["pre"] + r["y_lolo"], r["pre"])
        xh, _ = cr.split(m.x)
        wh, _ = cr.split(m.w)
        out["lo terms dropped"] = _share(cr.conv_acc(xh, wh, m.geom) + m.bias, r["pre"])
        out["dw: lo*lo included"] = _share(r["dw"] + r["dw_lolo"], r["dw"])
    return out


@pytest.mark.parametrize("name", cr.HOST_FULL)
def test_every_mutation_breaks_equality(name):
    m = cr.get(name)
    res = _mutations(m)
    for k, v in res.items():
        print(f"[mutation] {name:22s} {k:38s} changes {100 * v:6.2f}% of the elements")
        assert v > 0, (name, k)


# ----------------------------------------------------------------------------------------------------------------------
# row lists (the row-list conv kernels of the cone head)
# ----------------------------------------------------------------------------------------------------------------------
ROW_IDS = [f"{m}-{l}" for m, l, _, _ in cr.ROW_CASES]


def _rows_plan(m, rl, dtype, swap=False):
    from nerf_rpn_amd import lib
    if not os.path.exists(lib.SO_PATH):
        lib.build()
    ci, co = (m.cout, m.cin) if swap else (m.cin, m.cout)
    return cr.rows_plan_class(lib.query("conv3d_fwd_rows_workspace_bytes", rl.n, ci, co, m.k, lib.BF16 if dtype == BF else lib.F32), rl.n, co)


def test_tap_words_equal_the_oracle_lists():
    """Two derivations of one format: conv_ref.cone_sets / tap_words against oracle.cone.cone_lists on the cone sample."""
    from oracle import cone as OC
    pos, neg = cr.cone_sample()
    want = OC.cone_lists(pos, neg, cr.CONE_GRIDS, cr.CONE_ANCHORS, 2)
    prev = 0
    for k, (ids, words) in enumerate(want):
        rl = cr.row_list(f"cone{k}")
        assert rl.words.dtype == np.uint32 and rl.words.shape == (len(ids), 2)
        np.testing.assert_array_equal(rl.words[:, 0], ids)
        np.testing.assert_array_equal(rl.words[:, 1], words)
        assert rl.n > prev and np.isin(cr.row_list(f"cone{max(k - 1, 0)}").ids, rl.ids).all()
        prev = rl.n
    # the other lists: bit 13 set, segment ids in order, and the word of a listed voxel says what Geometry says
    for name in ("ragA", "ragB", "r26", "w2100"):
        rl = cr.row_list(name)
        g = cr.Geometry(rl.segs)
        for j, t in enumerate(g.taps()):
            _, ok = g.tap(t, rl.ids)
            np.testing.assert_array_equal((rl.words[:, 1] >> np.uint32(j)) & 1, ok.numpy().astype(np.uint32))
        assert (np.diff((rl.words[:, 1] >> np.uint32(27)).astype(np.int64)) >= 0).all()


@pytest.mark.parametrize("name,lname,fwd,wgrad", cr.ROW_CASES, ids=ROW_IDS)
def test_row_lists_exact_ok(name, lname, fwd, wgrad):
    """sum|a||b| < 2^24 for y and dx on the evaluated rows of the list and for dw, db over the listed rows (+ 8: the second weight-gradient
    call of the GPU test accumulates onto integers in [-8, 8])."""
    m, rl = cr.get(name), cr.row_list(lname)
    gy, vox, u = rl.gy(m), rl.vox(), m.unit
    if m.kind == "x3":
        def mag(a, b, fn):
            (ah, al), (bh, bl) = cr.split(a), cr.split(b)
            return fn(ah.abs(), bh.abs()) + fn(ah.abs(), bl.abs()) + fn(al.abs(), bh.abs())
    else:
        mag = lambda a, b, fn: fn(a.abs(), b.abs())
    fig = {}
    if fwd:
        fig["y"] = (mag(m.x, m.w, lambda a, b: cr.conv_acc(a, b, m.geom, vox)) + m.bias.abs()).max().item() / u
        fig["dx"] = mag(gy, m.w, lambda a, b: cr.conv_dx(a, b, m.geom, vox)).max().item() / u
    if wgrad:
        fig["dw"] = mag(m.x, gy, lambda a, b: cr.conv_dw(a, b, m.geom, rl.ids)[0]).max().item() / u + 8
        fig["db"] = gy[rl.ids].abs().sum(0).max().item() + 8
    print(f"[rows exact_ok] {name:18s} {lname:6s} n={rl.n:5d} " + " ".join(f"{k}={v:.4g}" for k, v in fig.items()))
    assert max(fig.values()) < cr.TWO24, fig
    assert torch.equal(gy.float().double(), gy) and (m.kind != "i8" or torch.equal(gy.bfloat16().double(), gy))


@pytest.mark.parametrize("name,lname,fwd,wgrad", cr.ROW_CASES, ids=ROW_IDS)
def test_row_cases_reach_their_plans(name, lname, fwd, wgrad):
    """The plans of conv_plan.h through the size queries (pure host functions): the short lists run on K slices, the 16421-row list unsliced
    at Cout 128 (129 tiles) and with its last tile on 4 K slices at Cout 512 (516 tiles = 512 + 4), 1x1x1 never sliced; the weight gradients
    of the 2100-row list on >= 2 slices, and the 256 x 256 bf16 weight gradient in its 256x256 form from 5057 rows on (80 chunks of 64 rows:
    wgrad_plan tries k <= chunks / 16 slices and needs k >= 5 to fill half a round of the chip with 27 k tiles)."""
    from nerf_rpn_amd import lib
    m, rl = cr.get(name), cr.row_list(lname)
    dt = F32 if m.kind in ("f32", "x3") else BF
    if fwd:
        want = cr.ROW_PLANS.get(f"{name}-{lname}", (("ksplit",), ("ksplit",)))
        got = _rows_plan(m, rl, dt)
        print(f"[rows plan] {name:18s} {lname:6s} n={rl.n:5d} forward {got}")
        assert got[:len(want[0])] == want[0], got
        if (m.cout * (2 if dt == BF else 4)) % 128 == 0:
            got = _rows_plan(m, rl, dt, swap=True)
            print(f"[rows plan] {name:18s} {lname:6s} n={rl.n:5d} dgrad   {got}")
            assert got[:len(want[1])] == want[1], got
    if wgrad:
        code = lib.BF16 if m.kind in ("i8", "x3") else lib.F32       # the bf16x3 weight gradient runs three bf16 launches
        a = (1, rl.n, 1, 1, m.cin, m.cout, m.cout, m.k, code)
        slices, big = lib.query("conv3d_wgrad_slices", *a), lib.query("conv3d_wgrad_plan", *a)
        print(f"[rows plan] {name:18s} {lname:6s} n={rl.n:5d} wgrad slices {slices} 256x256 form {big}")
        assert big == (1 if lname == "r18" else 0)
        assert slices >= (5 if lname == "r18" else 2 if lname == "w2100" else 1)
    if lname == "r18":              # the threshold of the 256x256 row-list form at Cin = Cout = 256
        q = lambda n: lib.query("conv3d_wgrad_plan", 1, n, 1, 1, 256, 256, 256, 3, lib.BF16)
        assert q(5057) == 1 and q(5056) == 0 and q(300) == 0


@pytest.mark.parametrize("name,lname,fwd,wgrad", cr.ROW_CASES, ids=ROW_IDS)
def test_row_lists_are_not_vacuous(name, lname, fwd, wgrad):
    """The data rules of the row-list cases: a listed row reads a voxel that is NOT listed (so x indexed by list position is another tensor;
    impossible for the two lists that hold every voxel), a listed row on each of the six faces of a segment that is more than one voxel
    deep there, gy nonzero on listed rows of the last partial tile and the last partial chunk, and gy nonzero off the list."""
    m, rl = cr.get(name), cr.row_list(lname)
    listed, gy = rl.listed(), rl.gy(m)
    assert rl.n % 128 and rl.n % 64 and rl.n % 32            # a partial tile and a partial chunk of either element size
    if not rl.whole:
        g, hit = cr.Geometry(rl.segs), 0
        for t in g.taps():
            idx, ok = g.tap(t, rl.ids)
            hit += int((ok.numpy() & ~listed[idx.numpy()]).sum())
        assert hit > 0 and not (rl.ids == np.arange(rl.n)).all()
        assert (gy[~listed] != 0).any()
    co = m.geom.co[rl.ids]
    for d in range(3):
        deep = co[:, 3 + d] > 1
        assert (deep & (co[:, d] == 0)).any() and (deep & (co[:, d] == co[:, 3 + d] - 1)).any(), (lname, d)
    for chunk in (rl.tile, 128, 64, 32):
        assert (gy[rl.ids[rl.n // chunk * chunk:]] != 0).any(), chunk
    assert (gy[rl.ids[0]] != 0).any() or (gy[rl.ids[:32]] != 0).any()
    if lname == "cone0":
        assert (~rl.reads()).sum() > 0                       # voxels no tap of the list reads: the GPU test holds NaN there
    print(f"[rows] {name:18s} {lname:6s} n={rl.n:5d} of {rl.total}: {100 * rl.reads(m.k).mean():.1f}% of the voxels read, "
          f"gy != 0 on {100 * (gy[rl.ids] != 0).any(1).double().mean().item():.1f}% of the listed rows")


def _one_grid(rl):
    return len(rl.segs) == 1


def _row_mutations(m, rl, fwd, wgrad):
    out = {}
    vox, ev, gy = rl.vox(), rl.ev, rl.gy(m)
    if fwd:
        acc = m.acc(vox)
        pre = acc + m.bias
        if m.k == 3:
            out["rows: tap word ignored"] = _share(m.acc(vox, geom=cr.Geometry(rl.segs, 3, 1, wrap=True)), acc)
            if len({s[1:] for s in rl.segs}) > 1:
                out["rows: segment id ignored"] = _share(m.acc(vox, geom=cr.Geometry(rl.segs, 3, 1, seg0=True)), acc)
        if not rl.whole:
            out["rows: x by list position"] = _share(cr.conv_acc(m.x, m.w, m.geom, vox, shift=ev - vox), acc)
            a, b = torch.zeros(rl.total, m.cout, dtype=torch.float64), torch.zeros(rl.total, m.cout, dtype=torch.float64)
            a[vox], b[ev] = pre, pre
            out["rows: y by list position"] = _share(b, a)
            out["rows: ReLU mask by list position"] = _share(cr.epilogue(acc, m.bias, mask=m.gy[ev]), cr.epilogue(acc, m.bias, mask=m.gy[vox]))
        y = pre.clone()
        y[ev >= rl.n // rl.tile * rl.tile] = 0
        out["rows: last partial tile unwritten"] = _share(y, pre)
        plan = _rows_plan(m, rl, F32 if m.kind in ("f32", "x3") else BF)
        if plan[0] == "tail":
            ks, tail = plan[1], ev >= plan[2] * 128
            y = pre.clone()
            y[tail] = acc[tail] + m.bias * ks
            out["rows: bias once per K slice on the tail rows"] = _share(y[tail], pre[tail])
            nk = 27 * m.cin // 64                      # K-steps of 128 bytes; the slices hold ceil(nk / ks) of them
            per = -(-nk // ks) * 64
            out["rows: tail rows summed without the first slice"] = _share(m.acc(vox[tail], krange=(per, nk * 64)), acc[tail])
            last = _share(m.acc(vox[tail], krange=(0, per * (ks - 1))), acc[tail])
            if _one_grid(rl):
                # an ascending list over ONE grid ends on the face x = X - 1: the taps 18..26 of its last rows -- all of the last slice at
                # Cin 64 -- are out of bounds, and the mutation cannot show; the two-grid list next to it is there for this
                assert last == 0 and ks == 4 and m.cin == 64
            else:
                out["rows: tail rows summed without the last slice"] = last
    if wgrad and not rl.whole:
        fn = lambda a, b, rows: cr.conv_dw(a, b, m.geom, rows)[0]
        if m.kind == "x3":
            dw, dw_all = (cr.x3_terms(m.x, gy, lambda a, b: fn(a, b, r))[0] for r in (rl.ids, None))
        else:
            dw, dw_all = fn(m.x, gy, rl.ids), fn(m.x, gy, None)
        out["rows: dW over all rows"] = _share(dw_all, dw)
        out["rows: db over all rows"] = _share(gy.sum(0), gy[rl.ids].sum(0))
    if wgrad and m.kind == "x3":
        kept, lolo = cr.x3_terms(m.x, gy, lambda a, b: cr.conv_dw(a, b, m.geom, rl.ids)[0])
        out["rows: dw lo*lo included"] = _share(kept + lolo, kept)
    return out


@pytest.mark.parametrize("name,lname,fwd,wgrad", cr.ROW_CASES, ids=ROW_IDS)
def test_every_row_list_mutation_breaks_equality(name, lname, fwd, wgrad):
    m, rl = cr.get(name), cr.row_list(lname)
    res = _row_mutations(m, rl, fwd, wgrad)
    assert res
    for k, v in res.items():
        print(f"[mutation] {name:18s} {lname:6s} {k:48s} changes {100 * v:6.2f}% of the elements")
        assert v > 0, (name, lname, k)
