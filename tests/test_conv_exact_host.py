"""CPU only: the float64 conv reference of tests/conv_ref.py is anchored against torch's float64 convolution and its autograd (EQUAL), torch's
fp32 CPU convolution reaches the same equality (so an fp32 implementation that is not the code under test can), every family member
satisfies its exactness condition and is not vacuous, and every mutation of the reference breaks equality.  ``-s`` prints the measured
figures that stand in conv_ref's docstring."""
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
    if m.ragged:
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
