"""Host side of tests/test_gpu_roi_kernels.py (no GPU): the float64 references of tests/roi_ref.py are anchored -- RoIAlign to oracle/roialign
(an fp32 restatement of the reference op, parity unpinned) and, independently, to closed forms (an affine map pools to the affine function
at each bin's centroid for any angle; the zeroth and first moments of the backward); ROIPool to oracle/roipool.py (pinned bit-exact to the
reference's outputs), forward and through autograd -- and their per-element bounds are shown to be satisfiable (the torch fp32 evaluation of
the kernels' expressions stays inside every bound; its worst |err| / bound r is printed: run with -s) and sharp (one mutation per decision
lands outside 2 x bound on a stated share of the elements or breaks an equality).  The caps on undecided elements are asserted here on
every fixture: at most 1 % for the random families, none for the exact ones."""
import math

import pytest
import torch

import roi_ref as R

F32, F64 = torch.float32, torch.float64
ALIGN = R.align_cases()
POOL = {kind: R.pool_cases(kind) for kind in ("aabb", "pooling", "interpolation")}
_cache = {}


def align(name, bf16=False):
    key = (name, bf16)
    if key not in _cache:
        c = ALIGN[name]()
        feat, top = (R.bf16_round(c.feat), R.bf16_round(c.top)) if bf16 else (c.feat, c.top)
        _cache[key] = (c, R.align_case(feat, c.rois, c.scale, c.pooled, c.sampling, top, bf16=bf16, exact=c.exact))
    return _cache[key]


def pool(kind, name, bf16=False):
    key = (kind, name, bf16)
    if key not in _cache:
        c = POOL[kind][name]()
        feats = [R.bf16_round(f) for f in c.feats] if bf16 else c.feats
        args = (kind, feats, c.meta, c.level_of, c.scales, c.out_size)
        _cache[key] = (c, R.pool_eval(*args, F64, c.dout, bf16=bf16, exact=c.exact), R.pool_eval(*args, F32, c.dout, bf16=bf16, exact=c.exact))
    return _cache[key]


def close(got, want, floor, decided=None):
    """|got - want| <= 1e-6 |want| + floor per element: the oracles evaluate in fp32, so the floor is the element's own derived fp32 bound
    (an element that is small by cancellation carries the rounding of its terms, not of itself)."""
    ok = (got - want).abs() <= 1e-6 * want.abs() + floor
    return bool((ok if decided is None else ok[decided]).all())


def share_outside(got, want, bound, decided, k=2.0):
    m = R._ratio((got.double() - want).abs()[decided], k * bound[decided])
    return (m > 1).double().mean().item()


# ======================================================================================================================
# anchors
# ======================================================================================================================
@pytest.mark.parametrize("name", ["exact", "exact-half", "random-c4", "random-c12-half", "right-angles", "bad-batch"])
def test_align_reference_agrees_with_the_c_oracle(name):
    from oracle import roialign as OR
    c, o = align(name)
    ok = o.geo.good
    x = c.feat.permute(0, 4, 1, 2, 3).contiguous()
    N, C = x.shape[:2]
    rois = c.rois[ok]
    ref = OR.roi_align_rotated_3d_forward(x, rois, c.scale, c.pooled, c.sampling).permute(0, 2, 3, 4, 1).reshape(-1, o.geo.nbins, C)
    top = c.top[ok].permute(0, 4, 1, 2, 3).contiguous()
    gref = OR.roi_align_rotated_3d_backward(top, rois, c.scale, c.pooled, tuple(x.shape), c.sampling).permute(0, 2, 3, 4, 1).reshape(-1, C)
    if c.exact:
        assert torch.equal(o.out[ok], ref.double()) and torch.equal(o.grad, gref)
        return
    assert close(o.out[ok], ref.double(), o.out_bound[ok], o.out_decided[ok])
    assert close(o.grad, gref, o.grad_bound, o.grad_decided)


@pytest.mark.parametrize("theta", [0.0, 33.0, -117.5, 90.0])
def test_align_reference_on_an_affine_map_equals_the_closed_form(theta):
    """Samples inside [0, dim - 1]: trilinear interpolation reproduces an affine function, so a bin is the function at the centroid of
    its samples = the bin's centre in the rotated frame; the backward conserves sum(top) and the first moments."""
    dims, pooled = (7, 6, 5), (2, 3, 2)
    a = torch.tensor([0.75, -1.25, 0.5], dtype=F64)          # dyadic: the fp32 map holds the function exactly
    ii = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=F64) for n in dims], indexing="ij"), -1)
    feat = ((ii * a).sum(-1) + 2.5)[None, ..., None].repeat(1, 1, 1, 1, 4).float()
    rois = torch.tensor([[0, 3.0, 2.5, 2.0, 2.5, 2.0, 1.5, theta], [0, 3.25, 2.5, 2.0, 1.0, 3.0, 2.5, theta]])
    top = torch.randn(2, *pooled, 4, generator=torch.Generator().manual_seed(1))
    for sampling in (0, 2):
        o = R.align_case(feat, rois, 1.0, pooled, sampling, top, want32=False)
        assert o.geo.valid.all() and (o.geo.pos >= 0).all() and (o.geo.pos <= torch.tensor(dims, dtype=F64) - 1).all()
        th = (rois[:, 7].double() * math.pi / 180).float().double()
        p = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=F64) for n in pooled], indexing="ij"), -1).reshape(-1, 3)
        e, c = rois[:, 4:7].double(), rois[:, 1:4].double()
        loc = -e[:, None] / 2 + (p[None] + 0.5) * e[:, None] / torch.tensor(pooled, dtype=F64)
        cx = loc[..., 0] * th.cos()[:, None] + loc[..., 1] * th.sin()[:, None] + c[:, None, 0]
        cy = loc[..., 1] * th.cos()[:, None] - loc[..., 0] * th.sin()[:, None] + c[:, None, 1]
        cz = loc[..., 2] + c[:, None, 2]
        want = a[0] * cx + a[1] * cy + a[2] * cz + 2.5
        assert (o.out[..., 0] - want).abs().max().item() <= 1e-12
        t64 = top.double().reshape(2, -1, 4)
        g = o.grad.reshape(*dims, 4)
        assert (g.sum((0, 1, 2)) - t64.sum((0, 1))).abs().max().item() <= 1e-12
        for ax, cen in enumerate((cx, cy, cz)):
            mom = (g * ii[..., ax, None]).sum((0, 1, 2))
            assert (mom - (t64 * cen[..., None]).sum((0, 1))).abs().max().item() <= 1e-11


@pytest.mark.parametrize("kind,name", [(kind, name) for kind in POOL for name in ("exact", "exact-222", "random-c3", "random-c32", "right-angles") if name in POOL[kind]])
def test_pool_reference_agrees_with_the_pinned_oracle(kind, name):
    from oracle.roipool import ROIPoolOracle
    c, o, _ = pool(kind, name)
    rot = kind != "aabb"
    keep = torch.ones(c.rois.shape[0], dtype=torch.bool)
    if not rot:
        # the oracle (like the reference) raises on an empty crop, where the kernel pools zeros: those rows are left out on its side and
        # carry no upstream gradient on the side of roi_ref, so the gradients of every level compare in full
        keep = (c.meta[:, 3:] > 0).all(1)
        assert keep.any() and not o.out[~keep].any()
        dout = c.dout * keep[:, None, None, None, None]
        o = R.pool_eval(kind, c.feats, c.meta, c.level_of, c.scales, c.out_size, F64, dout, exact=c.exact)
    feats = [f.permute(3, 0, 1, 2).clone().requires_grad_(True) for f in c.feats]
    orc = ROIPoolOracle(list(c.out_size), c.scales, 0.0 if rot else 0.2, rot, kind if rot else "pooling")
    rows = c.rois[keep].clone()
    oo = orc([feats], rows[None] if rot else [rows])[0]
    (oo * c.dout[keep].permute(0, 4, 1, 2, 3)).sum().backward()
    got = o.out[keep].permute(0, 4, 1, 2, 3)
    if c.exact:
        assert torch.equal(got, oo.detach().double())
    else:
        dec = o.out_decided[keep][:, None].expand_as(got)
        assert close(got, oo.detach().double(), o.out_bound[keep].permute(0, 4, 1, 2, 3), dec)
    assert any(f.grad is not None and f.grad.any() for f in feats)
    for g, b, f, m in zip(o.grads, o.grad_bounds, feats, o.grad_decided):
        want = torch.zeros_like(g) if f.grad is None else f.grad.permute(1, 2, 3, 0).double()
        if c.exact:
            assert torch.equal(g, want)
        else:
            # autograd accumulates the oracle's gradient in fp32: a sum that cancels carries the rounding of one upstream term
            assert close(g, want, b + 1e-6 * c.dout.abs().max().item(), m)


def test_aabb_crops_follow_python_slicing():
    """Clipped at the high side and wrapped at a negative low corner, as ``f[lo:hi + 1]`` does."""
    rois = torch.tensor(R.POOL_EXACT_AABB, dtype=F32)
    crops = R.aabb_crops(rois, R.POOL_DIMS, R.POOL_SCALES)
    for row, cr in zip(rois, crops):
        lv = int(row[0])
        s = R.POOL_SCALES[lv]
        ext, ctr = (row[4:] - row[1:4]) / 2 * 1.2, (row[4:] + row[1:4]) / 2
        lo, hi = torch.floor((ctr - 0.5 * ext) / s).long().tolist(), torch.floor((ctr + 0.5 * ext) / s).long().tolist()
        for a in range(3):
            idx = list(range(R.POOL_DIMS[lv][a]))[lo[a]:hi[a] + 1]
            assert len(idx) == int(cr[3 + a]) and (not idx or idx[0] == int(cr[a]))
    assert (crops[:, :3] > 0).any() and (rois[:, 1:4] < 0).any() and (crops[:, 3:] == 0).any()


# ======================================================================================================================
# the bounds hold for torch fp32; the caps
# ======================================================================================================================
@pytest.mark.parametrize("name", list(ALIGN))
def test_align_bounds_hold_for_torch_fp32(name):
    c, o = align(name)
    d = o.out_decided[..., None].expand_as(o.out)
    r_o = R.ratio(o.out32[d], o.out[d], o.out_bound[d])
    r_g = R.ratio(o.grad32[o.grad_decided], o.grad[o.grad_decided], o.grad_bound[o.grad_decided])
    su, sg = R.undecided_share(o.out_decided), R.undecided_share(o.grad_decided)
    print(f"roialign {name}: torch fp32 r forward {r_o:.3f} backward {r_g:.3f}; undecided bins {100 * su:.3f} % voxels {100 * sg:.3f} %")
    assert r_o <= 1.0 and r_g <= 1.0
    assert su <= c.cap and sg <= c.cap
    if c.exact:
        assert torch.equal(o.geo.pos, o.geo32.pos.double()) and torch.equal(o.out, o.out32.double()) and torch.equal(o.grad.float(), o.grad32)
        pos, dims = o.geo.pos, torch.tensor(c.feat.shape[1:4], dtype=F64)
        for hit in ((pos == -1).any(), (pos == dims).any(), ((pos > -1) & (pos < 0)).any(), (pos == dims - 1).any(), ((pos > dims - 1) & (pos < dims)).any(),
                    (pos > dims).any(), (pos % 1 == 0.5).any(), (o.geo.g > 1).any()):
            assert hit
    if name == "bad-batch":
        assert not o.out[~o.geo.good].any() and not o.out_bound[~o.geo.good].any() and (~o.geo.good).sum() == 3


@pytest.mark.parametrize("name", ["random-c4", "random-c12-half", "offset", "exact", "stacked"])
def test_align_bounds_hold_for_torch_fp32_with_bf16_storage(name):
    c, o = align(name, bf16=True)
    d = o.out_decided[..., None].expand_as(o.out)
    r_o = R.ratio(o.out32[d], o.out[d], o.out_bound[d])
    r_g = R.ratio(o.grad32[o.grad_decided], o.grad[o.grad_decided], o.grad_bound[o.grad_decided])
    print(f"roialign {name} bf16: torch r forward {r_o:.3f} backward {r_g:.3f}")
    assert r_o <= 1.0 and r_g <= 1.0
    assert R.undecided_share(o.out_decided) <= c.cap and R.undecided_share(o.grad_decided) <= c.cap


@pytest.mark.parametrize("kind,name", [(kind, name) for kind in POOL for name in ("random-c3", "random-c130", "offset", "exact")])
def test_pool_bounds_hold_for_torch_fp32_with_bf16_maps(kind, name):
    c, o, e = pool(kind, name, bf16=True)
    d = o.out_decided[..., None].expand_as(o.out)
    r_o = R.ratio(e.out[d], o.out[d], o.out_bound[d])
    r_g = [R.ratio(a[m], b[m], bb[m]) for a, b, bb, m in zip(e.grads, o.grads, o.grad_bounds, o.grad_decided)]
    su, sg = R.undecided_share(o.out_decided), max(R.undecided_share(m) for m in o.grad_decided)
    print(f"roipool {kind} {name} bf16: torch r forward {r_o:.3f} backward {max(r_g):.3f}; undecided outputs {100 * su:.3f} % voxels {100 * sg:.3f} %")
    assert r_o <= 1.0 and max(r_g) <= 1.0
    assert su <= c.cap and sg <= R.grad_cap(c, True)
    if (kind, name) == ("pooling", "offset"):
        assert su == 0.0 and any(m.any() for m in o.grad_decided)      # the forward is checked in full, and part of the gradient is left


@pytest.mark.parametrize("kind,name", [(kind, name) for kind in POOL for name in POOL[kind]])
def test_pool_bounds_hold_for_torch_fp32(kind, name):
    c, o, e = pool(kind, name)
    d = o.out_decided[..., None].expand_as(o.out)
    r_o = R.ratio(e.out[d], o.out[d], o.out_bound[d])
    r_g = [R.ratio(a[m], b[m], bb[m]) for a, b, bb, m in zip(e.grads, o.grads, o.grad_bounds, o.grad_decided)]
    su, sg = R.undecided_share(o.out_decided), max(R.undecided_share(m) for m in o.grad_decided)
    print(f"roipool {kind} {name}: torch fp32 r forward {r_o:.3f} backward {max(r_g):.3f}; undecided outputs {100 * su:.3f} % voxels {100 * sg:.3f} %")
    assert r_o <= 1.0 and max(r_g) <= 1.0
    assert su <= c.cap and sg <= c.cap
    if kind == "aabb" or c.exact:
        assert torch.equal(o.out, e.out.double())
    if c.exact:
        assert all(torch.equal(a.double(), b) for a, b in zip(e.grads, o.grads))
    if name == "ties-negative":
        assert (o.out == 0).any(), "no window in which the padding zero wins"
    if name == "unused-level":
        assert not o.grads[1].any() and not o.grad_bounds[1].any()


def test_exact_pool_fixture_reaches_its_edges():
    rows = torch.tensor(R.POOL_EXACT_OBB, dtype=F64)
    integer = half = outside = False
    for row in rows:
        s = R.POOL_SCALES[int(row[0])]
        g, pos, _ = R._obb_geometry(torch.cat([row[1:], torch.zeros(1, dtype=F64)]).float(), s, F64)
        assert torch.equal(pos * 2, torch.round(pos * 2)) and all(float(row[4 + a]) / s == gg or gg == 1 for a, gg in enumerate(g))
        integer |= bool((pos % 1 == 0).all(1).any())
        half |= bool((pos % 1 == 0.5).all(1).any())
        outside |= bool((pos < 0).any() or (pos > torch.tensor(R.POOL_DIMS[int(row[0])], dtype=F64) - 1).any())
    assert integer and half and outside
    c = POOL["interpolation"]["random-c32"]()
    g = [R._obb_geometry(m, c.scales[int(l)], F64)[0] for m, l in zip(c.meta, c.level_of)]
    assert c.out_size == (1, 1, 1) and any(1 in gg for gg in g)                  # lin_tap with out == 1 and in == 1
    c = POOL["interpolation"]["random-c3"]()
    g = [R._obb_geometry(m, c.scales[int(l)], F64)[0] for m, l in zip(c.meta, c.level_of)]
    assert any(gg[0] < 3 and gg[0] > 1 for gg in g) and any(1 in gg for gg in g)  # output larger than the grid


# ======================================================================================================================
# sharpness
# ======================================================================================================================
ALIGN_MUTATIONS = [("no_half", "random-c4", 0.5), ("sin_sign", "random-c4", 0.5), ("ref_index", "random-c4", 0.5), ("valid_count", "random-c4", 0.05)]


@pytest.mark.parametrize("mut,name,share", ALIGN_MUTATIONS)
def test_align_mutations_land_outside_the_bound(mut, name, share):
    c, o = align(name)
    m = R.align_case(c.feat, c.rois, c.scale, c.pooled, c.sampling, c.top, mutate=mut)
    d = o.out_decided[..., None].expand_as(o.out)
    got = share_outside(m.out32, o.out, o.out_bound, d)
    print(f"roialign {mut}: {100 * got:.1f} % of the forward elements outside 2 x bound (stated: > {100 * share:.0f} %)")
    assert got > share
    if mut != "valid_count":
        live = o.grad_decided[:, None] & (o.grad != 0)
        gg = share_outside(m.grad32, o.grad, o.grad_bound, live)
        print(f"   backward: {100 * gg:.1f} % of the touched voxels")
        assert gg > share


def test_align_high_border_clamp_without_zeroing_breaks_an_equality():
    """x in (width - 1, width]: both taps are voxel width - 1, so keeping lx only splits one weight into hx + lx = 1 -- the VALUE stays
    inside the bound (asserted: the mutation is not an error of value), the weights are what differs: the exact family holds samples
    beyond width - 1, where the kernel's weights are exactly (1, 0) and the mutation's are not."""
    c, o = align("exact")
    m = R.align_case(c.feat, c.rois, c.scale, c.pooled, c.sampling, c.top, mutate="no_zero_high", exact=True)
    assert not torch.equal(m.geo32.w.double(), o.geo.w) and torch.equal(o.geo32.w.double(), o.geo.w)
    d = o.out_decided[..., None].expand_as(o.out)
    assert share_outside(m.out32, o.out, o.out_bound, d) == 0.0


POOL_MUTATIONS = [("trilinear", "pooling", "random-c3", 0.5), ("trilinear", "interpolation", "random-c3", 0.5), ("rot_sign", "pooling", "random-c3", 0.5),
                  ("rot_sign", "interpolation", "random-c3", 0.5), ("align_false", "interpolation", "random-c3", 0.3)]


@pytest.mark.parametrize("mut,kind,name,share", POOL_MUTATIONS)
def test_pool_mutations_land_outside_the_bound(mut, kind, name, share):
    c, o, _ = pool(kind, name)
    m = R.pool_eval(kind, c.feats, c.meta, c.level_of, c.scales, c.out_size, F32, c.dout, mutate=mut)
    d = o.out_decided[..., None].expand_as(o.out) & (o.out != 0)
    got = share_outside(m.out, o.out, o.out_bound, d)
    print(f"roipool {kind} {mut}: {100 * got:.1f} % of the non-zero forward elements outside 2 x bound (stated: > {100 * share:.0f} %)")
    assert got > share


@pytest.mark.parametrize("kind", ["aabb", "pooling"])
@pytest.mark.parametrize("mut,name", [("ties_last", "exact"), ("no_pad", "ties-negative")])
def test_pool_tie_mutations_break_an_equality(kind, mut, name):
    c, o, _ = pool(kind, name)
    m = R.pool_eval(kind, c.feats, c.meta, c.level_of, c.scales, c.out_size, F32, c.dout, mutate=mut, exact=True)
    if mut == "ties_last":       # the value of a tie is the same: the voxel that receives the gradient is not
        assert torch.equal(m.out.double(), o.out) and not all(torch.equal(a.double(), b) for a, b in zip(m.grads, o.grads))
    else:
        assert not torch.equal(m.out.double(), o.out)
