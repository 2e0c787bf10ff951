"""GPU: the stamped twins of the K-sliced conv launches (nrpn_conv3d_fwd_stamped) write the bits of the unstamped call -- outputs and
workspace partials -- plus one well-formed record per workgroup, inside the bytes the layout query states, and refuse what has no stamped
form before anything is launched.  No ordering across workgroups or across the two kernels is asserted: tools/launch_anatomy.py reports it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 64          # guard words behind the used part of the record buffer
WS_FILL = 3.0e38    # no partial sum of these operands comes near it

# (id, grid, cin, cout, ksize, ConvOpts fields, plan code, stamped instantiation the case reaches)
CASES = [
    ("g5_512_256_k1", (5, 5, 5), 512, 256, 1, {}, 0, "128-row BN 128, unsliced"),
    ("g5x4x3_64_64_k1", (5, 4, 3), 64, 64, 1, {}, 0, "128-row BN 64, unsliced, one partial M tile"),
    ("g5x4x3_64_64_k3", (5, 4, 3), 64, 64, 3, {}, 3, "128-row BN 64 on K slices + epilogue, one partial M tile"),
    ("g5_512_512_k3", (5, 5, 5), 512, 512, 3, {}, 3, "128-row BN 128 on 27 K slices + epilogue"),
    ("g10_512_512_k3", (10, 10, 10), 512, 512, 3, {}, 3, "128-row BN 128 on 12 K slices, partial last M tile"),
    ("g20_256_256_k3", (20, 20, 20), 256, 256, 3, {}, 3, "128-row BN 128 on 4 K slices, 504 workgroups, 4096 epilogue workgroups"),
    ("g20_512_512_k3", (20, 20, 20), 512, 512, 3, {}, 2, "256x256 (rotated loop) on 4 K slices"),
    ("g20_512_512_k3_plain", (20, 20, 20), 512, 512, 3, {"stagger": 0}, 2, "256x256 (plain loop) on 4 K slices"),
    ("g20_512_512_k3_whole", (20, 20, 20), 512, 512, 3, {"tile": 512, "big_split": 0}, 1, "256x256 unsliced: its own store epilogues"),
]
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def operands(dev):
    """Seeded bf16 operands per case, made once."""
    from nerf_rpn_amd import ops
    out = {}
    for i, (name, grid, cin, cout, k, _, _, _) in enumerate(CASES):
        key = (grid, cin, cout, k)
        if key in out:
            continue
        g = torch.Generator().manual_seed(1234 + i)
        x = torch.randn((1, *grid, cin), generator=g).to(BF).to(dev)
        w = (torch.randn((cout, cin, k, k, k), generator=g) * (cin * k ** 3) ** -0.5).to(dev)
        bias = torch.randn((cout,), generator=g).to(dev)
        wp, _ = ops.PackedWeight().get([w], BF, cout, False)
        out[key] = (x, wp, bias)
    return out


def _run(lib, ops, stamped, x, wp, bias, cout, k, flags, opts, out_dtype, wsb, rec=None, rec_bytes=None, y=None):
    """One direct C call with a workspace of its own, pre-filled so that unwritten partials would show."""
    n, gx, gy, gz, cin = x.shape
    if y is None:
        y = torch.full((n, gx, gy, gz, cout), 7.0, dtype=out_dtype, device=x.device)
    ws = torch.full((max(wsb, 4) // 4,), WS_FILL, dtype=torch.float32, device=x.device)
    a = (ops._p(x), ops._p(wp), ops._p(bias), ops._p(y), n, gx, gy, gz, cin, cout, cout, k, lib.BF16, flags, ops._p(ws) if wsb else 0, opts.ptr(), ops._s())
    if stamped:
        lib.call("conv3d_fwd_stamped", *a, ops._p(rec), rec.numel() * 8 if rec_bytes is None else rec_bytes)
    else:
        lib.call("conv3d_fwd_ex", *a)
    torch.cuda.synchronize()
    return y, ws


@pytest.mark.parametrize("out_f32", [False, True], ids=["bf16out", "f32out"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stamped_launch_same_bits_and_well_formed_records(case, out_f32, operands, dev):
    from nerf_rpn_amd import lib, ops, stamps
    name, grid, cin, cout, k, kw, code, _ = case
    x, wp, bias = operands[(grid, cin, cout, k)]
    opts = lib.ConvOpts(**kw)
    q = (1, *grid, cin, cout, k, lib.BF16, opts.ptr())
    assert lib.query("conv3d_fwd_plan_ex", *q) == code                       # the case runs the kernel it is listed for
    lay = ops.conv3d_stamp_layout(1, *grid, cin, cout, k, lib.BF16, opts)
    wsb = lib.query("conv3d_fwd_workspace_bytes_ex", *q)
    assert lay.plan_code == code and (wsb > 0) == (lay.epilogue_records > 0) == (code in (2, 3))
    flags = lib.CONV_BIAS | lib.CONV_RELU | (lib.CONV_OUT_F32 if out_f32 else 0)
    odt = torch.float32 if out_f32 else BF
    used = lay.conv_records + lay.epilogue_records
    assert lay.nbytes == used * lay.words * 8

    def records():
        return torch.full((used * lay.words + GUARD,), stamps.FILL_I64, dtype=torch.int64, device=dev)

    # 1. the bits of the unstamped call, outputs and workspace partials
    want, ws_want = _run(lib, ops, False, x, wp, bias, cout, k, flags, opts, odt, wsb)
    rec = records()
    y, ws = _run(lib, ops, True, x, wp, bias, cout, k, flags, opts, odt, wsb, rec, rec_bytes=lay.nbytes)
    assert torch.equal(y, want) and not bool((y == 7.0).all())
    assert torch.equal(ws, ws_want) and (wsb == 0 or not bool((ws == WS_FILL).any()))
    # 2. two stamped calls agree
    rec2 = records()
    y2, _ = _run(lib, ops, True, x, wp, bias, cout, k, flags, opts, odt, wsb, rec2, rec_bytes=lay.nbytes)
    assert torch.equal(y2, y)

    # 3. coverage: every record of the used part written, every guard word untouched
    a = rec.cpu().numpy().view(np.uint64)
    assert (a[used * lay.words:] == np.uint64(stamps.FILL)).all(), "guard words behind the records were written"
    a = a[:used * lay.words].reshape(used, lay.words)
    assert not (a == np.uint64(stamps.FILL)).any(), "a record (or part of one) was not written"
    assert (a[:, stamps.W_VERSION] == np.uint64(stamps.VERSION)).all()
    a = a.astype(np.int64)
    conv, epi = a[:lay.conv_records], a[lay.conv_records:]
    P0 = stamps.W_PHASE0

    # 4. clocks inside a record
    rt, cy = conv[:, P0:P0 + 14:2], conv[:, P0 + 1:P0 + 14:2]
    assert (np.diff(rt, axis=1) >= 0).all() and (np.diff(cy, axis=1) >= 0).all() and (rt > 0).all() and (cy > 0).all()
    steps = conv[:, stamps.W_KSTEPS]
    ks = conv[:, stamps.W_KSTEP0:stamps.W_KSTEP0 + 8]
    for q8 in range(8):
        ran = steps > q8
        assert (ks[~ran, q8] == 0).all()
        assert (ks[ran, q8] >= cy[ran, 2]).all() and (ks[ran, q8] <= cy[ran, 3]).all()          # between "first tile landed" and "end of loop"
        if q8:
            both = steps > q8
            assert (ks[both, q8] >= ks[both, q8 - 1]).all()
    loop = cy[:, 3] - cy[:, 2]
    wsum, wmax = conv[:, stamps.W_WAIT_SUM], conv[:, stamps.W_WAIT_MAX]
    assert (wsum <= loop).all() and (wmax <= wsum).all() and (wmax > 0).all()
    if len(epi):
        ert, ecy = epi[:, P0:P0 + 10:2], epi[:, P0 + 1:P0 + 10:2]
        assert (np.diff(ert, axis=1) >= 0).all() and (np.diff(ecy, axis=1) >= 0).all() and (ert > 0).all()
        assert (epi[:, P0 + 10:] == 0).all()                                                   # words the epilogue has no value for

    # 5. identity fields
    want_kernel = stamps.KERNEL_CONV256 if code in (1, 2) else stamps.KERNEL_CONV128
    assert (conv[:, stamps.W_KERNEL] == want_kernel).all()
    assert (conv[:, stamps.W_WG] == np.arange(lay.conv_records)).all()
    mt, nt, kz = conv[:, stamps.W_MTILE], conv[:, stamps.W_NTILE], conv[:, stamps.W_KSLICE]
    assert (mt >= 0).all() and (mt < lay.m_tiles).all() and (nt >= 0).all() and (nt < lay.n_tiles).all() and (kz >= 0).all() and (kz < lay.k_slices).all()
    assert len({(int(m), int(n_), int(z)) for m, n_, z in zip(mt, nt, kz)}) == lay.conv_records == lay.m_tiles * lay.n_tiles * lay.k_slices
    assert (steps == np.asarray(lay.slice_steps)[kz]).all()
    assert (a[:, stamps.W_XCD] >= 0).all() and (a[:, stamps.W_XCD] < 8).all()
    if len(epi):
        total = grid[0] * grid[1] * grid[2] * cout
        assert (epi[:, stamps.W_KERNEL] == stamps.KERNEL_EPILOGUE).all() and (epi[:, stamps.W_WG] == np.arange(lay.epilogue_records)).all()
        # lane 0 of workgroup b handles elements 256 b + 256 * blocks * i < total
        b = np.arange(lay.epilogue_records)
        assert (epi[:, stamps.W_KSTEPS] == -(-(total - 256 * b) // (256 * lay.epilogue_records))).all()

    # 7. the decoder takes the real records
    d = stamps.decode(rec[:used * lay.words].view(used, lay.words), lay)
    assert d["conv"]["records"] == lay.conv_records and (d["epilogue"] is None) == (lay.epilogue_records == 0)
    assert 0.0 < d["conv"]["wait_share"] <= 1.0 and d["conv"]["kstep_cycles_mean"] > 0
    y3, rec3 = ops.conv3d_fwd_stamped(x, wp, bias, cout, cout, k, lib.CONV_RELU, odt, opts)    # the ops wrapper: same call, same bits
    assert torch.equal(y3, want) and tuple(rec3.shape) == (used, lay.words)
    stamps.decode(rec3, lay)


def test_refusals_launch_nothing(operands, dev):
    """6. NRPN_ERR_ARG, with y and the record buffer untouched: null buffer, short buffer, debug != 0, plans without a stamped form."""
    from nerf_rpn_amd import lib, ops, stamps
    flags = lib.CONV_BIAS | lib.CONV_RELU
    sliced, whole = ((5, 5, 5), 512, 512, 3), ((5, 5, 5), 512, 256, 1)      # plan codes 3 and 0 by default
    lay = ops.conv3d_stamp_layout(1, *sliced[0], *sliced[1:])

    def refused(match, opts=None, rec_none=False, rec_bytes=None, key=sliced, f32=False):
        grid, cin, cout, k = key
        x, wp, bias = operands[key]
        xx, dt = (x.float(), torch.float32) if f32 else (x, BF)
        opts = opts or lib.ConvOpts()
        nwords = 4096 * 32
        wsb = lib.query("conv3d_fwd_workspace_bytes", 1, *grid, cin, cout, k, lib.BF16)
        rec = torch.full((nwords + GUARD,), stamps.FILL_I64, dtype=torch.int64, device=dev)
        y = torch.full((1, *grid, cout), 7.0, dtype=dt, device=dev)
        n, gx, gy, gz, ci = xx.shape
        ws = torch.full((max(wsb, 4) // 4,), WS_FILL, dtype=torch.float32, device=dev)
        with pytest.raises(lib.NrpnError, match=match):
            lib.call("conv3d_fwd_stamped", ops._p(xx), ops._p(wp), ops._p(bias), ops._p(y), n, gx, gy, gz, ci, cout, cout, k, ops._dt(xx), flags,
                     ops._p(ws), opts.ptr(), ops._s(), 0 if rec_none else ops._p(rec), nwords * 8 if rec_bytes is None else rec_bytes)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()) and bool((rec == stamps.FILL_I64).all()) and bool((ws == WS_FILL).all())

    refused(r"\(-1\): conv3d_fwd_stamped: null stamp buffer", rec_none=True)
    refused(r"\(-1\): conv3d_fwd_stamped: the stamp buffer holds \d+ bytes, plan code 3 needs \d+", rec_bytes=lay.nbytes - 8)
    refused(r"\(-1\): conv3d_fwd_stamped: the debug variants have no stamped form", opts=lib.ConvOpts(debug=1 << 12))
    refused(r"\(-1\): conv3d_fwd_stamped: plan code 3 has no stamped form for the 64-byte K-step", opts=lib.ConvOpts(kstep_bytes=64))
    refused(r"\(-1\): conv3d_fwd_stamped: plan code 3 has no stamped form for register-staged loads", opts=lib.ConvOpts(lds_dma=0))
    refused(r"\(-1\): conv3d_fwd_stamped: plan code 7 has no stamped form for the halo form", opts=lib.ConvOpts(tile=lib.TILE_HALO))
    refused(r"\(-1\): conv3d_fwd_stamped: plan code 4 has no stamped form for the wave-specialised", opts=lib.ConvOpts(tile=lib.TILE_256X128_WS), key=whole)
    refused(r"\(-1\): conv3d_fwd_stamped: plan code 5 has no stamped form for the 4-wave", opts=lib.ConvOpts(tile=lib.TILE_256X256_W4), key=whole)
    refused(r"\(-1\): conv3d_fwd_stamped: plan code 3 has no stamped form for fp32", f32=True)
