"""GPU: the bytes a conv size query returns are the bytes the launch writes.  The C entry points take no buffer length, so every family that
writes a workspace is called directly with EXACTLY the queried bytes placed inside a larger allocation, a 4 KiB band of a fixed byte
pattern on either side: after the launch the bands are unchanged (a wrong size shows up inside the allocation: nothing faults) and the
output is bit-equal to the one ops produces for the same call."""
import numpy as np
import pytest
import torch

import conv_ref as cr
from test_gpu_conv_exact import BF, T128, T256, TW4, _backward, _x5

pytestmark = pytest.mark.gpu
BAND, FILL = 4096, 0xA5


class Banded:
    """``nbytes`` of device memory between two bands."""

    def __init__(self, nbytes, dev):
        assert nbytes > 0
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * BAND,), FILL, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() + BAND

    def inner(self):
        return self.buf[BAND:BAND + self.n]

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:BAND] == FILL).all()), f"{what}: bytes before the buffer were written"
        assert bool((self.buf[BAND + self.n:] == FILL).all()), f"{what}: bytes past the buffer were written"
        assert not bool((self.inner() == FILL).all()), f"{what}: the buffer was not written at all"


@pytest.mark.parametrize("name,tile,plan", [("g555_c128_256", T128, 3), ("gk20_c128_512", T256, 2), ("gk20_c128_512", TW4, 6), ("gtail_c64_256", 0, 1)],
                         ids=["ksplit-128row", "ksplit-256x256", "ksplit-256x256-w4", "tail-split"])
def test_forward_workspace_is_exactly_the_queried_bytes(name, tile, plan, dev):
    from nerf_rpn_amd import lib, ops
    m = cr.get(name)
    x = _x5(m, m.x, dev, BF)
    n, gx, gy, gz, cin = x.shape
    opts = lib.ConvOpts(tile=tile)
    a = (n, gx, gy, gz, cin, m.cout, m.k, lib.BF16, opts.ptr())
    wsb = lib.query("conv3d_fwd_workspace_bytes_ex", *a)
    assert lib.query("conv3d_fwd_plan_ex", *a) == plan and wsb > 0, (plan, wsb)
    per = n * gx * gy * gz * m.cout * 4
    assert (wsb % per == 0) == (plan != 1)      # K slices over every row, or (plan 1) over the tail rows only
    wp, _ = ops.PackedWeight().get([m.w.float().to(dev)], BF, m.cout, False)
    bias = m.bias.float().to(dev)
    want = ops._conv_fwd(x, wp, bias, m.cout, m.cout, m.k, lib.CONV_RELU, BF, tile=tile)
    ws = Banded(wsb, dev)
    y = torch.empty_like(want)
    lib.call("conv3d_fwd_ex", ops._p(x), ops._p(wp), ops._p(bias), ops._p(y), n, gx, gy, gz, cin, m.cout, m.cout, m.k, lib.BF16,
             lib.CONV_BIAS | lib.CONV_RELU, ws.ptr, opts.ptr(), ops._s())
    ws.check(f"{name} forward workspace")
    assert torch.equal(y, want)


@pytest.mark.parametrize("name,plan", [("gw2_c64_128", 0), ("gw_c256_512", 1)], ids=["128x128", "256x256"])
def test_weight_gradient_workspace_and_partials_are_exactly_the_queried_sizes(name, plan, dev):
    """Dense weight gradient with a bias: bands around the workspace (tap mask + bias partials) and around the partial gradients
    [slices][taps][Cout][Cin] sized by nrpn_conv3d_wgrad_slices."""
    from nerf_rpn_amd import lib, ops
    m = cr.get(name)
    x, dy = _x5(m, m.x, dev, BF), _x5(m, m.gy, dev, BF, out=True)
    n, gx, gy, gz, cin = x.shape
    a = (n, gx, gy, gz, cin, m.cout, m.cout, m.k, lib.BF16)
    slices, wsb = lib.query("conv3d_wgrad_slices", *a), lib.query("conv3d_wgrad_workspace_bytes", *a)
    assert lib.query("conv3d_wgrad_plan", *a) == plan and slices >= 2 and wsb > 0
    want = _backward(m, dev, BF, False)
    taps = m.k ** 3
    ws, gwp = Banded(wsb, dev), Banded(slices * taps * m.cout * cin * 4, dev)
    gb = torch.empty(m.cout, dtype=torch.float32, device=dev)
    lib.call("conv3d_wgrad", ops._p(x), ops._p(dy), gwp.ptr, ops._p(gb), n, gx, gy, gz, cin, m.cout, m.cout, m.k, lib.BF16, 0, ws.ptr, ops._s())
    ws.check(f"{name} wgrad workspace")
    gwp.check(f"{name} wgrad partials")
    gw = torch.empty_like(want["dw"], dtype=torch.float32)
    lib.call("unpack_conv_wgrad", gwp.ptr, m.cout, cin, taps, m.cout, 0, ops._p(gw), 0, slices, ops._s())
    assert torch.equal(gw, want["dw"].float()) and torch.equal(gb, want["db"].float())


def _row_list(grid, nrows, dev):
    """An ops.ConePlan over one grid whose list 0 = ``nrows`` seeded voxels in ascending order, with their in-bounds tap words
    (csrc/cone.hip: bit t = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1), segment id 0)."""
    from nerf_rpn_amd import ops
    X, Y, Z = grid
    ids = np.sort(np.random.default_rng(nrows).permutation(X * Y * Z)[:nrows])
    x, y, z = ids // (Y * Z), (ids // Z) % Y, ids % Z
    word = np.zeros(nrows, dtype=np.uint32)
    for t in range(27):
        dx, dy, dz = t // 9 - 1, (t // 3) % 3 - 1, t % 3 - 1
        inside = (x + dx >= 0) & (x + dx < X) & (y + dy >= 0) & (y + dy < Y) & (z + dz >= 0) & (z + dz < Z)
        word |= inside.astype(np.uint32) << np.uint32(t)
    plan = ops.ConePlan([grid], 1, 0, dev)
    plan.lists[0, :nrows] = torch.from_numpy(np.stack([ids.astype(np.uint32), word], axis=1).view(np.int32)).to(dev)
    plan.counts = [nrows]
    return plan, torch.from_numpy(ids).to(dev)


@pytest.mark.parametrize("nrows,cout,tail", [(300, 128, False), (33000, 256, True)], ids=["rows-ksplit", "rows-tail-split"])
def test_row_list_workspace_is_exactly_the_queried_bytes(nrows, cout, tail, dev):
    """300 rows = 3 tiles: the whole list on K slices (rows_ksplit).  33 000 rows x 2 column tiles = 516 workgroups = one round of the 512
    slots + 4: the last two M tiles on K slices (rows_tail_split)."""
    from nerf_rpn_amd import lib, ops
    grid, cin = (32, 32, 33), 128
    wsb = lib.query("conv3d_fwd_rows_workspace_bytes", nrows, cin, cout, 3, lib.BF16)
    assert wsb > 0 and (wsb < nrows * cout * 4) == tail and (wsb % (nrows * cout * 4) == 0) != tail, wsb
    plan, ids = _row_list(grid, nrows, dev)
    g = torch.Generator().manual_seed(nrows)
    x = torch.randint(-4, 5, (plan.total, cin), generator=g).to(BF).to(dev)
    w = torch.randint(-2, 3, (cout, cin, 3, 3, 3), generator=g).float()
    bias = torch.randint(-8, 9, (cout,), generator=g).float().to(dev)
    wp, _ = ops.PackedWeight().get([w.to(dev)], BF, cout, False, cin)
    want = torch.full((plan.total, cout), 3.0, dtype=BF, device=dev)
    ops.conv_rows_fwd(x, wp, bias, want, plan, 0, cin, cout, cout, 3, lib.CONV_RELU)
    ws = Banded(wsb, dev)
    y = torch.full_like(want, 3.0)
    rows, _ = plan.rows(0)
    lib.call("conv3d_fwd_rows", ops._p(x), ops._p(wp), ops._p(bias), ops._p(y), rows, nrows, plan.nseg, plan.dims_ptr, cin, cout, cout, 3, lib.BF16,
             lib.CONV_BIAS | lib.CONV_RELU, 0, ws.ptr, ops._s())
    ws.check(f"{nrows}-row list workspace")
    assert torch.equal(y, want)
    rest = torch.ones(plan.total, dtype=torch.bool, device=dev)
    rest[ids] = False
    assert bool((y[rest] == 3.0).all()) and not bool((y[ids] == 3.0).all())
