"""The sampled RPN loss taken from the cone head's rows (csrc/postproc.hip: nrpn_rpn_sampled_loss_rows_f32, nrpn_head_grad_rows; ops.ConeHeadFn
with a loss pack).

The new entries replace head_flatten -> rpn_sampled_loss -> (dense gradient x upstream scalar) -> head_unflatten on the rows of S_0 with the
same fp32 operations in the same order, so every comparison here is bit equality against that chain; the arithmetic of the shared loss
expressions is held to fp64 in tests/test_gpu_rpn_kernels.py.  Kernel level: losses, compact factors, deltas of the positives, rows outside
S_0 never read (NaN there) and never written (sentinel kept), zeros in the unsampled and padding columns.  Step level: one forward + backward
of the whole model with the switch on and off gives equal losses and equal parameter gradients."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRIDS = [(6, 5, 4), (3, 3, 2)]
LD = 128
BETA = 1.0 / 9
SENTINEL = 7.0
_cache = {}


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(n, A, dw, npos, dev):
    """Random head rows, an ascending sample, its S_0, and -- computed once -- the flattened chain's results on the same rows."""
    key = (n, A, dw, npos)
    if key in _cache:
        return _cache[key]
    from nerf_rpn_amd import lib, ops
    rng = np.random.default_rng(100 * n + 10 * A + dw + npos)
    cells = [g[0] * g[1] * g[2] for g in GRIDS]
    T = sum(cells) * A
    pick = np.sort(rng.choice(n * T, size=npos + 40, replace=False)).astype(np.int64)      # pos and neg never share an anchor
    is_pos = np.zeros(npos + 40, dtype=bool)
    is_pos[rng.choice(npos + 40, size=npos, replace=False)] = True
    pos, neg = torch.from_numpy(pick[is_pos]).to(dev), torch.from_numpy(pick[~is_pos]).to(dev)
    table = type("Tab", (), {})()      # what cone_build reads of ops.AnchorTable
    table.A, table.counts = A, [c * A for c in cells]
    table.offsets = [0] + list(np.cumsum(table.counts))
    table.total = T
    plan = ops.cone_from_indices(ops.ConePlan(GRIDS, n, 0, dev), pos, neg, table)
    V = plan.total
    s0 = plan.lists[0, :plan.counts[0], 0].long()
    assert 0 < s0.numel() < V
    g = torch.Generator().manual_seed(int(rng.integers(1 << 30)))
    head = (torch.randn(V, LD, generator=g) * 2.0).to(dev)
    targets = torch.randn(npos, dw, generator=g).to(dev)      # |d| on both sides of beta
    st = _stream()
    logits = torch.empty((n, T), dtype=torch.float32, device=dev)
    deltas = torch.empty((n, T, dw), dtype=torch.float32, device=dev)
    off = 0
    for l, c in enumerate(cells):
        for i in range(n):
            r0 = plan.level_start[l] + i * c
            lib.call("head_flatten_f32", head[r0:r0 + c].data_ptr(), c, LD, A, dw, logits[i, off:].data_ptr(), deltas[i, off:].data_ptr(), st)
        off += c * A
    loss2 = torch.empty(2, dtype=torch.float32, device=dev)
    g_logits, g_deltas = torch.zeros_like(logits), torch.zeros_like(deltas)
    lib.call("rpn_sampled_loss_f32", logits.data_ptr(), deltas.data_ptr(), dw, targets.data_ptr(), pos.data_ptr(), npos, neg.data_ptr(), 40, BETA,
             loss2.data_ptr(), g_logits.data_ptr(), g_deltas.data_ptr(), st)
    c = dict(n=n, A=A, dw=dw, npos=npos, T=T, V=V, cells=cells, plan=plan, s0=s0, head=head, targets=targets, pos=pos, neg=neg, logits=logits,
             deltas=deltas, loss2=loss2, g_logits=g_logits, g_deltas=g_deltas)
    _cache[key] = c
    return c


def _loss_rows(c, head):
    from nerf_rpn_amd import lib, ops
    dev = head.device
    npos, dw = c["npos"], c["dw"]
    loss2 = torch.full((2,), SENTINEL, dtype=torch.float32, device=dev)
    g_obj = torch.full((npos + 40,), SENTINEL, dtype=torch.float32, device=dev)
    g_reg = torch.full((npos, dw), SENTINEL, dtype=torch.float32, device=dev)
    dpos = torch.full((npos, dw), SENTINEL, dtype=torch.float32, device=dev)
    lib.call("rpn_sampled_loss_rows_f32", head.data_ptr(), LD, *ops._head_levels(c["plan"]), c["n"], c["T"], c["A"], dw, c["targets"].data_ptr(),
             c["pos"].data_ptr(), npos, c["neg"].data_ptr(), 40, BETA, loss2.data_ptr(), g_obj.data_ptr(), g_reg.data_ptr(), dpos.data_ptr(), _stream())
    return loss2, g_obj, g_reg, dpos


CASES = [(n, A, dw, npos) for n in (1, 2) for A in (3, 13) for dw in (6, 8) for npos in (24,)] + [(2, 13, 8, 0), (1, 3, 6, 0)]


@pytest.mark.parametrize("n,A,dw,npos", CASES)
def test_loss_and_factors_equal_the_flattened_chain(n, A, dw, npos, dev):
    c = _case(n, A, dw, npos, dev)
    loss2, g_obj, g_reg, dpos = _loss_rows(c, c["head"])
    print(f"loss2 rows {loss2.tolist()} flattened {c['loss2'].tolist()}")
    assert torch.equal(bits(loss2), bits(c["loss2"]))
    flat_gl, flat_gd, flat_d = c["g_logits"].reshape(-1), c["g_deltas"].reshape(-1, dw), c["deltas"].reshape(-1, dw)
    assert torch.equal(bits(g_obj), bits(torch.cat([flat_gl[c["pos"]], flat_gl[c["neg"]]])))
    assert torch.equal(bits(g_reg), bits(flat_gd[c["pos"]]))
    assert torch.equal(bits(dpos), bits(flat_d[c["pos"]]))
    # nothing outside S_0 is read: NaN there, same bits
    poisoned = torch.full_like(c["head"], float("nan"))
    poisoned[c["s0"]] = c["head"][c["s0"]]
    for got, want in zip(_loss_rows(c, poisoned), (loss2, g_obj, g_reg, dpos)):
        assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("scales", [(1.0, 5.0), (0.37, -2.5)])
@pytest.mark.parametrize("n,A,dw,npos", CASES)
def test_head_grad_rows_equals_unflatten_of_the_scaled_dense_gradient(n, A, dw, npos, scales, dtype, dev):
    from nerf_rpn_amd import lib, ops
    c = _case(n, A, dw, npos, dev)
    _, g_obj, g_reg, _ = _loss_rows(c, c["head"])
    plan, V, st = c["plan"], c["V"], _stream()
    dt = lib.F32 if dtype == torch.float32 else lib.BF16
    s_obj, s_reg = torch.tensor(scales[0], device=dev), torch.tensor(scales[1], device=dev)
    # today's chain: torch's fp32 multiply of the dense gradients, then head_unflatten (no scale) per (level, scene)
    gl, gd = (c["g_logits"] * s_obj).contiguous(), (c["g_deltas"] * s_reg).contiguous()
    want = torch.empty((V, LD), dtype=dtype, device=dev)
    off = 0
    for l, cl in enumerate(c["cells"]):
        for i in range(n):
            r0 = plan.level_start[l] + i * cl
            lib.call("head_unflatten", gl[i, off:].data_ptr(), gd[i, off:].data_ptr(), cl, LD, A, dw, 0, want[r0:r0 + cl].data_ptr(), dt, st)
        off += cl * A
    got = torch.full((V, LD), SENTINEL, dtype=dtype, device=dev)
    rows, nrows = plan.rows(0)
    lib.call("head_grad_rows", got.data_ptr(), dt, LD, rows, nrows, *ops._head_levels(plan), n, c["T"], A, dw, c["pos"].data_ptr(), npos,
             c["neg"].data_ptr(), 40, g_obj.data_ptr(), g_reg.data_ptr(), s_obj.data_ptr(), s_reg.data_ptr(), st)
    s0 = c["s0"]
    assert torch.equal(got[s0], want[s0])      # values, and the zeros of unsampled and padding columns
    assert (want[s0] != 0).any() and (want[s0] == 0).any()
    # where the row is written with a zero it is +0, whatever the sign of the upstream scalar
    zero = got[s0] == 0
    assert torch.all(bits(got[s0])[zero] == 0)
    rest = torch.ones(V, dtype=torch.bool, device=dev)
    rest[s0] = False
    assert torch.all(got[rest] == SENTINEL)      # rows outside S_0 are not written


def test_bad_level_table_is_refused(dev):
    from nerf_rpn_amd import lib, ops
    c = _case(1, 3, 6, 24, dev)
    with pytest.raises(lib.NrpnError, match="anchors per scene"):
        lib.call("rpn_sampled_loss_rows_f32", c["head"].data_ptr(), LD, *ops._head_levels(c["plan"]), 1, c["T"] + 1, 3, 6, c["targets"].data_ptr(),
                 c["pos"].data_ptr(), 24, c["neg"].data_ptr(), 40, BETA, c["loss2"].data_ptr(), c["loss2"].data_ptr(), c["loss2"].data_ptr(),
                 c["loss2"].data_ptr(), _stream())


def _hook(labels):
    """A deterministic sample from the matcher's labels: up to 24 positives and 40 negatives per scene, flat over the batch."""
    g = torch.Generator().manual_seed(5)
    T = labels[0].numel()
    pos, neg = [], []
    for i, lab in enumerate(labels):
        lab = lab.cpu()
        p, q = torch.where(lab == 1)[0], torch.where(lab == 0)[0]
        pos.append(p[torch.randperm(p.numel(), generator=g)[:24]] + i * T)
        neg.append(q[torch.randperm(q.numel(), generator=g)[:40]] + i * T)
    return torch.cat(pos), torch.cat(neg)


def test_step_with_one_loss_term_left_out(dev, monkeypatch):
    """Only loss_objectness in the total: the box loss's upstream gradient never arrives (None on the row path, zeros on the flattened one)."""
    _step_on_and_off([(48, 40, 32)], True, torch.float32, dev, monkeypatch, lambda losses: losses["loss_objectness"] * 1.5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shapes,rotated", [([(48, 40, 32)], True), ([(48, 48, 32), (40, 32, 32)], False)])
def test_step_with_rows_loss_equals_step_without(shapes, rotated, dtype, dev, monkeypatch):
    """loss_2d_requires_grad = False (what the trainers set at reg_loss_weight_2d = 0), injected sample: the three reported losses and every
    parameter gradient are equal with the switch on and off, and each run took the path it names."""
    _step_on_and_off(shapes, rotated, dtype, dev, monkeypatch, lambda losses: losses["loss_objectness"] + 5.0 * losses["loss_rpn_box_reg"])


def _step_on_and_off(shapes, rotated, dtype, dev, monkeypatch, total):
    from nerf_rpn_amd import ops
    from test_gpu_cone import rand_boxes
    from test_gpu_e2e import build, scene
    xs = [scene(s, 300 + i).to(dev) for i, s in enumerate(shapes)]
    gts = [rand_boxes(5, s, rotated, 90 + i).to(dev) for i, s in enumerate(shapes)]
    names = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    res = {}
    monkeypatch.setattr(ops, "CONE_ROWS_LOSS", [True])
    for on in (True, False):
        ops.CONE_ROWS_LOSS[0] = on
        m = build(rotated, 160, dev).train()
        m.set_compute_dtype(dtype)
        m.rpn.loss_2d_requires_grad = False
        m.rpn.sampler_hook = _hook
        del names[:]
        torch.manual_seed(11)
        _, losses, _ = m(xs, gts)
        total(losses).backward()
        fused = "rpn_sampled_loss_rows_f32" in names and "head_grad_rows" in names
        old = "head_flatten_f32" in names and "head_unflatten" in names and "rpn_sampled_loss_f32" in names
        assert (fused, old) == (on, not on), (on, sorted(set(names)))
        assert m.rpn.last_aux["pos"].numel() > 0
        res[on] = ({k: v.detach().clone() for k, v in losses.items()}, {k: p.grad.detach().clone() for k, p in m.named_parameters()})
    assert set(res[True][0]) == {"loss_objectness", "loss_rpn_box_reg", "loss_rpn_box_reg_2d"}
    for k, v in res[False][0].items():
        print(k, v.item(), res[True][0][k].item())
        assert torch.equal(res[True][0][k], v), k
    assert res[True][1].keys() == res[False][1].keys()
    for k, g in res[False][1].items():
        assert torch.equal(res[True][1][k], g), k
