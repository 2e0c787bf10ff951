"""Host tests of the bf16x3 checker (tests/nerf_split_ref.py): the emulation restates the float32 checker, its bound
is satisfiable by another summation order and sharp against a missing product, the gradient cases' construction terminates and holds,
and the Python layers know the mode's name.  No GPU."""
import numpy as np
import pytest
import torch

import nerf_extract_ref as R
import nerf_query_ref as Q
import nerf_split_ref as S
from nerf_split_ref import records, refs  # noqa: F401  (fixtures)

from nerf_rpn_amd import NeRF, lib, ops


def raw_of(c, mode):
    return S.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, mode=mode)["raw"]


@pytest.mark.parametrize("name", S.NAMES)
def test_exact_residuals_restate_the_float32_checker(name, refs):
    """With the residuals unrounded and all four partial products, a product is x w again: the emulation is then as far from float64
    as the float32 checker is, up to the rounding of four sums in place of one."""
    c, _, o64 = refs(name)
    o32 = Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, dtype=torch.float32, want_pre=False)["raw"]
    exact = raw_of(c, "exact_residuals")
    err32, err = S.deviation(o32, o64["raw"]), S.deviation(exact, o64["raw"])
    floor = float(np.spacing(np.float32(np.abs(o64["raw"]).max())))
    print(f"{name}: float32 checker {err32:.3g}, exact residuals {err:.3g}, split {S.deviation(raw_of(c, 'split'), o64['raw']):.3g}")
    assert err <= max(4 * err32, floor)
    assert S.deviation(exact, o32) <= max(4 * err32, floor)


@pytest.mark.parametrize("name", S.NAMES)
def test_blocked_order_is_within_the_bound_and_mutations_are_not(name, refs):
    c, emu, o64 = refs(name)
    bound = S.bound_of(emu["raw"], o64["raw"])
    blocked = S.deviation(raw_of(c, "blocked"), o64["raw"])
    print(f"{name}: bound {bound:.3g}, blocked order {blocked:.3g}")
    assert blocked <= bound
    for m in S.MUTATIONS:
        err = S.deviation(raw_of(c, m), o64["raw"])
        print(f"{name}: {m} {err:.3g}, {err / bound:.3g} x the bound")
        assert err > bound, m


@pytest.mark.parametrize("name", S.GRAD_NAMES)
def test_nudged_cases_hold_their_margins(name, refs):
    c, emu, o64 = refs(name, True)
    assert c.nudge["holds"] and c.nudge["passes"] < S.MAX_PASSES and S.margins_hold(c)
    plain = S.case_inputs(S.CASES[S.NAMES.index(name)])
    assert all(torch.equal(v, plain.state[k]) for k, v in c.state.items() if not k.endswith(".bias"))
    assert all(v.dtype == torch.float32 for v in c.state.values())
    # with no relu near zero the emulation's gradients are near the float64 ones, as its raw is
    for k in emu:
        rel = S.deviation(emu[k], o64[k]) / max(float(np.abs(o64[k]).max()), 1e-30)
        assert rel < 1e-4, (k, rel)


def test_smallest_shift():
    p = torch.tensor([[0.5, 0.01, -0.02], [-0.3, 0.04, 0.03]], dtype=torch.float64)
    d = S.smallest_shift(p, 0.05)
    assert d[0] == 0
    assert ((p + d).abs() >= 0.05 * (1 - 1e-12)).all()
    assert abs(float(d[1]) - 0.04) < 1e-12          # 0.01 -> 0.05 is the nearest exit: -0.06 and -0.09 are farther
    assert abs(float(d[2]) - 0.07) < 1e-12          # between the two there is no room: up past -0.02


def test_emulation_backward_is_the_float32_linear():
    g = torch.Generator().manual_seed(5)
    x, w, b = (torch.randn(s, generator=g, requires_grad=True) for s in ((7, 32), (5, 32), (5,)))
    dy = torch.randn(7, 5, generator=g)
    got = torch.autograd.grad((S.SplitLinear.apply(x, w, b, "split") * dy).sum(), (x, w, b))
    want = torch.autograd.grad((torch.nn.functional.linear(x, w, b) * dy).sum(), (x, w, b))
    for a, e in zip(got, want):
        assert torch.allclose(a, e, rtol=1e-6, atol=1e-6)


def test_emulated_swaps_the_float32_model_only():
    state = R.make_state(3)
    with S.emulated():
        assert isinstance(R.build_model(state), S.SplitNeRF)
        assert not isinstance(R.build_model(state, None, torch.float64), S.SplitNeRF)
    assert not isinstance(R.build_model(state), S.SplitNeRF)


def test_recorded_figures_are_this_checkers(records, refs):
    """tests/golden/nerf_split_bounds.json is a record, not a bound: its host figures are what this checker gives."""
    assert sorted(records["cases"]) == sorted(S.NAMES) and sorted(records["gradient_cases"]) == sorted(S.GRAD_NAMES)
    assert records["factor"] == S.FACTOR and records["margin"] == S.MARGIN
    for name in S.NAMES:
        _, emu, o64 = refs(name)
        # the host's matmul sums in an order that depends on its threads and CPU: the same figure up to what another order changes
        assert 0.5 <= records["cases"][name]["raw"]["emulation"] / S.deviation(emu["raw"], o64["raw"]) <= 2.0


# ---- the mode's name through the Python layers -----------------------------------------------------------------------------------
def test_dtype_names():
    assert ops.NERF_DTYPES == ("fp32", "bf16x3")
    state = R.make_state(3)
    for f in (lambda d: ops.nerf_grid_pack(state, R.DEFAULT_CFG, dtype=d), lambda d: NeRF(R.DEFAULT_CFG, dtype=d),
              lambda d: NeRF(R.DEFAULT_CFG).set_compute_dtype(d),
              lambda d: ops.nerf_query(state, R.DEFAULT_CFG, torch.zeros(1, 1, 3), torch.zeros(1, 3), dtype=d),
              lambda d: ops.nerf_grid_query(state, R.DEFAULT_CFG, [0.], [0.], [0.], (0., 0., 0.), 1., torch.eye(4)[None], dtype=d),
              lambda d: ops.nerf_render(state, R.DEFAULT_CFG, rays=torch.zeros(1, 6), near=0.1, far=1., n_samples=4, dtype=d)):
        for bad in ("bf16", "fp16", "BF16X3", torch.float32):
            with pytest.raises(ValueError, match="dtype"):
                f(bad)
        for good in ops.NERF_DTYPES:
            try:
                f(good)
            except lib.NrpnError as e:           # without a device the name is accepted and the missing device reported
                assert "gfx950" in str(e) and not torch.cuda.is_available()
    m = NeRF(R.DEFAULT_CFG, dtype="bf16x3")
    assert m.compute_dtype == "bf16x3" and NeRF(R.DEFAULT_CFG).compute_dtype == "fp32"
    assert m.set_compute_dtype("fp32") is m and m.compute_dtype == "fp32"
    assert len(list(m.parameters())) == 24 and all(p.dtype == torch.float32 for p in m.parameters())


def test_given_weights_carry_their_dtype():
    w = ops.NerfGridWeights(None, None, None, ops.nerf_grid_config(R.DEFAULT_CFG), dtype="bf16x3", split=torch.zeros(8, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="packed for 'bf16x3'"):
        ops._nerf_weights("t", w, R.DEFAULT_CFG, "fp32")
    assert ops._nerf_weights("t", w, R.DEFAULT_CFG) is w and ops._nerf_weights("t", w, R.DEFAULT_CFG, "bf16x3") is w
    name, head = w.entry("nerfgrid_query", 1, 2)
    assert name == "nerfgrid_query_bf16x3" and head[:2] == (1, 2) and len(head) == 3
    w32 = ops.NerfGridWeights(None, None, None, w.config)
    assert w32.dtype == "fp32" and w32.entry("nerfgrid_query", 1, 2) == ("nerfgrid_query", (1, 2))


def test_command_lines_take_the_flag():
    from nerf_rpn_amd.scripts import nerf_extract, nerf_render, nerf_test, nerf_train
    for mod in (nerf_extract, nerf_render, nerf_test, nerf_train):
        p = mod.build_parser()
        assert p.parse_args([]).dtype == "fp32"
        assert p.parse_args(["--dtype", "bf16x3"]).dtype == "bf16x3"
        with pytest.raises(SystemExit):
            p.parse_args(["--dtype", "bf16"])


def test_extract_hands_the_op_a_state_dict_in_fp32_and_packed_weights_in_the_mode(monkeypatch, tmp_path):
    """scripts.nerf_extract.extract: in fp32 the op is called as before the mode existed (a state dict, no dtype argument); in the
    mode it gets the weights ops.nerf_grid_pack made for it."""
    from nerf_rpn_amd.scripts import nerf_extract as X
    c = R.case_inputs(R.CASES[0])
    bbox = str(tmp_path / "bbox.json")
    R.write_bbox_json(bbox, c.bbox)
    seen = []

    def query(state_dict, cfg, xs, ys, zs, bb_center, bb_scale, poses, layout="flat", chunk=None):
        seen.append(state_dict)
        return torch.zeros(len(xs) * len(ys) * len(zs), 4)
    monkeypatch.setattr(ops, "nerf_grid_query", query)
    monkeypatch.setattr(ops, "nerf_grid_pack", lambda state, cfg, dtype="fp32": ("packed", dtype))
    X.extract(c.cfg, c.state, c.poses, bbox, c.max_res, c.bb_center, c.bb_scale)
    X.extract(c.cfg, c.state, c.poses, bbox, c.max_res, c.bb_center, c.bb_scale, dtype="bf16x3")
    assert seen[0] is c.state and seen[1] == ("packed", "bf16x3")


def test_abi_twins_are_declared_and_exported():
    twins = ["nerfgrid_pack", "nerfgrid_query", "nerfrender_rays", "nerfrender_frame", "nerfquery_forward", "nerfquery_backward"]
    L = lib.load()
    declared = lib.declared_symbols(tools=False)
    protos = lib._prototypes()
    for t in twins:
        name = f"nrpn_{t}_bf16x3"
        assert name in declared and hasattr(L, name)
        if t != "nerfgrid_pack":                  # a twin: its fp32 entry's arguments plus the planes
            assert len(protos[name][1]) == len(protos[f"nrpn_{t}"][1]) + 1
    assert L.nrpn_abi_version() == 3
    assert lib.query("nerfgrid_work_bytes", 2, 0) == 2 * 2 * (lib.query("nerfgrid_work_bytes", 0, 0) // 4 - 9 * 256 - 256 - 4 - 3 * 128 - 4)
