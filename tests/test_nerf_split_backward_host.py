"""Host tests of the checker of the bf16x3 backward (tests/nerf_split_backward_ref.py): the kernels' summation order
lies within the bound the arithmetic's emulation gives, dropping any cross term of the backward products leaves that bound on every
tensor the mode touches, and what the mode does not touch is the forward mode's emulation bit for bit.  Also the switch through the
Python layers and the C declarations.  No tolerance is typed in: every bound is S.bound_of(emulation, float64)."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import nerf_extract_ref as R
import nerf_query_ref as Q
import nerf_split_backward_ref as B
import nerf_split_ref as S
from nerf_split_backward_ref import brefs  # noqa: F401  (fixture)

from nerf_rpn_amd import NeRF, lib, nerf_train, ops


# ---- the emulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_cases_keep_their_relu_margins(name, brefs):
    c = brefs(name).c
    assert c.nudge["holds"] and S.margins_hold(c)
    if name == "p65x65":
        assert c.pts.shape == (325, 13, 3) and -(-c.pts.shape[0] * c.pts.shape[1] // B.TILE) == 67       # slices of two tiles


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_blocked_order_is_within_the_bound_of_split(name, brefs):
    r = brefs(name)
    blocked = r.mode("blocked")
    for k in Q.tensor_names(r.c.cfg):
        S.assert_within(f"{name}/{k}", blocked[k], r.split[k], r.f64[k])


@pytest.mark.parametrize("mutation", B.MUTATIONS)
@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_a_dropped_term_leaves_the_bound_on_every_touched_tensor(name, mutation, brefs):
    r = brefs(name)
    mutant = r.mode(mutation)
    assert np.array_equal(mutant["raw"], r.split["raw"])          # the forward is not mutated
    kept = []
    for k in B.touched_names(r.c.cfg):
        err, bound = S.deviation(mutant[k], r.f64[k]), S.bound_of(r.split[k], r.f64[k])
        print(f"{name}/{mutation}/{k}: error {err:.3g}, bound {bound:.3g}, ratio {err / bound:.3g}")
        if err <= bound:
            kept.append((k, err, bound))
    assert not kept, kept


@pytest.mark.parametrize("name", B.CASE_NAMES)
def test_untouched_tensors_are_the_forward_modes(name, brefs):
    r = brefs(name)
    assert len(B.touched_names(r.c.cfg)) == 19
    assert np.array_equal(r.split["raw"], r.old["raw"])
    for k in B.untouched_names(r.c.cfg):
        assert np.array_equal(r.split[k], r.old[k]), k
    assert not np.array_equal(r.split["pts_linears.0.weight"], r.old["pts_linears.0.weight"])      # another arithmetic


def test_wgrad_product_slices_and_terms():
    """The blocked wgrad cuts 67 tiles into slices of two; on bf16-valued operands (lo = 0) every variant is the exact product."""
    gen = torch.Generator().manual_seed(5)
    dy, x = torch.randn(4225, 8, generator=gen), torch.randn(4225, 5, generator=gen)
    want = dy.double().T @ x.double()
    split = B.wgrad_product(dy, x)
    assert S.deviation(B.wgrad_product(dy, x, "blocked"), want) <= S.bound_of(split, want)
    assert S.deviation(B.wgrad_product(dy, x, "hihi"), want) > S.bound_of(split, want)
    small = torch.randint(-8, 9, (130, 8), generator=gen).float(), torch.randint(-8, 9, (130, 5), generator=gen).float()
    for mode in B.MODES:
        assert torch.equal(B.wgrad_product(*small, mode), small[0].T @ small[1]), mode


def test_substitution_is_undone():
    before = S.SplitLinear
    with B.backward_emulated("hihi"):
        assert S.SplitLinear is not before
    assert S.SplitLinear is before


# ---- the switch through the Python layers -----------------------------------------------------------------------------------------
def test_switch_names_and_pairing():
    assert ops.nerf_check_backward_dtype("fp32", "fp32") == "fp32" and ops.nerf_check_backward_dtype("bf16x3", "fp32") == "fp32"
    assert ops.nerf_check_backward_dtype("bf16x3", "bf16x3") == "bf16x3"
    for dtype, bad in (("fp32", "bf16x3"), ("bf16x3", "bf16"), ("bf16x3", torch.bfloat16), ("fp32", None)):
        with pytest.raises(ValueError, match="backward_dtype"):
            ops.nerf_check_backward_dtype(dtype, bad)
    state = R.make_state(3)
    for dtype, bad in (("fp32", "bf16x3"), ("bf16x3", "fp16")):          # refused before a device is asked for
        with pytest.raises(ValueError, match="backward_dtype"):
            ops.nerf_query(state, R.DEFAULT_CFG, torch.zeros(1, 1, 3), torch.zeros(1, 3), dtype=dtype, backward_dtype=bad)
        with pytest.raises(ValueError, match="backward_dtype"):
            NeRF(R.DEFAULT_CFG, dtype=dtype, backward_dtype=bad)
    m = NeRF(R.DEFAULT_CFG, dtype="bf16x3", backward_dtype="bf16x3")
    assert (m.compute_dtype, m.backward_dtype) == ("bf16x3", "bf16x3")
    assert NeRF(R.DEFAULT_CFG).backward_dtype == "fp32" and NeRF(R.DEFAULT_CFG, dtype="bf16x3").backward_dtype == "fp32"
    assert m.set_compute_dtype("fp32").backward_dtype == "fp32"


def test_command_line_takes_and_records_the_switch(tmp_path):
    from nerf_rpn_amd.scripts import nerf_train as X
    p = X.build_parser()
    assert p.parse_args([]).backward_dtype == "fp32"
    assert p.parse_args(["--dtype", "bf16x3", "--backward_dtype", "bf16x3"]).backward_dtype == "bf16x3"
    with pytest.raises(SystemExit):
        p.parse_args(["--backward_dtype", "bf16"])
    for flags in (["--backward_dtype", "bf16x3"], ["--dtype", "fp32", "--backward_dtype", "bf16x3"]):
        with pytest.raises(SystemExit):                                   # before any file is read: the directories do not exist
            X.main(["--ckpt_dir", str(tmp_path / "none"), "--data_dir", str(tmp_path / "none"), "--scene_id", "s", "--image_hw", "6", "8"] + flags)
    assert not (tmp_path / "none").exists()
    args = Namespace(expname="run", ckpt_dir=str(tmp_path), dtype="bf16x3", backward_dtype="bf16x3")
    with open(os.path.join(nerf_train.write_args(args), "args.json")) as f:
        assert json.load(f)["backward_dtype"] == "bf16x3"


def test_abi_entries_are_declared_and_exported():
    L = lib.load()
    declared, protos = lib.declared_symbols(tools=False), lib._prototypes()
    for name in ("nrpn_nerfquery_pack_t_bf16x3", "nrpn_nerfquery_backward_bf16x3_split"):
        assert name in declared and hasattr(L, name)
    # planes of the transposes in place of the float transposes: the same argument count as the twin it extends
    assert len(protos["nrpn_nerfquery_backward_bf16x3_split"][1]) == len(protos["nrpn_nerfquery_backward_bf16x3"][1])
    assert len(protos["nrpn_nerfquery_pack_t_bf16x3"][1]) == len(protos["nrpn_nerfquery_pack_t"][1])
    size = (1, 1, 64, 9, 0, 4)
    assert lib.query("nerfquery_work_bytes", 5, *size) == lib.query("nerfquery_work_bytes", 2, *size)      # two bf16 per float
    assert L.nrpn_abi_version() == 3
