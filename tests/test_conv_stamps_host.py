"""CPU: the decoder of the in-kernel phase stamps on synthetic records with known phase lengths, the host-only layout query of the stamped
conv launches through the built library, and where the two tools-only entry points are declared."""
import os
import re
import subprocess

import numpy as np
import pytest

from nerf_rpn_amd import lib, stamps

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

# (grid, cin, cout, ksize): the shapes of tests/test_gpu_conv_stamps.py
SHAPES = [((5, 5, 5), 512, 256, 1), ((5, 5, 5), 512, 512, 3), ((10, 10, 10), 512, 512, 3), ((20, 20, 20), 256, 256, 3),
          ((20, 20, 20), 512, 512, 3), ((5, 4, 3), 64, 64, 3), ((5, 4, 3), 64, 64, 1), ((12, 12, 12), 256, 512, 3)]


# ---------------------------------------------------------------------------------------------------------------------
# synthetic launch: 4 conv workgroups on 2 XCDs + 2 epilogue workgroups, every phase length chosen here
# ---------------------------------------------------------------------------------------------------------------------
CONV_TICKS = (100, 20, 600, 30, 40, 10)          # constant-rate ticks of the six conv phases, workgroup 0
CONV_CYCLES = (2400, 480, 14400, 720, 960, 240)  # ... and their cycles
EPI_TICKS = (50, 200, 30, 10)
EPI_CYCLES = (1200, 4800, 720, 240)
ENTRY = (1000, 1010, 1020, 1040)                 # conv entries: ramp = 40 ticks
KSTEPS, WAIT = 8, (1440, 2880, 1440, 2880)       # per-workgroup wait sums


def _synthetic():
    lay = stamps.Layout(words=stamps.WORDS, plan_code=3, conv_records=4, epilogue_records=2, nbytes=6 * stamps.WORDS * 8, m_tiles=1, n_tiles=2,
                        k_slices=2, k_steps=16, slice_steps=(8, 8))
    a = np.zeros((6, stamps.WORDS), dtype=np.uint64)
    a[:, stamps.W_VERSION] = stamps.VERSION
    for r in range(4):
        # workgroup r: every phase r ticks (and 24 r cycles) longer than workgroup 0's
        rt = ENTRY[r] + np.concatenate([[0], np.cumsum(np.array(CONV_TICKS) + r)])
        cy = 5_000_000 * (r + 1) + np.concatenate([[0], np.cumsum(np.array(CONV_CYCLES) + 24 * r)])
        a[r, stamps.W_KERNEL], a[r, stamps.W_WG], a[r, stamps.W_NTILE], a[r, stamps.W_KSLICE] = stamps.KERNEL_CONV128, r, r % 2, r // 2
        a[r, stamps.W_XCD], a[r, stamps.W_KSTEPS] = r % 2, KSTEPS
        a[r, stamps.W_PHASE0:stamps.W_PHASE0 + 14:2], a[r, stamps.W_PHASE0 + 1:stamps.W_PHASE0 + 14:2] = rt, cy
        a[r, stamps.W_WAIT_SUM], a[r, stamps.W_WAIT_MAX] = WAIT[r], WAIT[r] // 4
        a[r, stamps.W_KSTEP0:stamps.W_KSTEP0 + 8] = cy[2] + (np.arange(8) + 1) * ((cy[3] - cy[2]) // 8)
    last_exit = max(int(a[r, stamps.W_PHASE0 + 12]) for r in range(4))
    for e in range(2):
        rt = last_exit + 300 + 5 * e + np.concatenate([[0], np.cumsum(np.array(EPI_TICKS) + 2 * e)])      # seam = 300 ticks, ramp = 5
        cy = 9_000_000 + np.concatenate([[0], np.cumsum(np.array(EPI_CYCLES) + 48 * e)])
        q = 4 + e
        a[q, stamps.W_KERNEL], a[q, stamps.W_WG], a[q, stamps.W_XCD], a[q, stamps.W_KSTEPS] = stamps.KERNEL_EPILOGUE, e, e, 3
        a[q, stamps.W_PHASE0:stamps.W_PHASE0 + 10:2], a[q, stamps.W_PHASE0 + 1:stamps.W_PHASE0 + 10:2] = rt, cy
    return a, lay


def _pct(values):
    p = np.percentile(np.asarray(values, dtype=np.float64), [10, 50, 90])
    return {"p10": float(p[0]), "median": float(p[1]), "p90": float(p[2])}


def test_decoder_gives_the_constructed_table():
    a, lay = _synthetic()
    d = stamps.decode(a.view(np.int64), lay)
    assert d["plan_code"] == 3
    c, e = d["conv"], d["epilogue"]
    assert c["records"] == 4 and e["records"] == 2
    for i, name in enumerate(stamps.CONV_PHASES):
        assert c["phases"][name]["ns"] == _pct([(CONV_TICKS[i] + r) * 10 for r in range(4)]), name
        assert c["phases"][name]["cycles"] == _pct([CONV_CYCLES[i] + 24 * r for r in range(4)]), name
    # workgroup 0's phases are the p10 - 0.3 step away: spot-check one number by hand (ticks 600..603 -> 6000..6030 ns, median 6015)
    assert c["phases"]["k_loop"]["ns"]["median"] == 6015.0 and c["phases"]["k_loop"]["cycles"]["median"] == 14436.0
    for i, name in enumerate(stamps.EPILOGUE_PHASES):
        assert e["phases"][name]["ns"] == _pct([(EPI_TICKS[i] + 2 * q) * 10 for q in range(2)]), name
        assert e["phases"][name]["cycles"] == _pct([EPI_CYCLES[i] + 48 * q for q in range(2)]), name
    # ramp, span and seam as constructed: conv exits at entry + sum(ticks) + 6 r
    exits = [ENTRY[r] + sum(CONV_TICKS) + 6 * r for r in range(4)]
    assert c["ramp_ns"] == 400.0 and c["span_ns"] == (max(exits) - ENTRY[0]) * 10.0
    assert c["xcd_entry_skew_ns"] == 100.0 and c["xcds"] == 2             # XCD 0 first seen at 1000, XCD 1 at 1010
    assert d["seam_ns"] == 3000.0 and e["ramp_ns"] == 50.0
    epi_exit = max(exits) + 300 + 5 + sum(EPI_TICKS) + 8
    assert e["span_ns"] == (epi_exit - (max(exits) + 300)) * 10.0 and d["span_ns"] == (epi_exit - ENTRY[0]) * 10.0
    loops = [CONV_CYCLES[2] + 24 * r for r in range(4)]
    assert c["kstep_cycles_mean"] == float(np.mean([v / KSTEPS for v in loops]))
    assert c["wait_share"] == sum(WAIT) / sum(loops)


def test_decoder_without_epilogue():
    a, lay = _synthetic()
    lay = lay._replace(conv_records=4, epilogue_records=0)
    d = stamps.decode(a[:4], lay)
    assert d["epilogue"] is None and d["seam_ns"] is None and d["span_ns"] == d["conv"]["span_ns"]


def test_decoder_refuses_fill_version_and_backwards_phases():
    a, lay = _synthetic()
    b = a.copy(); b[2, :] = stamps.FILL
    with pytest.raises(stamps.StampError, match="conv record 2 still holds the fill pattern"):
        stamps.decode(b, lay)
    b = a.copy(); b[5, 9:] = stamps.FILL                                     # a half-written epilogue record
    with pytest.raises(stamps.StampError, match="epilogue record 1 still holds the fill pattern"):
        stamps.decode(b, lay)
    assert np.int64(stamps.FILL_I64).view(np.uint64) == np.uint64(stamps.FILL)
    b = a.copy(); b[1, stamps.W_VERSION] = stamps.VERSION + 1
    with pytest.raises(stamps.StampError, match="conv record 1: version word"):
        stamps.decode(b, lay)
    b = a.copy(); b[3, stamps.W_PHASE0 + 2 * 4] = b[3, stamps.W_PHASE0 + 2 * 3] - 1      # stores issued before the loop ended
    with pytest.raises(stamps.StampError, match="conv record 3: the constant-rate clock runs backwards"):
        stamps.decode(b, lay)
    b = a.copy(); b[4, stamps.W_PHASE0 + 2 * 2 + 1] = b[4, stamps.W_PHASE0 + 2 * 1 + 1] - 1
    with pytest.raises(stamps.StampError, match="epilogue record 0: the cycle clock runs backwards"):
        stamps.decode(b, lay)
    with pytest.raises(stamps.StampError, match="do not fit the layout"):
        stamps.decode(a[:5], lay)


# ---------------------------------------------------------------------------------------------------------------------
# nrpn_conv3d_fwd_stamp_layout through the built library (host only: no device call)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,cin,cout,k", SHAPES, ids=[f"{'x'.join(map(str, s[0]))}_{s[1]}_{s[2]}_k{s[3]}" for s in SHAPES])
@pytest.mark.parametrize("kw", [{}, {"tile": lib.TILE_256X256, "big_split": 0}, {"stagger": 0}], ids=["default", "tile256-unsliced", "plain-loop"])
def test_layout_matches_the_plan(grid, cin, cout, k, kw):
    from nerf_rpn_amd import ops
    if not os.path.exists(lib.SO_PATH):
        lib.build()
    opts = lib.ConvOpts(**kw)
    a = (1, *grid, cin, cout, k, lib.BF16, opts.ptr())
    code, wsb = lib.query("conv3d_fwd_plan_ex", *a), lib.query("conv3d_fwd_workspace_bytes_ex", *a)
    lay = ops.conv3d_stamp_layout(1, *grid, cin, cout, k, lib.BF16, opts)
    M = grid[0] * grid[1] * grid[2]
    assert lay.plan_code == code and code in (0, 1, 2, 3) and lay.words == stamps.WORDS == 32
    big = code in (1, 2)
    bm, bn = (256, 256) if big else (128, 64 if cout <= 64 else 128)
    slices = wsb // (M * cout * 4) if wsb else 1                              # the plan's K slices, from the workspace it asks for
    assert wsb % (M * cout * 4) == 0 and (slices > 1) == (code in (2, 3))
    assert (lay.m_tiles, lay.n_tiles, lay.k_slices) == (-(-M // bm), -(-cout // bn), slices)
    assert lay.conv_records == lay.m_tiles * lay.n_tiles * slices             # the plan's workgroup count
    assert (lay.epilogue_records == 0) == (slices == 1)
    if slices > 1:
        assert lay.epilogue_records == min(4096, -(-M * cout // 256))
    assert lay.nbytes == (lay.conv_records + lay.epilogue_records) * 32 * 8
    assert lay.k_steps == k ** 3 * cin * 2 // 128 and len(lay.slice_steps) == slices
    assert sum(lay.slice_steps) == lay.k_steps and min(lay.slice_steps) >= 1 and max(lay.slice_steps) == -(-lay.k_steps // slices)


@pytest.mark.parametrize("what,dtype,kw", [("fp32", lib.F32, {}), ("64-byte K-step", lib.BF16, {"kstep_bytes": 64}),
                                           ("register-staged", lib.BF16, {"lds_dma": 0}), ("halo form", lib.BF16, {"tile": lib.TILE_HALO}),
                                           ("wave-specialised", lib.BF16, {"tile": lib.TILE_256X128_WS}),
                                           ("4-wave", lib.BF16, {"tile": lib.TILE_256X256_W4})])
def test_layout_refuses_plans_without_a_stamped_form(what, dtype, kw):
    if not os.path.exists(lib.SO_PATH):
        lib.build()
    opts, lay = lib.ConvOpts(**kw), lib.StampLayout()
    lay.words = -7
    a = (1, 20, 20, 20, 512, 512, 3, dtype, opts.ptr())
    code = lib.query("conv3d_fwd_plan_ex", *a)
    with pytest.raises(lib.NrpnError, match=rf"\(-1\): conv3d_fwd_stamp_layout: plan code {code} has no stamped form for .*{what}"):
        lib.call("conv3d_fwd_stamp_layout", *a, lay.ptr())
    assert lay.words == -7                                                    # a refused query writes nothing


# ---------------------------------------------------------------------------------------------------------------------
# where the entries are declared
# ---------------------------------------------------------------------------------------------------------------------
def _declared(header, tmp_path):
    src = tmp_path / (header + ".c")
    src.write_text(f'#include "{header}"\n')
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-E", "-P", str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return set(re.findall(r"\b(nrpn_[a-z0-9_]+)\s*\(", out.stdout))


def test_entries_are_declared_by_the_tools_header_only(tmp_path):
    """A program that includes nerfrpn_tools.h sees both entry points (and the record's word order); one that includes the drop-in
    boundary nerfrpn.h sees neither, and nothing named *stamp* at all."""
    tools, public = _declared("nerfrpn_tools.h", tmp_path), _declared("nerfrpn.h", tmp_path)
    assert {"nrpn_conv3d_fwd_stamp_layout", "nrpn_conv3d_fwd_stamped"} <= tools
    assert not [n for n in public if "stamp" in n]
    assert "stamp" not in open(os.path.join(INCLUDE, "nerfrpn.h")).read().lower()
    text = open(os.path.join(INCLUDE, "nerfrpn_stamps.h")).read()
    for name, value in (("NRPN_STAMP_WORDS", stamps.WORDS), ("NRPN_STAMP_REALTIME_NS", stamps.REALTIME_NS), ("NRPN_SW_XCD", stamps.W_XCD),
                        ("NRPN_SW_KSTEPS", stamps.W_KSTEPS), ("NRPN_SW_PHASE0", stamps.W_PHASE0), ("NRPN_SW_WAIT_SUM", stamps.W_WAIT_SUM),
                        ("NRPN_SW_WAIT_MAX", stamps.W_WAIT_MAX), ("NRPN_SW_KSTEP0", stamps.W_KSTEP0), ("NRPN_SP_CONV_PHASES", len(stamps.CONV_STAMPS)),
                        ("NRPN_SE_PHASES", len(stamps.EPILOGUE_STAMPS)), ("NRPN_STAMP_MAX_SLICES", lib.STAMP_MAX_SLICES)):
        assert re.search(rf"#define {name} {value}\b", text), name
    assert int(re.search(r"#define NRPN_STAMP_VERSION (0x[0-9A-Fa-f]+)ull", text).group(1), 16) == stamps.VERSION
    lib_ = lib.load()
    assert lib_.nrpn_abi_version() == 3 and hasattr(lib_, "nrpn_conv3d_fwd_stamped")
