"""CPU: the conv launch plans (csrc/conv_plan.h).  The size / plan queries are pure host functions, so the library loads without a GPU.

tests/golden/conv_plans.npz was recorded (tools/record_conv_plans.py) from a build of the commit before the plans became one value per
call: the in-tree library must reproduce every query of it.  The plans' own invariants are checked twice: on the plan structs by a
stand-alone C++ program that includes the planning header, and through the queries on the table's sweep."""
import os
import subprocess

import numpy as np
import pytest

from conv_plan_sweep import columns, sweep
from nerf_rpn_amd import lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table():
    if not os.path.exists(lib.SO_PATH):
        lib.build()
    return sweep(lib.load())


def test_plans_equal_the_recorded_table(table):
    want = dict(np.load(os.path.join(HERE, "golden", "conv_plans.npz"), allow_pickle=False))
    assert sorted(table) == sorted(want)
    assert sum(v.shape[0] for k, v in want.items() if k.endswith("_shapes")) >= 3000 and len(want) >= 100
    for name in sorted(want):
        bad = np.flatnonzero((table[name] != want[name]).reshape(want[name].shape[0], -1).any(axis=1))
        assert bad.size == 0, (name, bad.size, [(int(i), table[name][i].tolist(), want[name][i].tolist()) for i in bad[:5]])


def test_plan_invariants_on_the_plan_structs(tmp_path):
    """No empty K slice, workgroup counts below 2^31, whole rows + tail rows = M, workspace bytes = slices x rows covered x Cout x 4,
    statistics rows only on the plans with fused statistics -- for every plan family, knob and per-call fact."""
    exe = str(tmp_path / "conv_plan_invariants")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(HERE, "conv_plan_invariants.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:]
    assert int(run.stdout.split()[0]) > 1_000_000, run.stdout


def test_plan_invariants_through_the_queries(table):
    s = table["fwd_shapes"]
    M, cin, cout, es = s[:, 0] * s[:, 1] * s[:, 2] * s[:, 3], s[:, 4], s[:, 5], np.where(s[:, 7] == lib.F32, 4, 2)
    plans, bytes_, stats = (columns(table, "conv3d_fwd_" + q) | {"ex " + k: v for k, v in columns(table, f"conv3d_fwd_{q}_ex").items()}
                            for q in ("plan", "workspace_bytes", "stats_rows"))
    for tag, code in plans.items():
        ws, st = bytes_[tag], stats[tag]
        assert set(np.unique(code)) <= set(range(8)), tag
        sliced = np.isin(code, (2, 3, 6))
        per = M * cout * 4
        # K slices over every row: a whole number (>= 2) of [M][Cout] fp32 partials; halo form: none
        assert (ws[sliced] % per[sliced] == 0).all() and (ws[sliced] // per[sliced] >= 2).all() and (ws[sliced] // per[sliced] <= 64).all(), tag
        assert (ws[code == 7] == 0).all() and (ws[np.isin(code, (0, 4, 5))] == 0).all(), tag
        # tail split of the 256x256 tile: ks slices of the rows from a 256-row tile boundary on, the whole rows before it cover the rest
        tail = (code == 1) & (ws > 0)
        for i in np.flatnonzero(tail):
            mt = -(-int(M[i]) // 256)
            t0 = mt - mt % 256          # the tail = the tiles past the last whole round of 256
            assert 0 < t0 < mt and any(ks * (int(M[i]) - t0 * 256) * int(cout[i]) * 4 == int(ws[i]) for ks in range(2, 9)), (tag, s[i].tolist(), int(ws[i]))
        # statistics rows: 0 exactly when the plan is one without fused statistics
        # (fused: bf16 LDS-DMA kernels with a staged epilogue -- 256x256, halo, and the 128-row tile on the 128-byte K-step)
        fused = (es == 2) & (cout % 8 == 0) & (np.isin(code, (1, 5, 7)) | ((code == 0) & ((cin * 2) % 128 == 0) & ("kstep_bytes=64" not in tag)))
        if "lds_dma=0" in tag or tag.endswith(("tile=256", "tile_m=256")):
            fused[:] = False
        assert ((st > 0) == fused).all(), tag
        assert (st[code == 1] == 2 * -(-M[code == 1] // 256)).all() and (st < 2 ** 31).all(), tag
    # weight gradient: no empty slice of the voxel axis; workspace = tap mask + slices x wrows fp32 bias partials
    w = table["wgrad_shapes"]
    Mw, wrows, k3, kv = w[:, 0] * w[:, 1] * w[:, 2] * w[:, 3], w[:, 6], w[:, 7] == 3, np.where(w[:, 8] == lib.F32, 32, 64)
    chunks = -(-Mw // kv)
    for tag, sl in columns(table, "conv3d_wgrad_slices").items():
        assert (sl >= 1).all() and (-(-chunks // -(-chunks // sl)) == sl).all(), tag
        mask = np.where(k3, (Mw * 4 + 255) // 256 * 256, 0)
        assert (columns(table, "conv3d_wgrad_workspace_bytes")[tag] == mask + sl * wrows * 4).all(), tag
        big = columns(table, "conv3d_wgrad_plan")[tag]
        assert set(np.unique(big)) <= {0, 1} and not big[w[:, 8] == lib.F32].any(), tag
    st_ = table["stem_shapes"]
    for tag, sl in columns(table, "stem_wgrad_slices").items():
        assert (sl >= 1).all() and (columns(table, "stem_wgrad_workspace_bytes")[tag] == sl * st_[:, 4] * 4).all(), tag
    # row lists: a whole number of partial rows of Cout fp32 each, on 2..32 slices
    r = table["rows_shapes"]
    for tag, ws in columns(table, "conv3d_fwd_rows_workspace_bytes").items():
        assert (ws % (r[:, 2] * 4) == 0).all() and (ws <= 32 * r[:, 0] * r[:, 2] * 4).all(), tag
