"""The sweep of the conv size / plan queries behind tests/golden/conv_plans.npz (host only: the queries are pure functions).

``sweep(L)`` calls every query of the table on the loaded library ``L`` and returns {name: int64 array}.  tools/record_conv_plans.py writes
that dict for a build of the commit BEFORE a change to the planning code; tests/test_conv_plans.py asserts the in-tree library reproduces it.
"""
import ctypes

import numpy as np

from nerf_rpn_amd import lib

GRIDS = [(5, 5, 5), (10, 10, 10), (20, 20, 20), (40, 40, 40), (80, 80, 80), (160, 160, 160), (200, 200, 130), (42, 42, 40), (13, 11, 9),
         (420, 1, 1), (8000, 1, 1), (70560, 1, 1)]            # the last three with n = 1: the ragged-style (1, V, 1, 1)
CHANNELS = [16, 32, 64, 96, 128, 256, 264, 512]
NROWS = [1, 127, 128, 129, 300, 9000, 33000, 35000, 66000, 70000]
TILES = [lib.TILE_128, lib.TILE_256X128_WS, lib.TILE_256X256, lib.TILE_256X256_W4, lib.TILE_HALO]
# nrpn_conv_opts variants of the _ex queries: the default, then every field of the issue set alone
OPTS = [dict()] + [dict(tile=t) for t in TILES] + [dict(lds_dma=0), dict(kstep_bytes=64), dict(stagger=0), dict(big_split=0),
                                                     dict(halo_pairing=1), dict(halo_pairing=2)]
# process-wide tools switches: (setter, non-default values, default to restore)
FWD_SWITCHES = [("set_conv_kstep_bytes", [64], 128), ("set_conv_lds_dma", [0], 1), ("set_conv_tile_m", TILES, 0), ("set_conv_halo_auto", [0], 1),
                ("set_conv_halo_pairing", [0, 1], 2), ("set_conv_stagger", [0], 1), ("set_conv_big_split", [0], 1)]
WGRAD_SWITCHES = [("set_wgrad_big_tile", [0], 1), ("set_wgrad_pack2", [0], 1), ("set_wgrad_transpose_read", [0], 1)]
ROWS_SWITCHES = [("set_rows_big_tile", [1], 0), ("set_rows_tail_split", [0], 1)]
ES = {lib.F32: 4, lib.BF16: 2}


def grids():
    """(n, gx, gy, gz): n in {1, 2} on the classic grids, n = 1 on the voxel lists."""
    return [(n,) + g for g in GRIDS for n in ((1, 2) if g[1] > 1 else (1,))]


def fwd_shapes():
    """Every (n, gx, gy, gz, cin, cout, ksize, dtype) nrpn_conv3d_fwd accepts: Cin * elemsize a multiple of 64 bytes."""
    return [g + (ci, co, k, dt) for g in grids() for ci in CHANNELS for co in CHANNELS for k in (1, 3) for dt in (lib.F32, lib.BF16)
            if (ci * ES[dt]) % 64 == 0]


def wgrad_shapes():
    """(n, gx, gy, gz, cin, cout, wrows, ksize, dtype) of nrpn_conv3d_wgrad (16-byte channel rows: every channel count of the list);
    wrows = cout and, as for a layer packed with others, 2 * cout."""
    return [g + (ci, co, wr, k, dt) for g in grids() for ci in CHANNELS for co in CHANNELS for wr in (co, 2 * co) for k in (1, 3)
            for dt in (lib.F32, lib.BF16)]


def rows_shapes():
    """(nrows, cin, cout, ksize, dtype) of nrpn_conv3d_fwd_rows: Cin * elemsize a multiple of 128 bytes."""
    return [(r, ci, co, k, dt) for r in NROWS for ci in CHANNELS for co in CHANNELS for k in (1, 3) for dt in (lib.F32, lib.BF16)
            if (ci * ES[dt]) % 128 == 0]


def stem_shapes():
    """(n, gx, gy, gz, cout, stride, dtype) of the stem weight gradient on the classic grids."""
    return [g + (co, s, dt) for g in grids() if g[2] > 1 for co in CHANNELS for s in (1, 2) for dt in (lib.F32, lib.BF16)]


class switched:
    """One process-wide tools switch at a non-default value; restored on exit."""

    def __init__(self, setter, value, default):
        self.setter, self.value, self.default = setter, value, default

    def __enter__(self):
        lib.call(self.setter, self.value)

    def __exit__(self, *exc):
        lib.call(self.setter, self.default)


def _switch_settings(switches):
    for setter, values, default in switches:
        for v in values:
            yield f"{setter}={v}", switched(setter, v, default)


def _col(fn, shapes, *tail):
    return np.array([fn(*s, *tail) for s in shapes], dtype=np.int64)


def sweep(L):
    out = {}
    fs, ws, rs, ss = fwd_shapes(), wgrad_shapes(), rows_shapes(), stem_shapes()
    out["fwd_shapes"], out["wgrad_shapes"] = np.array(fs, dtype=np.int64), np.array(ws, dtype=np.int64)
    out["rows_shapes"], out["stem_shapes"] = np.array(rs, dtype=np.int64), np.array(ss, dtype=np.int64)
    fwd_q = ("conv3d_fwd_plan", "conv3d_fwd_workspace_bytes", "conv3d_fwd_stats_rows")
    wgrad_q = ("conv3d_wgrad_plan", "conv3d_wgrad_slices", "conv3d_wgrad_workspace_bytes")
    stem_q = ("stem_wgrad_slices", "stem_wgrad_slice_floats", "stem_wgrad_workspace_bytes")
    bias_shapes = [g + (k,) for g in grids() for k in (1, 3)]

    def fwd(tag):
        for q in fwd_q:
            out[f"{q}|{tag}"] = _col(getattr(L, "nrpn_" + q), fs)

    def wgrad(tag):
        for q in wgrad_q:
            out[f"{q}|{tag}"] = _col(getattr(L, "nrpn_" + q), ws)
        for q in stem_q:
            out[f"{q}|{tag}"] = _col(getattr(L, "nrpn_" + q), ss)
        out[f"conv3d_wgrad_bias_offset|{tag}"] = _col(L.nrpn_conv3d_wgrad_bias_offset, bias_shapes)

    def rows(tag):
        out[f"conv3d_fwd_rows_workspace_bytes|{tag}"] = _col(L.nrpn_conv3d_fwd_rows_workspace_bytes, rs)

    fwd("default"), wgrad("default"), rows("default")
    for kw in OPTS:
        o = lib.ConvOpts(**kw)
        tag = "opts:" + (",".join(f"{k}={v}" for k, v in kw.items()) or "default")
        for q in fwd_q:
            out[f"{q}_ex|{tag}"] = _col(getattr(L, f"nrpn_{q}_ex"), fs, ctypes.c_void_p(o.ptr()))
    for family, switches in ((fwd, FWD_SWITCHES), (wgrad, WGRAD_SWITCHES), (rows, ROWS_SWITCHES)):
        for tag, ctx in _switch_settings(switches):
            with ctx:
                family(tag)
    return out


def columns(table, prefix):
    """{tag: column} of one query of a table."""
    return {k.split("|", 1)[1]: v for k, v in table.items() if k.split("|", 1)[0] == prefix}

