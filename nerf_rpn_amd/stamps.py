"""Decoder of the in-kernel phase stamps of the K-sliced conv launches (``include/nerfrpn_stamps.h``, ``ops.conv3d_fwd_stamped``).

Pure functions over numpy arrays: importing this module needs neither a GPU nor the shared library.  A launch's records are
``[records, words]`` 64-bit words, the conv launch's first (record r = workgroup r), then its split-K epilogue's.

Two clocks per stamp: the constant-rate device clock (``REALTIME_NS`` per tick) and the shader-cycle clock.  Everything that spans
workgroups (span, ramp, seam, skew) is taken from the constant-rate clock; cycles are only ever subtracted inside one record.
Read the table as SHARES of a launch, not as lengths: the stamped build's fences forbid overlaps the real kernel has.
"""
from collections import namedtuple

import numpy as np

VERSION = 0x4E52535400000001          # NRPN_STAMP_VERSION
WORDS = 32                            # NRPN_STAMP_WORDS
REALTIME_NS = 10                      # NRPN_STAMP_REALTIME_NS
FILL = 0xA5A5A5A5A5A5A5A5             # what callers fill the buffer with: a record that still holds it was never written
FILL_I64 = FILL - (1 << 64)           # the same bits as a torch.int64 value
KERNEL_CONV128, KERNEL_CONV256, KERNEL_EPILOGUE = 1, 2, 3
W_VERSION, W_KERNEL, W_WG, W_MTILE, W_NTILE, W_KSLICE, W_XCD, W_KSTEPS, W_PHASE0 = range(9)
W_WAIT_SUM, W_WAIT_MAX, W_KSTEP0 = 22, 23, 24
CONV_STAMPS = ("entry", "prologue_end", "first_tile", "loop_end", "stores_issued", "stores_done", "exit")
EPILOGUE_STAMPS = ("entry", "first_loads", "last_store", "stores_done", "exit")
# a phase = the stretch between two consecutive stamps, named for what runs in it
CONV_PHASES = ("prologue", "first_tile", "k_loop", "store_issue", "store_drain", "exit")
EPILOGUE_PHASES = ("first_loads", "sum_and_store", "store_drain", "exit")

Layout = namedtuple("Layout", "words plan_code conv_records epilogue_records nbytes m_tiles n_tiles k_slices k_steps slice_steps")


class StampError(ValueError):
    pass


def _words(records, layout):
    a = np.asarray(records.cpu() if hasattr(records, "cpu") else records)
    if a.dtype not in (np.int64, np.uint64):
        raise StampError(f"records must be 64-bit words, got {a.dtype}")
    a = np.ascontiguousarray(a).view(np.uint64)
    want = layout.conv_records + layout.epilogue_records
    if a.ndim != 2 or a.shape[1] != layout.words or layout.words != WORDS or a.shape[0] < want:
        raise StampError(f"records of shape {a.shape} do not fit the layout ({want} records of {layout.words} words)")
    return a[:want]


def _check(a, nstamps, what, kernels):
    unwritten = np.nonzero((a == np.uint64(FILL)).any(axis=1))[0]
    if unwritten.size:
        raise StampError(f"{what} record {int(unwritten[0])} still holds the fill pattern: its workgroup wrote nothing (or not all of it)")
    if (a[:, W_VERSION] != np.uint64(VERSION)).any():
        r = int(np.nonzero(a[:, W_VERSION] != np.uint64(VERSION))[0][0])
        raise StampError(f"{what} record {r}: version word {int(a[r, W_VERSION]):#x}, this decoder reads {VERSION:#x}")
    if not np.isin(a[:, W_KERNEL], np.array(kernels, dtype=np.uint64)).all():
        raise StampError(f"{what} records: kernel id not in {kernels}")
    rt = a[:, W_PHASE0:W_PHASE0 + 2 * nstamps:2].astype(np.int64)
    cy = a[:, W_PHASE0 + 1:W_PHASE0 + 2 * nstamps:2].astype(np.int64)
    for name, t in (("constant-rate clock", rt), ("cycle clock", cy)):
        back = np.nonzero((np.diff(t, axis=1) < 0).any(axis=1))[0]
        if back.size:
            raise StampError(f"{what} record {int(back[0])}: the {name} runs backwards in phase order")
    return rt, cy


def _pcts(v):
    p10, med, p90 = np.percentile(np.asarray(v, dtype=np.float64), [10, 50, 90])
    return {"p10": float(p10), "median": float(med), "p90": float(p90)}


def _phases(rt, cy, names):
    return {n: {"ns": _pcts((rt[:, i + 1] - rt[:, i]) * REALTIME_NS), "cycles": _pcts(cy[:, i + 1] - cy[:, i])} for i, n in enumerate(names)}


def _launch(a, rt, cy, names):
    xcd = a[:, W_XCD].astype(np.int64)
    first = {int(x): int(rt[xcd == x, 0].min()) for x in np.unique(xcd)}      # earliest entry seen on each XCD
    return {"records": int(a.shape[0]),
            "span_ns": float((rt[:, -1].max() - rt[:, 0].min()) * REALTIME_NS),
            "ramp_ns": float((rt[:, 0].max() - rt[:, 0].min()) * REALTIME_NS),
            "xcd_entry_skew_ns": float((max(first.values()) - min(first.values())) * REALTIME_NS),
            "xcds": len(first),
            "phases": _phases(rt, cy, names)}


def decode(records, layout):
    """One stamped launch -> {"plan_code", "conv": {...}, "epilogue": {...} or None, "seam_ns", "span_ns"}.

    conv / epilogue: records, span_ns (max exit - min entry), ramp_ns (max entry - min entry), xcd_entry_skew_ns (spread of the earliest
    entry of each XCD: how far apart the constant-rate clock, or the dispatcher, puts the XCDs), phases {name: {"ns" | "cycles":
    {"p10", "median", "p90"}}} over workgroups; conv also kstep_cycles_mean (K-loop cycles per K-step, mean over workgroups) and
    wait_share (cycles in the per-step wait + barrier over K-loop cycles).  seam_ns = min epilogue entry - max conv exit.
    Raises StampError on a record that still holds the fill pattern, a wrong version word or a phase that runs backwards."""
    a = _words(records, layout)
    conv, epi = a[:layout.conv_records], a[layout.conv_records:]
    rt, cy = _check(conv, len(CONV_STAMPS), "conv", (KERNEL_CONV128, KERNEL_CONV256))
    out = {"plan_code": int(layout.plan_code), "conv": _launch(conv, rt, cy, CONV_PHASES), "epilogue": None, "seam_ns": None}
    loop = cy[:, 3] - cy[:, 2]
    steps = conv[:, W_KSTEPS].astype(np.int64)
    if (steps <= 0).any():
        raise StampError("conv record without K-steps")
    out["conv"]["kstep_cycles_mean"] = float(np.mean(loop / steps))
    out["conv"]["wait_share"] = float(conv[:, W_WAIT_SUM].astype(np.int64).sum() / max(int(loop.sum()), 1))
    out["span_ns"] = out["conv"]["span_ns"]
    if layout.epilogue_records:
        ert, ecy = _check(epi, len(EPILOGUE_STAMPS), "epilogue", (KERNEL_EPILOGUE,))
        out["epilogue"] = _launch(epi, ert, ecy, EPILOGUE_PHASES)
        out["seam_ns"] = float((ert[:, 0].min() - rt[:, -1].max()) * REALTIME_NS)
        out["span_ns"] = float((ert[:, -1].max() - rt[:, 0].min()) * REALTIME_NS)
    return out
