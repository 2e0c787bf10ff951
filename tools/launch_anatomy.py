"""Where the small forward launches spend their time: in-kernel phase stamps (nerf_rpn_amd/stamps.py, include/nerfrpn_stamps.h) of the conv
launches of the 5^3 / 10^3 / 20^3 pyramid levels, bf16, n = 1.

Per shape: warm up, LAUNCHES stamped launches on seeded random operands (not zeros: zero MFMA operands raise the clock), decode each, and
report the median over launches of the decoder's per-launch figures.  Beside every table stands what stamping costs: the HIP-event time of
conv + epilogue for the stamped and the unstamped call, alternated in windows of WINDOW launches.

Shares, not lengths: the stamped build's fences forbid overlaps the real kernel has.  Cycles are compared inside one record only;
whether the constant-rate clock is common to the eight XCDs is not known, so the cross-XCD entry skew is reported and no cross-workgroup
conclusion is drawn in cycles.

    python tools/launch_anatomy.py [--out profiles/launch_anatomy.json] [--launches 20] [--window 200] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nerf_rpn_amd import lib, ops, stamps  # noqa: E402

SENTENCE = "shares, not lengths: the stamped build's fences forbid overlaps the real kernel has"
# (grid, cin, cout, ksize): the shapes VERDICT.md names
SHAPES = [(5, 512, 256, 1), (10, 512, 256, 1), (20, 256, 256, 1), (5, 512, 512, 3), (10, 512, 512, 3), (10, 256, 256, 3), (20, 256, 256, 3),
          (20, 512, 512, 3)]
BF = torch.bfloat16


def _median_tree(trees):
    """Median, leaf by leaf, over a list of equally shaped nested dicts of numbers (None stays None)."""
    t0 = trees[0]
    if isinstance(t0, dict):
        return {k: _median_tree([t[k] for t in trees]) for k in t0}
    if t0 is None:
        return None
    return statistics.median(trees)


def _event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def measure(g, cin, cout, k, dev, launches, window, rounds):
    gen = torch.Generator().manual_seed(g * 1000 + cin + cout + k)
    x = torch.randn((1, g, g, g, cin), generator=gen).to(BF).to(dev)
    w = (torch.randn((cout, cin, k, k, k), generator=gen) * (cin * k ** 3) ** -0.5).to(dev)
    bias = torch.randn((cout,), generator=gen).to(dev)
    wp, _ = ops.PackedWeight().get([w], BF, cout, False)
    opts = lib.ConvOpts()
    q = (1, g, g, g, cin, cout, k, lib.BF16)
    lay = ops.conv3d_stamp_layout(*q, opts)
    assert lay.plan_code == lib.query("conv3d_fwd_plan", *q)
    wsb = lib.query("conv3d_fwd_workspace_bytes", *q)
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    y = torch.empty((1, g, g, g, cout), dtype=BF, device=dev)
    rec = torch.empty((lay.conv_records + lay.epilogue_records, lay.words), dtype=torch.int64, device=dev)
    flags = lib.CONV_BIAS | lib.CONV_RELU
    args = (ops._p(x), ops._p(wp), ops._p(bias), ops._p(y), 1, g, g, g, cin, cout, cout, k, lib.BF16, flags, ops._p(ws) if wsb else 0, opts.ptr(), ops._s())

    def plain():
        lib.call("conv3d_fwd_ex", *args)

    def stamped():
        lib.call("conv3d_fwd_stamped", *args, ops._p(rec), rec.numel() * 8)

    for _ in range(20):
        plain()
        stamped()
    torch.cuda.synchronize()
    per_launch = []
    for _ in range(launches):
        rec.fill_(stamps.FILL_I64)
        stamped()
        torch.cuda.synchronize()
        per_launch.append(stamps.decode(rec, lay))
    t_plain, t_stamped = [], []
    for _ in range(rounds):                  # alternating windows, one process
        t_plain.append(_event_us(plain, window))
        t_stamped.append(_event_us(stamped, window))
    tp, ts = statistics.median(t_plain), statistics.median(t_stamped)
    return {"shape": f"{g}^3 {cin}->{cout} k{k}", "plan_code": lay.plan_code, "conv_workgroups": lay.conv_records,
            "epilogue_workgroups": lay.epilogue_records, "k_slices": lay.k_slices, "k_steps_per_slice": list(lay.slice_steps),
            "launches": launches, "median_over_launches": _median_tree(per_launch),
            "event_us": {"unstamped": tp, "stamped": ts, "stamping_cost_pct": 100.0 * (ts - tp) / tp, "window": window, "rounds": rounds}}


def _row(r):
    m = r["median_over_launches"]
    c = m["conv"]
    ph = " ".join(f"{n} {c['phases'][n]['ns']['median']:.0f}" for n in stamps.CONV_PHASES)
    line = (f"{r['shape']:<18} plan {r['plan_code']} wgs {r['conv_workgroups']:>4}+{r['epilogue_workgroups']:<4} | conv span {c['span_ns']:.0f} ns ramp "
            f"{c['ramp_ns']:.0f} xcd-skew {c['xcd_entry_skew_ns']:.0f} | median ns/wg: {ph} | k-step {c['kstep_cycles_mean']:.0f} cyc, wait {100 * c['wait_share']:.0f} %")
    if m["epilogue"]:
        e = m["epilogue"]
        line += f" | seam {m['seam_ns']:.0f} ns, epilogue span {e['span_ns']:.0f} ns"
    ev = r["event_us"]
    return line + f" | events: {ev['unstamped']:.1f} us plain, {ev['stamped']:.1f} us stamped ({ev['stamping_cost_pct']:+.0f} %)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "launch_anatomy.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--window", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert a.launches >= 20 and a.window >= 200, "at least 20 stamped launches per shape and windows of at least 200 launches"
    lib.call("check_device", 0)
    dev = torch.device("cuda:0")
    rows = []
    for g, cin, cout, k in SHAPES:
        rows.append(measure(g, cin, cout, k, dev, a.launches, a.window, a.rounds))
        print(_row(rows[-1]), flush=True)
    doc = {"device": torch.cuda.get_device_name(0), "note": SENTENCE,
           "clocks": {"ns": f"constant-rate device clock (s_memrealtime), {stamps.REALTIME_NS} ns per tick", "cycles": "shader clock (s_memtime)"},
           "method": f"median over {a.launches} stamped launches of the per-launch figures of nerf_rpn_amd.stamps.decode (percentiles over workgroups); "
                     f"events: {a.rounds} alternating windows of {a.window} launches, seeded random bf16 operands, bias + ReLU",
           "cross_xcd": "xcd_entry_skew_ns is the spread of the earliest entry seen on each XCD; it mixes dispatch order with any offset between the "
                        "XCDs' clocks, so nothing here compares cycles across workgroups",
           "stamp_phases": {"conv": list(stamps.CONV_PHASES), "epilogue": list(stamps.EPILOGUE_PHASES)},
           "shapes": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", os.path.normpath(a.out))


if __name__ == "__main__":
    main()
