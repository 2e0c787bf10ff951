"""A/B of the cone head's row loss (ops.CONE_ROWS_LOSS) against a checkout of the parent commit -> profiles/cone_rows_loss_ab.json.

    python tools/cone_rows_loss_ab.py --parent DIR --parent-hash HASH [--runs 5] [--out profiles/cone_rows_loss_ab.json]
                                      [--previous EARLIER.json ...] [--trace-only]

DIR is a built checkout of the parent commit (its own libnerfrpn_hip.so).  Every measurement is a fresh child process started in the tree it
measures, under its own time limit; the first child that does not exit cleanly ends the whole run.
  1. `bench.py --gpus 1 --steps 100 --warmup 10`, the two trees alternating, --runs times each: medians, max - min spreads and the verdict
     (a gain only if the new median lies below the parent's by more than the larger spread).
  2. one `--full` run of each tree (no CPU baseline, probe or extras): host.enqueue_ms_per_step and host.c_abi_calls_per_step.
  3. `--dump-outputs` of both trees with the same arguments: the loss, every loss term and params must be the same bytes.
  4. `rocprofv3 --kernel-trace --stats` of `bench.py --steps 10 --warmup 3` for each tree, in a run of its own: launches and microseconds per
     step of the kernels the change removes and adds."""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATCHED = ("head_flatten_kernel<float, true>", "head_flatten_kernel<unsigned short, false>", "MulFunctor<float>", "FillFunctor<float>",
           "FillFunctor<c10::BFloat16>", "fillBufferAligned", "sampled_loss_kernel", "sampled_loss_rows_kernel", "head_grad_rows_kernel")
PROFILE_STEPS = 13      # --steps 10 --warmup 3


def child(tree, argv, limit, prefix=()):
    """Run bench.py of ``tree`` in a fresh process; returns its JSON line.  Anything but a clean exit stops the tool."""
    cmd = [*prefix, sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", *argv]
    try:
        p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f"time limit ({limit} s) reached: {' '.join(cmd)}")
    if p.returncode != 0:
        raise SystemExit(f"rc {p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def median(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def kernel_table(tree, tmp, tag, keep_dir):
    d = os.path.join(tmp, "prof_" + tag)
    child(tree, ["--steps", "10", "--warmup", "3"], 300, ("rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "p", "--output-format", "csv", "--"))
    found = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith("kernel_stats.csv")]
    shutil.copyfile(found[0], os.path.join(keep_dir, f"cone_rows_loss_{tag}_kernel_stats.csv"))      # the whole table, next to the JSON
    rows, total_ns, launches = {}, 0, 0
    with open(found[0]) as fh:
        for row in csv.DictReader(fh):
            total_ns += int(row["TotalDurationNs"])
            launches += int(row["Calls"])
            for w in WATCHED:
                if w in row["Name"]:
                    e = rows.setdefault(w, {"launches_per_step": 0.0, "us_per_step": 0.0})
                    e["launches_per_step"] = round(e["launches_per_step"] + int(row["Calls"]) / PROFILE_STEPS, 2)
                    e["us_per_step"] = round(e["us_per_step"] + int(row["TotalDurationNs"]) / PROFILE_STEPS / 1e3, 2)
    return {"kernels": rows, "all_kernels_ms_per_step": round(total_ns / PROFILE_STEPS / 1e6, 3), "all_launches_per_step": round(launches / PROFILE_STEPS, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--parent-hash", required=True)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "cone_rows_loss_ab.json"))
    ap.add_argument("--trace-only", action="store_true", help="keep the figures of the file at --out and take the two kernel traces (step 4) again")
    ap.add_argument("--previous", nargs="*", default=[], help="output files of earlier runs of this tool: their timing sets are copied into the new file")
    args = ap.parse_args()
    trees = {"parent": os.path.abspath(args.parent), "new": HERE}
    if args.trace_only:
        res = json.load(open(args.out))
        with tempfile.TemporaryDirectory() as tmp:
            for tag in ("parent", "new"):
                res["kernel_trace_per_step"][tag] = kernel_table(trees[tag], tmp, tag, os.path.dirname(os.path.abspath(args.out)))
                print(f"kernels {tag}: {json.dumps(res['kernel_trace_per_step'][tag])}", flush=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
        return
    res = {"what": "bench.py --gpus 1 --steps 100 --warmup 10, one MI355X, the parent commit and this tree alternating (tools/cone_rows_loss_ab.py)",
           "parent_commit": args.parent_hash, "runs_each": args.runs, "ms_per_step": {"parent": [], "new": []}}
    if args.previous:      # earlier sets (other boxes, other days) stay on record next to this one, verdict and all
        keys = ("ms_per_step", "median_ms_per_step", "spread_ms", "median_gain_ms", "counts_as_gain", "host")
        res["previous_sets"] = [{"file": os.path.basename(f), **{k: v for k, v in json.load(open(f)).items() if k in keys}} for f in args.previous]

    def save():      # after every phase: a later child that fails leaves the earlier figures on disk
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    for i in range(args.runs):
        for tag in ("parent", "new"):
            ms = child(trees[tag], ["--steps", "100", "--warmup", "10"], 240)["ms_per_step"]
            res["ms_per_step"][tag].append(ms)
            print(f"run {i} {tag}: {ms} ms/step", flush=True)
    med = {t: median(v) for t, v in res["ms_per_step"].items()}
    spread = {t: round(max(v) - min(v), 3) for t, v in res["ms_per_step"].items()}
    gain = med["parent"] - med["new"]
    res["median_ms_per_step"], res["spread_ms"] = med, spread
    res["median_gain_ms"] = round(gain, 3)
    res["counts_as_gain"] = bool(gain > max(spread.values()))
    res["rule"] = "a gain only if the new median lies below the parent's median by more than the larger of the two max - min spreads"
    print(json.dumps({k: res[k] for k in ("median_ms_per_step", "spread_ms", "median_gain_ms", "counts_as_gain")}), flush=True)
    save()
    res["host"] = {}
    for tag in ("parent", "new"):
        h = child(trees[tag], ["--full", "--no-cpu-baseline", "--no-probe", "--no-extras", "--steps", "100", "--warmup", "10"], 300)["host"]
        res["host"][tag] = {k: h[k] for k in ("enqueue_ms_per_step", "c_abi_calls_per_step")}
        print(f"host {tag}: {res['host'][tag]}", flush=True)
    save()
    with tempfile.TemporaryDirectory() as tmp:
        for tag in ("parent", "new"):
            child(trees[tag], ["--steps", "10", "--warmup", "3", "--dump-outputs", os.path.join(tmp, "dump_" + tag)], 240)
        names = sorted(os.listdir(os.path.join(tmp, "dump_parent")))
        same = {}
        for n in names:
            a, b = (open(os.path.join(tmp, "dump_" + t, n), "rb").read() for t in ("parent", "new"))
            same[n[:-4]] = a == b
        res["dump_outputs_identical"] = same
        print(f"dump-outputs identical: {same}", flush=True)
        save()
        res["kernel_trace_per_step"] = {"what": f"rocprofv3 --kernel-trace --stats of bench.py --steps 10 --warmup 3, totals / {PROFILE_STEPS} steps"}
        for tag in ("parent", "new"):
            res["kernel_trace_per_step"][tag] = kernel_table(trees[tag], tmp, tag, os.path.dirname(os.path.abspath(args.out)))
            print(f"kernels {tag}: {json.dumps(res['kernel_trace_per_step'][tag])}", flush=True)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
