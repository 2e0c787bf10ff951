"""Writes the host part of tests/golden/nerf_split_bounds.json: the deviations of the bf16x3 emulation (tests/nerf_split_ref.py), of
its variants and of the float32 checker from the float64 checker, per case, and what the bias nudging of the gradient cases did.  The
file is a record: the tests compute their bounds from the emulation at run time.  The "gpu" section holds what a run of
tests/test_gpu_nerf_split.py on an MI355X printed (error / bound per tensor) and is kept when this script rewrites the rest.

Run from the repository root: ``python tests/golden/make_nerf_split_golden.py``."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import nerf_query_ref as Q  # noqa: E402
import nerf_split_ref as S  # noqa: E402


def main():
    torch.set_num_threads(1)
    path = os.path.join(HERE, "nerf_split_bounds.json")
    old = json.load(open(path)) if os.path.exists(path) else {}
    out = {"factor": S.FACTOR, "margin": S.MARGIN, "cases": {}, "gradient_cases": {}, "gpu": old.get("gpu", {})}
    for case in S.CASES:
        c = S.case_inputs(case)
        o64 = Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, dtype=torch.float64)["raw"]
        o32 = Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, dtype=torch.float32)["raw"]
        raws = {m: S.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, mode=m)["raw"] for m in S.MODES}
        out["cases"][case["name"]] = {"points": case["R"] * case["S"], "raw": {
            "top": float(o64.abs().max()), "fp32": S.deviation(o32, o64), "emulation": S.deviation(raws["split"], o64),
            "bound": S.bound_of(raws["split"], o64), **{m: S.deviation(raws[m], o64) for m in S.MODES if m != "split"}}}
    for name in S.GRAD_NAMES:
        c = S.case_inputs(S.CASES[S.NAMES.index(name)], nudged=True)
        e, o64, o32 = (S.tensors_of(f()) for f in (lambda: S.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot),
                                                   lambda: Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot, torch.float64),
                                                   lambda: Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot, torch.float32)))
        out["gradient_cases"][name] = {"nudge": c.nudge, "tensors": {
            k: {"top": float(o64[k].abs().max()), "fp32": S.deviation(o32[k], o64[k]), "emulation": S.deviation(e[k], o64[k]),
                "bound": S.bound_of(e[k], o64[k])} for k in Q.tensor_names(c.cfg)}}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
