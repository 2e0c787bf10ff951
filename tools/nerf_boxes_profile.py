"""Time the NeRF render restricted to 3D boxes against the plain render of the same tree in the same process, and
write profiles/nerf_boxes.json.  Recorded, not gated -- but for one condition: in (c), skip=True must beat skip=False by more than the
spread of the repeats, or the skip path has no reason to exist.

    python tools/nerf_boxes_profile.py --out profiles/nerf_boxes.json

One 468 x 624 frame at 128 + 128 samples with random weights (the skipped share depends on geometry only), per arithmetic (fp32,
bf16x3), HIP-event times of ``--repeats`` calls after a warm-up call (all of them are kept; ``best`` is their minimum):
  a  ops.nerf_render, the yardstick;
  b  ops.nerf_render_boxes with a box that holds every sample, skip=True: b - a is what the mask passes cost;
  c  keep with one box on the optical axis, sized (by bisection on its width, from the device's own tile counts) so that about a
     tenth of the tiles run, with skip=True and with skip=False;
  d  remove with the same box.
Per configuration also tiles_run / tiles_total per pass and, from torch.profiler, the device time and the launches of every kernel of
the call (launches per chunk = launches / chunks).  Without a GPU the file is written with those fields empty.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_render_ref as V  # noqa: E402
from nerf_profile import window_times  # noqa: E402

H, W, S, NEAR, FAR, SHARE = 468, 624, 128, 0.1, 4.0, 0.1
MODES = ("fp32", "bf16x3")


def kernels_of(fn):
    """name -> {ms, launches} of every device kernel of one call of fn, from torch.profiler; None if it records none."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0))
        if t > 0 and ("nerfrender" in e.key or "trunk" in e.key):
            out[e.key.replace("(anonymous namespace)::", "")] = {"ms": round(t / 1e3, 4), "launches": int(e.count)}
    return out or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_boxes.json"))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    rec = {"image_hw": [H, W], "samples": [S, S], "target_share": SHARE, "device": None, "chunk": None, "chunks": None, "box": None,
           "configs": None, "summary": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import ops
        dev = torch.device("cuda")
        rec["device"] = torch.cuda.get_device_name(0)
        cfg = {"multires_views": 0, "input_ch_cam": 4}
        state = {k: v.to(dev) for k, v in V.make_state(1, dict(V.R.DEFAULT_CFG, **cfg), V.SIGMA_SCALE).items()}
        intrinsic = torch.tensor([580., 580., W / 2., H / 2.])
        c2w = V.R.make_poses(1, 1)[0]
        z = V.precompute_quadratic_samples(NEAR, FAR, S)
        frame = dict(H=H, W=W, intrinsic=intrinsic, c2w=c2w[:3, :4], near=NEAR, far=FAR, bb_center=torch.zeros(3), bb_scale=0.25, z_samples=z)
        rec["chunk"], rec["chunks"] = ops.NERF_RENDER_DEFAULT_CHUNK, -(-H * W // ops.NERF_RENDER_DEFAULT_CHUNK)
        o = c2w[:3, 3].double().numpy()
        axis = -c2w[:3, 2].double().numpy()                   # the ray of the principal point
        everything = np.concatenate([o, [40.0, 40.0, 40.0], [0.0]])[None]

        def box(width):
            return np.concatenate([o + 2.6 * axis, [width, width, 0.8 * width], [0.5]])[None]

        def share(out):
            return float(out["tiles_run"].sum()) / float(out["tiles_total"].sum())

        rec["configs"], rec["summary"] = {}, {}
        for m in MODES:
            weights = ops.nerf_grid_pack(state, cfg, dtype=m)
            if rec["box"] is None:              # geometry only: found once
                lo, hi = 0.05, 4.0
                for _ in range(10):
                    mid = 0.5 * (lo + hi)
                    lo, hi = (mid, hi) if share(ops.nerf_render_boxes(weights, cfg, box(mid), "keep", **frame)) < SHARE else (lo, mid)
                rec["box"] = box(0.5 * (lo + hi))[0].tolist()
            one = np.array([rec["box"]])
            calls = {"a_plain": lambda: ops.nerf_render(weights, cfg, **frame),
                     "b_all_skip": lambda: ops.nerf_render_boxes(weights, cfg, everything, "keep", **frame),
                     "c_keep_skip": lambda: ops.nerf_render_boxes(weights, cfg, one, "keep", **frame),
                     "c_keep_noskip": lambda: ops.nerf_render_boxes(weights, cfg, one, "keep", skip=False, **frame),
                     "d_remove_skip": lambda: ops.nerf_render_boxes(weights, cfg, one, "remove", **frame),
                     "d_remove_noskip": lambda: ops.nerf_render_boxes(weights, cfg, one, "remove", skip=False, **frame)}
            res = {}
            for name, fn in calls.items():
                ms = window_times(fn, args.repeats)
                out = fn()
                r = {"ms": [round(x, 4) for x in ms], "best": round(min(ms), 4), "spread": round(max(ms) - min(ms), 4)}
                if "tiles_run" in out:
                    r["tiles_run"], r["tiles_total"] = out["tiles_run"].tolist(), out["tiles_total"].tolist()
                    r["share"] = round(share(out), 4)
                try:
                    r["kernels"] = kernels_of(fn)
                except Exception as e:      # the profiler is optional: the event times stand without it
                    r["kernels"], rec["note"] = None, f"torch.profiler failed: {type(e).__name__}"
                res[name] = r
            rec["configs"][m] = res
            a, b, cs, cn = (res[k]["best"] for k in ("a_plain", "b_all_skip", "c_keep_skip", "c_keep_noskip"))
            spread = max(res["c_keep_skip"]["spread"], res["c_keep_noskip"]["spread"])
            rec["summary"][m] = {"mask_passes_ms": round(b - a, 4), "keep_skip_over_plain": round(cs / a, 4),
                                 "skip_gain_ms": round(cn - cs, 4), "spread_ms": spread, "skip_beats_noskip": bool(cn - cs > spread)}
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
