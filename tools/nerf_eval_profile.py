"""Time the NeRF test-view metrics (ops.nerf_view_metrics, csrc/nerfmetrics.hip) on one synthetic 468 x 624 frame and write
profiles/nerf_eval.json; optionally record the errors the MI355X gives against the checker.  Recorded, not gated.

    python tools/nerf_eval_profile.py --out profiles/nerf_eval.json [--errors-out FILE]

Fields: the host-visible time of one ops.nerf_view_metrics call with return_images (metrics, reduction, both quantisers, the copy of the
eight sums and the host arithmetic; it ends in a device synchronise) -- median and best of ``--repeats`` calls after a warm-up --, the
same with the 8- and 16-bit images copied to the host as nerf_test does, the device time per kernel from one run under
torch.profiler, the render time of the same frame size as profiles/nerf_render.json recorded it, and the bytes that cross to the host
per frame next to what the float32 rgb and depth maps would be.  Nothing else has been timed on this workload: there is no
comparison in this file.  Without a GPU the file is written with the timing fields empty.

--errors-out writes what tests/golden/make_nerf_eval_golden.py --gpu-errors merges into nerf_eval_bounds.json: per synthetic size the
largest error against the float64 checker next to the derived bound, and per golden case the largest error of render + metrics against
the reference's recorded values.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_eval_ref as E  # noqa: E402
from nerf_profile import kernel_times  # noqa: E402

FRAME = (468, 624)
KERNELS = ("nerfmetrics_tile_kernel", "nerfmetrics_reduce_kernel", "nerfmetrics_to8b_kernel", "nerfmetrics_to16b_kernel")


def wall_ms(fn, repeats, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def measured_errors(ops, lib):
    T = lib.query("nerfmetrics_tile")
    out = {"tile": T, "fp64": {}, "cases": {}}
    for H, W in ((7, 7), (7, 40), (13, 9), (T + 6, T + 6), (T + 7, 2 * T + 5), (96, 130)):
        n, windows, rec = H * W * 3, (H - 6) * (W - 6), {}
        for noise in E.NOISES:
            f = E.synth_frame(H, W, noise)
            ref = E.frame_ref(f, torch.float64, form="windows")
            got = ops.nerf_view_metrics(f.rgb, f.target, f.depth, f.target_depth, f.valid)
            for k, bound in (("img_loss", 2. * E.mse_rel_bound(n) * ref["img_loss"]), ("ssim", 2. * E.ssim_bound(windows)),
                             ("depth_rmse", 2. * E.mse_rel_bound(ref["n_valid"]) * ref["depth_rmse"])):
                r = rec.setdefault(k, {"error": 0.0, "bound": 0.0})
                r["error"], r["bound"] = max(r["error"], abs(got[k] - ref[k])), max(r["bound"], bound)
        out["fp64"][f"{H}x{W}"] = rec
    golden = dict(np.load(os.path.join(E.GOLDEN, "nerf_eval.npz"), allow_pickle=False))
    for case in E.CASES:
        c = E.case_inputs(case)
        images, depths, valid = E.load_targets(c, golden[f"{c.name}/target_rgb8"], golden[f"{c.name}/target_depth16"])
        weights, rec = ops.nerf_grid_pack(c.state, c.cfg), {}
        for i in range(c.frames):
            r = ops.nerf_render(weights, c.cfg, H=c.H, W=c.W, intrinsic=c.intrinsic, c2w=c.poses[i][:3, :4], near=c.near, far=c.far,
                                bb_center=c.bb_center, bb_scale=c.bb_scale, z_samples=c.z_samples, n_samples=c.n_samples)
            got = ops.nerf_view_metrics(r["rgb_map"], images[i], r["depth_map"], depths[i], valid[i])
            for k, want in zip(E.METRICS, golden[f"{c.name}/frame_metrics"][i]):
                if not np.isnan(want):
                    rec[k] = max(rec.get(k, 0.0), abs(got[k] - float(want)))
        out["cases"][c.name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_eval.json"))
    ap.add_argument("--errors-out", default=None)
    ap.add_argument("--repeats", type=int, default=200)
    args = ap.parse_args()
    H, W = FRAME
    render_ms = None
    try:
        with open(os.path.join(ROOT, "profiles", "nerf_render.json")) as f:
            prev = json.load(f)
        if prev.get("frame") == list(FRAME):
            render_ms = prev.get("two_pass_frame_ms")
    except OSError:
        pass
    crossing = 8 * 8 + H * W * 3 + H * W * 2
    rec = {"frame": list(FRAME), "repeats": args.repeats, "metrics_call_ms_median": None, "metrics_call_ms_best": None,
           "metrics_call_with_image_copies_ms_median": None, "metrics_call_with_image_copies_ms_best": None, "kernel_ms": None,
           "render_frame_ms_from_nerf_render_profile": render_ms, "metrics_share_of_render": None,
           "bytes_to_host_per_frame": crossing, "bytes_of_float32_rgb_and_depth_maps": H * W * 4 * 4,
           "bytes_read_by_the_metrics_kernel": H * W * (3 + 3 + 1 + 1) * 4 + H * W, "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import lib, ops
        f = E.synth_frame(H, W, 0.05)
        dev = torch.device("cuda", torch.cuda.current_device())
        g = {k: getattr(f, k).to(dev) for k in ("rgb", "target", "depth", "target_depth", "valid")}

        def call():
            return ops.nerf_view_metrics(g["rgb"], g["target"], g["depth"], g["target_depth"], g["valid"], far=f.far, return_images=True)

        def call_and_copy():
            m = call()
            return m["rgb8"].cpu(), m["depth16"].cpu()
        med, best = wall_ms(call, args.repeats)
        med_c, best_c = wall_ms(call_and_copy, args.repeats)
        rec.update(metrics_call_ms_median=round(med, 4), metrics_call_ms_best=round(best, 4),
                   metrics_call_with_image_copies_ms_median=round(med_c, 4), metrics_call_with_image_copies_ms_best=round(best_c, 4),
                   device=torch.cuda.get_device_name(0))
        if render_ms:
            rec["metrics_share_of_render"] = round(med_c / render_ms, 5)
        try:
            km = kernel_times(call, KERNELS)
        except Exception as e:      # the profiler is optional: the times above stand without it
            km, rec["note"] = None, f"torch.profiler failed: {type(e).__name__}"
        if km:
            rec["kernel_ms"] = {k: round(v, 4) for k, v in km.items()}
        if args.errors_out:
            os.makedirs(os.path.dirname(os.path.abspath(args.errors_out)), exist_ok=True)
            with open(args.errors_out, "w") as fo:
                json.dump(measured_errors(ops, lib), fo, indent=1)
                fo.write("\n")
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(rec, fo, indent=1)
        fo.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
