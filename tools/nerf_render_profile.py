"""Time the NeRF view rendering (ops.nerf_render, csrc/nerfrender.hip) on one synthetic 468 x 624 frame at N_samples = 256 (two passes of
128 samples per ray) and write profiles/nerf_render.json.  Recorded, not gated.

    python tools/nerf_render_profile.py --out profiles/nerf_render.json

Fields: HIP-event time of ops.nerf_render on weights packed beforehand (best of ``--repeats``), the same for the plain path at 256
samples, and -- from one run under torch.profiler -- the device time of each kernel family summed over the chunks, from which the
trunk's share of the kernel time and its achieved fp32 rate against the 157 TFLOP/s matrix peak follow.  Nothing else has been timed
on this workload: there is no comparison in this file.  Without a GPU the file is written with those fields empty.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_extract_ref as R  # noqa: E402
from nerf_profile import kernel_times, timed, trunk_kernel  # noqa: E402

FRAME = (468, 624)
N_SAMPLES = 256
PEAK_TFLOPS = 157.0
TRUNK_FLOP_PER_POINT = 2 * (57 * 256 + 4 * 256 * 256 + 313 * 256 + 2 * 256 * 256 + 256 * 256 + 256 + 256 * 128)
TRUNK = trunk_kernel("RayTile")
KERNELS = (TRUNK, "nerfrender_head_kernel", "nerfrender_sample_kernel", "nerfrender_composite_kernel",
           "nerfrender_rays_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_render.json"))
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    H, W = FRAME
    points = H * W * N_SAMPLES
    rec = {"frame": list(FRAME), "n_samples": N_SAMPLES, "mlp_queries": points, "trunk_flop_per_point": TRUNK_FLOP_PER_POINT,
           "matrix_peak_tflops_fp32": PEAK_TFLOPS, "chunk_rays": None, "two_pass_frame_ms": None, "plain_frame_ms": None,
           "kernel_ms": None, "trunk_share_of_kernel_time": None, "trunk_tflops": None, "trunk_fraction_of_peak": None, "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import ops
        from nerf_rpn_amd.scripts.nerf_render import precompute_quadratic_samples
        state = R.make_state(1, "a")
        weights = ops.nerf_grid_pack(state, R.DEFAULT_CFG)
        pose = R.make_poses(3, 1)[0]
        kw = dict(H=H, W=W, intrinsic=(580.0, 585.0, 311.5, 233.5), c2w=pose[:3, :4], near=0.1, far=5.0, bb_center=(0.05, -0.02, 0.1),
                  bb_scale=0.15)
        z = precompute_quadratic_samples(0.1, 5.0, N_SAMPLES // 2)
        t_two = timed(lambda: ops.nerf_render(weights, R.DEFAULT_CFG, z_samples=z, **kw), args.repeats)
        t_plain = timed(lambda: ops.nerf_render(weights, R.DEFAULT_CFG, n_samples=N_SAMPLES, **kw), args.repeats)
        rec.update(chunk_rays=ops.NERF_RENDER_DEFAULT_CHUNK, two_pass_frame_ms=round(t_two, 2), plain_frame_ms=round(t_plain, 2),
                   device=torch.cuda.get_device_name(0))
        try:
            km = kernel_times(lambda: ops.nerf_render(weights, R.DEFAULT_CFG, z_samples=z, **kw), KERNELS)
        except Exception as e:      # the profiler is optional: the event times above stand without it
            km, rec["note"] = None, f"torch.profiler failed: {type(e).__name__}"
        if km:
            trunk = km[TRUNK]
            tf = points * TRUNK_FLOP_PER_POINT / (trunk * 1e-3) / 1e12
            rec.update(kernel_ms={k: round(v, 3) for k, v in km.items()}, trunk_share_of_kernel_time=round(trunk / sum(km.values()), 4),
                       trunk_tflops=round(tf, 2), trunk_fraction_of_peak=round(tf / PEAK_TFLOPS, 3))
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
