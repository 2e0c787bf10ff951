"""Time the camera-embedding objective (ops.nerf_camopt_prepare / ops.nerf_camopt_eval, csrc/nerfrender.hip) on one synthetic
468 x 624 frame at N_samples = 256 (two passes of 128 samples per ray) and write profiles/nerf_camopt.json.  Recorded, not gated.

    python tools/nerf_camopt_profile.py --out profiles/nerf_camopt.json

Fields: HIP-event times (best of ``--repeats``) of prepare, of one evaluation with every chunk's g cached as far as the default
budget allows (half of the free device memory; ``g_bytes`` and ``cached_chunks`` say how far that was) and of one evaluation with
``cache_bytes = 0``, which re-runs the trunk and so costs what looping ops.nerf_render would; from one cached evaluation under
torch.profiler the device time of each kernel family summed over the chunks; and the cached head forward's achieved bandwidth on g
(512 bytes per sample of a cached chunk) next to the 6.0 - 6.3 TB/s the hardware guide reports as attainable.  Nothing else has been
timed on this workload: the reference's torch loop has not been run, and no speed-up over it is claimed.  Without a GPU the file is
written with those fields empty.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_extract_ref as R  # noqa: E402
from nerf_profile import kernel_times, timed, trunk_kernel  # noqa: E402
from nerf_render_profile import FRAME, N_SAMPLES  # noqa: E402

ATTAINABLE_TBPS = (6.0, 6.3)
KERNELS = ("nerfcamopt_head_kernel", "nerfcamopt_colour_kernel", "nerfcamopt_backward_kernel", "nerfcamopt_sum_rows_kernel",
           "nerfcamopt_finish_kernel", trunk_kernel("RayTile"), "Memcpy")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_camopt.json"))
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    H, W = FRAME
    rec = {"frame": list(FRAME), "n_samples": N_SAMPLES, "samples": H * W * N_SAMPLES, "chunk_rays": None, "chunks": None,
           "cached_chunks": None, "g_bytes": None, "prepare_ms": None, "eval_cached_ms": None, "eval_uncached_ms": None,
           "kernel_ms": None, "head_forward_tbps": None, "attainable_tbps": list(ATTAINABLE_TBPS), "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import ops
        from nerf_rpn_amd.scripts.nerf_render import precompute_quadratic_samples
        cfg = R.DEFAULT_CFG
        weights = ops.nerf_grid_pack(R.make_state(1, "a"), cfg)
        pose = R.make_poses(3, 1)[0]
        kw = dict(H=H, W=W, intrinsic=(580.0, 585.0, 311.5, 233.5), c2w=pose[:3, :4], near=0.1, far=5.0, bb_center=(0.05, -0.02, 0.1),
                  bb_scale=0.15, z_samples=precompute_quadratic_samples(0.1, 5.0, N_SAMPLES // 2))
        target = torch.rand(H * W, 3, generator=torch.Generator().manual_seed(0))
        cam = torch.tensor([0.3, -0.2, 0.1, 0.4])
        held = {}

        def prepare(budget):
            held.clear()                  # one state's cache at a time
            held["state"] = ops.nerf_camopt_prepare(weights, cfg, target, cache_bytes=budget, **kw)
        t_prepare = timed(lambda: prepare(None), args.repeats)
        st = held["state"]
        t_cached = timed(lambda: ops.nerf_camopt_eval(st, cam), args.repeats)
        rec.update(chunk_rays=st.chunk, chunks=st.chunks, cached_chunks=st.cached_chunks, g_bytes=st.g_bytes,
                   prepare_ms=round(t_prepare, 2), eval_cached_ms=round(t_cached, 2), device=torch.cuda.get_device_name(0))
        try:
            km = kernel_times(lambda: ops.nerf_camopt_eval(st, cam), KERNELS)
        except Exception as e:      # the profiler is optional: the event times stand without it
            km, rec["note"] = None, f"torch.profiler failed: {type(e).__name__}"
        if km:
            rec["kernel_ms"] = {k: round(v, 3) for k, v in km.items()}
            if st.cached_chunks == st.chunks:      # every head launch read its g from the cache
                rec["head_forward_tbps"] = round(H * W * N_SAMPLES * 512 / (km["nerfcamopt_head_kernel"] * 1e-3) / 1e12, 3)
        prepare(0)
        rec["eval_uncached_ms"] = round(timed(lambda: ops.nerf_camopt_eval(held["state"], cam), args.repeats), 2)
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
