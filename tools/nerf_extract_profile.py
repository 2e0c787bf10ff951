"""Time the NeRF grid extraction (ops.nerf_grid_query, csrc/nerfgrid.hip) on one synthetic 256 x 208 x 96 grid at P = 100 poses and write
profiles/nerf_extract.json.  Recorded, not gated.

    python tools/nerf_extract_profile.py --out profiles/nerf_extract.json

Fields: HIP-event time of ops.nerf_grid_query on weights packed beforehand (ops.nerf_grid_pack, timed on its own as ``pack_ms``) at
P = 100 and at P = 1.  The query time is the trunk and head launches of every chunk plus what surrounds them in the op: the P x 128
view table (a few small torch kernels), the upload of the three axis arrays and two allocations -- tens of microseconds against tens
of milliseconds.  The P = 1 run is the trunk plus one head pass, so the trunk's achieved fp32 rate is reported from it as a lower
bound, against the 157 TFLOP/s matrix peak.  On the same GPU, the reference's formulation: every pose through the whole MLP as torch
fp32 matmuls in chunks of 2^18 rows, timed on ``--reference-poses`` poses and scaled to P.  Without a GPU the file is written with those fields empty.
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
from nerf_profile import timed  # noqa: E402

RES = (256, 208, 96)
POSES = 100
PEAK_TFLOPS = 157.0
TRUNK_FLOP_PER_POINT = 2 * (57 * 256 + 4 * 256 * 256 + 313 * 256 + 2 * 256 * 256 + 256 * 256 + 256 + 256 * 128)
HEAD_FLOP_PER_POINT_POSE = 2 * 128 + 2 * 3 * 128


@torch.no_grad()
def reference_formulation(state, xs, ys, zs, center, scale, poses, dev, rows=1024 * 64 * 4):
    """The reference's formulation on the device: every pose through the whole network, ``rows`` input rows at a time."""
    model = R.build_model(state).to(dev)
    embed_pts, _ = R.get_embedder(9)
    embed_dirs, _ = R.get_embedder(0)
    points = R.grid_points(xs, ys, zs).to(dev)
    look = torch.tensor([0., 0., -1.], device=dev)
    total = torch.zeros((points.shape[0], 3), device=dev)
    for pose in poses:
        x = R.network_input(points, embed_pts, embed_dirs, pose[:3, :3] @ look, 4, center, scale)
        out = torch.cat([model(x[r:r + rows]) for r in range(0, x.shape[0], rows)])
        total += torch.sigmoid(out[:, :3])
    return total / len(poses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_extract.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reference-poses", type=int, default=2)
    args = ap.parse_args()
    n = RES[0] * RES[1] * RES[2]
    rec = {"resolution": list(RES), "points": n, "poses": POSES, "trunk_flop_per_point": TRUNK_FLOP_PER_POINT,
           "head_flop_per_point_per_pose": HEAD_FLOP_PER_POINT_POSE, "matrix_peak_tflops_fp32": PEAK_TFLOPS,
           "pack_ms": None, "query_ms_at_100_poses": None, "query_ms_at_1_pose": None, "trunk_tflops_lower_bound": None, "trunk_fraction_of_peak": None,
           "head_ms_per_pose": None, "reference_formulation_ms_at_100_poses": None, "reference_poses_timed": None,
           "speedup_over_reference_formulation": None, "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import ops
        dev = torch.device("cuda:0")
        state = R.make_state(1, "a")
        xs, ys, zs = (torch.linspace(-1.0, 1.0, r) * s for r, s in zip(RES, (1.0, 0.8, 0.4)))
        center, scale = torch.tensor([0.05, -0.02, 0.1]), torch.tensor(0.8)
        poses = R.make_poses(3, POSES)

        t_pack = timed(lambda: ops.nerf_grid_pack(state, R.DEFAULT_CFG), args.repeats)
        weights = ops.nerf_grid_pack(state, R.DEFAULT_CFG)

        def run(p):
            return ops.nerf_grid_query(weights, R.DEFAULT_CFG, xs, ys, zs, center, scale, poses[:p], layout="wlh")
        t100, t1 = timed(lambda: run(POSES), args.repeats), timed(lambda: run(1), args.repeats)
        k = args.reference_poses
        dstate = {a: b.to(dev) for a, b in state.items()}
        dargs = (dstate, xs.to(dev), ys.to(dev), zs.to(dev), center.to(dev), scale.to(dev), poses[:k].to(dev), dev)
        tref = timed(lambda: reference_formulation(*dargs), 1) * POSES / k
        tf = n * TRUNK_FLOP_PER_POINT / (t1 * 1e-3) / 1e12
        rec.update(pack_ms=round(t_pack, 3), query_ms_at_100_poses=round(t100, 3), query_ms_at_1_pose=round(t1, 3), trunk_tflops_lower_bound=round(tf, 2),
                   trunk_fraction_of_peak=round(tf / PEAK_TFLOPS, 3), head_ms_per_pose=round((t100 - t1) / (POSES - 1), 4),
                   reference_formulation_ms_at_100_poses=round(tref, 1), reference_poses_timed=k,
                   speedup_over_reference_formulation=round(tref / t100, 1), device=torch.cuda.get_device_name(0))
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
