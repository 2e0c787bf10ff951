"""Time the NeRF MLP trunk in its two arithmetics, fp32 and bf16x3, in one process, and write
profiles/nerf_bf16x3.json.  Recorded, not gated.

    python tools/nerf_split_profile.py --out profiles/nerf_bf16x3.json

Per mode, HIP-event times (best of ``--repeats`` after a warm-up call; the fp32 path of the same tree in the same run is the yardstick):
  query_forward_ms    ops.nerf_query under no_grad at 2^16 and 2^18 points (rays of 128 samples): pack, rays, trunk and head;
  trunk_kernel_ms     the trunk kernel's device time inside that call, from torch.profiler (None if the profiler records nothing);
  step_ms             a whole nerf_train step of 1024 rays x (128 + 128) samples, as tools/nerf_train_profile.py times it
                      (``--iters`` steps per window), and query_ms, its two queries forward and backward on their own;
  frame_ms            one 468 x 624 ops.nerf_render frame at 128 + 128 samples (the two-pass path) with packed weights.
``speedup`` has fp32 / bf16x3 of each.  Without a GPU the file is written with those fields empty.
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

import nerf_train_ref as T  # noqa: E402
from nerf_profile import kernel_times, timed, trunk_kernel  # noqa: E402

RAYS, S, H, W, NEAR, FAR = 1024, 128, 468, 624, 0.1, 4.0
POINTS = (1 << 16, 1 << 18)
MODES = ("fp32", "bf16x3")
TRUNK = {m: trunk_kernel("PointTile", m) for m in ("fp32", "bf16x3")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_bf16x3.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    rec = {"points": list(POINTS), "rays": RAYS, "samples": [S, S], "image_hw": [H, W], "iters_per_window": args.iters,
           "query_forward_ms": None, "trunk_kernel_ms": None, "step_ms": None, "query_ms": None, "frame_ms": None, "speedup": None,
           "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import NeRF, nerf_train, ops
        dev = torch.device("cuda")
        rec["device"] = torch.cuda.get_device_name(0)
        gen = torch.Generator().manual_seed(0)
        cfg = {"multires_views": 0, "input_ch_cam": 4}
        state = {k: v.to(dev) for k, v in T.R.make_state(1, "a", dict(T.R.DEFAULT_CFG, **cfg)).items()}
        cam = torch.zeros(4, device=dev)
        center, scale = torch.zeros(3, device=dev), torch.tensor(0.25, device=dev)

        # ---- the trunk forward ----
        fwd, kern = {m: {} for m in MODES}, {m: {} for m in MODES}
        for n in POINTS:
            pts = (torch.rand(n // S, S, 3, generator=gen) * 2 - 1).to(dev)
            dirs = torch.nn.functional.normalize(torch.randn(n // S, 3, generator=gen), dim=-1).to(dev)
            for m in MODES:
                def call(m=m):
                    with torch.no_grad():
                        return ops.nerf_query(state, cfg, pts, dirs, cam, dtype=m)
                fwd[m][str(n)] = round(timed(call, args.repeats), 4)
                try:
                    km = kernel_times(call, (TRUNK[m],))
                    kern[m][str(n)] = round(km[TRUNK[m]], 4) if km else None
                except Exception as e:      # the profiler is optional: the event times stand without it
                    rec["note"] = f"torch.profiler failed: {type(e).__name__}"
                    kern[m][str(n)] = None
        rec["query_forward_ms"], rec["trunk_kernel_ms"] = fwd, kern

        # ---- a training step ----
        image = torch.rand(H, W, 3, generator=gen)
        d = torch.rand(H, W, generator=gen) * 3.5 + 0.3
        s = torch.rand(H, W, generator=gen) * 0.3 + 0.03
        valid = torch.rand(H, W, generator=gen) < 0.5
        depth = torch.stack([torch.where(valid, d, torch.zeros(())), torch.where(valid, s, torch.zeros(()))], -1)
        intrinsic = torch.tensor([580., 580., W / 2., H / 2.])
        c2w = T.R.make_poses(1, 1)[0]
        z = T.V.precompute_quadratic_samples(NEAR, FAR, S)
        lower_bound = float(z[-1] - z[-2])
        intrinsic_host = intrinsic
        image, depth, valid, intrinsic, c2w_d, z = (x.to(dev) for x in (image, depth, valid, intrinsic, c2w, z))
        dgen = torch.Generator(device=dev).manual_seed(0)
        pix = torch.from_numpy(np.random.RandomState(0).choice(H * W, RAYS, replace=False).astype(np.int32)).to(dev)
        step_ms, query_ms = {}, {}
        for m in MODES:
            model = NeRF(cfg, dtype=m).to(dev)
            model.load_state_dict(state)
            params = list(model.parameters())
            opt = torch.optim.Adam(params, lr=5e-4, betas=(0.9, 0.999))

            def step():
                t_rand, u = (torch.rand((RAYS, S), generator=dgen, device=dev) for _ in range(2))
                b = ops.nerf_train_batch(intrinsic, c2w_d, H, W, pix, image, depth, valid, z, t_rand)
                out = nerf_train.render_rays_train(model, b["rays"][:, :3], b["rays"][:, 3:], b["viewdirs"], b["z1"], "draw", cam, center,
                                                   scale, depth_range=b["depth_range"], u=u, lower_bound=lower_bound, near=NEAR, far=FAR)
                opt.zero_grad()
                loss, _, _ = nerf_train.training_loss(out, b["target_s"], b["target_d"], b["target_vd"], 0.004)
                loss.backward()
                torch.nn.utils.clip_grad_value_(params, 0.1)
                opt.step()
                return b, out

            b0, out0 = step()
            o, dd, z2s = b0["rays"][:, :3], b0["rays"][:, 3:], torch.sort(out0["z_vals_2"], -1).values

            def query_part():
                for zz in (b0["z1"], z2s):
                    raw = model.query(o[:, None, :] + dd[:, None, :] * zz[..., :, None], b0["viewdirs"], cam, center, scale)
                    raw.backward(torch.ones_like(raw))

            def per_step(fn):
                return round(timed(lambda: [fn() for _ in range(args.iters)], args.repeats) / args.iters, 4)
            step_ms[m], query_ms[m] = per_step(step), per_step(query_part)
        rec["step_ms"], rec["query_ms"] = step_ms, query_ms

        # ---- a frame ----
        frame_ms = {}
        for m in MODES:
            weights = ops.nerf_grid_pack(state, cfg, dtype=m)
            frame_ms[m] = round(timed(lambda: ops.nerf_render(weights, cfg, H=H, W=W, intrinsic=intrinsic_host, c2w=c2w[:3, :4], near=NEAR, far=FAR,
                                                              bb_center=center, bb_scale=scale, z_samples=z), args.repeats), 4)
        rec["frame_ms"] = frame_ms

        def ratio(x):
            if isinstance(x["fp32"], dict):
                return {k: (round(x["fp32"][k] / x["bf16x3"][k], 3) if x["fp32"][k] and x["bf16x3"][k] else None) for k in x["fp32"]}
            return round(x["fp32"] / x["bf16x3"], 3)
        rec["speedup"] = {k: ratio(rec[k]) for k in ("query_forward_ms", "trunk_kernel_ms", "step_ms", "query_ms", "frame_ms")}
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
