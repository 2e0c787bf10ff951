"""Time a nerf_train step and its two queries in dtype bf16x3 with the backward's products in fp32 (the switch off: the arithmetic the
mode had before the switch existed, the yardstick) and in bf16x3 (backward_dtype), in one process, and write
profiles/nerf_bf16x3_backward.json.  Recorded, not gated.

    python tools/nerf_split_backward_profile.py --out profiles/nerf_bf16x3_backward.json

Per setting of the switch, at 1024 rays x (128 + 128) samples as tools/nerf_split_profile.py has them:
  step_ms       a whole nerf_train step, HIP-event time: ``--repeats`` windows of ``--iters`` steps after a warm-up window; per step the
                fastest window (min), the median window and the slowest (max), so that the spread is on record;
  query_ms      its two queries, forward and backward, on their own, timed the same way;
  kernels_ms    device time per kernel family summed over the two queries of one step, from torch.profiler (None if it records nothing).
``speedup`` has off / on of step_ms and query_ms (of their min, and ``*_median`` of their median), and of the dgrad and wgrad
families (the split wgrad together with the column-sum kernel that takes the bias gradients it no longer takes itself).  Without a GPU the file is written with those fields empty.
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
from nerf_profile import kernel_times, trunk_kernel, window_times  # noqa: E402

RAYS, S, H, W, NEAR, FAR = 1024, 128, 468, 624, 0.1, 4.0
SWITCH = ("fp32", "bf16x3")
FAMILIES = (trunk_kernel("KeepTile", "bf16x3"), "nerfquery_headbwd_kernel", "nerfquery_dgrad_kernel", "nerfquery_dgrad_split_kernel",
            "nerfquery_wgrad_kernel", "nerfquery_wgrad_split_kernel", "nerfquery_colsum_kernel", "nerfquery_reduce_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_bf16x3_backward.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    rec = {"rays": RAYS, "samples": [S, S], "dtype": "bf16x3", "iters_per_window": args.iters, "windows": args.repeats, "step_ms": None,
           "query_ms": None, "kernels_ms": None, "speedup": None, "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import NeRF, nerf_train, ops
        dev = torch.device("cuda")
        rec["device"] = torch.cuda.get_device_name(0)
        gen = torch.Generator().manual_seed(0)
        cfg = {"multires_views": 0, "input_ch_cam": 4}
        state = {k: v.to(dev) for k, v in T.R.make_state(1, "a", dict(T.R.DEFAULT_CFG, **cfg)).items()}
        cam = torch.zeros(4, device=dev)
        center, scale = torch.zeros(3, device=dev), torch.tensor(0.25, device=dev)
        image = torch.rand(H, W, 3, generator=gen)
        d = torch.rand(H, W, generator=gen) * 3.5 + 0.3
        s = torch.rand(H, W, generator=gen) * 0.3 + 0.03
        valid = torch.rand(H, W, generator=gen) < 0.5
        depth = torch.stack([torch.where(valid, d, torch.zeros(())), torch.where(valid, s, torch.zeros(()))], -1)
        intrinsic = torch.tensor([580., 580., W / 2., H / 2.])
        c2w = T.R.make_poses(1, 1)[0]
        z = T.V.precompute_quadratic_samples(NEAR, FAR, S)
        lower_bound = float(z[-1] - z[-2])
        image, depth, valid, intrinsic, c2w_d, z = (x.to(dev) for x in (image, depth, valid, intrinsic, c2w, z))
        dgen = torch.Generator(device=dev).manual_seed(0)
        pix = torch.from_numpy(np.random.RandomState(0).choice(H * W, RAYS, replace=False).astype(np.int32)).to(dev)
        step_ms, query_ms, kernels_ms = {}, {}, {}
        for sw in SWITCH:
            model = NeRF(cfg, dtype="bf16x3", backward_dtype=sw).to(dev)
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
                w = sorted(t / args.iters for t in window_times(lambda: [fn() for _ in range(args.iters)], args.repeats))
                return {"min": round(w[0], 4), "median": round(float(np.median(w)), 4), "max": round(w[-1], 4)}
            step_ms[sw], query_ms[sw] = per_step(step), per_step(query_part)
            try:
                km = kernel_times(query_part, FAMILIES)
                kernels_ms[sw] = {k: round(v, 4) for k, v in km.items()} if km else None
            except Exception as e:      # the profiler is optional: the event times stand without it
                rec["note"] = f"torch.profiler failed: {type(e).__name__}"
                kernels_ms[sw] = None
        rec["step_ms"], rec["query_ms"], rec["kernels_ms"] = step_ms, query_ms, kernels_ms
        speedup = {k: round(rec[k]["fp32"]["min"] / rec[k]["bf16x3"]["min"], 3) for k in ("step_ms", "query_ms")}
        speedup.update({k + "_median": round(rec[k]["fp32"]["median"] / rec[k]["bf16x3"]["median"], 3) for k in ("step_ms", "query_ms")})
        off, on = kernels_ms["fp32"], kernels_ms["bf16x3"]
        if off and on:
            speedup["dgrad"] = round(off["nerfquery_dgrad_kernel"] / on["nerfquery_dgrad_split_kernel"], 3)
            wg_on = on["nerfquery_wgrad_kernel"] + on["nerfquery_wgrad_split_kernel"] + on["nerfquery_colsum_kernel"]
            speedup["wgrad"] = round(off["nerfquery_wgrad_kernel"] / wg_on, 3)
        rec["speedup"] = speedup
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
