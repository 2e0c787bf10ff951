"""Time the front end of a NeRF training step (ops.nerf_train_batch + ops.nerf_train_samples, csrc/nerftrain.hip) and the whole step
around it on one batch of 1024 rays x (128 + 128) samples of a 468 x 624 view with depth priors, and write profiles/nerf_train.json.
Recorded, not gated.

    python tools/nerf_train_profile.py --out profiles/nerf_train.json

Fields: HIP-event times per step (``--iters`` steps per timed window, best of ``--repeats`` windows after a warm-up window) of
  front_end_ms        the uniforms, the batch kernel, the samples kernel on a given raw1 and the sort of z2, with its device launches;
  torch_front_end_ms  the yardstick: the same front end through the checker (tests/nerf_train_ref.py: get_rays of the whole image,
                      five gathers, perturb_z_vals, the two masked sample_3sigma / sample_pdf assignments) in float32 torch on the same
                      device, with its launches -- the only other way the project has to run this stage;
  step_ms             a whole step (front end, both queries forward and backward, the ray stage, clip_grad_value_ and Adam) and its
                      parts timed on their own: query_ms, ray_stage_ms, clip_adam_ms;
  host_draw_ms        the host's np.random.choice(H W, N_rand, replace=False) per step (wall clock);
  wall_step_ms, wall_step_with_draw_ms   wall clock per step of a loop of steps without and with the host draw, synchronised once at
                      the end: the draw hides behind the device if the two agree.
Without a GPU the file is written with those fields empty.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_train_ref as T  # noqa: E402
from nerf_composite_profile import device_launches  # noqa: E402
from nerf_profile import kernel_times, timed  # noqa: E402

RAYS, S, H, W, NEAR, FAR = 1024, 128, 468, 624, 0.1, 4.0
KERNELS = ("nerftrain_batch_kernel", "nerftrain_samples_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_train.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    rec = {"rays": RAYS, "samples": [S, S], "image_hw": [H, W], "iters_per_window": args.iters, "front_end_ms": None, "launches": None,
           "kernel_ms": None, "torch_front_end_ms": None, "torch_launches": None, "step_ms": None, "query_ms": None, "ray_stage_ms": None,
           "clip_adam_ms": None, "host_draw_ms": None, "wall_step_ms": None, "wall_step_with_draw_ms": None, "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import NeRF, nerf_train, ops
        dev = torch.device("cuda")
        gen = torch.Generator().manual_seed(0)
        image = torch.rand(H, W, 3, generator=gen)
        d = torch.rand(H, W, generator=gen) * 3.5 + 0.3
        s = torch.rand(H, W, generator=gen) * 0.3 + 0.03
        valid = torch.rand(H, W, generator=gen) < 0.5
        depth = torch.stack([torch.where(valid, d, torch.zeros(())), torch.where(valid, s, torch.zeros(()))], -1)
        intrinsic = torch.tensor([580., 580., W / 2., H / 2.])
        c2w = T.R.make_poses(1, 1)[0]
        z = T.V.precompute_quadratic_samples(NEAR, FAR, S)
        lower_bound = float(z[-1] - z[-2])
        raw1 = torch.cat([torch.randn(RAYS, S, 3, generator=gen), 3. * torch.randn(RAYS, S, 1, generator=gen)], -1)
        image, depth, valid, intrinsic, c2w, z, raw1 = (x.to(dev) for x in (image, depth, valid, intrinsic, c2w, z, raw1))
        dgen = torch.Generator(device=dev).manual_seed(0)
        pix_host = np.random.RandomState(0).choice(H * W, RAYS, replace=False).astype(np.int32)
        pix = torch.from_numpy(pix_host).to(dev)

        def front(raw=raw1):
            t_rand, u = (torch.rand((RAYS, S), generator=dgen, device=dev) for _ in range(2))
            b = ops.nerf_train_batch(intrinsic, c2w, H, W, pix, image, depth, valid, z, t_rand)
            z2 = ops.nerf_train_samples(raw, b["z1"], b["rays"], NEAR, FAR, lower_bound, b["depth_range"], u)
            return b, torch.sort(z2, -1).values

        near_t, far_t = torch.tensor(NEAR, device=dev), torch.tensor(FAR, device=dev)

        def theirs():
            t_rand, u = (torch.rand((RAYS, S), generator=dgen, device=dev) for _ in range(2))
            b = T.ray_batch(intrinsic, c2w, pix, image, depth, valid, hw=(H, W))
            z1 = T.perturb_z_vals(z.unsqueeze(0).expand(RAYS, S), t_rand)
            z2, _ = T.second_list(raw1, z1, b["rays"][:, 3:], b["depth_range"], u, z[-1] - z[-2], near_t, far_t)
            return b, torch.sort(z2, -1).values

        def per_step(fn):
            return round(timed(lambda: [fn() for _ in range(args.iters)], args.repeats) / args.iters, 4)

        rec["device"] = torch.cuda.get_device_name(0)
        rec["front_end_ms"] = per_step(front)
        torch.set_default_device(dev)                    # the checker builds its constants on the default device
        rec["torch_front_end_ms"] = per_step(theirs)
        torch.set_default_device("cpu")

        model = NeRF({"multires_views": 0, "input_ch_cam": 4}).to(dev)
        params = list(model.parameters())
        opt = torch.optim.Adam(params, lr=5e-4, betas=(0.9, 0.999))
        cam = torch.zeros(4, device=dev)
        center, scale = torch.zeros(3, device=dev), torch.tensor(0.25, device=dev)

        def step(draw=False):
            global_pix = pix
            if draw:
                host = np.random.choice(H * W, RAYS, replace=False).astype(np.int32)
                global_pix = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
            t_rand, u = (torch.rand((RAYS, S), generator=dgen, device=dev) for _ in range(2))
            b = ops.nerf_train_batch(intrinsic, c2w, H, W, global_pix, image, depth, valid, z, t_rand)
            out = nerf_train.render_rays_train(model, b["rays"][:, :3], b["rays"][:, 3:], b["viewdirs"], b["z1"], "draw", cam, center, scale,
                                               depth_range=b["depth_range"], u=u, lower_bound=lower_bound, near=NEAR, far=FAR)
            opt.zero_grad()
            loss, _, _ = nerf_train.training_loss(out, b["target_s"], b["target_d"], b["target_vd"], 0.004)
            loss.backward()
            torch.nn.utils.clip_grad_value_(params, 0.1)
            opt.step()

        b0, z2s = front()
        o, dd = b0["rays"][:, :3], b0["rays"][:, 3:]

        def query_part():
            for zz in (b0["z1"], z2s):
                raw = model.query(o[:, None, :] + dd[:, None, :] * zz[..., :, None], b0["viewdirs"], cam, center, scale)
                raw.backward(torch.ones_like(raw))

        ra, rb = raw1.clone().requires_grad_(True), raw1.flip(0).clone().requires_grad_(True)

        def ray_part():
            rgb, _, _, w, dep, zv = ops.nerf_composite(ra, b0["z1"], dd, rb, z2s)
            img, dl = ops.nerf_ray_losses(rgb, b0["target_s"], dep, zv, w, b0["target_d"], b0["target_vd"])
            torch.autograd.grad(img + 0.004 * dl, [ra, rb])

        def clip_adam():
            torch.nn.utils.clip_grad_value_(params, 0.1)
            opt.step()

        rec["step_ms"] = per_step(step)
        rec["query_ms"], rec["ray_stage_ms"], rec["clip_adam_ms"] = per_step(query_part), per_step(ray_part), per_step(clip_adam)

        t0 = time.perf_counter()
        for _ in range(20):
            np.random.choice(H * W, RAYS, replace=False)
        rec["host_draw_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 4)

        def wall(draw):
            best = float("inf")
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(args.iters):
                    step(draw)
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t) / args.iters * 1e3)
            return round(best, 4)
        rec["wall_step_ms"], rec["wall_step_with_draw_ms"] = wall(False), wall(True)
        try:
            km = kernel_times(front, KERNELS)
            rec["kernel_ms"] = {k: round(v, 4) for k, v in km.items()} if km else None
            rec["launches"] = device_launches(front)
            torch.set_default_device(dev)
            rec["torch_launches"] = device_launches(theirs)
            torch.set_default_device("cpu")
        except Exception as e:      # the profiler is optional: the event times stand without it
            rec["note"] = f"torch.profiler failed: {type(e).__name__}"
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
