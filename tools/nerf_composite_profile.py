"""Time the differentiable ray stage (ops.nerf_composite + ops.nerf_ray_losses, csrc/nerfcomposite.hip) on one training batch of
1024 rays x (128 + 128) samples and write profiles/nerf_composite.json.  Recorded, not gated.

    python tools/nerf_composite_profile.py --out profiles/nerf_composite.json

Fields: HIP-event times per step (``--iters`` steps per timed window, best of ``--repeats`` windows after a warm-up window) of the
forward alone (composite and both losses) and of forward plus backward down to raw1 and raw2; from one step under torch.profiler the
device time of each kernel and the number of device kernels launched; and as the yardstick the same step -- the same raw, samples,
noise and targets -- through the checker (tests/nerf_composite_ref.py) in float32 torch on the same device, the only other way the
project has to run this stage.  The MLP query is not part of either.  Without a GPU the file is written with those fields empty.
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

import nerf_composite_ref as C  # noqa: E402
from nerf_profile import kernel_times, timed  # noqa: E402

RAYS, S1, S2 = 1024, 128, 128
KERNELS = ("nerfcomposite_forward_kernel", "nerfcomposite_backward_kernel", "nerfraylosses_terms_kernel", "nerfraylosses_sum_kernel",
           "nerfraylosses_backward_kernel")


def device_launches(fn):
    """Device kernels launched by one call of fn, from torch.profiler."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_composite.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    rec = {"rays": RAYS, "samples": [S1, S2], "iters_per_window": args.iters, "forward_ms": None, "forward_backward_ms": None, "kernel_ms": None,
           "launches": None, "torch_forward_ms": None, "torch_forward_backward_ms": None, "torch_launches": None, "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import ops
        dev = "cuda"
        gen = torch.Generator().manual_seed(0)
        raw = torch.cat([torch.randn(RAYS, S1 + S2, 3, generator=gen), 3. * torch.randn(RAYS, S1 + S2, 1, generator=gen)], -1)
        raw1 = raw[:, :S1].contiguous().to(dev).requires_grad_(True)
        raw2 = raw[:, S1:].contiguous().to(dev).requires_grad_(True)
        z1 = torch.sort(torch.rand(RAYS, S1, generator=gen) * 3.9 + 0.1, -1).values.to(dev)
        z2 = torch.sort(torch.rand(RAYS, S2, generator=gen) * 3.9 + 0.1, -1).values.to(dev)
        d = torch.randn(RAYS, 3, generator=gen).to(dev)
        noise = torch.randn(RAYS, S1 + S2, generator=gen).to(dev)
        target_s = torch.rand(RAYS, 3, generator=gen).to(dev)
        target_d = torch.stack([torch.rand(RAYS, generator=gen) * 3.9 + 0.1, torch.rand(RAYS, generator=gen) * 0.45 + 0.05], -1).to(dev)
        target_vd = (torch.arange(RAYS) % 4 != 3).to(dev)
        weight = C.DEPTH_LOSS_WEIGHT

        def ours():
            rgb, _, _, w, depth, z = ops.nerf_composite(raw1, z1, d, raw2, z2, noise)
            img, dep = ops.nerf_ray_losses(rgb, target_s, depth, z, w, target_d, target_vd)
            return img + weight * dep

        def theirs():
            o = C.ray_stage(raw1, z1, d, raw2, z2, noise)
            return C.img2mse(o["rgb_map"], target_s) + weight * C.depth_loss(o["depth_map"], o["z_vals"], o["weights"], target_d, target_vd)

        def forward(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def step(fn):
            return lambda: torch.autograd.grad(fn(), [raw1, raw2])

        def per_step(fn):
            return round(timed(lambda: [fn() for _ in range(args.iters)], args.repeats) / args.iters, 4)
        # the checker builds its constants on the default device
        torch.set_default_device(dev)
        rec.update(forward_ms=per_step(forward(ours)), forward_backward_ms=per_step(step(ours)), torch_forward_ms=per_step(forward(theirs)),
                   torch_forward_backward_ms=per_step(step(theirs)), device=torch.cuda.get_device_name(0))
        a, b = step(ours)(), step(theirs)()
        rec["largest_gradient_difference"] = max(float((x - y).abs().max()) for x, y in zip(a, b))
        try:
            km = kernel_times(step(ours), KERNELS)
            rec["kernel_ms"] = {k: round(v, 4) for k, v in km.items()} if km else None
            rec["launches"], rec["torch_launches"] = device_launches(step(ours)), device_launches(step(theirs))
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
