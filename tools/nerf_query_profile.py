"""Time the differentiable NeRF query (ops.nerf_query, csrc/nerfquery.hip) on one training batch of 1024 rays x 256 samples and write
profiles/nerf_query.json.  Recorded, not gated.

    python tools/nerf_query_profile.py --out profiles/nerf_query.json

Fields: HIP-event times (best of ``--repeats`` after a warm-up call) of the forward alone and of forward plus backward with respect to
the 24 parameter tensors and the camera embedding, at the default chunk; from one forward-plus-backward under torch.profiler the
device time of each kernel family; the arithmetic of the step (2 x multiply-adds of the forward, the recomputed forward, dgrad and
wgrad) and the rate it implies; and as a yardstick the same step -- the same weights, points and cotangent -- through torch's own
float32 autograd of the checker model (tests/nerf_extract_ref.NeRF) on the same device.  Nothing else has been timed on this
workload: the reference's training loop has not been run.  Without a GPU the file is written with those fields empty.
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

RAYS, SAMPLES = 1024, 256
KERNELS = (trunk_kernel("KeepTile"), trunk_kernel("PointTile"), "nerfquery_head_kernel", "nerfquery_headbwd_kernel",
           "nerfquery_dgrad_kernel", "nerfquery_wgrad_kernel", "nerfquery_reduce_kernel", "nerfquery_finish_kernel",
           "nerfmlp_pack_kernel", "nerfquery_rays_kernel")


def step_flops(points, input_ch=57, tail=7):
    """2 x the multiply-adds of one forward, and of forward + recomputed forward + dgrad + wgrad."""
    fwd = input_ch * 256 + 4 * 256 * 256 + (input_ch + 256) * 256 + 2 * 256 * 256 + 256 * 256 + 256 + (256 + tail) * 128 + 128 * 3
    dgrad = fwd - input_ch * 256 * 2 - tail * 128         # nothing flows into the encoding, the view direction or (per point) cam
    return 2 * points * fwd, 2 * points * (2 * fwd + dgrad + fwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_query.json"))
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    points = RAYS * SAMPLES
    f_fwd, f_step = step_flops(points)
    rec = {"rays": RAYS, "samples": SAMPLES, "points": points, "chunk": None, "forward_ms": None, "forward_backward_ms": None,
           "kernel_ms": None, "forward_flop": f_fwd, "step_flop": f_step, "step_tflops": None, "torch_forward_ms": None,
           "torch_forward_backward_ms": None, "device": None}
    if torch.cuda.is_available():
        from nerf_rpn_amd import ops
        cfg, dev = R.DEFAULT_CFG, "cuda"
        state = R.make_state(1, "a")
        gen = torch.Generator().manual_seed(0)
        pts = (torch.rand(RAYS, SAMPLES, 3, generator=gen) * 2 - 1).to(dev)
        d = torch.randn(RAYS, 3, generator=gen)
        viewdirs = (d / d.norm(dim=-1, keepdim=True)).to(dev)
        cot = torch.randn(RAYS, SAMPLES, 4, generator=gen).to(dev)
        cam = torch.tensor([0.3, -0.2, 0.1, 0.4], device=dev, requires_grad=True)
        params = {k: v.to(dev).requires_grad_(True) for k, v in state.items()}
        wrt = list(params.values()) + [cam]

        def forward():
            with torch.no_grad():
                return ops.nerf_query(params, cfg, pts, viewdirs, cam)

        def step():
            return torch.autograd.grad((ops.nerf_query(params, cfg, pts, viewdirs, cam) * cot).sum(), wrt)
        rec.update(chunk=ops.NERF_QUERY_DEFAULT_CHUNK, forward_ms=round(timed(forward, args.repeats), 2),
                   forward_backward_ms=round(timed(step, args.repeats), 2), device=torch.cuda.get_device_name(0))
        rec["step_tflops"] = round(f_step / (rec["forward_backward_ms"] * 1e-3) / 1e12, 2)
        try:
            km = kernel_times(step, KERNELS)
        except Exception as e:      # the profiler is optional: the event times stand without it
            km, rec["note"] = None, f"torch.profiler failed: {type(e).__name__}"
        if km:
            # the two trunk families name different tiles, so they do not overlap
            rec["kernel_ms"] = {k: round(v, 3) for k, v in km.items()}

        model = R.build_model(state, cfg).to(dev).train()
        embed_fn, _ = R.get_embedder(cfg["multires"], cfg["i_embed"])
        embeddirs_fn, _ = R.get_embedder(cfg["multires_views"], cfg["i_embed"])
        twrt = list(model.parameters()) + [cam]

        def torch_query():
            dirs = embeddirs_fn(viewdirs[:, None].expand(pts.shape).reshape(-1, 3))
            x = torch.cat([embed_fn(pts.reshape(-1, 3)), dirs, cam.unsqueeze(0).expand(dirs.shape[0], cam.shape[0])], -1)
            return model(x).reshape(RAYS, SAMPLES, 4)

        def torch_forward():
            with torch.no_grad():
                return torch_query()

        def torch_step():
            return torch.autograd.grad((torch_query() * cot).sum(), twrt)
        rec.update(torch_forward_ms=round(timed(torch_forward, args.repeats), 2),
                   torch_forward_backward_ms=round(timed(torch_step, args.repeats), 2))
    else:
        rec["note"] = "no GPU run: the timing fields are empty"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
