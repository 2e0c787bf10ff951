"""Generate tests/golden/nerf_camopt.npz and nerf_camopt_bounds.json from the REFERENCE's data/scannet/run_nerf.py (build container
only: it reads the reference tree).

run_nerf.py is imported as make_nerf_render_golden.py imports it; get_rays, sample_pdf, img2mse, mse2psnr and create_random_subsets
come from the fork, which is not on disk: the checkers' definitions are set as the module's globals.  Only
recorded results are stored; no reference text.

nerf_camopt.npz
  <case>/<cam>/<partition>/losses, grad   the reference's own render(H, W, None, rays=batch_rays, **render_kwargs_test) with a leaf
                                          embedded_cam, img2mse and backward() per batch, on the CPU with one thread: the batch
                                          losses and the gradient accumulated in embedded_cam.grad
  <case>/loop/embedding, partition        the reference's own optimize_camera_embedding (100 steps): what it leaves in
                                          render_kwargs_test["embedded_cam"], and the seeded partition it drew
nerf_camopt_bounds.json
  golden_difference    the largest |float32 checker - reference| of losses and grad (0 if bit-equal)
  cases/<case>/given_z2 | end_to_end / loss, rgb_map, grad, pre: 8 x the largest |float32 checker - float64 checker| over the
                       embeddings and partitions, the measured value next to it; given_z2: the float64 checker on the float32
                       checker's z2
  cases/<case>/allow/<mode>/<cam>/<partition>   the flip allowance of the gradient and |F| (tests/nerf_camopt_ref.py flip_allowance).
                       Asserted: allow <= 0.01 max|grad| and |F| <= 8 per 2^16 pre-activations (at least 8).  F is taken within the given-z2 pre bound; end to end within
                       twice it (the end-to-end pre figure holds the float32 checker's z2 error, which the kernels do not have)
  loop4/<case>         the largest |float32-checker loop - float64-checker loop| of the embedding after 4 steps, for the command
                       line test's frames

    python tests/golden/make_nerf_camopt_golden.py       rewrites both files; the same bytes on every run
"""
import json
import os
import sys
import tempfile
from argparse import Namespace

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.dont_write_bytecode = True       # the reference tree is read-only

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_camopt_ref as C                                 # noqa: E402
import nerf_eval_ref as E                                   # noqa: E402
import nerf_render_ref as V                                 # noqa: E402
from make_nerf_extract_golden import reference_module       # noqa: E402
from make_scannet_golden import save_stable                 # noqa: E402
from nerf_rpn_amd import camopt                             # noqa: E402

BOUND_FACTOR = 8.0
LOOP_N_RAND = {"views_cam_3x5": 2, "odd_5x7": 4}          # batches of 2 N_rand: 4, 4, 4, 3 and 8, 8, 8, 8, 3
LOOP_SEED = 11
OUTPUTS = ("loss", "rgb_map", "grad", "pre")


def reference_kwargs(RN, c, tmp, tag):
    exp = os.path.join(tmp, tag)
    os.makedirs(exp)
    state = {"module." + k: v for k, v in c.state.items()}
    dummy = torch.optim.Adam([torch.nn.Parameter(v.clone()) for v in state.values()], lr=5e-4, betas=(0.9, 0.999))
    torch.save({"global_step": 100000, "network_fn_state_dict": state, "optimizer_state_dict": dummy.state_dict()},
               os.path.join(exp, "100000.tar"))
    args = Namespace(expname=tag, ckpt_dir=tmp, no_reload=False, lrate=5e-4, netdepth=c.cfg["netdepth"], netwidth=c.cfg["netwidth"],
                     netdepth_fine=8, netwidth_fine=256, multires=c.cfg["multires"], multires_views=c.cfg["multires_views"],
                     i_embed=c.cfg["i_embed"], use_viewdirs=True, N_importance=0, input_ch_cam=c.cfg["input_ch_cam"],
                     netchunk_per_gpu=1024 * 64 * 4, n_gpus=1, perturb=1., N_samples=c.n_samples, raw_noise_std=0., lindisp=c.lindisp,
                     bb_center=c.bb_center, bb_scale=c.bb_scale, chunk=1024 * 32)
    _, kw, _, grad_vars, _ = RN.create_nerf(args, {"precomputed_z_samples": c.z_samples, "near": c.near, "far": c.far})
    for p in grad_vars:              # run_nerf.py:1099-1100
        p.requires_grad = False
    return args, kw


def reference_batches(RN, c, kw, cam, target, batches):
    """The body of optimize_camera_embedding's batch loop (:212-221) with the reference's render -> (losses, accumulated grad)."""
    leaf = torch.tensor(cam, dtype=torch.float32, requires_grad=True)
    kw = dict(kw, embedded_cam=leaf)
    rays_o, rays_d = V.get_rays(c.H, c.W, c.intrinsic, c.c2w[:3, :4])
    rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    losses = []
    for b in batches:
        batch_rays = torch.stack([rays_o[b], rays_d[b]], 0)
        rgb, _, _, _ = RN.render(c.H, c.W, None, chunk=1024 * 32, rays=batch_rays, **kw)
        loss = E.img2mse(rgb, target[b])
        loss.backward()
        losses.append(loss.detach())
    return torch.stack(losses).numpy(), leaf.grad.numpy().copy()


def main():
    torch.set_num_threads(1)
    RN = reference_module()
    RN.get_rays, RN.sample_pdf, RN.img2mse, RN.mse2psnr = V.get_rays, V.sample_pdf, E.img2mse, E.mse2psnr
    drawn = {}

    def create_random_subsets(indices, subset_size, device=None):
        parts = camopt.random_subsets(len(indices), subset_size, torch.Generator().manual_seed(LOOP_SEED))
        drawn["partition"] = parts
        return parts
    RN.create_random_subsets = create_random_subsets

    class Plateau(torch.optim.lr_scheduler.ReduceLROnPlateau):        # this torch no longer takes the reference's verbose=True
        def __init__(self, *a, verbose=False, **k):
            super().__init__(*a, **k)
    torch.optim.lr_scheduler.ReduceLROnPlateau = Plateau
    out, cases, golden_diff = {}, {}, {"losses": 0.0, "grad": 0.0}
    with tempfile.TemporaryDirectory() as tmp:
        for name in C.CASE_NAMES:
            c = C.case(name)
            n = C.num_rays(c)
            args, kw = reference_kwargs(RN, c, tmp, name)
            target = C.target_for(c)
            z2 = None
            if not c.plain:
                with torch.no_grad():
                    z2 = C._render_rays(c, C.frame_rays(c, torch.float32), torch.zeros(4), torch.float32)["z2"]
            err = {mode: {k: 0.0 for k in OUTPUTS} for mode in ("given_z2", "end_to_end")}
            allow = {}
            for cam_name, cam in C.CAMS.items():
                t32 = C.head_terms(c, cam, torch.float32)
                t64 = {"given_z2": C.head_terms(c, cam, torch.float64, z2), "end_to_end": C.head_terms(c, cam, torch.float64)}
                for mode in err:
                    err[mode]["pre"] = max(err[mode]["pre"], float((t32["pre"].double() - t64[mode]["pre"]).abs().max()))
                for part in C.PARTITIONS:
                    batches = C.partition(n, part)
                    ref_losses, ref_grad = reference_batches(RN, c, kw, cam, target, batches)
                    o32 = C.objective(c, cam, target, batches, torch.float32)
                    golden_diff["losses"] = max(golden_diff["losses"], float(np.abs(o32["losses"].numpy() - ref_losses).max()))
                    golden_diff["grad"] = max(golden_diff["grad"], float(np.abs(o32["grad"].numpy() - ref_grad).max()))
                    out[f"{name}/{cam_name}/{part}/losses"], out[f"{name}/{cam_name}/{part}/grad"] = ref_losses, ref_grad
                    for mode in err:
                        o64 = C.objective(c, cam, target, batches, torch.float64, z2 if mode == "given_z2" else None)
                        e = err[mode]
                        e["loss"] = max(e["loss"], float((o32["losses"].double().sum() - o64["losses"].sum()).abs()))
                        e["rgb_map"] = max(e["rgb_map"], float((o32["rgb_map"].double() - o64["rgb_map"]).abs().max()))
                        e["grad"] = max(e["grad"], float((o32["grad"].double() - o64["grad"]).abs().max()))
                        allow.setdefault(mode, {}).setdefault(cam_name, {})[part] = (o64, batches)
            b = {mode: {k: {"bound": BOUND_FACTOR * v, "fp32_error": v} for k, v in err[mode].items()} for mode in err}
            # the flip allowance needs the case's pre bound, known only now
            b["allow"] = {}
            for mode in err:
                for cam_name, cam in C.CAMS.items():
                    t = C.head_terms(c, cam, torch.float64, z2 if mode == "given_z2" else None)
                    for part in C.PARTITIONS:
                        o64, batches = allow[mode][cam_name][part]
                        fg = C.fixed_gradient(c, t, target, C.ray_weights(batches, n))
                        # end to end the kernels draw z2 in float64 and round it once: their pre-activations carry the given-z2 error plus
                        # that of one more float32 rounding of z (the points are rounded to float32 anyway), not the float32
                        # checker's z2 error that the end-to-end pre figure holds -- twice the given-z2 bound
                        al, nf = C.flip_allowance(c, t, fg["d"], (1. if mode == "given_z2" else 2.) * b["given_z2"]["pre"]["bound"])
                        gmax = float(o64["grad"].abs().max())
                        # |F| grows with the number of pre-activations at a given bound: 8 up to 2^16 of them (every 16-sample case), in
                        # proportion beyond (full_3x3 has 9 x 256 x 128)
                        nf_max = 8 * max(1., t["pre"].numel() / 65536.)
                        assert float(al.max()) <= 0.01 * gmax and nf <= nf_max, (name, mode, cam_name, part, al.tolist(), gmax, nf)
                        b["allow"].setdefault(mode, {}).setdefault(cam_name, {})[part] = {"allow": al.tolist(), "F": nf, "grad_max": gmax}
            cases[name] = b
            print(f"{name}: " + "; ".join(f"{mode} " + ", ".join(f"{k} {v:.2g}" for k, v in err[mode].items()) for mode in err))
            if name in C.LOOP_CASES:
                args.N_rand = LOOP_N_RAND[name]
                kw_loop = dict(kw)
                image = target.reshape(c.H, c.W, 3)
                RN.optimize_camera_embedding(image, c.c2w[:3, :4], c.H, c.W, c.intrinsic, args, kw_loop)
                out[f"{name}/loop/embedding"] = kw_loop["embedded_cam"].detach().numpy().copy()
                parts = drawn["partition"]
                out[f"{name}/loop/partition"] = torch.cat(parts).numpy()
                out[f"{name}/loop/sizes"] = np.array([len(p) for p in parts])
                print(f"{name}: loop embedding {out[f'{name}/loop/embedding']}, batches {[len(p) for p in parts]}")
    loop4 = {}
    for name, (H, W) in C.CLI_FRAMES.items():
        c, target, batches = C.cli_case(name)
        got = [camopt.optimize_embedding(C.value_and_grad(c, target, batches, dt), 4, steps=4) for dt in (torch.float32, torch.float64)]
        d = float((got[0].double() - got[1].double()).abs().max())
        loop4[name] = {"bound": BOUND_FACTOR * d, "fp32_error": d, "embedding64": got[1].tolist()}
        print(f"{name}: 4-step loops differ by {d:.3g}")
    print(f"float32 checker vs reference: losses {golden_diff['losses']:.3g}, grad {golden_diff['grad']:.3g}")
    out["cases"] = np.array(C.CASE_NAMES)
    path = os.path.join(HERE, "nerf_camopt.npz")
    save_stable(path, out)
    with open(os.path.join(HERE, "nerf_camopt_bounds.json"), "w") as f:
        json.dump({"factor": BOUND_FACTOR, "golden_difference": golden_diff, "cases": cases, "loop4": loop4}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
