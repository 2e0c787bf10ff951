"""Generate tests/golden/nerf_render.npz and nerf_render_bounds.json from the REFERENCE's data/scannet/run_nerf.py (build container
only: it reads the reference tree).

run_nerf.py is imported as make_nerf_extract_golden.py imports it (stand-ins for the modules this machine lacks, the checker's NeRF /
get_embedder for the fork's).  get_rays and sample_pdf also come from the fork; the checker's definitions (tests/nerf_render_ref.py,
the assumptions of DESIGN.md 3.16) are set as the module's globals.  For every case the reference's own create_nerf loads a
checkpoint and its own render(H, W, intrinsic, chunk, c2w=pose, **render_kwargs_test) runs on the CPU -- render_rays, run_network,
compute_samples_around_depth, sample_3sigma, forward_with_additonal_samples and raw2outputs are the reference's code.  Only recorded
results are stored; no reference text.

nerf_render.npz          <case>/rgb_map, depth_map, acc_map, disp_map, z_vals, weights as the reference returns them, flattened to rays
nerf_render_bounds.json  per case and output: 8 x the largest |float32 checker - float64 checker|, the measured error next to it.
                         Outputs: the six above, depth_std, the stages raw1_rgb, raw1_sigma, z2, and under "given_raw1" / "given_z2"
                         the same for the float64 checker fed the float32 checker's raw1 / z2 (the staged GPU tests).

The float32 checker must equal the reference bit for bit in every stored array (asserted) or nothing is written.  Also asserted:
every case of more than one ray has rays with acc_map below 0.5 and above 0.9 and at least four rays with acc_map between 0.05 and 0.95,
so that the compositing error is sampled by several rays (the one-ray case: between 0.1 and 0.9); in the float64
run no inverse-CDF sample lies in a bin whose cdf difference is between 1e-6 and 1e-4 -- within a factor 10 of sample_pdf's 1e-5
branch -- unless the bin has zero width; the clamped case has ties in its merged samples and bins clamped at both ends.

    python tests/golden/make_nerf_render_golden.py       rewrites both files; the same bytes on every run
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

import nerf_render_ref as V                                 # noqa: E402
from make_nerf_extract_golden import reference_module       # noqa: E402
from make_scannet_golden import save_stable                 # noqa: E402

BOUND_FACTOR = 8.0
STORED = ("rgb_map", "depth_map", "acc_map", "disp_map", "z_vals", "weights")


def reference_render(RN, c, tmp):
    """The reference's create_nerf + render on one case -> dict of flat numpy arrays."""
    exp = os.path.join(tmp, c.name)
    os.makedirs(exp)
    state = {"module." + k: v for k, v in c.state.items()}
    dummy = torch.optim.Adam([torch.nn.Parameter(v.clone()) for v in state.values()], lr=5e-4, betas=(0.9, 0.999))
    torch.save({"global_step": 100000, "network_fn_state_dict": state, "optimizer_state_dict": dummy.state_dict()},
               os.path.join(exp, "100000.tar"))
    args = Namespace(expname=c.name, ckpt_dir=tmp, no_reload=False, lrate=5e-4, netdepth=c.cfg["netdepth"], netwidth=c.cfg["netwidth"],
                     netdepth_fine=8, netwidth_fine=256, multires=c.cfg["multires"], multires_views=c.cfg["multires_views"],
                     i_embed=c.cfg["i_embed"], use_viewdirs=True, N_importance=0, input_ch_cam=c.cfg["input_ch_cam"],
                     netchunk_per_gpu=1024 * 64 * 4, n_gpus=1, perturb=1., N_samples=c.n_samples, raw_noise_std=0., lindisp=c.lindisp,
                     bb_center=c.bb_center, bb_scale=c.bb_scale)
    _, kw, _, _, _ = RN.create_nerf(args, {"precomputed_z_samples": c.z_samples, "near": c.near, "far": c.far})
    if c.cfg["input_ch_cam"] > 0:         # render_video :175-176; the camera case renders with a non-zero embedding
        kw["embedded_cam"] = torch.zeros(c.cfg["input_ch_cam"]) if c.embedded_cam is None else c.embedded_cam
    with torch.no_grad():
        rgb, disp, acc, extras = RN.render(c.H, c.W, c.intrinsic, chunk=1024 * 32, c2w=c.c2w[:3, :4], **kw)
    out = dict(extras, rgb_map=rgb, disp_map=disp, acc_map=acc)
    n = c.H * c.W
    return {k: out[k].reshape(n, *out[k].shape[2:]).numpy() for k in STORED}


def errors(o32, o64, keys):
    return {k: float((o32[k].double() - o64[k]).abs().max()) for k in keys}


def with_raw(o):
    return dict(o, raw1_rgb=o["raw1"][..., :3], raw1_sigma=o["raw1"][..., 3])


def main():
    torch.set_num_threads(1)
    RN = reference_module()
    RN.get_rays = V.get_rays
    RN.sample_pdf = V.sample_pdf
    out, bounds = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in V.CASES:
            c = V.case_inputs(case)
            ref = reference_render(RN, c, tmp)
            o32 = V.render_case(c, torch.float32)
            for k in STORED:
                assert o32[k].numpy().dtype == ref[k].dtype == np.float32 and np.array_equal(o32[k].numpy(), ref[k], equal_nan=False), \
                    f"{c.name}/{k}: checker != reference"
            o64 = V.render_case(c, torch.float64)
            assert all(torch.isfinite(o64[k]).all() for k in V.OUTPUTS), c.name
            acc = o64["acc_map"]
            if c.H * c.W > 1:
                assert acc.min() < 0.5 and acc.max() > 0.9, (c.name, float(acc.min()), float(acc.max()))
                # the largest compositing error of a case is a sample over its partially opaque rays (a ray that ends opaque has
                # acc_map = 1 whatever the rounding): with fewer than a handful the bound is a sample of one or two
                partial = int(((acc > 0.05) & (acc < 0.95)).sum())
                assert partial >= 4, (c.name, partial)
            else:
                assert 0.1 < acc.min() and acc.max() < 0.9, (c.name, float(acc.min()))
            keys = list(V.OUTPUTS) + ["raw1_rgb", "raw1_sigma"]
            b = {"acc_min": float(acc.min()), "acc_max": float(acc.max())}
            err = errors(with_raw(o32), with_raw(o64), keys + ([] if c.plain else ["z2"]))
            if not c.plain:
                last = V.sample_pdf.last            # of the float64 run's compute_samples_around_depth
                near_branch = (last.denom > 1e-6) & (last.denom < 1e-4) & (last.width != 0)
                assert not near_branch.any(), (c.name, last.denom[near_branch])
                z = o32["z_vals"]
                b["ties"] = int((z[:, 1:] == z[:, :-1]).sum())
                if c.name.startswith("clamped"):
                    assert b["ties"] > 0 and (o32["z2"][:, 0] == c.near).any() and (o32["z2"][:, -1] == c.far).any(), c.name
                g1 = V.render_case(c, torch.float64, raw1=o32["raw1"])
                g2 = V.render_case(c, torch.float64, z2=o32["z2"])
                for name, g, ks in (("given_raw1", g1, ["z2"]), ("given_z2", g2, list(V.OUTPUTS))):
                    e = errors(o32, g, ks)
                    b[name] = {k: {"bound": BOUND_FACTOR * v, "fp32_error": v} for k, v in e.items()}
            b.update({k: {"bound": BOUND_FACTOR * v, "fp32_error": v} for k, v in err.items()})
            bounds[c.name] = b
            for k in STORED:
                out[f"{c.name}/{k}"] = ref[k]
            print(f"{c.name}: acc in [{acc.min():.3f}, {acc.max():.3f}], ties {b.get('ties')}, fp32 errors "
                  + ", ".join(f"{k} {v:.2g}" for k, v in err.items()))
    out["cases"] = np.array(V.NAMES)
    path = os.path.join(HERE, "nerf_render.npz")
    save_stable(path, out)
    with open(os.path.join(HERE, "nerf_render_bounds.json"), "w") as f:
        json.dump({"factor": BOUND_FACTOR, "cases": bounds}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
