"""Generate tests/golden/nerf_extract.npz and nerf_extract_bounds.json from the REFERENCE's data/scannet/run_nerf.py (build container
only: it reads the reference tree).

run_nerf.py is imported from the read-only tree with stand-ins in sys.modules for what it imports and this machine lacks or does not
need (``configargparse``, ``skimage``, ``lpips``, ``cv2``, ``torchvision``, tensorboard, and the Dense-Depth-Priors modules ``model``,
``data``, ``train_utils``, ``metric``).  The fork's ``NeRF`` and ``get_embedder`` are not on disk: the checker's classes
(tests/nerf_extract_ref.py) stand in for them -- the assumed model of DESIGN.md 3.16.  For every case of the checker a checkpoint
directory is written, the reference's own create_nerf / load_checkpoint load it (DataParallel's ``module.`` prefix included) and the
reference's own extract_nerf and get_scene_bounding_box run on the CPU.  Only recorded results are stored; no reference text.

nerf_extract.npz       <case>/rgbsigma (N, 4) float32, <case>/resolution, <case>/bbox_min, <case>/bbox_max
nerf_extract_cli.json  the reference parser's extract flags with their defaults and types
nerf_extract_bounds.json   per case: 8 x the largest |float32 checker in reference order - float64 checker| for rgb and for sigma
                       (the measured error is recorded next to it).  The float32 checker must equal the reference bit for bit
                       (asserted here) or nothing is written.

    python tests/golden/make_nerf_extract_golden.py       rewrites both files; the same bytes on every run
"""
import json
import os
import sys
import tempfile
import types
from argparse import Namespace

# the suite runs under MKL's reproducible branch (tests/conftest.py); the recorded bits must come from the same one
os.environ.setdefault("MKL_CBWR", "COMPATIBLE")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.dont_write_bytecode = True       # the reference tree is read-only

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_DIR = "/root/reference/data/scannet"
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_extract_ref as R                       # noqa: E402
from make_scannet_golden import save_stable        # noqa: E402

BOUND_FACTOR = 8.0
EXTRACT_FLAGS = ("expname", "ckpt_dir", "data_dir", "scene_id", "max_res", "extract_dir", "bbox_json")


def reference_module():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    import argparse

    class ConfigParser(argparse.ArgumentParser):      # configargparse's one extra keyword
        def add_argument(self, *a, is_config_file=False, **k):
            return super().add_argument(*a, **k)
    mod("configargparse", ArgumentParser=ConfigParser)
    mod("skimage")
    mod("skimage.metrics", structural_similarity=None)
    mod("lpips", LPIPS=None)
    mod("cv2")
    mod("torchvision")
    tb = mod("torch.utils.tensorboard", SummaryWriter=None)
    torch.utils.tensorboard = tb
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            mod("tqdm", tqdm=lambda it, *a, **k: it, trange=lambda *a, **k: range(*a))
    names = ("get_rays precompute_quadratic_samples sample_pdf img2mse mse2psnr to8b compute_depth_loss select_coordinates to16b "
             "resnet18_skip").split()
    mod("model", NeRF=R.NeRF, get_embedder=R.get_embedder, **{n: None for n in names})
    mod("data", **{n: None for n in ("create_random_subsets load_scene convert_depth_completion_scaling_to_m "
                                     "convert_m_to_depth_completion_scaling get_pretrained_normalize resize_sparse_depth").split()})
    mod("train_utils", MeanTracker=None, update_learning_rate=None)
    mod("metric", compute_rmse=None)
    sys.path.insert(0, REF_DIR)
    import run_nerf
    return run_nerf


def reference_extract(RN, c, tmp):
    """The reference's create_nerf + extract_nerf on one case -> (rgbsigma, resolution, bbox_min, bbox_max) as run_nerf() saves them."""
    exp = os.path.join(tmp, c.name)
    os.makedirs(exp)
    bbox_json = os.path.join(tmp, f"{c.name}_bbox.json")
    R.write_bbox_json(bbox_json, c.bbox)
    state = {"module." + k: v for k, v in c.state.items()}
    dummy = torch.optim.Adam([torch.nn.Parameter(v.clone()) for v in state.values()], lr=5e-4, betas=(0.9, 0.999))
    torch.save({"global_step": 100000, "network_fn_state_dict": state, "optimizer_state_dict": dummy.state_dict()},
               os.path.join(exp, "100000.tar"))
    args = Namespace(expname=c.name, ckpt_dir=tmp, no_reload=False, lrate=5e-4, netdepth=c.cfg["netdepth"], netwidth=c.cfg["netwidth"],
                     netdepth_fine=8, netwidth_fine=256, multires=c.cfg["multires"], multires_views=c.cfg["multires_views"],
                     i_embed=c.cfg["i_embed"], use_viewdirs=True, N_importance=0, input_ch_cam=c.cfg["input_ch_cam"],
                     netchunk_per_gpu=1024 * 64 * 4, n_gpus=1, perturb=1., N_samples=256, raw_noise_std=0., lindisp=False,
                     bb_center=c.bb_center, bb_scale=c.bb_scale, max_res=c.max_res, bbox_json=bbox_json)
    _, render_kwargs_test, _, _, _ = RN.create_nerf(args, {"precomputed_z_samples": None, "near": 0.1, "far": 5.0})
    rgbsigma, res, bbox_min, bbox_max = RN.extract_nerf(torch.Tensor(c.poses), args, render_kwargs_test)
    lo, hi = RN.get_scene_bounding_box(bbox_json)
    assert torch.equal(lo, bbox_min) and torch.equal(hi, bbox_max)
    return rgbsigma.cpu().numpy(), res, bbox_min.cpu().numpy(), bbox_max.cpu().numpy()


def main():
    torch.set_num_threads(1)
    RN = reference_module()
    out, bounds = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, case in enumerate(R.CASES):
            c = R.case_inputs(case, i)
            rgbsigma, res, lo, hi = reference_extract(RN, c, tmp)
            assert list(res) == case["res"] == c.res, (case["name"], res, c.res)
            args = (c.state, c.cfg, c.xs, c.ys, c.zs, c.bb_center, c.bb_scale, c.poses)
            f32 = R.extract(*args, dtype=torch.float32).numpy()
            assert f32.dtype == rgbsigma.dtype == np.float32 and np.array_equal(f32, rgbsigma), f"{case['name']}: checker != reference"
            f64 = R.extract(*args, dtype=torch.float64).numpy()
            err = np.abs(f32.astype(np.float64) - f64)
            e_rgb, e_sigma = float(err[:, :3].max()), float(err[:, 3].max())
            bounds[case["name"]] = {"rgb": BOUND_FACTOR * e_rgb, "sigma": BOUND_FACTOR * e_sigma, "fp32_error_rgb": e_rgb,
                                    "fp32_error_sigma": e_sigma, "sigma_min": float(f64[:, 3].min()), "sigma_max": float(f64[:, 3].max())}
            out[f"{case['name']}/rgbsigma"] = rgbsigma
            out[f"{case['name']}/resolution"] = np.array(res)
            out[f"{case['name']}/bbox_min"], out[f"{case['name']}/bbox_max"] = lo, hi
            print(f"{case['name']}: res {res}, P {case['P']}, fp32 error rgb {e_rgb:.3g} sigma {e_sigma:.3g}, sigma in "
                  f"[{f64[:, 3].min():.3g}, {f64[:, 3].max():.3g}]")
    out["cases"] = np.array([c["name"] for c in R.CASES])
    path = os.path.join(HERE, "nerf_extract.npz")
    save_stable(path, out)
    with open(os.path.join(HERE, "nerf_extract_bounds.json"), "w") as f:
        json.dump({"factor": BOUND_FACTOR, "cases": bounds}, f, indent=1)
        f.write("\n")
    flags = {a.dest: {"default": a.default, "type": getattr(a.type, "__name__", None)} for a in RN.config_parser()._actions
             if a.dest in EXTRACT_FLAGS}
    assert sorted(flags) == sorted(EXTRACT_FLAGS)
    with open(os.path.join(HERE, "nerf_extract_cli.json"), "w") as f:
        json.dump(flags, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
