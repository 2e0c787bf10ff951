"""Generate tests/golden/nerf_eval.npz and nerf_eval_bounds.json from the REFERENCE's data/scannet/run_nerf.py (build container only:
it reads the reference tree).

run_nerf.py is imported as make_nerf_extract_golden.py imports it.  What it takes from the Dense-Depth-Priors fork and from packages
this machine lacks is set to the checker's definitions (tests/nerf_eval_ref.py, tests/nerf_render_ref.py -- the assumptions of
DESIGN.md 3.16 - 3.18): get_rays, sample_pdf, structural_similarity, img2mse, mse2psnr, compute_rmse, MeanTracker, to8b, to16b; LPIPS is
a stand-in that returns zeros; cv2.cvtColor / cv2.imwrite are stand-ins that record the arrays they are handed.  For every case the
reference's own create_nerf, render_images_with_metrics and write_images_with_metrics then run on the CPU.  What this pins is the
reference's orchestration: which tensor is clamped before which metric, depth / far, the channel order handed to imwrite, the
separate depth tracker, the file names and the lines of metrics.txt.

SSIM IS NOT PINNED BY THE REFERENCE HERE: skimage is not installed, so the recorded ``ssim`` is the checker's own float32 value.  It is
pinned by the checker's two formulations agreeing and by closed-form answers (tests/test_nerf_eval_host.py).

nerf_eval.npz          per case <name>/: the inputs target_rgb8 [F, H, W, 3] uint8 and target_depth16 [F, H, W] uint16 (0 = invalid);
                       what the reference returned and wrote: frame_metrics [F, 4] and mean_metrics [4] float64 in the order img_loss,
                       psnr, ssim, depth_rmse (NaN = absent), rgbs [F, 3, H, W], depths [F, 1, H, W] float32, rgb8 [F, H, W, 3] (what
                       cvtColor was handed), depth16 [F, H, W] (what imwrite was handed), files, metrics_txt (its lines but lpips').
nerf_eval_bounds.json  "cases": per case and metric 8 x the largest |float32 checker - float64 checker| over the frames and the mean,
                       the measured float32 error next to it; "derived": the derived float64 bounds of the checker at this build;
                       "gpu_measured": errors recorded on the MI355X, carried over from the existing file (tools/nerf_eval_profile.py
                       writes them).

The float32 checker must equal the reference bit for bit in every stored value (asserted) or nothing is written.

    python tests/golden/make_nerf_eval_golden.py [--gpu-errors FILE]      rewrites both files; the same bytes on every run
--gpu-errors FILE replaces the "gpu_measured" section by the file tools/nerf_eval_profile.py --errors-out wrote.
"""
import json
import math
import os
import sys
import tempfile
import types
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

import nerf_eval_ref as E                                   # noqa: E402
import nerf_render_ref as V                                 # noqa: E402
from make_nerf_extract_golden import reference_module       # noqa: E402
from make_scannet_golden import save_stable                 # noqa: E402

BOUND_FACTOR = 8.0
COLOR_RGB2BGR = 4


class RecordingTracker(E.MeanTracker):
    instances = []

    def __init__(self):
        super().__init__()
        RecordingTracker.instances.append(self)


def reference_test(RN, c, targets, tmp, task):
    """The reference's test task on one case -> dict of what it computed and wrote."""
    images, depths, valid = targets
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
                     bb_center=c.bb_center, bb_scale=c.bb_scale, chunk=1024 * 64, task=task, scene_id="scene0000_00")
    _, kw, _, _, _ = RN.create_nerf(args, {"precomputed_z_samples": c.z_samples, "near": c.near, "far": c.far})
    handed = {"cvt": [], "write": []}

    def cvt_color(arr, code):
        assert code == COLOR_RGB2BGR
        handed["cvt"].append(arr)
        return arr[..., ::-1]

    def imwrite(path, arr):
        handed["write"].append((path, arr))
        return True
    RN.cv2 = types.SimpleNamespace(cvtColor=cvt_color, imwrite=imwrite, COLOR_RGB2BGR=COLOR_RGB2BGR)
    RecordingTracker.instances = []
    lpips = lambda a, b, normalize: torch.zeros(1, 1, 1, 1)       # noqa: E731
    intrinsics = c.intrinsic.unsqueeze(0).expand(c.frames, 4)
    mean, res = RN.render_images_with_metrics(None, np.arange(c.frames), images, depths.unsqueeze(-1), valid, c.poses, c.H, c.W,
                                              intrinsics, lpips, args, kw)
    RN.write_images_with_metrics(res, mean, c.far, args)
    per_frame, depth_frames = RecordingTracker.instances[0].history, RecordingTracker.instances[1].history
    assert len(per_frame) == c.frames
    result_dir = os.path.join(tmp, c.name, ("test_images_" if task == "test" else "train_depth_") + "scene0000_00")
    with open(os.path.join(result_dir, "metrics.txt")) as f:
        lines = [ln for ln in f.read().splitlines() if not ln.startswith("lpips")]
    rgb_writes, d_writes = handed["write"][0::2], handed["write"][1::2]
    for a, (_, w) in zip(handed["cvt"], rgb_writes):
        assert np.array_equal(a[..., ::-1], w)            # imwrite is handed BGR: the file holds the frame in RGB order
    assert all(w.shape == (c.H, c.W, 1) for _, w in d_writes)
    means = mean.as_dict()
    return dict(frames=per_frame, depth_frames=depth_frames, mean={k: float(means[k]) for k in E.METRICS if k in means}, rgbs=res["rgbs"],
                depths=res["depths"], rgb8=np.stack(handed["cvt"]), depth16=np.stack([w[..., 0] for _, w in d_writes]),       # imwrite is handed (H, W, 1)
                files=[os.path.relpath(p, tmp) for p, _ in handed["write"]] + [os.path.join(os.path.relpath(result_dir, tmp), "metrics.txt")],
                lines=lines)


def row(m):
    return [float("nan") if m.get(k) is None else float(m[k]) for k in E.METRICS]


def main():
    torch.set_num_threads(1)
    RN = reference_module()
    RN.get_rays, RN.sample_pdf = V.get_rays, V.sample_pdf
    RN.structural_similarity = E.structural_similarity
    RN.img2mse, RN.mse2psnr, RN.compute_rmse, RN.to8b, RN.to16b = E.img2mse, E.mse2psnr, E.compute_rmse, E.to8b, E.to16b
    RN.MeanTracker = RecordingTracker
    out, bounds = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in E.CASES:
            c = E.case_inputs(case)
            rgb8, raw16 = E.make_targets(c)
            targets = E.load_targets(c, rgb8, raw16)
            task = "render_train_depth" if c.plain else "test"
            ref = reference_test(RN, c, targets, tmp, task)
            f32 = E.eval_case(c, targets, torch.float32)
            f64 = E.eval_case(c, targets, torch.float64, form="windows")
            # the float32 checker against the reference, bit for bit
            depth_it = iter(ref["depth_frames"])
            for got, want in zip(f32["frames"], ref["frames"]):
                for k in ("img_loss", "psnr", "ssim"):
                    assert got[k] == float(want[k]), (c.name, k, got[k], want[k])
                if got["depth_rmse"] is not None:
                    assert got["depth_rmse"] == next(depth_it)["depth_rmse"], c.name
            assert next(depth_it, None) is None, c.name
            assert f32["mean"] == ref["mean"] and list(f32["mean"]) == list(ref["mean"]), (c.name, f32["mean"], ref["mean"])
            assert torch.equal(f32["rgbs"], ref["rgbs"]) and torch.equal(f32["depths"], ref["depths"]), c.name
            assert np.array_equal(f32["rgb8"], ref["rgb8"]) and np.array_equal(f32["depth16"], ref["depth16"]), c.name
            assert ref["depth16"].dtype == np.uint16 and ref["rgb8"].dtype == np.uint8
            assert ref["lines"] == [f"{k}: {v}" for k, v in f32["mean"].items()], (c.name, ref["lines"])
            # what the cases are for
            has = [m["depth_rmse"] is not None for m in f32["frames"]]
            assert {"some": has[0] and not any(has[1:]), "none": not any(has), "nan": all(has)}[c.depth], (c.name, has)
            if c.depth == "nan":
                assert not torch.isfinite(targets[1][~targets[2]]).any() and (~targets[2]).any()
            err = {}
            for k in E.METRICS:
                pairs = [(a[k], b[k]) for a, b in zip(f32["frames"] + [f32["mean"]], f64["frames"] + [f64["mean"]]) if a.get(k) is not None]
                if pairs:
                    e = max(abs(a - b) for a, b in pairs)
                    err[k] = {"bound": BOUND_FACTOR * e, "fp32_error": e}
            bounds[c.name] = err
            pre = c.name + "/"
            out.update({pre + "target_rgb8": rgb8, pre + "target_depth16": raw16,
                        pre + "frame_metrics": np.array([row(dict(m, depth_rmse=g["depth_rmse"])) for m, g in zip(ref["frames"], f32["frames"])]),
                        pre + "mean_metrics": np.array(row(ref["mean"])), pre + "rgbs": ref["rgbs"].numpy(), pre + "depths": ref["depths"].numpy(),
                        pre + "rgb8": ref["rgb8"], pre + "depth16": ref["depth16"], pre + "files": np.array(ref["files"]),
                        pre + "metrics_txt": np.array(ref["lines"])})
            print(f"{c.name}: " + ", ".join(f"{k} {v}" for k, v in f32["mean"].items()) + "; fp32 errors "
                  + ", ".join(f"{k} {v['fp32_error']:.2g}" for k, v in err.items()))
    out["cases"] = np.array(E.NAMES)
    path = os.path.join(HERE, "nerf_eval.npz")
    bpath = os.path.join(HERE, "nerf_eval_bounds.json")
    measured = {}
    if os.path.exists(bpath):
        with open(bpath) as f:
            measured = json.load(f).get("gpu_measured", {})
    if "--gpu-errors" in sys.argv:
        with open(sys.argv[sys.argv.index("--gpu-errors") + 1]) as f:
            measured = json.load(f)
    save_stable(path, out)
    derived = {"u": E.U, "ssim_pixel_bound": E.ssim_pixel_bound(), "ssim_pixel_bound_first_order": (408. / E.C1 + 621. / E.C2) * E.U}
    assert math.isclose(derived["ssim_pixel_bound"], derived["ssim_pixel_bound_first_order"], rel_tol=0.05)
    with open(bpath, "w") as f:
        json.dump({"factor": BOUND_FACTOR, "cases": bounds, "derived": derived, "gpu_measured": measured}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
