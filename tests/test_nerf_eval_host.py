"""Host tests of the NeRF test-view evaluation: the checker (tests/nerf_eval_ref.py) against what the reference's own
render_images_with_metrics / write_images_with_metrics recorded (tests/golden/nerf_eval.npz), the derived float64 bounds -- that they
can be met (two independent float64 SSIM formulations lie inside them) and that they bite (float32 arithmetic and nine mutations lie
outside) -- closed-form SSIM answers, the quantisers, and everything of scripts/nerf_test.py that needs no device."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import nerf_eval_ref as E
from nerf_eval_ref import bounds, evals, golden_npz  # noqa: F401  (fixtures)
from nerf_rpn_amd.scripts import nerf_test as X

SIZES = [(7, 7), (7, 40), (13, 9), (38, 38), (39, 69), (96, 130)]


@pytest.mark.parametrize("name", E.NAMES)
def test_fp32_checker_equals_the_reference_bit_for_bit(evals, golden_npz, name):
    c, _, f32, _ = evals(name)
    g = {k[len(name) + 1:]: v for k, v in golden_npz.items() if k.startswith(name + "/")}
    assert list(golden_npz["cases"]) == E.NAMES
    for i, m in enumerate(f32["frames"]):
        row = [np.nan if m[k] is None else m[k] for k in E.METRICS]
        assert np.array_equal(np.array(row), g["frame_metrics"][i], equal_nan=True), (i, row, g["frame_metrics"][i])
    mean = [f32["mean"].get(k, np.nan) for k in E.METRICS]
    assert np.array_equal(np.array(mean), g["mean_metrics"], equal_nan=True)
    assert np.array_equal(f32["rgbs"].numpy(), g["rgbs"]) and np.array_equal(f32["depths"].numpy(), g["depths"])
    assert np.array_equal(f32["rgb8"], g["rgb8"]) and np.array_equal(f32["depth16"], g["depth16"])
    assert g["rgb8"].dtype == np.uint8 and g["depth16"].dtype == np.uint16


@pytest.mark.parametrize("name", E.NAMES)
def test_orchestration_the_reference_recorded(evals, golden_npz, name):
    """File names, the lines of metrics.txt, and the separate depth tracker."""
    c, _, f32, _ = evals(name)
    sub = ("train_depth_" if c.plain else "test_images_") + "scene0000_00"
    want = [os.path.join(name, sub, f"{n}_{kind}") for n in range(c.frames) for kind in ("rgb.jpg", "d.png")]
    assert list(golden_npz[f"{name}/files"]) == want + [os.path.join(name, sub, "metrics.txt")]
    lines = list(golden_npz[f"{name}/metrics_txt"])
    assert X.format_metrics(X.mean_metrics(f32["frames"])) == "".join(ln + "\n" for ln in lines)
    assert [ln.split(":")[0] for ln in lines] == [k for k in E.METRICS if k in f32["mean"]]
    has = [m["depth_rmse"] is not None for m in f32["frames"]]
    if c.depth == "none":
        assert not any(has) and "depth_rmse" not in f32["mean"] and len(lines) == 3
    if c.depth == "some":           # depth_rmse is the mean over the one frame that has it, the others over both
        assert has == [True] + [False] * (c.frames - 1) and f32["mean"]["depth_rmse"] == f32["frames"][0]["depth_rmse"]
        assert f32["mean"]["psnr"] == (f32["frames"][0]["psnr"] + f32["frames"][1]["psnr"]) / 2.


@pytest.mark.parametrize("name", E.NAMES)
def test_case_bounds_are_the_measured_fp32_error(evals, bounds, name):
    _, targets, f32, _ = evals(name)
    c = evals(name)[0]
    f64 = E.eval_case(c, targets, torch.float64, form="windows")
    assert bounds["factor"] == 8.0
    for k, rec in bounds["cases"][name].items():
        pairs = [(a[k], b[k]) for a, b in zip(f32["frames"] + [f32["mean"]], f64["frames"] + [f64["mean"]]) if a.get(k) is not None]
        err = max(abs(a - b) for a, b in pairs)
        assert rec["fp32_error"] == pytest.approx(err, rel=0.25) and rec["bound"] == 8.0 * rec["fp32_error"] and 0 < rec["bound"] < 1e-3, (k, err)
    assert ("depth_rmse" in bounds["cases"][name]) == (c.depth != "none")


def test_derived_bound_is_the_committed_function():
    b = E.ssim_pixel_bound()
    print(f"ssim_pixel_bound {b:.4g}")
    assert 1e-10 < b < 1e-9 and b == pytest.approx((408. / E.C1 + 621. / E.C2) * E.U, rel=0.02)
    assert E.ssim_pixel_bound(u=2.0 ** -24) > 1e-2           # float32 arithmetic has no useful bound of this kind
    assert E.C1 == (0.01 * 1.0) ** 2 and E.C2 == (0.03 * 1.0) ** 2


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("noise", E.NOISES)
def test_both_fp64_formulations_lie_inside_the_derived_bound(hw, noise):
    f = E.synth_frame(*hw, noise)
    a, b = E.frame_ref(f, torch.float64, form="filter"), E.frame_ref(f, torch.float64, form="windows")
    windows = (hw[0] - 6) * (hw[1] - 6)
    print(f"{hw} noise {noise}: ssim {a['ssim']:.6f}, |filter - windows| {abs(a['ssim'] - b['ssim']):.3g}, bound {2 * E.ssim_bound(windows):.3g}")
    assert abs(a["ssim"] - b["ssim"]) <= 2. * E.ssim_bound(windows)
    E.check_against_fp64(a, b, *hw, name=f"{hw} {noise}")
    if noise == 0.0:
        assert a["img_loss"] == 0.0 and math.isinf(a["psnr"]) and abs(a["ssim"] - 1.0) <= E.ssim_bound(windows)


@pytest.mark.parametrize("name", E.NAMES)
def test_both_fp64_formulations_agree_on_the_golden_cases(evals, name):
    c, targets, _, f64 = evals(name)
    other = E.eval_case(c, targets, torch.float64, form="windows")
    for a, b in zip(f64["frames"], other["frames"]):
        E.check_against_fp64(a, b, c.H, c.W, name=name)


def test_fp32_arithmetic_cannot_pass_the_ssim_bound(evals):
    outside = []
    for name in E.NAMES:
        c, _, f32, f64 = evals(name)
        for a, b in zip(f32["frames"], f64["frames"]):
            err, bound = abs(a["ssim"] - b["ssim"]), 2. * E.ssim_bound((c.H - 6) * (c.W - 6))
            print(f"{name}: float32 ssim error {err:.3g}, derived bound {bound:.3g}")
            outside.append(err > bound)
    f = E.synth_frame(96, 130, 0.02)
    err = abs(E.frame_ref(f, torch.float32)["ssim"] - E.frame_ref(f, torch.float64)["ssim"])
    print(f"96x130: float32 ssim error {err:.3g}")
    assert any(outside) and err > 2. * E.ssim_bound(90 * 124)


def golden_frame(evals, name, i):
    c, (images, depths, valid), _, f64 = evals(name)
    rgb, depth = f64["maps"][i]
    return E.SimpleNamespace(H=c.H, W=c.W, rgb=rgb.float(), target=images[i], depth=depth.float(), target_depth=depths[i], valid=valid[i])


# mutation, the committed case that shows it, the metric it must move
@pytest.mark.parametrize("mutation, source, key", [
    ("cov_factor_1", "two_pass_9x8", "ssim"), ("window_5", "two_pass_9x8", "ssim"), ("no_crop", "plain_no_depth_7x10", "ssim"),
    ("k2_001", "nan_masked_8x9", "ssim"), ("data_range_255", "two_pass_9x8", "ssim"), ("channel_mean_first", "nan_masked_8x9", "ssim"),
    ("cov_factor_1", "synth", "ssim"), ("window_5", "synth", "ssim"), ("no_crop", "synth", "ssim"), ("k2_001", "synth", "ssim"),
    ("data_range_255", "synth", "ssim"), ("channel_mean_first", "synth", "ssim"),
    ("unclamped_ssim", "synth_over", "ssim"), ("clamped_img_loss", "synth_over", "img_loss"), ("clamped_img_loss", "synth_over", "psnr"),
    ("mask_by_multiplication", "nan_masked_8x9", "depth_rmse")])
def test_mutations_exceed_the_bounds(evals, bounds, mutation, source, key):
    f = E.synth_frame(13, 9, 0.02, over=source == "synth_over") if source.startswith("synth") else golden_frame(evals, source, 0)
    good, bad = E.frame_ref(f, torch.float64), E.frame_ref(f, torch.float64, mutation=mutation)
    n, windows = f.H * f.W * 3, (f.H - 6) * (f.W - 6)
    derived = {"ssim": 2. * E.ssim_bound(windows), "img_loss": 2. * E.mse_rel_bound(n) * good["img_loss"],
               "psnr": E.psnr_bound(good["psnr"], n), "depth_rmse": 2. * E.mse_rel_bound(max(good["n_valid"], 1)) * (good["depth_rmse"] or 0.)}[key]
    limit = max(derived, bounds["cases"][source][key]["bound"]) if source in E.NAMES else derived
    if mutation == "mask_by_multiplication":        # NaN times zero: the mutated metric is not even a number
        assert good["depth_rmse"] is not None and bad["depth_rmse"] is None
        return
    err = abs(bad[key] - good[key])
    print(f"{mutation} on {source}: {key} moves by {err:.3g}, bound {limit:.3g}")
    assert err > 10. * limit


def test_known_answers():
    x = E.synth_frame(13, 9, 0.0).target.numpy()
    for dt in (np.float32, np.float64):
        for form in ("filter", "windows"):
            assert E.structural_similarity(x, x, data_range=1., channel_axis=-1, dtype=dt, form=form) == pytest.approx(1.0, abs=1e-6 if dt == np.float32 else 1e-12)
    for a, b in ((0.25, 0.75), (0.0, 1.0), (0.5, 0.5), (0.125, 0.0)):       # two constant images: both variances and the covariance vanish
        im1, im2 = np.full((9, 11, 3), a, np.float32), np.full((9, 11, 3), b, np.float32)
        want = (2 * a * b + E.C1) / (a * a + b * b + E.C1)
        for form in ("filter", "windows"):
            got = E.structural_similarity(im1, im2, data_range=1., channel_axis=-1, dtype=np.float64, form=form)
            assert got == pytest.approx(want, abs=E.ssim_bound(15)), (a, b, form)


def test_quantiser_table_against_exact_arithmetic():
    x = E.quantiser_table()
    assert (x < 0).any() and (x > 1).any() and (x == 1).any()
    for q, fn, dt in ((255, E.to8b, np.uint8), (65535, E.to16b, np.uint16)):
        got = fn(x)
        assert got.dtype == dt
        for v, g in zip(x, got):
            c = min(max(Fraction(float(v)), Fraction(0)), Fraction(1))
            want = int(np.float32(float(q * c)))         # q * c has at most 40 significant bits: exact as a double, rounded once to float32
            assert int(g) == want, (float(v), int(g), want)
    assert E.to8b(np.float32([1.0, 0.999, 63 / 255]))[0] == 255 and E.to16b(np.float32([1.0]))[0] == 65535
    # both sides of a step are present
    assert len(set(E.to8b(x).tolist())) > 8 and len(set(E.to16b(x).tolist())) > 16


def test_parser_tasks_and_directories():
    p = X.build_parser()
    a = p.parse_args(["--expname", "e", "--ckpt_dir", "c", "--data_dir", "d", "--scene_id", "s", "--image_hw", "468", "624"])
    assert a.task == "test" and a.output_dir is None and X.result_dir(a) == os.path.join("c", "e", "test_images_s")
    b = p.parse_args(["--expname", "e", "--ckpt_dir", "c", "--scene_id", "s", "--task", "render_train_depth", "--N_samples", "64"])
    assert X.result_dir(b) == os.path.join("c", "e", "train_depth_s") and X.TASKS[b.task][0] == "transforms_train.json" and b.N_samples == 64
    assert X.result_dir(p.parse_args(["--output_dir", "o"])) == "o" and X.TASKS["test"][0] == "transforms_test.json"
    with pytest.raises(SystemExit):
        p.parse_args(["--task", "test_opt"])
    with pytest.raises(SystemExit, match="nerf_test: --expname"):
        X.main([])


def test_metrics_file_format_and_image_files(tmp_path):
    from PIL import Image
    frames = [dict(img_loss=0.25, psnr=6.0, ssim=0.5, depth_rmse=None, n_valid=0), dict(img_loss=0.75, psnr=2.0, ssim=0.25, depth_rmse=0.125, n_valid=3)]
    means = X.mean_metrics(frames)
    assert means == {"img_loss": 0.5, "psnr": 4.0, "ssim": 0.375, "depth_rmse": 0.125} and list(means) == list(E.METRICS)
    assert X.format_metrics(means) == "img_loss: 0.5\npsnr: 4.0\nssim: 0.375\ndepth_rmse: 0.125\n"
    assert X.format_metrics(X.mean_metrics(frames[:1])) == "img_loss: 0.25\npsnr: 6.0\nssim: 0.5\n"
    assert means == E.mean_metrics(frames)
    g = np.random.default_rng(0)
    rgb8, d16 = g.integers(0, 256, (8, 9, 3), dtype=np.uint8), g.integers(0, 65536, (8, 9), dtype=np.uint16)
    jpg, png = X.write_images(str(tmp_path), 4, rgb8, d16)
    assert (os.path.basename(jpg), os.path.basename(png)) == ("4_rgb.jpg", "4_d.png")
    back = np.asarray(Image.open(png))
    assert back.dtype == np.uint16 and np.array_equal(back, d16)
    img = Image.open(jpg)
    assert img.format == "JPEG" and img.size == (9, 8) and img.mode == "RGB"


def test_target_loader_matches_the_checker(evals, golden_npz, tmp_path):
    name = "two_pass_9x8"
    c, (images, depths, valid), _, _ = evals(name)
    argv = E.write_run(tmp_path, c, golden_npz[f"{name}/target_rgb8"], golden_npz[f"{name}/target_depth16"])
    a = X.build_parser().parse_args(argv)
    path = os.path.join(a.data_dir, a.scene_id, "transforms_test.json")
    _, _, _, meta = X.NR.load_transforms(path, with_meta=True)
    assert "depth_file_path" in meta["frames"][0] and "depth_file_path" not in meta["frames"][1]
    for i, fr in enumerate(meta["frames"]):
        img, d, v = X.load_targets(os.path.dirname(path), fr, c.H, c.W, meta["depth_scaling_factor"])
        assert img.dtype == np.float32 and np.array_equal(img, images[i].numpy())
        if i == 0:
            assert d.dtype == np.float32 and np.array_equal(d, depths[0].numpy()) and np.array_equal(v, valid[0].numpy()) and v.any() and not v.all()
        else:
            assert d is None and v is None
    with pytest.raises(SystemExit, match="--image_hw"):
        X.load_targets(os.path.dirname(path), meta["frames"][0], c.H + 1, c.W, 1000.0)
