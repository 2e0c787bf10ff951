"""Checker of the NeRF test-view evaluation (scripts/nerf_test.py, ops.nerf_view_metrics, csrc/nerfmetrics.hip): the project's own
restatement, with a dtype and a mutation argument, of what the reference's data/scannet/run_nerf.py computes per held-out view
(render_images_with_metrics :231-311, write_images_with_metrics :313-331) and of what it imports for that from code that is not on
disk -- the assumed definitions of DESIGN.md 3.18:
  * img2mse, mse2psnr, to8b, to16b (the fork's model.py), compute_rmse (metric.py), MeanTracker (train_utils.py),
  * skimage.metrics.structural_similarity with its defaults, in two independent formulations: scipy's uniform_filter over the whole
    image followed by skimage's crop (``ssim_filter``), and plain sums over the 7 x 7 windows that lie inside the image
    (``ssim_windows``).
float32 is what the reference's torch / skimage code computes on float32 frames (skimage keeps float32 images in float32); float64 is
the reference the GPU tests are bounded against.  float32 inputs are widened, never recomputed.

The bounds (``ssim_pixel_bound`` and the functions after it) are derived, not measured; the derivation is in their docstrings.
Host-only numpy / scipy / torch.
"""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nerf_extract_ref as R
import nerf_render_ref as V

WIN, K1, K2 = 7, 0.01, 0.03
MUTATIONS = ("cov_factor_1", "window_5", "no_crop", "k2_001", "data_range_255", "channel_mean_first", "unclamped_ssim",
             "mask_by_multiplication", "clamped_img_loss")
METRICS = ("img_loss", "psnr", "ssim", "depth_rmse")


# ----------------------------------------------------------------------------------------------------------------------
# the assumed functions of the fork (float32 torch / numpy, as the reference calls them)
# ----------------------------------------------------------------------------------------------------------------------
def img2mse(x, y):
    return torch.mean((x - y) ** 2)


def mse2psnr(x):
    return -10. * torch.log(x) / torch.log(torch.full((1,), 10., dtype=x.dtype))


def compute_rmse(prediction, target):
    return torch.sqrt((prediction - target).pow(2).mean())


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def to16b(x):
    return ((2 ** 16 - 1) * np.clip(x, 0, 1)).astype(np.uint16)


class MeanTracker:
    """Running means per key; ``print`` writes one ``key: value`` line per key in insertion order.  ``history`` (not in the fork)
    keeps what every add was handed, which is how the golden script records the reference's per-frame metrics."""
    def __init__(self):
        self.sums, self.counts, self.history = {}, {}, []

    def add(self, values, weight=1.):
        self.history.append(dict(values))
        for k, v in values.items():
            self.sums[k] = self.sums.get(k, 0.) + v * weight
            self.counts[k] = self.counts.get(k, 0.) + weight

    def has(self, key):
        return key in self.sums

    def get(self, key):
        return self.sums[key] / self.counts[key]

    def as_dict(self):
        return {k: self.get(k) for k in self.sums}

    def print(self, f=None):
        for k in self.sums:
            print("{}: {}".format(k, self.get(k)), file=f)


# ----------------------------------------------------------------------------------------------------------------------
# structural similarity, two formulations
# ----------------------------------------------------------------------------------------------------------------------
def _ssim_terms(ux, uy, uxx, uyy, uxy, win, cov_factor, k2, data_range):
    NP = win ** 2
    cov_norm = NP / (NP - 1) if cov_factor is None else cov_factor
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * data_range) ** 2, (k2 * data_range) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def ssim_filter(x, y, dtype=np.float64, win=WIN, cov_factor=None, k2=K2, data_range=1., crop=True):
    """skimage's own steps for one channel: uniform_filter (reflecting borders) of x, y, xx, yy, xy, the SSIM map, its crop by
    (win - 1) // 2, the float64 mean."""
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    S = _ssim_terms(uniform_filter(x, size=win), uniform_filter(y, size=win), uniform_filter(x * x, size=win),
                    uniform_filter(y * y, size=win), uniform_filter(x * y, size=win), win, cov_factor, k2, data_range)
    assert S.dtype == dtype
    pad = (win - 1) // 2
    return (S[pad:-pad, pad:-pad] if crop else S).mean(dtype=np.float64)


def ssim_windows(x, y, dtype=np.float64, win=WIN, cov_factor=None, k2=K2, data_range=1.):
    """The valid-window form (what the kernel evaluates): the means are sums over each win x win window inside the image / win^2."""
    from numpy.lib.stride_tricks import sliding_window_view
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)

    def mean(a):
        return sliding_window_view(a, (win, win)).sum(axis=(-1, -2), dtype=dtype) / dtype(win * win)
    S = _ssim_terms(mean(x), mean(y), mean(x * x), mean(y * y), mean(x * y), win, cov_factor, k2, data_range)
    assert S.dtype == dtype
    return S.mean(dtype=np.float64)


def structural_similarity(im1, im2, *, data_range, channel_axis, dtype=None, form="filter", **kw):
    """The call of run_nerf.py:287 (skimage's signature): per-channel mean SSIM, then the mean over the channels.  skimage computes a
    float32 image pair in float32 -- ``dtype`` None follows that rule."""
    assert channel_axis == -1 and im1.shape == im2.shape and min(im1.shape[:2]) >= WIN
    dtype = (np.float32 if im1.dtype == np.float32 else np.float64) if dtype is None else dtype
    fn = ssim_filter if form == "filter" else ssim_windows
    per_channel = np.array([fn(im1[..., c], im2[..., c], dtype, data_range=data_range, **kw) for c in range(im1.shape[-1])])
    return per_channel.mean()


# ----------------------------------------------------------------------------------------------------------------------
# one frame's metrics and images
# ----------------------------------------------------------------------------------------------------------------------
def frame_metrics(rgb, target, depth=None, target_depth=None, valid=None, dtype=torch.float32, mutation=None, form="filter"):
    """render_images_with_metrics :276-296 for one frame, on float32 torch tensors carried in ``dtype`` -> dict of Python numbers
    img_loss, psnr, ssim, depth_rmse (None where the reference adds nothing to its depth tracker) and n_valid."""
    assert mutation is None or mutation in MUTATIONS
    np_dt = np.float32 if dtype == torch.float32 else np.float64
    rgb, target = rgb.to(dtype), target.to(dtype)
    out = {"depth_rmse": None, "n_valid": 0}
    if depth is not None:
        valid = valid.bool()
        out["n_valid"] = int(valid.sum())
        if mutation == "mask_by_multiplication":
            m = valid.to(dtype)
            rmse = torch.sqrt(((depth.to(dtype) * m - target_depth.to(dtype) * m) ** 2).sum() / m.sum())
        else:
            rmse = compute_rmse(depth.to(dtype)[valid], target_depth.to(dtype)[valid])
        if not torch.isnan(rmse):
            out["depth_rmse"] = rmse.item()
    clamped = torch.clamp(rgb, 0, 1)
    img_loss = img2mse(clamped if mutation == "clamped_img_loss" else rgb, target)
    if dtype == torch.float32:
        psnr = mse2psnr(img_loss).item()
    else:
        psnr = -10. * math.log10(img_loss.item()) if img_loss.item() > 0. else math.inf
    a, b = (rgb if mutation == "unclamped_ssim" else clamped).numpy(), target.numpy()
    kw = {"cov_factor_1": dict(cov_factor=1.), "window_5": dict(win=5), "no_crop": dict(crop=False), "k2_001": dict(k2=0.01)}.get(mutation, {})
    data_range = 255. if mutation == "data_range_255" else 1.
    if mutation == "channel_mean_first":
        a, b = a.mean(-1, keepdims=True), b.mean(-1, keepdims=True)
    if mutation in ("no_crop", "window_5"):
        form = "filter"
    ssim = structural_similarity(a, b, data_range=data_range, channel_axis=-1, dtype=np_dt, form=form, **kw)
    out.update(img_loss=img_loss.item(), psnr=psnr, ssim=float(ssim))
    return out


def frame_images(rgb, depth, far):
    """:291, :293 and :325, :327: the clamped frame and depth / far as float32 tensors, quantised as write_images_with_metrics does
    (float32 division, the reference's on the CPU) -> (uint8 [H, W, 3], uint16 [H, W])."""
    return to8b(torch.clamp(rgb, 0., 1.).numpy()), to16b((depth / far).numpy())


def mean_metrics(frames):
    """The two trackers of :251-252 and their union :309-310: depth_rmse is averaged over the frames that have one and absent if none
    has -> dict in the order metrics.txt lists them."""
    tracker, depth_tracker = MeanTracker(), MeanTracker()
    for m in frames:
        if m["depth_rmse"] is not None:
            depth_tracker.add({"depth_rmse": m["depth_rmse"]})
        tracker.add({k: m[k] for k in ("img_loss", "psnr", "ssim")})
    return {**tracker.as_dict(), **depth_tracker.as_dict()}


# ----------------------------------------------------------------------------------------------------------------------
# derived bounds
# ----------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -53
C1, C2 = (K1 * 1.) ** 2, (K2 * 1.) ** 2


def gamma(k, u=U):
    """Higham's gamma_k: a sum of k + 1 non-negative terms added in any order has relative error at most gamma_k."""
    return k * u / (1. - k * u)


def ssim_pixel_bound(u=U, n=WIN * WIN, c1=C1, c2=C2):
    """Bound on |S computed - S exact| for one window and channel, for any float64 evaluation that forms the five window moments as
    sums of the n = 49 terms (in any order) divided by n and then follows skimage's expressions operation by operation; x and y are
    float32 values in [0, 1] widened to float64.

    1. Moments.  x, y and the products xx, yy, xy are exact in float64 (a product of two 24-bit significands has 48 bits).  A sum of n
       non-negative terms has relative error <= gamma_{n-1}, the division adds one rounding: relative error <= gamma_n, and since each
       moment is <= 1 the absolute error of ux, uy, uxx, uyy, uxy is  e = gamma_n.
    2. Products of means.  fl(ux ux), fl(ux uy), fl(uy uy) are off by <= 2 e + e^2 + u (1 + e)^2 <= 2 e + 1.01 u.
    3. Variances.  uxx - ux ux is off by <= e + (2 e + 1.01 u) + u (the subtraction's rounding, result <= 1).  The factor
       c = n / (n - 1) is itself rounded and its product rounded once more, on a true value <= 1 / 4 (a covariance of values in
       [0, 1]): vx, vy, vxy are off by <= c (3 e + 3.02 u)(1 + 2 u) + c u / 2 <= ev = c (3 e + 4 u).
    4. A1 = 2 ux uy + C1 and B1 = ux^2 + uy^2 + C1 (values <= 2.0001): off by <= 2 (2 e + 1.01 u) + 2 * 2.0001 u <= e1 = 4 e + 8 u.
       A2 = 2 vxy + C2 and B2 = vx + vy + C2 (values <= 0.52): off by <= e2 = 2 ev + 2 u.
    5. Quotients.  With r = A / B, |r1| <= 1 (2 ab <= a^2 + b^2) and |r2| <= 1 (Cauchy-Schwarz), and the computed B >= C - eB:
       |A^ / B^ - A / B| <= (eA + |r| eB) / B^ <= d = 2 eX / (C - eX), X = 1 with C1 and X = 2 with C2.
    6. S = (A1 A2) / (B1 B2) = r1 r2 with three more roundings on a value <= 1 + d:  |S^ - S| <= d1 + d2 + d1 d2 + 4 u.
    The divisions by C1 = 1e-4 and C2 = 9e-4 dominate: the bound is about (408 / C1 + 621 / C2) u."""
    e = gamma(n, u)
    c = n / (n - 1.)
    ev = c * (3. * e + 4. * u)
    e1, e2 = 4. * e + 8. * u, 2. * ev + 2. * u
    d1, d2 = 2. * e1 / (c1 - e1), 2. * e2 / (c2 - e2)
    return d1 + d2 + d1 * d2 + 4. * u


def ssim_bound(windows):
    """One evaluation's mean SSIM against the exact one: the per-window bound, plus the mean of 3 * windows terms of magnitude <= 1
    + d added in any order (absolute error <= gamma of the number of terms) and the divisions."""
    return ssim_pixel_bound() + 2. * gamma(3 * windows + 4)


def mse_rel_bound(n):
    """Relative error of a float64 mean of n squared differences of widened float32 values: the difference and the square round once
    each (relative 2 u + u on the term), the n non-negative terms add in any order (gamma_{n-1}), one division: <= gamma_{n+3}.  The
    square root of depth_rmse halves it and rounds once more, which the same figure covers."""
    return gamma(n + 3)


def psnr_bound(psnr, n):
    """-10 log10 of two values with relative distance r differ by 10 / ln 10 * r (1 + r); log10 and the product are taken as good to
    two units in the last place of the result on each side."""
    r = 2. * mse_rel_bound(n)
    return 10. / math.log(10.) * r * (1. + r) + 8. * U * abs(psnr)


def check_against_fp64(got, ref, H, W, report=print, name=""):
    """got: ops.nerf_view_metrics' dict; ref: frame_metrics(..., torch.float64, form='windows').  Two float64 evaluations are each
    within the derived bound of the exact value, so they are within twice it of each other.  Prints every figure, then asserts."""
    n, windows = H * W * 3, (H - WIN + 1) * (W - WIN + 1)
    bad = []

    def one(key, err, bound):
        report(f"{name}: {key} error {err:.3g} (derived bound {bound:.3g})")
        if not err <= bound:
            bad.append((key, err, bound))
    one("img_loss", abs(got["img_loss"] - ref["img_loss"]), 2. * mse_rel_bound(n) * ref["img_loss"])
    if math.isinf(ref["psnr"]):
        one("psnr", 0. if got["psnr"] == ref["psnr"] else math.inf, 0.)
    else:
        one("psnr", abs(got["psnr"] - ref["psnr"]), psnr_bound(ref["psnr"], n))
    one("ssim", abs(got["ssim"] - ref["ssim"]), 2. * ssim_bound(windows))
    assert got["n_valid"] == ref["n_valid"], (name, got["n_valid"], ref["n_valid"])
    assert (got["depth_rmse"] is None) == (ref["depth_rmse"] is None), (name, got["depth_rmse"], ref["depth_rmse"])
    if ref["depth_rmse"] is not None:
        one("depth_rmse", abs(got["depth_rmse"] - ref["depth_rmse"]), 2. * mse_rel_bound(ref["n_valid"]) * ref["depth_rmse"])
    assert not bad, (name, bad)


# ----------------------------------------------------------------------------------------------------------------------
# seeded synthetic frames (the GPU tests and the sharpness tests)
# ----------------------------------------------------------------------------------------------------------------------
NOISES = (0.0, 0.02, 0.2)


def synth_frame(H, W, noise, seed=0, depth=True, over=False):
    """target: a smooth float32 image in [0, 1] on the k / 255 grid with texture; rgb = target + noise * normal, unclamped (at noise
    0.2 a good part of it lies outside [0, 1]); ``over`` adds 0.5 to a patch so that rgb > 1 whatever the noise.  depth in [0.5, 4],
    target_depth = depth + 5 noise * normal, valid on about half the pixels -> SimpleNamespace of float32 / bool torch tensors."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W)
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ph = torch.rand(3, 4, generator=g) * 6.28
    base = torch.stack([0.5 + 0.3 * torch.sin(0.23 * u + ph[c, 0]) * torch.cos(0.31 * v + ph[c, 1]) + 0.1 * torch.sin(1.7 * u + 1.1 * v + ph[c, 2])
                        for c in range(3)], -1)
    target = torch.round((base + 0.08 * (torch.rand(H, W, 3, generator=g) - 0.5)).clamp(0, 1) * 255) / 255
    rgb = target + noise * torch.randn(H, W, 3, generator=g)
    if over:
        rgb[: max(H // 2, 4), : max(W // 2, 4)] += 0.5
    out = SimpleNamespace(H=H, W=W, rgb=rgb.float().contiguous(), target=target.float().contiguous(), depth=None, target_depth=None,
                          valid=None, far=4.0)
    if depth:
        out.depth = (0.5 + 3.5 * torch.rand(H, W, generator=g)).float()
        out.target_depth = (out.depth + 5. * noise * torch.randn(H, W, generator=g)).float()
        out.valid = torch.rand(H, W, generator=g) < 0.5
    return out


def quantiser_table():
    """float32 values below 0, above 1, at 0 and 1, next to 1, and on both sides of k / 255 and k / 65535 for a spread of k."""
    vals = [-1., -0., 0., 1e-8, 0.5, 1., 2., float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2)))]
    for q, ks in ((255, (1, 2, 3, 63, 127, 128, 200, 254)), (65535, (1, 2, 255, 256, 257, 32767, 32768, 40000, 65534))):
        for k in ks:
            x = np.float32(k / q)
            vals += [float(x), float(np.nextafter(x, np.float32(0))), float(np.nextafter(x, np.float32(2)))]
    return np.array(vals, dtype=np.float32)


def frame_ref(f, dtype=torch.float32, mutation=None, form="filter"):
    return frame_metrics(f.rgb, f.target, f.depth, f.target_depth, f.valid, dtype=dtype, mutation=mutation, form=form)


# ----------------------------------------------------------------------------------------------------------------------
# the golden cases: tiny NeRF runs, built like those of tests/nerf_render_ref.py, with targets
# ----------------------------------------------------------------------------------------------------------------------
DEPTH_SCALING = 1000.0
# name, frame, samples, near / far, frames; depth: "some" = frame 0 has valid depths and the later frames have none (the separate depth
# tracker then averages over fewer frames), "none" = no valid pixel anywhere, "nan" = NaN / inf in the unselected targets
CASES = [
    dict(name="two_pass_9x8", H=9, W=8, N=16, near=0.1, far=4.0, frames=2, depth="some", seed=61),
    dict(name="plain_no_depth_7x10", H=7, W=10, N=12, near=0.1, far=4.0, frames=1, depth="none", plain=True, seed=62),
    dict(name="nan_masked_8x9", H=8, W=9, N=16, near=0.1, far=4.0, frames=2, depth="nan", seed=63),
]
NAMES = [c["name"] for c in CASES]


def case_inputs(case):
    """Everything of a case but its targets, regenerated from seeds: one network, ``frames`` poses."""
    index = NAMES.index(case["name"])
    cfg = dict(R.DEFAULT_CFG)
    H, W = case["H"], case["W"]
    focal = 1.2 * max(H, W, 3)
    intrinsic = torch.tensor([focal, focal * 1.03, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.125], dtype=torch.float32)
    plain = case.get("plain", False)
    z_samples = None if plain else V.precompute_quadratic_samples(case["near"], case["far"], case["N"] // 2)
    return SimpleNamespace(name=case["name"], cfg=cfg, H=H, W=W, intrinsic=intrinsic, poses=R.make_poses(500 + index, case["frames"]),
                           near=case["near"], far=case["far"], bb_center=torch.tensor([0.11, -0.07, 0.9]),
                           bb_scale=torch.tensor(2.0 / 13.0), state=V.make_state(case["seed"], cfg, V.SIGMA_SCALE), z_samples=z_samples,
                           n_samples=case["N"], lindisp=False, embedded_cam=None, plain=plain, frames=case["frames"], depth=case["depth"])


def render_frame(c, i, dtype=torch.float32):
    """-> (rgb_map [H, W, 3], depth_map [H, W]) of frame i in ``dtype``."""
    o = V.render(c.state, c.cfg, c.near, c.far, c.bb_center, c.bb_scale, z_samples=c.z_samples, n_samples=c.n_samples, H=c.H, W=c.W,
                 intrinsic=c.intrinsic, c2w=c.poses[i], lindisp=c.lindisp, dtype=dtype)
    return o["rgb_map"].reshape(c.H, c.W, 3), o["depth_map"].reshape(c.H, c.W)


def make_targets(c):
    """Targets for a case, made once by the golden script and stored: the float64 render plus seeded noise, quantised as an 8-bit image
    and a 16-bit depth file in millimetres would hold them -> (uint8 [F, H, W, 3], uint16 [F, H, W])."""
    g = torch.Generator().manual_seed(900 + NAMES.index(c.name))
    rgb8, raw16 = [], []
    for i in range(c.frames):
        rgb, depth = render_frame(c, i, torch.float64)
        rgb8.append(torch.round((rgb + 0.05 * torch.randn(rgb.shape, generator=g, dtype=torch.float64)).clamp(0, 1) * 255).to(torch.uint8))
        raw = torch.round((depth * (1. + 0.03 * torch.randn(depth.shape, generator=g, dtype=torch.float64))).clamp(0.001, 60.) * DEPTH_SCALING)
        keep = torch.rand(depth.shape, generator=g) < 0.6
        if c.depth == "none" or (c.depth == "some" and i > 0):
            keep = torch.zeros_like(keep)
        raw16.append(torch.where(keep, raw, torch.zeros_like(raw)).to(torch.int32))
    return torch.stack(rgb8).numpy(), torch.stack(raw16).numpy().astype(np.uint16)


def load_targets(c, rgb8, raw16):
    """The loader's assumed conversions: image / 255 and depth / depth_scaling_factor in float64, stored as float32;
    valid = raw > 0.  The "nan" case then overwrites its unselected depths with NaN and inf alternately.
    -> float32 [F, H, W, 3], float32 [F, H, W], bool [F, H, W] torch tensors."""
    images = torch.from_numpy((rgb8.astype(np.float64) / 255.).astype(np.float32))
    depths = (raw16.astype(np.float64) / DEPTH_SCALING).astype(np.float32)
    valid = raw16 > 0
    if c.depth == "nan":
        bad = np.where(np.arange(depths.size).reshape(depths.shape) % 2 == 0, np.float32(np.nan), np.float32(np.inf))
        depths = np.where(valid, depths, bad)
    return images, torch.from_numpy(depths), torch.from_numpy(valid)


def eval_case(c, targets, dtype=torch.float32, form="filter"):
    """The test task on a case in ``dtype``: per frame the render, its metrics and (float32 only meaningful) the quantised images ->
    dict(frames=[metrics dicts], mean=dict, rgbs=[F, 3, H, W], depths=[F, 1, H, W] as the reference returns them, rgb8, depth16,
    maps=[(rgb_map, depth_map) per frame])."""
    images, depths, valid = targets
    frames, rgbs, ds, rgb8, d16, maps = [], [], [], [], [], []
    for i in range(c.frames):
        rgb, depth = render_frame(c, i, dtype)
        maps.append((rgb, depth))
        frames.append(frame_metrics(rgb, images[i], depth, depths[i], valid[i], dtype=dtype, form=form))
        rgbs.append(torch.clamp(rgb, 0, 1).clamp(0., 1.).permute(2, 0, 1))
        ds.append((depth / float(np.float32(c.far))).unsqueeze(0))
        a, b = frame_images(rgb.float(), depth.float(), float(np.float32(c.far)))
        rgb8.append(a), d16.append(b)
    return dict(frames=frames, mean=mean_metrics(frames), rgbs=torch.stack(rgbs), depths=torch.stack(ds), rgb8=np.stack(rgb8),
                depth16=np.stack(d16), maps=maps)


# ----------------------------------------------------------------------------------------------------------------------
# shared by tests/test_nerf_eval_host.py and tests/test_gpu_nerf_eval.py
# ----------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden_npz():
    return dict(np.load(os.path.join(GOLDEN, "nerf_eval.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(GOLDEN, "nerf_eval_bounds.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def evals(golden_npz):
    """case name -> (inputs, targets, float32 checker result, float64 checker result); filled on first use, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            c = case_inputs(CASES[NAMES.index(name)])
            targets = load_targets(c, golden_npz[f"{name}/target_rgb8"], golden_npz[f"{name}/target_depth16"])
            threads = torch.get_num_threads()
            torch.set_num_threads(1)         # the golden file was recorded with one thread
            both = [eval_case(c, targets, dt) for dt in (torch.float32, torch.float64)]
            torch.set_num_threads(threads)
            cache[name] = (c, targets, *both)
        return cache[name]
    return get


def write_run(tmp_path, c, targets_rgb8, targets_raw16, transforms="transforms_test.json"):
    """A checkpoint directory and a scene directory with the transforms json, the target images and the 16-bit depth files of case
    ``c`` -> argv of nerf_test.  A frame without a valid depth gets no depth file."""
    from PIL import Image
    single = SimpleNamespace(**dict(vars(c), c2w=c.poses[0]))
    argv = V.write_run(tmp_path, single)
    scene = os.path.join(str(tmp_path), "data", "scene0000_00")
    os.makedirs(os.path.join(scene, "images"))
    os.makedirs(os.path.join(scene, "depth"))
    fx, fy, cx, cy = (float(v) for v in c.intrinsic)
    frames = []
    for i in range(c.frames):
        fr = {"transform_matrix": c.poses[i].tolist(), "fx": fx, "fy": fy, "cx": cx, "cy": cy, "file_path": f"images/{i}.png"}
        Image.fromarray(targets_rgb8[i]).save(os.path.join(scene, fr["file_path"]))
        if (targets_raw16[i] > 0).any():
            fr["depth_file_path"] = f"depth/{i}.png"
            Image.fromarray(targets_raw16[i]).save(os.path.join(scene, fr["depth_file_path"]))
        frames.append(fr)
    os.remove(os.path.join(scene, "transforms_test.json"))
    with open(os.path.join(scene, transforms), "w") as f:
        json.dump({"frames": frames, "near": c.near, "far": c.far, "depth_scaling_factor": DEPTH_SCALING}, f)
    return argv[: argv.index("--output_dir")]
