"""Checker of the NeRF view rendering (scripts/nerf_render.py, ops.nerf_render): a torch restatement, with a dtype and a mutation
argument, of what the reference's data/scannet/run_nerf.py does at test time (perturb 0, raw_noise_std 0, N_importance 0):
  * render (:82-157) and run_network (:50-65) around the model of tests/nerf_extract_ref.py,
  * both paths of render_rays (:514-614): precomputed samples plus depth-guided samples (compute_samples_around_depth :497-502,
    raw2depth :431-435, compute_weights :419-429, sample_3sigma :471-478, forward_with_additonal_samples :504-512), and the plain
    near .. far samples (:602-614), with raw2outputs (:437-469) and render_video's depth std (:184-185),
  * the functions the reference imports from the Dense-Depth-Priors code, which is not on disk -- the assumed definitions of
    DESIGN.md 3.16: get_rays, the deterministic sample_pdf (nerf-pytorch's), precompute_quadratic_samples and to8b.
In float32 every operation is the reference's, in its order (tests/golden/make_nerf_render_golden.py asserts bit equality with the
reference's own render); float64 gives the reference the GPU tests are bounded against.  float32 inputs (intrinsics, pose, samples,
weights, bounds) are widened, never recomputed.  Host-only torch.
"""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nerf_extract_ref as R

MUTATIONS = ("no_last_dist", "no_ray_norm", "no_std_clamp", "pdf_left_nofloor", "raw_viewdir", "plus_z", "reverse_merge")
OUTPUTS = ("rgb_map", "depth_map", "acc_map", "disp_map", "depth_std", "z_vals", "weights")


# ----------------------------------------------------------------------------------------------------------------------
# the assumed functions of the fork
# ----------------------------------------------------------------------------------------------------------------------
def get_rays(H, W, intrinsic, c2w, plus_z=False):
    """-> rays_o, rays_d (H, W, 3) in c2w's dtype: camera direction [(u - cx) / fx, -(v - cy) / fy, -1] for column u and row v,
    rotated by R with the three products added left to right, from the camera position t."""
    dt = c2w.dtype
    fx, fy, cx, cy = (x.to(dt) for x in torch.as_tensor(intrinsic))
    v, u = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    a, b, c = (u - cx) / fx, -(v - cy) / fy, torch.full_like(u, 1.0 if plus_z else -1.0)
    rot = c2w[:3, :3]
    rays_d = torch.stack([a * rot[k, 0] + b * rot[k, 1] + c * rot[k, 2] for k in range(3)], -1)
    return c2w[:3, 3].expand(rays_d.shape), rays_d


def sample_pdf(bins, weights, N_samples, det=False, pytest=False, mutated=False):
    """nerf-pytorch's sample_pdf, deterministic branch: the inverse CDF of the piecewise-constant pdf ``weights + 1e-5`` over
    ``bins`` at u = linspace(0, 1, N_samples).  ``mutated``: no 1e-5 and searchsorted from the left."""
    assert det
    if not mutated:
        weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    u = torch.linspace(0., 1., steps=N_samples, dtype=bins.dtype)
    u = u.expand(list(cdf.shape[:-1]) + [N_samples]).contiguous()
    inds = torch.searchsorted(cdf, u, right=not mutated)
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    inds_g = torch.stack([below, above], -1)
    matched_shape = [inds_g.shape[0], inds_g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(matched_shape), 2, inds_g)
    bins_g = torch.gather(bins.unsqueeze(1).expand(matched_shape), 2, inds_g)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    small = denom < 1e-5
    denom = torch.where(small, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    sample_pdf.last = SimpleNamespace(denom=cdf_g[..., 1] - cdf_g[..., 0], width=bins_g[..., 1] - bins_g[..., 0])
    return bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])


def precompute_quadratic_samples(near, far, num_samples):
    """A parabola through near at x = 0 and far at x = 1 whose slope at 0 is 0.2 a: samples dense near the camera."""
    start = 0.1
    x = torch.linspace(0, 1, num_samples)
    c = near
    a = (far - near) / (1. + 2. * start)
    b = 2. * start * a
    return a * x.pow(2) + b * x + c


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# run_nerf.py restated
# ----------------------------------------------------------------------------------------------------------------------
def compute_weights(raw, z_vals, rays_d, mutation=None):
    dists = z_vals[..., 1:] - z_vals[..., :-1]
    dists = torch.cat([dists, torch.full_like(dists[..., :1], 0. if mutation == "no_last_dist" else 1e10)], -1)
    if mutation != "no_ray_norm":
        dists = dists * torch.norm(rays_d[..., None, :], dim=-1)
    alpha = 1. - torch.exp(-torch.relu(raw[..., 3] + 0.) * dists)
    ones = torch.ones((alpha.shape[0], 1), dtype=alpha.dtype)
    return alpha * torch.cumprod(torch.cat([ones, 1. - alpha + 1e-10], -1), -1)[:, :-1]


def raw2depth(raw, z_vals, rays_d, mutation=None):
    weights = compute_weights(raw, z_vals, rays_d, mutation)
    depth = torch.sum(weights * z_vals, -1)
    std = (((z_vals - depth.unsqueeze(-1)).pow(2) * weights).sum(-1)).sqrt()
    return depth, std


def raw2outputs(raw, z_vals, rays_d, mutation=None):
    rgb = torch.sigmoid(raw[..., :3])
    weights = compute_weights(raw, z_vals, rays_d, mutation)
    rgb_map = torch.sum(weights[..., None] * rgb, -2)
    depth_map = torch.sum(weights * z_vals, -1)
    disp_map = 1. / torch.max(1e-10 * torch.ones_like(depth_map), depth_map / torch.sum(weights, -1))
    acc_map = torch.sum(weights, -1)
    return rgb_map, disp_map, acc_map, weights, depth_map


def sample_3sigma(low_3sigma, high_3sigma, N, near, far, mutation=None):
    dt = low_3sigma.dtype
    t_vals = torch.linspace(0., 1., steps=N, dtype=dt)
    step_size = (high_3sigma - low_3sigma) / (N - 1)
    bin_edges = (low_3sigma.unsqueeze(-1) * (1. - t_vals) + high_3sigma.unsqueeze(-1) * (t_vals)).clamp(near, far)
    factor = (bin_edges[..., 1:] - bin_edges[..., :-1]) / step_size.unsqueeze(-1)
    x_in_3sigma = torch.linspace(-3., 3., steps=(N - 1), dtype=dt)
    bin_weights = factor * (1. / math.sqrt(2 * np.pi) * torch.exp(-0.5 * x_in_3sigma.pow(2))).unsqueeze(0).expand(
        *bin_edges.shape[:-1], N - 1)
    return sample_pdf(bin_edges, bin_weights, N, det=True, mutated=mutation == "pdf_left_nofloor")


def samples_around_depth(raw, z_vals, rays_d, N, lower_bound, near, far, mutation=None):
    depth, std = raw2depth(raw, z_vals, rays_d, mutation)
    if mutation != "no_std_clamp":
        std = std.clamp(min=lower_bound)
    return sample_3sigma(depth - 3. * std, depth + 3. * std, N, near, far, mutation)


def merge_sorted(z1, z2):
    """Two-pointer merge of two non-decreasing rows, list 1 first on a tie (what the composite kernel does) -> (z, source index into
    cat([z1, z2]))."""
    z1, z2 = np.asarray(z1), np.asarray(z2)
    out, src, i, j = [], [], 0, 0
    while i < len(z1) or j < len(z2):
        if j >= len(z2) or (i < len(z1) and z1[i] <= z2[j]):
            out.append(z1[i]), src.append(i)
            i += 1
        else:
            out.append(z2[j]), src.append(len(z1) + j)
            j += 1
    return np.array(out, dtype=z1.dtype), np.array(src)


@torch.no_grad()
def render(state, cfg, near, far, bb_center, bb_scale, z_samples=None, n_samples=None, H=None, W=None, intrinsic=None, c2w=None,
           rays=None, lindisp=False, embedded_cam=None, dtype=torch.float32, mutation=None, raw1=None, z2=None):
    """render + render_rays of the reference for a frame (H, W, intrinsic, c2w) or for rays [R, 6] -> dict of flat per-ray tensors of
    ``dtype``: rgb_map [R, 3], depth_map, acc_map, disp_map, depth_std [R], z_vals, weights [R, S], and the stages raw1 [R, S1, 4],
    z2 [R, S1] (two-pass path), rays_o, rays_d.  z_samples (a float32 tensor) selects the two-pass path, None the plain one with
    n_samples.  ``raw1`` / ``z2``: use these instead of computing them (the staged GPU tests feed a stage the float32 checker's
    input)."""
    assert mutation is None or mutation in MUTATIONS
    cfg = dict(R.DEFAULT_CFG, **(cfg or {}))
    model = R.build_model(state, cfg, dtype)
    embed_fn, _ = R.get_embedder(cfg["multires"], cfg["i_embed"])
    embeddirs_fn, _ = R.get_embedder(cfg["multires_views"], cfg["i_embed"])
    bb_center, bb_scale = torch.as_tensor(bb_center).to(dtype), torch.as_tensor(bb_scale).to(dtype)
    cam = torch.zeros(cfg["input_ch_cam"]) if embedded_cam is None else torch.as_tensor(embedded_cam)
    cam = cam.to(dtype)
    if rays is None:
        rays_o, rays_d = get_rays(H, W, torch.as_tensor(intrinsic), torch.as_tensor(c2w).to(dtype), plus_z=mutation == "plus_z")
    else:
        rays_o, rays_d = torch.as_tensor(rays)[:, :3].to(dtype), torch.as_tensor(rays)[:, 3:6].to(dtype)
    viewdirs = rays_d
    if mutation != "raw_viewdir":
        viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
    viewdirs = torch.reshape(viewdirs, [-1, 3])
    rays_o, rays_d = torch.reshape(rays_o, [-1, 3]), torch.reshape(rays_d, [-1, 3])
    near, far = float(np.float32(near)), float(np.float32(far))      # the float32 bounds the reference and the kernels use, widened
    near_t, far_t = near * torch.ones_like(rays_d[..., :1]), far * torch.ones_like(rays_d[..., :1])
    N_rays = rays_o.shape[0]

    def query(z_vals):
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
        flat = (torch.reshape(pts, [-1, 3]) - bb_center) * bb_scale
        embedded = embed_fn(flat)
        dirs = embeddirs_fn(torch.reshape(viewdirs[:, None].expand(pts.shape), [-1, 3]))
        embedded = torch.cat([embedded, dirs, cam.unsqueeze(0).expand(dirs.shape[0], cam.shape[0])], -1)
        return torch.reshape(model(embedded), list(pts.shape[:-1]) + [4])

    out = {"rays_o": rays_o, "rays_d": rays_d}
    if z_samples is not None:
        zs = torch.as_tensor(z_samples).to(dtype)
        N_half = zs.shape[0]
        lower_bound = zs[-1] - zs[-2]
        z_vals = zs.unsqueeze(0).expand((N_rays, N_half))
        raw = query(z_vals) if raw1 is None else torch.as_tensor(raw1).to(dtype)
        if z2 is None:
            z_vals_2 = samples_around_depth(raw, z_vals, rays_d, N_half, lower_bound, near_t[0, 0], far_t[0, 0], mutation)
        else:
            z_vals_2 = torch.as_tensor(z2).to(dtype)
        out["raw1"], out["z2"] = raw, z_vals_2
        raw_2 = query(z_vals_2)
        z_vals = torch.cat((z_vals, z_vals_2), -1)
        raw = torch.cat((raw, raw_2), 1)
        z_vals, indices = z_vals.sort(descending=mutation == "reverse_merge")
        raw = torch.gather(raw, 1, indices.unsqueeze(-1).expand_as(raw))
    else:
        t_vals = torch.linspace(0., 1., steps=n_samples, dtype=dtype)
        if not lindisp:
            z_vals = near_t * (1. - t_vals) + far_t * (t_vals)
        else:
            z_vals = 1. / (1. / near_t * (1. - t_vals) + 1. / far_t * (t_vals))
        raw = query(z_vals)
        out["raw1"] = raw
    rgb_map, disp_map, acc_map, weights, depth_map = raw2outputs(raw, z_vals, rays_d, mutation)
    depth_var = ((z_vals - depth_map.unsqueeze(-1)).pow(2) * weights).sum(-1)
    out.update(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, depth_map=depth_map, z_vals=z_vals, weights=weights,
               depth_std=depth_var.clamp(0., 1.).sqrt())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the shared cases
# ----------------------------------------------------------------------------------------------------------------------
def make_state(seed, cfg, sigma_scale):
    """Family "a" of the extract checker with alpha_linear re-centred and scaled: the bias becomes minus the median of w . h over 256
    seeded probe points (rounded to 1 / 64, so that the last bits of the probe do not matter), then weight and bias x sigma_scale --
    sigma of both signs with optical depths of a sample around one, so that rays end up anywhere between empty and opaque."""
    sd = R.make_state(seed, "a", cfg)
    model = R.build_model(sd, cfg)
    embed_fn, _ = R.get_embedder(cfg["multires"], cfg["i_embed"])
    g = torch.Generator().manual_seed(seed)
    probe = embed_fn(torch.rand(256, 3, generator=g) * 1.2 - 0.6)
    with torch.no_grad():
        x = torch.cat([probe, probe.new_zeros(256, 3 + 6 * cfg["multires_views"] + cfg["input_ch_cam"])], -1)
        sigma = model(x)[:, 3] - sd["alpha_linear.bias"]
    sd["alpha_linear.bias"] = -torch.round(sigma.median() * 64).reshape(1) / 64 * sigma_scale
    sd["alpha_linear.weight"] = sd["alpha_linear.weight"] * sigma_scale
    return sd


# name, frame, samples (two-pass: N_samples = 2 * half), near / far, cfg overrides
CASES = [
    dict(name="odd_5x7", H=5, W=7, N=16, near=0.1, far=4.0, cfg={}),
    dict(name="one_ray", H=1, W=1, N=16, near=0.1, far=4.0, cfg={}, seed=60),
    dict(name="full_3x3", H=3, W=3, N=256, near=0.1, far=4.0, cfg={}),
    # near / far so narrow that depth -+ 3 std crosses both on most rays: zero-width bins, ties with z[0] = near and z[-1] = far
    dict(name="clamped_4x4", H=4, W=4, N=16, near=1.0, far=1.5, cfg={}, seed=72),
    dict(name="views_3x5", H=3, W=5, N=16, near=0.1, far=4.0, cfg=dict(multires_views=2, input_ch_cam=0)),
    dict(name="views_cam_3x5", H=3, W=5, N=16, near=0.1, far=4.0, cfg=dict(multires_views=2, input_ch_cam=4),
         cam=(0.7, -1.3, 0.4, 2.1)),
    dict(name="plain_4x6", H=4, W=6, N=24, near=0.1, far=4.0, cfg={}, plain=True),
    dict(name="plain_lindisp_4x6", H=4, W=6, N=24, near=0.1, far=4.0, cfg={}, plain=True, lindisp=True),
]
NAMES = [c["name"] for c in CASES]
SIGMA_SCALE = 10.0


def case_inputs(case):
    """Everything a case needs, regenerated from seeds."""
    index = NAMES.index(case["name"])
    cfg = dict(R.DEFAULT_CFG, **case["cfg"])
    H, W = case["H"], case["W"]
    focal = 1.2 * max(H, W, 3)
    intrinsic = torch.tensor([focal, focal * 1.03, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.125], dtype=torch.float32)
    c2w = R.make_poses(300 + index, 1)[0]
    plain = case.get("plain", False)
    z_samples = None if plain else precompute_quadratic_samples(case["near"], case["far"], case["N"] // 2)
    cam = None if "cam" not in case else torch.tensor(case["cam"], dtype=torch.float32)
    return SimpleNamespace(name=case["name"], cfg=cfg, H=H, W=W, intrinsic=intrinsic, c2w=c2w, near=case["near"], far=case["far"],
                           bb_center=torch.tensor([0.11, -0.07, 0.9]), bb_scale=torch.tensor(2.0 / 13.0),
                           state=make_state(case.get("seed", 40 + index), cfg, SIGMA_SCALE), z_samples=z_samples, n_samples=case["N"],
                           lindisp=case.get("lindisp", False), embedded_cam=cam, plain=plain)


def render_case(c, dtype=torch.float32, mutation=None, **kw):
    return render(c.state, c.cfg, c.near, c.far, c.bb_center, c.bb_scale, z_samples=c.z_samples, n_samples=c.n_samples, H=c.H,
                  W=c.W, intrinsic=c.intrinsic, c2w=c.c2w, lindisp=c.lindisp, embedded_cam=c.embedded_cam, dtype=dtype,
                  mutation=mutation, **kw)


# ----------------------------------------------------------------------------------------------------------------------
# shared by tests/test_nerf_render_host.py and tests/test_gpu_nerf_render.py
# ----------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden_npz():
    return dict(np.load(os.path.join(GOLDEN, "nerf_render.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(GOLDEN, "nerf_render_bounds.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def refs():
    """case name -> (inputs, float32 checker outputs, float64 checker outputs) as read-only numpy; filled on first use."""
    cache = {}

    def get(name):
        if name not in cache:
            c = case_inputs(CASES[NAMES.index(name)])
            both, threads = [], torch.get_num_threads()
            torch.set_num_threads(1)         # the golden file was recorded with one thread
            for dt in (torch.float32, torch.float64):
                o = {k: v.numpy() for k, v in render_case(c, dt).items()}
                for v in o.values():
                    v.setflags(write=False)
                both.append(o)
            torch.set_num_threads(threads)
            cache[name] = (c, *both)
        return cache[name]
    return get


def write_run(tmp_path, c, frames=1):
    """A checkpoint directory and transforms json for case inputs ``c`` -> argv of nerf_render (the frame of the case, ``frames``
    times)."""
    tmp = str(tmp_path)
    exp = os.path.join(tmp, "ckpt", "run1")
    os.makedirs(exp)
    with open(os.path.join(exp, "args.json"), "w") as f:
        json.dump(dict(c.cfg, expname="run1", N_samples=c.n_samples, depth_loss_weight=0.0 if c.plain else 0.004, lindisp=c.lindisp), f)
    torch.save({"global_step": 2, "network_fn_state_dict": {"module." + k: v for k, v in c.state.items()}},
               os.path.join(exp, "200000.tar"))
    scene = os.path.join(tmp, "data", "scene0000_00")
    os.makedirs(scene)
    fx, fy, cx, cy = (float(v) for v in c.intrinsic)
    fr = [{"transform_matrix": c.c2w.tolist(), "fx": fx, "fy": fy, "cx": cx, "cy": cy} for _ in range(frames)]
    with open(os.path.join(scene, "transforms_test.json"), "w") as f:
        json.dump({"frames": fr, "near": c.near, "far": c.far}, f)
    return ["--expname", "run1", "--ckpt_dir", os.path.join(tmp, "ckpt"), "--data_dir", os.path.join(tmp, "data"), "--scene_id",
            "scene0000_00", "--image_hw", str(c.H), str(c.W), "--bb_center", *(repr(float(v)) for v in c.bb_center), "--bb_scale",
            repr(float(c.bb_scale)), "--output_dir", os.path.join(tmp, "out")]
