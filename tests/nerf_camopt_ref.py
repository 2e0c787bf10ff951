"""Checker of the test-time optimisation of the camera embedding (ops.nerf_camopt_*, nerf_rpn_amd/camopt.py,
scripts/nerf_test_opt.py): the objective of the reference's optimize_camera_embedding (data/scannet/run_nerf.py:193-229) in torch, with a
dtype and mutation arguments.
  * objective: per batch of the partition, nerf_render_ref.render (the undecorated function, under enable_grad) on the batch's rays
    with a leaf embedding, img2mse against the batch's target pixels, backward -- autograd through the reference's whole graph, the
    depth-guided samples and the compositing weights included.
  * head_terms / fixed_gradient: the same gradient with samples and weights held fixed, by the formula the kernels use; with the
    mutations of tests/test_nerf_camopt_host.py.
In float32 objective repeats the reference's operations (tests/golden/make_nerf_camopt_golden.py records how closely); float64 gives
the reference the GPU tests are bounded against.  Host-only torch.
"""
import json
import os

import numpy as np
import pytest
import torch

import nerf_extract_ref as R
import nerf_render_ref as V

CASE_NAMES = ("views_cam_3x5", "odd_5x7", "one_ray", "clamped_4x4", "full_3x3", "plain_4x6")
LOOP_CASES = ("views_cam_3x5", "odd_5x7")
CAMS = {"zero": (0., 0., 0., 0.), "far": (0.7, -1.3, 0.4, 2.1)}
PARTITIONS = ("equal", "remainder")
GRAD_MUTATIONS = ("no_sigmoid_slope", "no_mask", "no_factor_2", "unit_weights")
TARGET_SEED = 900
_render = V.render.__wrapped__         # without torch.no_grad


def case(name):
    return V.case_inputs(V.CASES[V.NAMES.index(name)])


def num_rays(c):
    return c.H * c.W


def target_for(c, seed_shift=0):
    """Seeded uniform target image, float32 [R, 3]."""
    g = torch.Generator().manual_seed(TARGET_SEED + V.NAMES.index(c.name) + 1000 * seed_shift)
    return torch.rand(num_rays(c), 3, generator=g)


def partition(n, kind, seed=0):
    """A seeded random partition of 0 .. n - 1 -> list of index tensors.  "equal": as many equal batches as n's smallest divisor above
    1; "remainder": batches of 4 (5 if 4 divides n) with a smaller last one."""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7700 + 13 * n + seed))
    if kind == "equal":
        nb = next((d for d in range(2, n + 1) if n % d == 0), 1)
        return list(torch.split(perm, n // nb))
    assert kind == "remainder"
    return list(torch.split(perm, 5 if n % 4 == 0 else 4))


def ray_weights(batches, n, uniform=False):
    """rw[r] = 1 / (3 n_b) for a ray in a batch of n_b rays, so that sum_r rw[r] sum_ch e^2 is the sum of the batch means;
    ``uniform``: 1 / (3 n) x the number of batches (what equal batches would give) whatever the batch sizes."""
    rw = torch.zeros(n, dtype=torch.float64)
    for b in batches:
        rw[b] = len(batches) / (3. * n) if uniform else 1. / (3. * len(b))
    return rw


def frame_rays(c, dtype):
    o, d = V.get_rays(c.H, c.W, c.intrinsic, c.c2w.to(dtype))
    return torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], -1)


def _render_rays(c, rays, cam, dtype, z2=None):
    return _render(c.state, c.cfg, c.near, c.far, c.bb_center, c.bb_scale, z_samples=c.z_samples, n_samples=c.n_samples, rays=rays,
                   lindisp=c.lindisp, embedded_cam=cam, dtype=dtype, z2=z2)


def objective(c, cam, target, batches, dtype=torch.float32, z2=None, offset=None):
    """-> dict: losses [B] (the batch means, ``dtype``), m = sum(losses) / B accumulated as the reference does, grad [cam_ch] (the sum
    of the batches' gradients, accumulated in cam.grad), rgb_map [R, 3].  ``offset`` is added to the embedding in ``dtype`` (finite
    differences)."""
    rays = frame_rays(c, dtype)
    leaf = torch.as_tensor(cam, dtype=torch.float32).to(dtype).clone()
    leaf = (leaf if offset is None else leaf + offset.to(dtype)).requires_grad_(True)
    total = torch.zeros(1, dtype=dtype)
    losses, rgb_map = [], torch.zeros(num_rays(c), 3, dtype=dtype)
    with torch.enable_grad():
        for b in batches:
            out = _render_rays(c, rays[b], leaf, dtype, None if z2 is None else torch.as_tensor(z2)[b])
            loss = torch.mean((out["rgb_map"] - target[b].to(dtype)) ** 2)
            loss.backward()
            total += loss.detach()
            losses.append(loss.detach())
            rgb_map[b] = out["rgb_map"].detach()
    return dict(losses=torch.stack(losses), m=(total / len(batches))[0], grad=leaf.grad.detach().clone(), rgb_map=rgb_map)


def head_terms(c, cam, dtype=torch.float64, z2=None):
    """What the fixed-weights gradient is made of, at the embedding ``cam``: the frame rendered without autograd -> dict of z_vals,
    weights [R, S] (merged order), pre [R, S, 128] (views_linears.0's output g + c at every merged sample), raw_rgb [R, S, 3],
    rgb_map [R, 3], sigma [R, S] and z2."""
    cam_t = torch.as_tensor(cam, dtype=torch.float32).to(dtype)
    with torch.no_grad():
        out = _render_rays(c, frame_rays(c, dtype), cam_t, dtype, z2)
        model = R.build_model(c.state, c.cfg, dtype)
        embed_fn, _ = R.get_embedder(c.cfg["multires"], c.cfg["i_embed"])
        embeddirs_fn, _ = R.get_embedder(c.cfg["multires_views"], c.cfg["i_embed"])
        rays_o, rays_d = out["rays_o"], out["rays_d"]
        z = out["z_vals"]
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]
        flat = (pts.reshape(-1, 3) - c.bb_center.to(dtype)) * c.bb_scale.to(dtype)
        viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
        dirs = embeddirs_fn(viewdirs[:, None].expand(pts.shape).reshape(-1, 3))
        h = embed_fn(flat)
        e = h
        for i, l in enumerate(model.pts_linears):
            h = torch.relu(l(h))
            if i in model.skips:
                h = torch.cat([e, h], -1)
        sigma = model.alpha_linear(h)
        x = torch.cat([model.feature_linear(h), dirs, cam_t.unsqueeze(0).expand(dirs.shape[0], cam_t.shape[0])], -1)
        pre = model.views_linears[0](x)
        raw_rgb = model.rgb_linear(torch.relu(pre))
    n, s = z.shape
    return dict(z_vals=z, weights=out["weights"], pre=pre.reshape(n, s, -1), raw_rgb=raw_rgb.reshape(n, s, 3), rgb_map=out["rgb_map"],
                sigma=sigma.reshape(n, s), z2=out.get("z2"))


def head_weights(c, dtype):
    """-> W_rgb [3, 128], W_c [128, cam_ch] of the model."""
    sd = c.state
    ch = c.cfg["input_ch_cam"]
    wv = sd["views_linears.0.weight"].to(dtype)
    return sd["rgb_linear.weight"].to(dtype), wv[:, wv.shape[1] - ch:]


def fixed_gradient(c, terms, target, rw, mutation=None):
    """The gradient of L = sum_r rw[r] sum_ch (rgb_map - target)^2 with samples and weights held fixed, in the dtype of ``terms``:
    d[p][ch] = 2 rw e w s (1 - s), A[j][ch] = sum_p [pre[p][j] > 0] d[p][ch], grad[k] = sum_j W_c[j][k] sum_ch W_rgb[ch][j] A[j][ch].
    -> dict: loss, grad [cam_ch], abs_terms [cam_ch] (the sum of the absolute values of everything added into grad[k]), d [R, S, 3]."""
    assert mutation is None or mutation in GRAD_MUTATIONS
    dt = terms["pre"].dtype
    w_rgb, w_c = head_weights(c, dt)
    w = torch.ones_like(terms["weights"]) if mutation == "unit_weights" else terms["weights"]
    s = torch.sigmoid(terms["raw_rgb"])
    rgb_map = (w[..., None] * s).sum(1)
    e = rgb_map - target.to(dt)
    rw = rw.to(dt)
    loss = (rw * (e * e).sum(-1)).sum()
    dl = (1. if mutation == "no_factor_2" else 2.) * rw[:, None] * e
    slope = torch.ones_like(s) if mutation == "no_sigmoid_slope" else s * (1. - s)
    d = dl[:, None, :] * w[..., None] * slope
    mask = torch.ones_like(terms["pre"]) if mutation == "no_mask" else (terms["pre"] > 0).to(dt)
    a = torch.einsum("psj,psc->jc", mask, d)
    a_abs = torch.einsum("psj,psc->jc", mask, d.abs())
    dc = (w_rgb.T * a).sum(-1)
    return dict(loss=loss, grad=w_c.T @ dc, abs_terms=w_c.abs().T @ (w_rgb.abs().T * a_abs).sum(-1), d=d, rgb_map=rgb_map)


def flip_allowance(c, terms64, d64, pre_bound):
    """The gradient change if every relu whose float64 pre-activation lies within pre_bound of 0 flipped: F = those (point, j);
    allow[k] = sum over F of |W_c[j][k]| |sum_ch W_rgb[ch][j] d[p][ch]| -> (allow [cam_ch], |F|)."""
    w_rgb, w_c = head_weights(c, torch.float64)
    near = terms64["pre"].abs() <= pre_bound                         # [R, S, 128]
    per = torch.einsum("psc,cj->psj", d64, w_rgb).abs() * near       # |sum_ch W_rgb[ch][j] d[p][ch]| on F
    return per.sum((0, 1)) @ w_c.abs(), int(near.sum())


def value_and_grad(c, target, batches, dtype=torch.float32):
    """The callable camopt.optimize_embedding takes, on the checker."""
    def f(cam):
        o = objective(c, cam, target, batches, dtype)
        return o["m"], o["grad"]
    return f


# the command line's frames: the two loop cases' networks, poses and samples at the smallest frames nerf_view_metrics takes (its SSIM
# window is 7 x 7); 56 rays in batches of 2 N_rand = 16 leave a remainder batch of 8
CLI_FRAMES = {"views_cam_3x5": (7, 8), "odd_5x7": (8, 7)}
CLI_N_RAND, CLI_SEED, CLI_STEPS = 8, 3, 4


def cli_case(name):
    """-> (case inputs at the command line's frame with ``rgb8`` [1, H, W, 3], the seeded 8-bit target image; target float32 [R, 3] as
    the loader converts it; the batches nerf_test draws with --opt_seed CLI_SEED)."""
    from nerf_rpn_amd import camopt
    H, W = CLI_FRAMES[name]
    c = V.case_inputs(dict(V.CASES[V.NAMES.index(name)], H=H, W=W))
    g = torch.Generator().manual_seed(TARGET_SEED + 50 + V.NAMES.index(name))
    c.rgb8 = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8).numpy()
    target = torch.from_numpy((c.rgb8[0] / 255.).astype(np.float32)).reshape(-1, 3)
    batches = camopt.random_subsets(H * W, 2 * CLI_N_RAND, torch.Generator().manual_seed(CLI_SEED))
    return c, target, batches


# ----------------------------------------------------------------------------------------------------------------------
# shared by tests/test_nerf_camopt_host.py and tests/test_gpu_nerf_camopt.py
# ----------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def camopt_golden():
    return dict(np.load(os.path.join(GOLDEN, "nerf_camopt.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def camopt_bounds():
    with open(os.path.join(GOLDEN, "nerf_camopt_bounds.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def camopt_refs():
    """(case name, cam name, partition name, given_z2) -> namespace of the case, target, batches, rw and the float32 / float64
    objective; computed once with one thread (as the golden file was) and shared."""
    cache = {}

    def get(name, cam, part, given_z2=True):
        key = (name, cam, part, given_z2)
        if key not in cache:
            threads = torch.get_num_threads()
            torch.set_num_threads(1)
            c = case(name)
            target, batches = target_for(c), partition(num_rays(c), part)
            o32 = objective(c, CAMS[cam], target, batches, torch.float32)
            z2 = None
            if not c.plain:
                with torch.no_grad():
                    z2 = _render_rays(c, frame_rays(c, torch.float32), torch.zeros(4), torch.float32)["z2"]
            o64 = objective(c, CAMS[cam], target, batches, torch.float64, z2 if given_z2 else None)
            torch.set_num_threads(threads)
            cache[key] = dict(c=c, target=target, batches=batches, rw=ray_weights(batches, num_rays(c)), o32=o32, o64=o64, z2=z2)
        return cache[key]
    return get
