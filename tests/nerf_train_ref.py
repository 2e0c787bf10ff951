"""Checker of the front end of NeRF training (ops.nerf_train_batch, ops.nerf_train_samples, nerf_train.train): a torch restatement,
with a dtype and a mutation argument, of what the reference's data/scannet/run_nerf.py does at train time before and between its
network queries:
  * get_ray_batch_from_one_image (:650-670) after the pixel draw, with precompute_depth_sampling (:159-162) and the checker's get_rays,
  * perturb_z_vals (:480-495) with the uniforms given,
  * the second sample list of render_rays (:588-592): compute_samples_around_depth (:497-502) for the rays without a valid depth,
    sample_3sigma (:471-478) of the depth range for the others, both through nerf-pytorch's sample_pdf with its uniforms given,
  * render_rays at train time (:579-593) around a query function, and the loop of train_nerf (:811-849).
raw2depth, sample_3sigma and get_rays are tests/nerf_render_ref.py's, the ray stage and the losses tests/nerf_composite_ref.py's, the
network rows tests/nerf_query_ref.py's.  In float32 every operation is the reference's, in its order
(tests/golden/make_nerf_train_golden.py asserts bit equality with the reference's own functions); float64 gives the reference the GPU
tests are bounded against.  float32 inputs are widened, never recomputed.  Host-only torch.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nerf_composite_ref as C
import nerf_extract_ref as R
import nerf_query_ref as Q
import nerf_render_ref as V

FACTOR = 8.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MUTATIONS = ("searchsorted_left", "no_floor", "no_std_clamp", "valid_swapped", "range_cols_swapped", "perturb_swapped", "shared_z1")
BATCH = ("rays", "viewdirs", "target_s", "target_d", "target_vd", "depth_range", "z1")
STORED = BATCH + ("z2", "z_vals", "weights", "rgb_map", "depth_map")
REJECT_CAP = 0.10
# the flags of config_parser (:924-1008) that the train task reads
CLI_FLAGS = ("expname", "ckpt_dir", "data_dir", "scene_id", "N_rand", "lrate", "start_decay_lrate", "end_decay_lrate", "no_reload",
             "depth_loss_weight", "N_samples", "perturb", "multires_views", "input_ch_cam", "raw_noise_std", "lindisp", "i_print", "i_weights",
             "chunk", "netdepth", "netwidth", "multires", "i_embed", "N_importance", "use_viewdirs")
H, W, NEAR, FAR = 6, 8, 0.1, 4.0


# ----------------------------------------------------------------------------------------------------------------------
# the assumed functions of the fork
# ----------------------------------------------------------------------------------------------------------------------
def select_coordinates(coords, N_rand):
    """The pixel draw, with the drawn row-major indices supplied in ``select_coordinates.pix`` -> [N_rand, 2] (row, column), long."""
    flat = coords.reshape(-1, 2).long()
    return flat[select_coordinates.pix]


def sample_pdf(bins, weights, N_samples, det=False, pytest=False, u=None, mutation=None):
    """nerf-pytorch's sample_pdf: the inverse CDF of the piecewise-constant pdf ``weights + 1e-5`` over ``bins`` at u -- linspace(0, 1)
    if det, else the given u [rows, N_samples] (or the next entry of ``sample_pdf.feed``) in place of torch.rand."""
    if mutation != "no_floor":
        weights = weights + 1e-5
    pdf = weights / torch.sum(weights, -1, keepdim=True)
    cdf = torch.cumsum(pdf, -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    if det:
        u = torch.linspace(0., 1., steps=N_samples, dtype=bins.dtype)
        u = u.expand(list(cdf.shape[:-1]) + [N_samples])
    elif u is None:
        u = sample_pdf.feed.pop(0)
    u = u.to(bins.dtype).contiguous()
    inds = torch.searchsorted(cdf, u, right=mutation != "searchsorted_left")
    below = torch.max(torch.zeros_like(inds - 1), inds - 1)
    above = torch.min((cdf.shape[-1] - 1) * torch.ones_like(inds), inds)
    inds_g = torch.stack([below, above], -1)
    matched_shape = [inds_g.shape[0], inds_g.shape[1], cdf.shape[-1]]
    cdf_g = torch.gather(cdf.unsqueeze(1).expand(matched_shape), 2, inds_g)
    bins_g = torch.gather(bins.unsqueeze(1).expand(matched_shape), 2, inds_g)
    denom = cdf_g[..., 1] - cdf_g[..., 0]
    sample_pdf.last = SimpleNamespace(denom=denom, width=bins_g[..., 1] - bins_g[..., 0])
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    t = (u - cdf_g[..., 0]) / denom
    return bins_g[..., 0] + t * (bins_g[..., 1] - bins_g[..., 0])


sample_pdf.feed = []


def near_branch(last):
    """Rows with a sample in a bin of non-zero width whose cdf difference is within a factor 10 of sample_pdf's 1e-5 branch."""
    return ((last.denom > 1e-6) & (last.denom < 1e-4) & (last.width != 0)).any(-1)


# ----------------------------------------------------------------------------------------------------------------------
# run_nerf.py restated
# ----------------------------------------------------------------------------------------------------------------------
def precompute_depth_sampling(depth):
    depth_min = (depth[:, 0] - 3. * depth[:, 1])
    depth_max = depth[:, 0] + 3. * depth[:, 1]
    return torch.stack((depth[:, 0], depth_min, depth_max), -1)


def ray_batch(intrinsic, c2w, pix, image, depth, valid, dtype=torch.float32, hw=(H, W)):
    """get_ray_batch_from_one_image for the pixels pix [R] of one view of hw pixels -> dict over rays [R, 6], viewdirs, target_s,
    target_d, target_vd, depth_range."""
    h, w = hw
    rays_o, rays_d = V.get_rays(h, w, torch.as_tensor(intrinsic), torch.as_tensor(c2w).to(dtype))
    pix = torch.as_tensor(pix).long()
    row, col = pix // w, pix % w
    rays_o, rays_d = rays_o[row, col], rays_d[row, col]
    out = {"rays": torch.cat([rays_o, rays_d], -1), "viewdirs": rays_d / torch.norm(rays_d, dim=-1, keepdim=True),
           "target_s": image.to(dtype)[row, col]}
    if depth is not None:
        out["target_d"] = depth.to(dtype)[row, col]
        out["target_vd"] = valid[row, col]
        out["depth_range"] = precompute_depth_sampling(out["target_d"])
    return out


def perturb_z_vals(z_vals, t_rand, mutation=None):
    mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
    upper = torch.cat([mids, z_vals[..., -1:]], -1)
    lower = torch.cat([z_vals[..., :1], mids], -1)
    if mutation == "perturb_swapped":
        upper, lower = lower, upper
    return lower + (upper - lower) * t_rand


def sample_3sigma(lo, hi, N, near, far, u, mutation=None):
    """V.sample_3sigma with the stochastic sample_pdf at u (u None: its deterministic one)."""
    saved = V.sample_pdf
    if u is not None:
        V.sample_pdf = lambda bins, w, n, det=True, mutated=False: sample_pdf(bins, w, n, det=False, u=u, mutation=mutation)
    else:
        V.sample_pdf = lambda bins, w, n, det=True, mutated=False: sample_pdf(bins, w, n, det=True, mutation=mutation)
    try:
        return V.sample_3sigma(lo, hi, N, near, far)
    finally:
        V.sample_pdf = saved


def second_list(raw, z_vals, rays_d, depth_range, u, lower_bound, near, far, mutation=None, z_base=None):
    """z_vals_2 of render_rays at train time (:588-592) -> (z2 [R, S] in u's order, rejected [R] bool: near_branch of the ray)."""
    N = z_vals.shape[1]
    if depth_range is None:
        valid = torch.zeros(z_vals.shape[0], dtype=torch.bool)
    else:
        valid = depth_range[:, 0] >= near
        if mutation == "valid_swapped":
            valid = valid.logical_not()
    invalid = valid.logical_not()
    z2 = torch.empty_like(z_vals)
    rejected = torch.zeros(z_vals.shape[0], dtype=torch.bool)
    zw = z_base.to(z_vals.dtype).expand_as(z_vals) if mutation == "shared_z1" else z_vals
    depth, std = V.raw2depth(raw[invalid], zw[invalid], rays_d[invalid])
    if mutation != "no_std_clamp":
        std = std.clamp(min=lower_bound)
    z2[invalid] = sample_3sigma(depth - 3. * std, depth + 3. * std, N, near, far, None if u is None else u[invalid], mutation)
    rejected[invalid] = near_branch(sample_pdf.last)
    if depth_range is not None:
        a, b = (2, 1) if mutation == "range_cols_swapped" else (1, 2)
        z2[valid] = sample_3sigma(depth_range[valid, a], depth_range[valid, b], N, near, far, None if u is None else u[valid], mutation)
        rejected[valid] = near_branch(sample_pdf.last)
    return z2, rejected


def render_rays_train(query, rays, z, t_rand, depth_range, u, near, far, noise=None, mutation=None, raw1=None):
    """render_rays (:579-593) with perturb 1 for rays [R, 6] around ``query(z_vals, first?) -> raw`` -> dict: z1, z2 (unsorted), raw1,
    rejected and the ray stage's outputs.  The second query sees the sorted z2 (the query is pointwise: the reference's sort after the
    concatenation); raw1: use this instead of query(z1)."""
    rays_d = rays[:, 3:6]
    lower_bound = z[-1] - z[-2]
    z_vals = z.unsqueeze(0).expand((rays.shape[0], z.shape[0]))
    z1 = perturb_z_vals(z_vals, t_rand, mutation) if t_rand is not None else z_vals
    raw = query(z1, True) if raw1 is None else raw1
    z2, rejected = second_list(raw.detach(), z1, rays_d, depth_range, u, lower_bound, near, far, mutation, z)
    z2s = torch.sort(z2, -1).values
    out = C.ray_stage(raw, z1, rays_d, query(z2s, False), z2s, noise)
    return dict(out, z1=z1, z2=z2, raw1=raw, rejected=rejected)


# ----------------------------------------------------------------------------------------------------------------------
# the shared cases
# ----------------------------------------------------------------------------------------------------------------------
# R x S per list; valid: which pixels carry a depth; dscale: the factor on c2w's rotation, so that |rays_d| leaves 1
CASES = [
    dict(name="r1_s2", R=1, S=2, valid="mixed", dscale=1.0, first_pix=(1,)),
    dict(name="r3_s4_valid", R=3, S=4, valid="all", dscale=1.0, first_pix=(2, 0, 1)),
    dict(name="r5_s6_invalid", R=5, S=6, valid="none", dscale=0.55, first_pix=()),
    dict(name="r7_s13_mixed", R=7, S=13, valid="mixed", dscale=1.6, first_pix=(4, 0, 3, 2, 0)),
    dict(name="r130_s32_mixed", R=130, S=32, valid="mixed", dscale=0.55, first_pix=(47, 0, 2, 4, 6, 8)),
]
NAMES = [c["name"] for c in CASES]


def depth_image(gen, policy):
    """[H, W, 2] (depth, std) and valid [H, W].  Pixel 0: depth = near exactly (bins clamped at near); 2: clamped at far; 4: at both;
    6: a range wholly beyond far (every bin of zero width); 8: the smallest std the reference's depth completion leaves (0.03, :748-749).  "mixed": odd pixels carry no depth (0, 0, invalid)."""
    d = torch.rand(H * W, generator=gen) * (FAR - NEAR - 0.2) + NEAR + 0.1
    s = torch.rand(H * W, generator=gen) * 0.4 + 0.03
    d[0], s[0] = NEAR, 0.1
    d[2], s[2] = FAR - 0.05, 0.2
    d[4], s[4] = 2.0, 2.0
    d[6], s[6] = 5.0, 0.1
    d[8], s[8] = 1.5, 0.03
    valid = torch.ones(H * W, dtype=torch.bool)
    if policy == "none":
        valid[:] = False
    elif policy == "mixed":
        valid[1::2] = False
    d, s = torch.where(valid, d, torch.zeros_like(d)), torch.where(valid, s, torch.zeros_like(s))
    return torch.stack([d, s], -1).reshape(H, W, 2).contiguous(), valid.reshape(H, W)


def case_inputs(case):
    """Everything a case needs, regenerated from seeds (float32)."""
    index = NAMES.index(case["name"])
    gen = torch.Generator().manual_seed(7100 + index)
    nr, S = case["R"], case["S"]
    focal = 1.2 * max(H, W)
    intrinsic = torch.tensor([focal, focal * 1.03, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.125], dtype=torch.float32)
    c2w = R.make_poses(700 + index, 1)[0].clone()
    c2w[:3, :3] *= case["dscale"]
    image = torch.rand(H, W, 3, generator=gen)
    depth, valid = depth_image(gen, case["valid"])
    pix = torch.randint(0, H * W, (nr,), generator=gen)
    first = torch.tensor(case["first_pix"], dtype=torch.long)[:nr]
    pix[:first.shape[0]] = first
    z = V.precompute_quadratic_samples(NEAR, FAR, S)
    t_rand, u = torch.rand(nr, S, generator=gen), torch.rand(nr, S, generator=gen)
    u[0, 0], u[-1, -1] = 0.0, float(np.nextafter(np.float32(1), np.float32(0)))
    raw1, A = torch.randn(nr, S, 4, generator=gen), torch.randn(4, 4, generator=gen)
    raw1[..., 3] *= 30.
    A[:, 3] *= 10.
    r = torch.arange(nr)
    raw1[r % 4 == 0, :, 3] = -raw1[r % 4 == 0, :, 3].abs()              # no density at all: depth 0, std clamped at lower_bound
    raw1[r % 4 == 1, S // 2:, 3] = 1e4                                  # opaque from the middle sample on
    return SimpleNamespace(name=case["name"], R=nr, S=S, intrinsic=intrinsic, c2w=c2w, image=image, depth=depth, valid=valid, pix=pix,
                           z=z, t_rand=t_rand, u=u, raw1=raw1, A=A, near=NEAR, far=FAR)


def point_raw(pts, A):
    """The second query's stand-in for the network: pointwise and linear, one rounded torch operation at a time, so that a point's raw
    does not depend on where in a batch it stands.  A [4, 4]: rows x, y, z, bias."""
    return ((pts[..., 0:1] * A[0] + pts[..., 1:2] * A[1]) + pts[..., 2:3] * A[2]) + A[3]


def run_case(c, dtype=torch.float32, mutation=None, raw1=None):
    """The batch and render_rays_train of a case, with its recorded raw1 and point_raw in place of the network -> dict over STORED +
    rejected."""
    b = ray_batch(c.intrinsic, c.c2w, c.pix, c.image, c.depth, c.valid, dtype)
    given = c.raw1 if raw1 is None else torch.as_tensor(raw1)
    o, d = b["rays"][:, None, :3], b["rays"][:, None, 3:]

    def query(z_vals, first):
        return given.to(dtype) if first else point_raw(o + d * z_vals[..., :, None], c.A.to(dtype))
    near, far = (torch.tensor(x, dtype=torch.float32).to(dtype) for x in (c.near, c.far))
    out = render_rays_train(query, b["rays"], c.z.to(dtype), c.t_rand.to(dtype), b["depth_range"], c.u.to(dtype), near, far,
                            mutation=mutation)
    return dict(b, **out)


# ----------------------------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------------------------
LOOP = SimpleNamespace(steps=8, views=3, N_rand=16, N_samples=8, raw_noise_std=1.0, lrate=Q.TRAIN_LR, depth_loss_weight=0.004, clip=0.1,
                       cfg=dict(R.DEFAULT_CFG, multires_views=2, input_ch_cam=4), bb_center=(0.11, -0.07, 0.9), bb_scale=2.0 / 13.0)


def loop_inputs():
    """Three 6 x 8 views with a depth prior on half their pixels, a seeded network and camera embedding, and every random number of
    eight steps.  With a different view and different pixels at every step the losses of eight steps at the reference's rate differ more
    by their batch than by training: the seed is the first from 7300 on at which the float64 host loop's losses carry no depth-loss
    outlier (all below 0.2), so that "the last loss is below the first" reads the training (0.112 -> 0.043)."""
    gen = torch.Generator().manual_seed(7305)
    n, S = LOOP.views, LOOP.N_samples // 2
    focal = 1.2 * max(H, W)
    intrinsics = torch.tensor([[focal, focal * 1.03, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.125]] * n, dtype=torch.float32)
    images = torch.rand(n, H, W, 3, generator=gen) * 0.5 + 0.25
    both = [depth_image(gen, "mixed") for _ in range(n)]
    steps = []
    for _ in range(LOOP.steps):
        steps.append(SimpleNamespace(image=int(torch.randint(0, n, (1,), generator=gen)), pix=torch.randperm(H * W, generator=gen)[:LOOP.N_rand],
                                     t_rand=torch.rand(LOOP.N_rand, S, generator=gen), u=torch.rand(LOOP.N_rand, S, generator=gen),
                                     noise=torch.randn(LOOP.N_rand, 2 * S, generator=gen)))
    return SimpleNamespace(images=images, depths=torch.stack([d for d, _ in both]), valid_depths=torch.stack([v for _, v in both]),
                           poses=R.make_poses(730, n), intrinsics=intrinsics, near=NEAR, far=FAR, state=V.make_state(73, LOOP.cfg, 10.0),
                           embedcam=torch.randn(n, LOOP.cfg["input_ch_cam"], generator=gen), steps=steps,
                           z=V.precompute_quadratic_samples(NEAR, FAR, S))


def train_loop_host(L, dtype):
    """train_nerf's steps (:811-849) on the host -> the eight losses."""
    model = R.build_model(L.state, LOOP.cfg, dtype).train()
    embed_fn, _ = R.get_embedder(LOOP.cfg["multires"], LOOP.cfg["i_embed"])
    embeddirs_fn, _ = R.get_embedder(LOOP.cfg["multires_views"], LOOP.cfg["i_embed"])
    center, scale = torch.as_tensor(LOOP.bb_center).to(dtype), torch.as_tensor(LOOP.bb_scale, dtype=torch.float32).to(dtype)
    params = list(model.parameters())
    opt = torch.optim.Adam(params, lr=LOOP.lrate, betas=(0.9, 0.999))
    near, far = (torch.tensor(x, dtype=torch.float32).to(dtype) for x in (L.near, L.far))
    losses = []
    for s in L.steps:
        b = ray_batch(L.intrinsics[s.image], L.poses[s.image], s.pix, L.images[s.image], L.depths[s.image], L.valid_depths[s.image], dtype)
        o, d, cam = b["rays"][:, :3], b["rays"][:, 3:], L.embedcam[s.image].to(dtype)

        def query(z_vals, first):
            pts = o[:, None, :] + d[:, None, :] * z_vals[..., :, None]
            return model(Q.network_rows(pts, b["viewdirs"], cam, embed_fn, embeddirs_fn, center, scale)).reshape(*pts.shape[:2], 4)
        out = render_rays_train(query, b["rays"], L.z.to(dtype), s.t_rand.to(dtype), b["depth_range"], s.u.to(dtype), near, far,
                                noise=s.noise.to(dtype) * LOOP.raw_noise_std)
        opt.zero_grad()
        loss = C.img2mse(out["rgb_map"], b["target_s"]) + LOOP.depth_loss_weight * C.depth_loss(
            out["depth_map"], out["z_vals"], out["weights"], b["target_d"], b["target_vd"])
        loss.backward()
        torch.nn.utils.clip_grad_value_(params, LOOP.clip)
        opt.step()
        losses.append(loss.item())
    return losses


# ----------------------------------------------------------------------------------------------------------------------
# comparing; shared by tests/test_nerf_train_host.py and tests/test_gpu_nerf_train.py
# ----------------------------------------------------------------------------------------------------------------------
def bound_of(err32, o64):
    """8 x the float32 checker's error, floored at one float32 ulp of the tensor's largest float64 magnitude."""
    top = C.top_of(o64)
    return 0.0 if top == 0.0 else max(FACTOR * err32, float(np.spacing(np.float32(top))))


def z2_reference_for(c, raw1):
    """A case's second list for another first-list raw1 [R, S, 4] (float32, as a network gave it): both checkers on that raw1 ->
    (the float64 z2, rejected [R] bool by near_branch re-evaluated in that float64 run, the float32 checker's error, its bound)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    raw1 = torch.as_tensor(raw1, dtype=torch.float32).cpu()
    f32, f64 = run_case(c, torch.float32, raw1=raw1), run_case(c, torch.float64, raw1=raw1)
    torch.set_num_threads(threads)
    rejected = f64["rejected"].numpy()
    assert rejected.sum() <= REJECT_CAP * c.R, rejected.nonzero()
    err32 = C.max_error(kept(f32, "z2", rejected), kept(f64, "z2", rejected))
    return f64["z2"].numpy(), rejected, err32, bound_of(err32, kept(f64, "z2", rejected))


def kept(o, key, rejected):
    """A tensor of a case without the rejected rays where the rule applies: z2 and what is computed from it."""
    x = o[key]
    x = x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x[~np.asarray(rejected)] if key in ("z2", "z_vals", "weights", "rgb_map", "depth_map") else x


@pytest.fixture(scope="module")
def golden_npz():
    return dict(np.load(os.path.join(GOLDEN, "nerf_train.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(GOLDEN, "nerf_train_bounds.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def refs():
    """case name -> (inputs, float32 checker, float64 checker); filled on first use, with one thread as the golden file was recorded."""
    cache = {}

    def get(name):
        if name not in cache:
            threads = torch.get_num_threads()
            torch.set_num_threads(1)
            c = case_inputs(CASES[NAMES.index(name)])
            cache[name] = (c, run_case(c, torch.float32), run_case(c, torch.float64))
            torch.set_num_threads(threads)
        return cache[name]
    return get
