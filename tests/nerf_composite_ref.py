"""Checker of the differentiable ray stage (ops.nerf_composite, ops.nerf_ray_losses): host torch with a dtype
argument.
  * ``ray_stage``: concatenate, sort and gather as forward_with_additonal_samples does (data/scannet/run_nerf.py:507-510), then
    compute_weights (:419-429) and raw2outputs (:437-469); ``depth_loss``: the fork's compute_depth_loss as DESIGN.md 3.21 assumes it;
    gradients come from autograd.
  * ``manual``: the same outputs and gradients written out per sample (the formulas the kernels implement), with the mutations of the
    sharpness test.
  * the cases with their rays away from every decision boundary (regenerated from seeds, never committed), and the eight-step Adam
    loop through the ray stage.
float64 gives the reference the GPU tests are bounded against; tests/golden/make_nerf_composite_golden.py pins it to the reference.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf_extract_ref as R
import nerf_query_ref as Q

FACTOR = 8.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MUTATIONS = ("no_eps", "no_suffix", "no_relu_mask", "finite_last_dist", "v_no_eps", "clamp_zero_grad", "detached_m", "no_noise",
             "list2_first")
OUTPUTS = ("rgb_map", "disp_map", "acc_map", "weights", "depth_map", "z_vals")
LOSS_TENSORS = ("img_loss", "depth_loss", "img_draw1", "img_draw2", "depth_draw1", "depth_draw2")
DECISIONS = ("sigma", "outside", "spread", "clamp", "disp")       # sigma | 0, |m - t| - s | 0, s^2 | v, v | 1e-3, depth / acc | 1e-10

# rays x (list 1 + list 2); z1 shared by the rays or per ray; noise; depth targets: "all" valid, "none_valid", valid but
# "none_applied", "mixed" (ray r: r % 3 = 0 invalid, 1 as all, 2 as none_applied); empty / opaque: rays r with r % every = at whose
# sigma is all <= 0 / large enough for T to reach the 1e-10 floor early; thin: rays whose samples span 0.04 with sigma x 100, so that
# their weights spread over several samples while v stays below the 1e-3 clamp
CASES = [
    dict(name="one_sample", R=1, S1=1, S2=0, shared=True, noise=False, depth="all", opaque=(1, 0)),
    dict(name="shared_3x4", R=3, S1=4, S2=0, shared=True, noise=False, depth="none_valid", empty=(3, 0)),
    dict(name="two_lists_5x12", R=5, S1=6, S2=6, shared=False, noise=True, depth="all", opaque=(5, 1), empty=(5, 3), thin=(5, 0)),
    dict(name="uneven_7x18", R=7, S1=13, S2=5, shared=False, noise=False, depth="none_applied", opaque=(7, 2)),
    dict(name="blocks_130x64", R=130, S1=32, S2=32, shared=False, noise=True, depth="mixed", opaque=(13, 9), empty=(13, 5), thin=(13, 1)),
]
NAMES = [c["name"] for c in CASES]
POOL = 256


def tensor_names(case):
    two = case["S2"] > 0
    return OUTPUTS + ("draw1",) + (("draw2",) if two else ()) + tuple(k for k in LOSS_TENSORS if two or not k.endswith("2"))


# ----------------------------------------------------------------------------------------------------------------------
# the ray stage and the losses
# ----------------------------------------------------------------------------------------------------------------------
def merge(raw1, z1, raw2, z2, noise):
    """forward_with_additonal_samples :507-510 (a stable sort: list 1 first on a tie) -> raw, z_vals and noise in merged order."""
    nr = raw1.shape[0]
    z = z1.expand(nr, -1) if z1.dim() == 1 else z1
    raw = raw1
    if raw2 is not None:
        z, raw = torch.cat((z, z2), -1), torch.cat((raw1, raw2), 1)
        z, indices = z.sort(stable=True)
        raw = torch.gather(raw, 1, indices.unsqueeze(-1).expand_as(raw))
        if noise is not None:
            noise = torch.gather(noise, 1, indices)
    return raw, z, noise


def compute_weights(raw, z_vals, rays_d, noise=None):
    dists = z_vals[..., 1:] - z_vals[..., :-1]
    dists = torch.cat([dists, torch.full_like(z_vals[..., :1], 1e10)], -1)
    dists = dists * torch.norm(rays_d[..., None, :], dim=-1)
    alpha = 1. - torch.exp(-F.relu(raw[..., 3] + (0. if noise is None else noise)) * dists)
    ones = torch.ones((alpha.shape[0], 1), dtype=alpha.dtype)
    return alpha * torch.cumprod(torch.cat([ones, 1. - alpha + 1e-10], -1), -1)[:, :-1]


def raw2outputs(raw, z_vals, rays_d, noise=None):
    rgb = torch.sigmoid(raw[..., :3])
    weights = compute_weights(raw, z_vals, rays_d, noise)
    rgb_map = torch.sum(weights[..., None] * rgb, -2)
    depth_map = torch.sum(weights * z_vals, -1)
    disp_map = 1. / torch.max(1e-10 * torch.ones_like(depth_map), depth_map / torch.sum(weights, -1))
    acc_map = torch.sum(weights, -1)
    return rgb_map, disp_map, acc_map, weights, depth_map


def ray_stage(raw1, z1, rays_d, raw2=None, z2=None, noise=None):
    """-> dict over OUTPUTS; the dtype is the inputs'."""
    raw, z, nz = merge(raw1, z1, raw2, z2, noise)
    return dict(zip(OUTPUTS, (*raw2outputs(raw, z, rays_d, nz), z)))


def depth_terms(depth_map, z_vals, weights, target_d):
    """m, v, t, s of compute_depth_loss for every ray."""
    v = ((z_vals - depth_map.unsqueeze(-1)).pow(2) * weights).sum(-1) + 1e-5
    return depth_map, v, target_d[..., 0], target_d[..., 1]


def depth_loss(depth_map, z_vals, weights, target_d, target_vd):
    """compute_depth_loss of the fork: GaussianNLLLoss(eps=1e-3) over the valid rays outside their target's distribution, times their
    share of all rays; zero without such a ray."""
    zero = torch.zeros((), dtype=depth_map.dtype)
    m, v, t, s = depth_terms(depth_map, z_vals, weights, target_d)
    m, v, t, s = m[target_vd], v[target_vd], t[target_vd], s[target_vd]
    if m.shape[0] == 0:
        return zero
    applied = ((m - t).abs() - s > 0.) | (s.pow(2) < v)
    m, v, t = m[applied], v[applied], t[applied]
    if m.shape[0] == 0:
        return zero
    return float(m.shape[0]) / float(target_vd.shape[0]) * torch.nn.GaussianNLLLoss(eps=0.001)(m, t, v)


def img2mse(x, y):
    return torch.mean((x - y) ** 2)


def cot_sum(out, c, dtype):
    """The scalar whose gradient is the seeded cotangent of every differentiable output."""
    return ((out["rgb_map"] * c.g_rgb.to(dtype)).sum() + (out["depth_map"] * c.g_depth.to(dtype)).sum()
            + (out["acc_map"] * c.g_acc.to(dtype)).sum() + (out["weights"] * c.g_w.to(dtype)).sum())


def grads(y, wrt):
    g = torch.autograd.grad(y, wrt, retain_graph=True, allow_unused=True) if y.requires_grad else [None] * len(wrt)
    return [torch.zeros_like(x.detach()) if gi is None else gi for gi, x in zip(g, wrt)]


def check_case(c, dtype):
    """Every tensor a case is bounded on -> dict of detached tensors of ``dtype``."""
    raw1 = c.raw1.detach().clone().to(dtype).requires_grad_(True)
    raw2 = None if c.raw2 is None else c.raw2.detach().clone().to(dtype).requires_grad_(True)
    wrt = [raw1] + ([] if raw2 is None else [raw2])
    names = ["draw1"] + ([] if raw2 is None else ["draw2"])
    out = ray_stage(raw1, c.z1.to(dtype), c.rays_d.to(dtype), raw2, None if raw2 is None else c.z2.to(dtype),
                    None if c.noise is None else c.noise.to(dtype))
    res = {k: out[k].detach() for k in OUTPUTS}
    res.update(zip(names, grads(cot_sum(out, c, dtype), wrt)))
    img = img2mse(out["rgb_map"], c.target_s.to(dtype))
    dep = depth_loss(out["depth_map"], out["z_vals"], out["weights"], c.target_d.to(dtype), c.target_vd)
    res.update(img_loss=img.detach(), depth_loss=dep.detach())
    res.update(zip(["img_" + n for n in names], grads(img, wrt)))
    res.update(zip(["depth_" + n for n in names], grads(dep, wrt)))
    return res


# ----------------------------------------------------------------------------------------------------------------------
# the kernels' formulas, written out
# ----------------------------------------------------------------------------------------------------------------------
def manual(c, mutation=None):
    """What csrc/nerfcomposite.hip computes, per sample in merged order, in float64 -> the dict of check_case."""
    assert mutation is None or mutation in MUTATIONS
    dt = torch.float64
    nr, s1 = c.raw1.shape[:2]
    s2 = 0 if c.raw2 is None else c.raw2.shape[1]
    z = (c.z1.expand(nr, -1) if c.z1.dim() == 1 else c.z1).to(dt)
    raw = c.raw1.to(dt)
    src = torch.zeros(nr, s1, dtype=torch.long)
    if s2:
        z, raw = torch.cat((z, c.z2.to(dt)), -1), torch.cat((raw, c.raw2.to(dt)), 1)
        src = torch.cat((src, torch.ones(nr, s2, dtype=torch.long)), -1)
    if mutation == "list2_first":
        src = 1 - src
    # the two-pointer merge: by z, then by list
    order = torch.argsort(src, dim=-1, stable=True)
    order = torch.gather(order, 1, torch.argsort(torch.gather(z, 1, order), dim=-1, stable=True))
    z, raw = torch.gather(z, 1, order), torch.gather(raw, 1, order.unsqueeze(-1).expand_as(raw))
    sigma = raw[..., 3]
    if c.noise is not None and mutation != "no_noise":
        sigma = sigma + torch.gather(c.noise.to(dt), 1, order)
    nd = torch.norm(c.rays_d.to(dt), dim=-1, keepdim=True)
    last = (z[:, -1:] - z[:, -2:-1] if z.shape[1] > 1 else torch.ones_like(z[:, :1])) if mutation == "finite_last_dist" \
        else torch.full_like(z[:, :1], 1e10)
    delta = torch.cat([z[:, 1:] - z[:, :-1], last], -1) * nd
    e = torch.exp(-F.relu(sigma) * delta)
    alpha = 1. - e
    keep = 1. - alpha + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(keep[:, :1]), keep], -1), -1)[:, :-1]
    w = alpha * T
    s = torch.sigmoid(raw[..., :3])
    rgb_map, depth_map, acc_map = (w[..., None] * s).sum(-2), (w * z).sum(-1), w.sum(-1)
    disp_map = 1. / torch.max(1e-10 * torch.ones_like(depth_map), depth_map / acc_map)
    res = dict(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, weights=w, depth_map=depth_map, z_vals=z)

    def backward(g_rgb, g_depth, g_acc, g_w):
        G = g_w + (g_rgb[:, None, :] * s).sum(-1) + g_depth[:, None] * z + g_acc[:, None]
        gw = G * w
        suffix = torch.flip(torch.cumsum(torch.flip(gw, [-1]), -1), [-1]) - gw
        if mutation == "no_suffix":
            suffix = torch.zeros_like(suffix)
        dalpha = G * T - suffix / (1. - alpha if mutation == "no_eps" else keep)
        dsigma = dalpha * delta * e
        if mutation != "no_relu_mask":
            dsigma = dsigma * (sigma > 0)
        draw = torch.cat([g_rgb[:, None, :] * w[..., None] * s * (1. - s), dsigma[..., None]], -1)
        own = torch.empty_like(draw)
        own.scatter_(1, order.unsqueeze(-1).expand_as(draw), draw)       # back to each list's own order
        return [own[:, :s1], own[:, s1:]][:2 if s2 else 1]
    names = ["draw1", "draw2"][:2 if s2 else 1]
    res.update(zip(names, backward(c.g_rgb.to(dt), c.g_depth.to(dt), c.g_acc.to(dt), c.g_w.to(dt))))

    target_s, target_d = c.target_s.to(dt), c.target_d.to(dt)
    zeros_r, zeros_w = torch.zeros(nr, dtype=dt), torch.zeros_like(w)
    res["img_loss"] = ((rgb_map - target_s) ** 2).sum() / (3 * nr)
    res.update(zip(["img_" + n for n in names], backward(2. * (rgb_map - target_s) / (3 * nr), zeros_r, zeros_r, zeros_w)))
    m, t, sd = depth_map, target_d[:, 0], target_d[:, 1]
    dz = z - m[:, None]
    v = (dz ** 2 * w).sum(-1) + (0. if mutation == "v_no_eps" else 1e-5)
    applied = c.target_vd & (((m - t).abs() - sd > 0.) | (sd ** 2 < v))
    vc = v.clamp(min=1e-3)
    res["depth_loss"] = torch.where(applied, 0.5 * (torch.log(vc) + (m - t) ** 2 / vc), zeros_r).sum() / nr
    dv = torch.where(applied, 0.5 * (1. / vc - (m - t) ** 2 / vc ** 2) / nr, zeros_r)
    if mutation == "clamp_zero_grad":
        dv = dv * (v >= 1e-3)
    dm = torch.where(applied, (m - t) / vc / nr, zeros_r)
    if mutation != "detached_m":
        dm = dm + dv * (-2. * (dz * w).sum(-1))
    res.update(zip(["depth_" + n for n in names], backward(torch.zeros(nr, 3, dtype=dt), dm, zeros_r, dv[:, None] * dz ** 2)))
    return res


# ----------------------------------------------------------------------------------------------------------------------
# the cases: rays away from every decision boundary
# ----------------------------------------------------------------------------------------------------------------------
def ray_kinds(case, rays):
    """0 ordinary, 1 empty, 2 opaque, 3 thin, per ray index."""
    kind = torch.zeros(len(rays), dtype=torch.long)
    for k, key in ((1, "empty"), (2, "opaque"), (3, "thin")):
        if key in case:
            every, at = case[key]
            kind[rays % every == at] = k
    return kind


def depth_modes(case, rays):
    """0 invalid, 1 a seeded target, 2 a target the ray is inside of (not applied), per ray index."""
    mode = {"all": 1, "none_valid": 0, "none_applied": 2}.get(case["depth"])
    return torch.full((len(rays),), mode) if mode is not None else (rays % 3)


def shared_z1(case):
    gen = torch.Generator().manual_seed(7700 + NAMES.index(case["name"]))
    return torch.sort(torch.rand(case["S1"], generator=gen) * 3.9 + 0.1).values


def candidates(case, gen, rays):
    """One candidate per entry of ``rays`` (ray indices, which fix the ray's kind and depth mode) -> namespace of float32 tensors."""
    n, s1, s2 = len(rays), case["S1"], case["S2"]
    s = s1 + s2

    def rand(*shape):
        return torch.rand(*shape, generator=gen)

    def randn(*shape):
        return torch.randn(*shape, generator=gen)
    d = randn(n, 3)
    rays_d = d / d.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * rand(n, 1))
    z1 = shared_z1(case) if case["shared"] else torch.sort(rand(n, s1) * 3.9 + 0.1, -1).values
    z2 = torch.sort(rand(n, s2) * 3.9 + 0.1, -1).values if s2 else None
    raw = torch.cat([randn(n, s, 3), 3. * randn(n, s, 1)], -1)
    kind = ray_kinds(case, rays)
    if (kind == 3).any():
        assert not case["shared"]
        thin = (kind == 3)[:, None]
        z1 = torch.where(thin, 1. + (z1 - 0.1) * (0.04 / 3.9), z1)
        z2 = torch.where(thin, 1. + (z2 - 0.1) * (0.04 / 3.9), z2) if s2 else None
        raw[..., 3] = torch.where(thin, 100. * raw[..., 3], raw[..., 3])
    mag = raw[..., 3].abs()
    raw[..., 3] = torch.where(kind[:, None] == 1, -mag - 0.01, torch.where(kind[:, None] == 2, 100. * mag + 1000., raw[..., 3]))
    noise = randn(n, s) if case["noise"] else None
    if noise is not None:       # an empty ray stays empty under its noise
        noise = torch.where((kind[:, None] == 1) & (raw[..., 3] + noise > -0.005), -noise.abs(), noise)
    c = SimpleNamespace(raw1=raw[:, :s1].contiguous(), raw2=raw[:, s1:].contiguous() if s2 else None, z1=z1, z2=z2, rays_d=rays_d,
                        noise=noise, target_s=rand(n, 3), g_rgb=randn(n, 3), g_depth=randn(n), g_acc=randn(n), g_w=randn(n, s))
    mode = depth_modes(case, rays)
    c.target_vd = mode != 0
    t, sd, u = rand(n) * 3.9 + 0.1, rand(n) * 0.45 + 0.05, rand(n, 2)
    # inside: |m - t| = u0 s / 4 and s = (1.5 + u1) sqrt(v) + 0.1, from the float64 depth and variance rounded to 1 / 256
    o = ray_stage(c.raw1.double(), z1.double(), rays_d.double(), None if z2 is None else c.raw2.double(), None if z2 is None else z2.double(),
                  None if noise is None else noise.double())
    m, v, _, _ = depth_terms(o["depth_map"], o["z_vals"], o["weights"], torch.zeros(n, 2, dtype=torch.float64))
    m, sv = torch.round(m * 256) / 256, torch.ceil(v.sqrt() * 256) / 256
    sd_in = (1.5 + u[:, 1].double()) * sv + 0.1
    t_in = m + u[:, 0].double() * sd_in / 4
    c.target_d = torch.stack([torch.where(mode == 2, t_in.float(), t), torch.where(mode == 2, sd_in.float(), sd)], -1)
    return c


def margins(c, dtype=torch.float64):
    """The quantity every decision is made on, per ray (the smallest distance to the boundary over the ray's samples for sigma; inf
    where the decision is not made) -> {decision: [R]}, and the smallest gap between a z of list 1 and a z of list 2."""
    f = lambda x: None if x is None else x.to(dtype)      # noqa: E731
    raw, z, nz = merge(f(c.raw1), f(c.z1), f(c.raw2), f(c.z2), f(c.noise))
    o = dict(zip(OUTPUTS, (*raw2outputs(raw, z, f(c.rays_d), nz), z)))
    m, v, t, s = depth_terms(o["depth_map"], o["z_vals"], o["weights"], f(c.target_d))
    inf = torch.full_like(m, float("inf"))
    sigma = raw[..., 3] + (0. if nz is None else nz)
    q = {"sigma": sigma.abs().amin(-1), "outside": torch.where(c.target_vd, (m - t).abs() - s, inf),
         "spread": torch.where(c.target_vd, s.pow(2) - v, inf), "clamp": torch.where(c.target_vd, v - 1e-3, inf),
         "disp": torch.where(o["acc_map"] > 0, o["depth_map"] / o["acc_map"] - 1e-10, inf)}
    gap = torch.full_like(m, float("inf"))
    if c.z2 is not None:
        z1 = f(c.z1).expand(m.shape[0], -1) if c.z1.dim() == 1 else f(c.z1)
        gap = (z1[:, :, None] - f(c.z2)[:, None, :]).abs().amin((1, 2))
    return q, gap, dict(v=v, applied=c.target_vd & (((m - t).abs() - s > 0.) | (s.pow(2) < v)))


def pool_errors(case):
    """The float32 checker's largest error in each decision's quantity over a seeded pool of POOL candidate rays (the generator
    records 8 x these as the case's tau)."""
    gen = torch.Generator().manual_seed(7800 + NAMES.index(case["name"]))
    c = candidates(case, gen, torch.arange(POOL) % case["R"])
    q32, _, _ = margins(c, torch.float32)
    q64, _, _ = margins(c, torch.float64)
    out = {}
    for k in DECISIONS:
        ok = torch.isfinite(q64[k])
        out[k] = float((q32[k].double() - q64[k])[ok].abs().max()) if ok.any() else 0.0
    return out


def take(c, index):
    return SimpleNamespace(**{k: (v if v is None or (k == "z1" and v.dim() == 1) else v[index]) for k, v in vars(c).items()})


def case_inputs(case, tau):
    """The case's rays: every ray takes candidates, round after round, until one has all its decisions at least tau[decision] from
    their boundaries in float64 and no z shared by its two lists.  info: candidates and rejected."""
    gen = torch.Generator().manual_seed(7900 + NAMES.index(case["name"]))
    open_rays = torch.arange(case["R"])
    kept = {}
    info = dict(candidates=0, rejected=0)
    while len(open_rays):
        c = candidates(case, gen, open_rays)
        q, gap, _ = margins(c)
        ok = gap > 0
        for k in DECISIONS:
            ok &= q[k].abs() >= tau[k]
        for j in torch.nonzero(ok).flatten().tolist():
            kept[int(open_rays[j])] = take(c, j)
        info["candidates"] += len(open_rays)
        info["rejected"] += int((~ok).sum())
        open_rays = open_rays[~ok]
    rows = [kept[r] for r in range(case["R"])]
    out = SimpleNamespace(name=case["name"], case=case, info=info)
    for k, v in vars(rows[0]).items():
        setattr(out, k, v if v is None or (k == "z1" and case["shared"]) else torch.stack([getattr(r, k) for r in rows]))
    return out


def with_ties(c):
    """The inputs with list 2's first sample moved onto list 1's second (an exact tie), for the tie-order mutation."""
    z2 = c.z2.clone()
    z2[:, 0] = (c.z1.expand(z2.shape[0], -1) if c.z1.dim() == 1 else c.z1)[:, 1]
    return SimpleNamespace(**dict(vars(c), z2=torch.sort(z2, -1).values))


# ----------------------------------------------------------------------------------------------------------------------
# comparing
# ----------------------------------------------------------------------------------------------------------------------
def max_error(a, b):
    """max |a - b| over the entries that are not NaN in both (disp_map of a ray without weight); inf if one of a pair is NaN."""
    a, b = (np.asarray(x.detach() if isinstance(x, torch.Tensor) else x, dtype=np.float64).reshape(-1) for x in (a, b))
    both = np.isnan(a) & np.isnan(b)
    if both.all():
        return 0.0
    d = np.abs(a[~both] - b[~both])
    return float("inf") if np.isnan(d).any() else float(d.max())


def top_of(a):
    a = np.abs(np.asarray(a.detach() if isinstance(a, torch.Tensor) else a, dtype=np.float64).reshape(-1))
    a = a[~np.isnan(a)]
    return float(a.max()) if a.size else 0.0


def bound_of(err32, o64):
    """8 x the float32 checker's error, floored at one float32 ulp of the tensor's largest float64 magnitude; 0 for a tensor that is
    exactly zero in float64."""
    top = top_of(o64)
    if top == 0.0:
        return 0.0
    return max(FACTOR * err32, float(np.spacing(np.float32(top))))


# ----------------------------------------------------------------------------------------------------------------------
# eight Adam steps through the ray stage
# ----------------------------------------------------------------------------------------------------------------------
TRAIN_BB_CENTER, TRAIN_BB_SCALE, DEPTH_LOSS_WEIGHT = (0., 0., 0.), 0.25, 0.004      # depth_loss_weight: the reference's default (:955)


def train_inputs(c):
    """For nerf_query_ref's TRAIN_CASE inputs ``c``: its model, camera embedding and ray directions; its seeded sample depths, every
    other one to list 2 (shuffled: render_rays_train sorts them); seeded origins, colour and depth targets."""
    z, target_s = Q.train_inputs(c)
    gen = torch.Generator().manual_seed(9400)
    nr = z.shape[0]
    z2 = z[:, 1::2]
    z2 = z2[:, torch.randperm(z2.shape[1], generator=gen)].contiguous()
    return SimpleNamespace(rays_o=torch.rand(nr, 3, generator=gen) * 0.2 - 0.1, rays_d=c.viewdirs, z1=z[:, 0::2].contiguous(), z2=z2,
                           target_s=target_s,
                           target_d=torch.stack([torch.rand(nr, generator=gen) * 3.9 + 0.1, torch.rand(nr, generator=gen) * 0.2 + 0.05], -1),
                           target_vd=torch.arange(nr) % 4 != 3)


def train_loop(parameters, loss_fn):
    """Q.train_loop with loss_fn() -> the step's loss."""
    parameters = list(parameters)
    opt = torch.optim.Adam(parameters, lr=Q.TRAIN_LR, betas=(0.9, 0.999))
    losses = []
    for _ in range(Q.TRAIN_STEPS):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        torch.nn.utils.clip_grad_value_(parameters, Q.TRAIN_CLIP)
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        losses.append(loss_fn().item())
    return losses


def train_loop_host(c, dtype):
    model = R.build_model(c.state, c.cfg, dtype).train()
    embed_fn, _ = R.get_embedder(c.cfg["multires"], c.cfg["i_embed"])
    embeddirs_fn, _ = R.get_embedder(c.cfg["multires_views"], c.cfg["i_embed"])
    t = train_inputs(c)
    o, d, cam = t.rays_o.to(dtype), t.rays_d.to(dtype), c.cam.to(dtype)
    z1, z2 = t.z1.to(dtype), torch.sort(t.z2.to(dtype), -1).values
    center, scale = torch.as_tensor(TRAIN_BB_CENTER).to(dtype), torch.as_tensor(TRAIN_BB_SCALE).to(dtype)

    def query(z):
        pts = o[:, None, :] + d[:, None, :] * z[..., :, None]
        return model(Q.network_rows(pts, d, cam, embed_fn, embeddirs_fn, center, scale)).reshape(*pts.shape[:2], 4)

    def loss_fn():
        out = ray_stage(query(z1), z1, d, query(z2), z2)
        return img2mse(out["rgb_map"], t.target_s.to(dtype)) + DEPTH_LOSS_WEIGHT * depth_loss(
            out["depth_map"], out["z_vals"], out["weights"], t.target_d.to(dtype), t.target_vd)
    return train_loop(model.parameters(), loss_fn)


# ----------------------------------------------------------------------------------------------------------------------
# shared by tests/test_nerf_composite_host.py and tests/test_gpu_nerf_composite.py
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_npz():
    return dict(np.load(os.path.join(GOLDEN, "nerf_composite_golden.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(GOLDEN, "nerf_composite_bounds.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def refs(bounds):
    """case name -> (inputs, float32 checker, float64 checker): dicts of read-only numpy over tensor_names; filled on first use, with
    one thread as the golden file was recorded."""
    cache = {}

    def get(name):
        if name not in cache:
            threads = torch.get_num_threads()
            torch.set_num_threads(1)
            c = case_inputs(CASES[NAMES.index(name)], bounds["cases"][name]["tau"])
            both = []
            for dt in (torch.float32, torch.float64):
                o = {k: v.detach().numpy() for k, v in check_case(c, dt).items()}
                for v in o.values():
                    v.setflags(write=False)
                both.append(o)
            torch.set_num_threads(threads)
            cache[name] = (c, *both)
        return cache[name]
    return get
