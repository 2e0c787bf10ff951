"""Checker of the differentiable NeRF query (ops.nerf_query): host torch with a dtype argument.
  * ``query``: what run_network (data/scannet/run_nerf.py:50-65) computes on the checker model tests/nerf_extract_ref.NeRF, the
    loss sum(raw * cot) for a given cotangent, torch autograd's 24 parameter gradients and dcam, and every relu pre-activation of
    every point (8 x 256 in the trunk, 128 in the head).
  * ``manual_grads``: the same gradients written out layer by layer (the formulas the kernels implement), with the mutations of the
    sharpness test.
  * the flip-free test points (regenerated from seeds, never committed), the cases, and the eight-step Adam loop.
float64 gives the reference the GPU tests are bounded against; tests/golden/make_nerf_query_golden.py pins it to the reference.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf_extract_ref as R

CAM = (0.7, -1.3, 0.4, 2.1)
BB_CENTER, BB_SCALE = (0., 0., 0.), 1.0       # the points are normalised positions: (p - 0) * 1 is exact in every dtype
STATE_SEED = 11
PARAMS = tuple([f"pts_linears.{i}.weight" for i in range(8)]
               + ["feature_linear.weight", "alpha_linear.weight", "views_linears.0.weight", "rgb_linear.weight"]
               + [f"pts_linears.{i}.bias" for i in range(8)]
               + ["feature_linear.bias", "alpha_linear.bias", "views_linears.0.bias", "rgb_linear.bias"])
MUTATIONS = ("no_mask3", "no_mask_v", "no_skip_enc", "dh4_cols", "no_alpha_term", "bias_mean", "dcam_view_cols", "untransposed")

# name, rays x points, cfg overrides, weight family
CASES = [
    dict(name="one_point", R=1, S=1, cfg=dict(multires_views=0, input_ch_cam=4), family="a"),
    dict(name="tile_exact", R=4, S=16, cfg=dict(multires_views=0, input_ch_cam=4), family="a"),
    dict(name="tile_plus_one", R=5, S=13, cfg=dict(multires_views=0, input_ch_cam=4), family="a"),
    dict(name="straddle", R=5, S=56, cfg=dict(multires_views=4, input_ch_cam=4), family="b"),
    dict(name="no_cam", R=3, S=40, cfg=dict(multires_views=4, input_ch_cam=0), family="a"),
    dict(name="many_tiles", R=10, S=130, cfg=dict(multires_views=0, input_ch_cam=4), family="a"),
]
NAMES = [c["name"] for c in CASES]
MANY_TILES_CHUNKS = (None, 128, 64)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tensor_names(cfg):
    """The tensors a case is bounded on: raw, the 24 gradients and, with a camera embedding, dcam."""
    return ("raw",) + PARAMS + (("dcam",) if cfg["input_ch_cam"] else ())


# ----------------------------------------------------------------------------------------------------------------------
# the query and its gradients
# ----------------------------------------------------------------------------------------------------------------------
def network_rows(pts, viewdirs, cam, embed_fn, embeddirs_fn, bb_center, bb_scale):
    """The model's input rows for pts [R, S, 3] and viewdirs [R, 3]: [embed((p - centre) * scale), embed_dirs(the ray's direction),
    cam] per point, ray-major."""
    flat = (pts.reshape(-1, 3) - bb_center) * bb_scale
    dirs = embeddirs_fn(viewdirs[:, None].expand(pts.shape).reshape(-1, 3))
    return torch.cat([embed_fn(flat), dirs, cam.unsqueeze(0).expand(dirs.shape[0], cam.shape[0])], -1)


def query(state, cfg, pts, viewdirs, cam=None, cot=None, dtype=torch.float32, bb_center=BB_CENTER, bb_scale=BB_SCALE, want_pre=True):
    """-> dict: raw [R, S, 4]; with ``cot`` [R, S, 4] also grads {name: tensor} of sum(raw * cot) and dcam; pre [R * S, 2176] the relu
    pre-activations (trunk layers 0 .. 7, then views_linears.0).  float32 inputs are widened, never recomputed."""
    cfg = dict(R.DEFAULT_CFG, **(cfg or {}))
    model = R.build_model(state, cfg, dtype)
    embed_fn, _ = R.get_embedder(cfg["multires"], cfg["i_embed"])
    embeddirs_fn, _ = R.get_embedder(cfg["multires_views"], cfg["i_embed"])
    cam_t = (torch.zeros(cfg["input_ch_cam"]) if cam is None else torch.as_tensor(cam, dtype=torch.float32)).to(dtype).clone().requires_grad_(True)
    pre = []
    hooks = [l.register_forward_hook(lambda m, i, o: pre.append(o.detach())) for l in list(model.pts_linears) + [model.views_linears[0]]]
    x = network_rows(pts.to(dtype), viewdirs.to(dtype), cam_t, embed_fn, embeddirs_fn, torch.as_tensor(bb_center).to(dtype),
                     torch.as_tensor(bb_scale).to(dtype))
    raw = model(x).reshape(*pts.shape[:2], 4)
    for h in hooks:
        h.remove()
    out = {"raw": raw.detach()}
    if want_pre:
        out["pre"] = torch.cat(pre, -1)
    if cot is not None:
        params = dict(model.named_parameters())
        wrt = [params[k] for k in PARAMS] + ([cam_t] if cfg["input_ch_cam"] else [])
        g = torch.autograd.grad((raw * cot.to(dtype)).sum(), wrt)
        out["grads"] = dict(zip(PARAMS, g[:len(PARAMS)]))
        if cfg["input_ch_cam"]:
            out["grads"]["dcam"] = g[-1]
    return out


def manual_grads(state, cfg, pts, viewdirs, cam, cot, dtype=torch.float64, mutation=None, bb_center=BB_CENTER, bb_scale=BB_SCALE):
    """The gradients of sum(raw * cot) layer by layer, as csrc/nerfquery.hip computes them -> {name: tensor} (with dcam)."""
    assert mutation is None or mutation in MUTATIONS
    cfg = dict(R.DEFAULT_CFG, **(cfg or {}))
    sd = {k: v.to(dtype) for k, v in state.items()}
    embed_fn, in_ch = R.get_embedder(cfg["multires"], cfg["i_embed"])
    embeddirs_fn, views_ch = R.get_embedder(cfg["multires_views"], cfg["i_embed"])
    cam_ch = cfg["input_ch_cam"]
    cam_t = (torch.zeros(cam_ch) if cam is None else torch.as_tensor(cam, dtype=torch.float32)).to(dtype)
    x = network_rows(pts.to(dtype), viewdirs.to(dtype), cam_t, embed_fn, embeddirs_fn, torch.as_tensor(bb_center).to(dtype),
                     torch.as_tensor(bb_scale).to(dtype))
    e, xv_tail = x[:, :in_ch], x[:, in_ch:]
    ins, hs, h = [], [], e
    for i in range(8):
        ins.append(h)
        h = F.relu(F.linear(h, sd[f"pts_linears.{i}.weight"], sd[f"pts_linears.{i}.bias"]))
        hs.append(h)
        if i == 4:
            h = torch.cat([e, h], -1)
    f = F.linear(hs[7], sd["feature_linear.weight"], sd["feature_linear.bias"])
    xv = torch.cat([f, xv_tail], -1)
    v = F.relu(F.linear(xv, sd["views_linears.0.weight"], sd["views_linears.0.bias"]))
    draw = cot.to(dtype).reshape(-1, 4)
    d_rgb, d_sig = draw[:, :3], draw[:, 3:4]

    def bias(dy):
        return dy.mean(0) if mutation == "bias_mean" else dy.sum(0)
    g = {"rgb_linear.weight": d_rgb.T @ v, "rgb_linear.bias": bias(d_rgb)}
    dv = d_rgb @ sd["rgb_linear.weight"]
    if mutation != "no_mask_v":
        dv = dv * (v > 0)
    wv = sd["views_linears.0.weight"]
    g["views_linears.0.weight"], g["views_linears.0.bias"] = dv.T @ xv, bias(dv)
    c0 = 256 if mutation == "dcam_view_cols" else 256 + views_ch
    g["dcam"] = dv.sum(0) @ wv[:, c0:c0 + cam_ch]
    df = dv @ wv[:, :256]
    g["feature_linear.weight"], g["feature_linear.bias"] = df.T @ hs[7], bias(df)
    g["alpha_linear.weight"], g["alpha_linear.bias"] = d_sig.T @ hs[7], bias(d_sig)
    dh = df @ sd["feature_linear.weight"]
    if mutation != "no_alpha_term":
        dh = dh + d_sig * sd["alpha_linear.weight"]
    for i in range(7, -1, -1):
        dy = dh if (mutation == "no_mask3" and i == 3) else dh * (hs[i] > 0)
        dw = dy.T @ ins[i]
        if i == 5 and mutation == "no_skip_enc":
            dw[:, :in_ch] = 0
        g[f"pts_linears.{i}.weight"], g[f"pts_linears.{i}.bias"] = dw, bias(dy)
        if i > 0:
            w = sd[f"pts_linears.{i}.weight"]
            if i == 5:
                w = w[:, :256] if mutation == "dh4_cols" else w[:, in_ch:]
            dh = dy @ (w.T if (mutation == "untransposed" and i == 2) else w)
    if not cam_ch:
        del g["dcam"]
    return g


# ----------------------------------------------------------------------------------------------------------------------
# flip-free points
# ----------------------------------------------------------------------------------------------------------------------
def case_cfg(case):
    return dict(R.DEFAULT_CFG, **case["cfg"])


def case_state(case):
    return R.make_state(STATE_SEED, case["family"], case_cfg(case))


def case_cam(case):
    return torch.tensor(CAM[:case["cfg"]["input_ch_cam"]], dtype=torch.float32) if case["cfg"]["input_ch_cam"] else None


def candidates(gen, n):
    """n normalised positions uniform in [-1, 1]^3."""
    return torch.rand(n, 3, generator=gen) * 2 - 1


def unit_dirs(gen, n):
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return (d / d.norm(dim=-1, keepdim=True)).float()


POOL = 1024


def pool_error(case):
    """The float32 checker's largest pre-activation error over a seeded pool of POOL candidates on the case's rays (the generator
    records 8 x this as the case's tau)."""
    gen = torch.Generator().manual_seed(8000 + NAMES.index(case["name"]))
    state, cfg, cam = case_state(case), case_cfg(case), case_cam(case)
    viewdirs = unit_dirs(torch.Generator().manual_seed(9000 + NAMES.index(case["name"])), case["R"])
    cand, dirs = candidates(gen, POOL)[:, None], viewdirs[torch.arange(POOL) % case["R"]]
    o32, o64 = (query(state, cfg, cand, dirs, cam, dtype=dt) for dt in (torch.float32, torch.float64))
    return float((o32["pre"].double() - o64["pre"]).abs().max())


def draw_points(case, tau):
    """The case's points: every slot (ray, sample) takes candidates from the seeded pool, round after round, until one has all its
    2176 float64 pre-activations at least tau from zero -> (pts [R, S, 3], viewdirs [R, 3], info).  info: candidates and rejected."""
    index = NAMES.index(case["name"])
    gen = torch.Generator().manual_seed(9000 + index)
    nr, ns = case["R"], case["S"]
    state, cfg, cam = case_state(case), case_cfg(case), case_cam(case)
    viewdirs = unit_dirs(gen, nr)
    pts = torch.zeros(nr * ns, 3)
    ray_of = torch.arange(nr * ns) // ns
    open_slots = torch.arange(nr * ns)
    info = dict(candidates=0, rejected=0)
    while len(open_slots):
        cand = candidates(gen, len(open_slots))
        # a candidate meets its slot's ray: one "ray" of one point each
        o64 = query(state, cfg, cand[:, None], viewdirs[ray_of[open_slots]], cam, dtype=torch.float64)
        ok = o64["pre"].abs().amin(-1) >= tau
        pts[open_slots[ok]] = cand[ok]
        info["candidates"] += len(cand)
        info["rejected"] += int((~ok).sum())
        open_slots = open_slots[~ok]
    return pts.reshape(nr, ns, 3), viewdirs, info


def case_inputs(case, tau):
    """Everything a case needs, regenerated from seeds; tau: the case's recorded threshold."""
    pts, viewdirs, info = draw_points(case, tau)
    gen = torch.Generator().manual_seed(9100 + NAMES.index(case["name"]))
    cot = torch.randn(case["R"], case["S"], 4, generator=gen)
    return SimpleNamespace(name=case["name"], cfg=case_cfg(case), state=case_state(case), cam=case_cam(case), pts=pts, viewdirs=viewdirs,
                           cot=cot, info=info, bb_center=BB_CENTER, bb_scale=BB_SCALE)


def check_case(c, dtype):
    o = query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot, dtype)
    return dict(o["grads"], raw=o["raw"])


# ----------------------------------------------------------------------------------------------------------------------
# eight Adam steps
# ----------------------------------------------------------------------------------------------------------------------
TRAIN_CASE, TRAIN_STEPS, TRAIN_LR, TRAIN_CLIP = "tile_plus_one", 8, 5e-4, 0.1


def train_inputs(c):
    """Sample depths and a target colour per ray for the loop on case inputs ``c`` (the points need not lie on the rays)."""
    gen = torch.Generator().manual_seed(9200)
    nr, ns = c.pts.shape[:2]
    z = torch.sort(torch.rand(nr, ns, generator=gen) * 3.9 + 0.1, -1).values
    return z, torch.rand(nr, 3, generator=gen)


def composite_loss(raw, z, rays_d, target):
    """sigmoid, compute_weights (run_nerf.py:419-429) with |d| and the 1e10 last distance, rgb_map (:450-452), img2mse."""
    dists = torch.cat([z[..., 1:] - z[..., :-1], torch.full_like(z[..., :1], 1e10)], -1) * torch.norm(rays_d[..., None, :], dim=-1)
    alpha = 1. - torch.exp(-F.relu(raw[..., 3]) * dists)
    trans = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1. - alpha + 1e-10], -1), -1)[..., :-1]
    rgb_map = torch.sum((alpha * trans)[..., None] * torch.sigmoid(raw[..., :3]), -2)
    return torch.mean((rgb_map - target) ** 2)


def train_loop(parameters, query_fn, z, rays_d, target):
    """TRAIN_STEPS of Adam at TRAIN_LR with clip_grad_value_(TRAIN_CLIP), as train_nerf has them (:848-849) -> the loss before every
    step and after the last, TRAIN_STEPS + 1 Python floats.  query_fn() -> raw [R, S, 4] from the current parameters."""
    parameters = list(parameters)
    opt = torch.optim.Adam(parameters, lr=TRAIN_LR, betas=(0.9, 0.999))
    losses = []
    for _ in range(TRAIN_STEPS):
        opt.zero_grad()
        loss = composite_loss(query_fn(), z, rays_d, target)
        loss.backward()
        torch.nn.utils.clip_grad_value_(parameters, TRAIN_CLIP)
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        losses.append(composite_loss(query_fn(), z, rays_d, target).item())
    return losses


def train_loop_host(c, dtype):
    cfg = c.cfg
    model = R.build_model(c.state, cfg, dtype).train()
    embed_fn, _ = R.get_embedder(cfg["multires"], cfg["i_embed"])
    embeddirs_fn, _ = R.get_embedder(cfg["multires_views"], cfg["i_embed"])
    z, target = train_inputs(c)
    pts, viewdirs, cam = c.pts.to(dtype), c.viewdirs.to(dtype), c.cam.to(dtype)
    center, scale = torch.as_tensor(c.bb_center).to(dtype), torch.as_tensor(c.bb_scale).to(dtype)

    def query_fn():
        return model(network_rows(pts, viewdirs, cam, embed_fn, embeddirs_fn, center, scale)).reshape(*pts.shape[:2], 4)
    return train_loop(model.parameters(), query_fn, z.to(dtype), viewdirs, target.to(dtype))


# ----------------------------------------------------------------------------------------------------------------------
# what the golden file keeps of a tensor
# ----------------------------------------------------------------------------------------------------------------------
SAMPLES = 16


def summary(name, index, t):
    """sum, absolute sum and SAMPLES entries at seeded positions of a tensor -> float64 array [2 + SAMPLES]."""
    flat = np.ascontiguousarray(torch.as_tensor(t).detach().reshape(-1).double().numpy())       # numpy's sums: one thread, one order
    gen = torch.Generator().manual_seed(9300 + 31 * index + sum(map(ord, name)))
    pos = torch.randint(0, flat.size, (SAMPLES,), generator=gen).numpy()
    return np.concatenate([[flat.sum(), np.abs(flat).sum()], flat[pos]])


# ----------------------------------------------------------------------------------------------------------------------
# shared by tests/test_nerf_query_host.py and tests/test_gpu_nerf_query.py
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_npz():
    return dict(np.load(os.path.join(GOLDEN, "nerf_query.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(GOLDEN, "nerf_query_bounds.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def refs(bounds):
    """case name -> (inputs, float32 checker, float64 checker): dicts of read-only numpy over raw, the gradients and dcam; filled on
    first use, with one thread as the golden file was recorded."""
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
