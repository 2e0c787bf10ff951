"""Checker of the NeRF grid extraction (scripts/nerf_extract.py, ops.nerf_grid_query): a torch restatement, with a dtype argument, of
  * the MLP the reference's run_nerf.py imports from the Dense-Depth-Priors NeRF code (``NeRF``, ``get_embedder``: the nerf-pytorch
    model plus a camera embedding; the assumed model of DESIGN.md 3.16),
  * what ``run_network`` (data/scannet/run_nerf.py:50-65) and ``extract_nerf`` (:1157-1194) compute, in the reference's order of
    arithmetic -- every pose through the whole network, sigmoid(rgb) summed in pose order, sigma of the last pose,
  * the scene-bounds formula (:1063-1072 with the fork's get_rays).
It also builds deterministic weights from a seed (regenerated, never committed) and the cases the golden file and the tests share.
Host-only torch; float64 gives the reference the GPU tests are bounded against.
"""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

MUTATIONS = ("no_skip", "swap_sincos", "plus_z", "last_pose", "swap_xz")
DEFAULT_CFG = dict(netdepth=8, netwidth=256, multires=9, multires_views=0, input_ch_cam=4, use_viewdirs=True, N_importance=0, i_embed=0)


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
class Embedder:
    def __init__(self, multires, swap_sincos=False):
        self.freq_bands = 2. ** torch.linspace(0., multires - 1, steps=multires)
        self.fns = (torch.cos, torch.sin) if swap_sincos else (torch.sin, torch.cos)
        self.out_dim = 3 + 6 * multires

    def __call__(self, x):
        out = [x]
        for freq in self.freq_bands:
            for fn in self.fns:
                out.append(fn(x * freq.to(x.dtype)))
        return torch.cat(out, -1)


def get_embedder(multires, i=0, swap_sincos=False):
    if i == -1:
        return nn.Identity(), 3
    e = Embedder(multires, swap_sincos)
    return e, e.out_dim


class NeRF(nn.Module):
    def __init__(self, D=8, W=256, input_ch=3, input_ch_views=3, input_ch_cam=0, output_ch=4, skips=[4], use_viewdirs=False):
        super().__init__()
        self.D, self.W, self.input_ch, self.input_ch_views, self.input_ch_cam = D, W, input_ch, input_ch_views, input_ch_cam
        self.skips, self.use_viewdirs = skips, use_viewdirs
        self.pts_linears = nn.ModuleList(
            [nn.Linear(input_ch, W)] + [nn.Linear(W, W) if i not in skips else nn.Linear(W + input_ch, W) for i in range(D - 1)])
        self.views_linears = nn.ModuleList([nn.Linear(input_ch_views + input_ch_cam + W, W // 2)])
        if use_viewdirs:
            self.feature_linear = nn.Linear(W, W)
            self.alpha_linear = nn.Linear(W, 1)
            self.rgb_linear = nn.Linear(W // 2, 3)
        else:
            self.output_linear = nn.Linear(W, output_ch)
        self.drop_skip = False      # mutation "no_skip": the concatenated encoding is zeroed

    def forward(self, x):
        input_pts, input_views = torch.split(x, [self.input_ch, self.input_ch_views + self.input_ch_cam], dim=-1)
        h = input_pts
        for i, l in enumerate(self.pts_linears):
            h = F.relu(l(h))
            if i in self.skips:
                h = torch.cat([torch.zeros_like(input_pts) if self.drop_skip else input_pts, h], -1)
        if not self.use_viewdirs:
            return self.output_linear(h)
        alpha = self.alpha_linear(h)
        feature = self.feature_linear(h)
        h = torch.cat([feature, input_views], -1)
        for l in self.views_linears:
            h = F.relu(l(h))
        rgb = self.rgb_linear(h)
        return torch.cat([rgb, alpha], -1)


def network_input(points, embed_pts, embed_dirs, viewdir, cam_ch, bb_center, bb_scale):
    """One pose's input rows of the model (what run_network, run_nerf.py:50-65, assembles): [embed((x - centre) * scale),
    embed_dirs(d) repeated for every row, cam_ch zeros]."""
    e = embed_pts((points - bb_center) * bb_scale)
    n = e.shape[0]
    return torch.cat([e, embed_dirs(viewdir.reshape(1, 3)).expand(n, -1), e.new_zeros(n, cam_ch)], -1)


# ----------------------------------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------------------------------
def make_state(seed, family="a", cfg=None, prefix=""):
    """Deterministic float32 state dict of the model: torch's default Linear init (uniform in +-1 / sqrt(fan_in)) from a seeded
    generator, weights x 1.6 and biases x 3 so the relus neither die nor saturate (family "a"); family "b" also multiplies
    alpha_linear.weight by 300 so sigma takes both signs up to about 1e2."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    W, D = cfg["netwidth"], cfg["netdepth"]
    input_ch, views = 3 + 6 * cfg["multires"], 3 + 6 * cfg["multires_views"]
    shapes = [(f"pts_linears.{i}", W, input_ch if i == 0 else W + input_ch if i == 5 else W) for i in range(D)]
    shapes += [("feature_linear", W, W), ("alpha_linear", 1, W), ("views_linears.0", W // 2, views + cfg["input_ch_cam"] + W),
               ("rgb_linear", 3, W // 2)]
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, out_ch, in_ch in shapes:
        bound = 1.0 / math.sqrt(in_ch)
        sd[f"{prefix}{name}.weight"] = ((torch.rand(out_ch, in_ch, generator=g) * 2 - 1) * bound * 1.6).float()
        sd[f"{prefix}{name}.bias"] = ((torch.rand(out_ch, generator=g) * 2 - 1) * bound * 3).float()
    if family == "b":
        sd[f"{prefix}alpha_linear.weight"] = sd[f"{prefix}alpha_linear.weight"] * 300
    elif family != "a":
        raise ValueError(family)
    return sd


def build_model(state, cfg=None, dtype=torch.float32):
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    state = {k[len("module."):] if k.startswith("module.") else k: v for k, v in state.items()}
    m = NeRF(D=cfg["netdepth"], W=cfg["netwidth"], input_ch=3 + 6 * cfg["multires"], output_ch=4, skips=[4],
             input_ch_views=3 + 6 * cfg["multires_views"], input_ch_cam=cfg["input_ch_cam"], use_viewdirs=True)
    m.load_state_dict(state)
    return m.to(dtype).eval()


# ----------------------------------------------------------------------------------------------------------------------
# grid
# ----------------------------------------------------------------------------------------------------------------------
def scene_bounding_box(bbox):
    """Float32 corner-wise min and max over the instances of a parsed bbox json (get_scene_bounding_box, run_nerf.py:1197-1210)."""
    lo = torch.tensor([inst["min_pt"] for inst in bbox["instances"]]).amin(0)
    hi = torch.tensor([inst["max_pt"] for inst in bbox["instances"]]).amax(0)
    return lo, hi


def grid_axes(lo, hi, max_res):
    """[res_x, res_y, res_z] = round(extent / largest extent * max_res), half to even, and the three float32 linspace arrays
    (run_nerf.py:1160-1168)."""
    extent = hi - lo
    res = torch.round(extent / extent.max() * max_res).int().tolist()
    return (res, *(torch.linspace(lo[a], hi[a], res[a]) for a in range(3)))


def grid_points(xs, ys, zs, swap_xz=False):
    """(N, 3) rows in the reference's order (run_nerf.py:1170-1171): meshgrid(z, y, x) flattened."""
    if swap_xz:
        x, y, z = torch.meshgrid(xs, ys, zs, indexing="ij")
    else:
        z, y, x = torch.meshgrid(zs, ys, xs, indexing="ij")
    return torch.stack([x, y, z], dim=-1).reshape(-1, 3)


def flat_to_wlh(flat, resolution):
    """The README's transform of the reference's (N, 4) array into the (W, L, H, 4) grid datasets.py reads."""
    res = resolution
    return np.ascontiguousarray(np.asarray(flat).reshape(res[2], res[1], res[0], -1).transpose(2, 1, 0, 3))


# ----------------------------------------------------------------------------------------------------------------------
# extraction
# ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def extract(state, cfg, xs, ys, zs, bb_center, bb_scale, poses, dtype=torch.float32, mutation=None):
    """extract_nerf (run_nerf.py:1157-1194) in the reference's order of arithmetic -> (N, 4) tensor of ``dtype``: every pose through
    the whole network, sigmoid(rgb) added up in pose order and divided by P, sigma from the last pose.  float32 inputs are widened,
    never recomputed: the grid coordinates, centre, scale and poses are the float32 values in every dtype."""
    assert mutation is None or mutation in MUTATIONS
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    model = build_model(state, cfg, dtype)
    model.drop_skip = mutation == "no_skip"
    swap = mutation == "swap_sincos"
    embed_pts, _ = get_embedder(cfg["multires"], cfg["i_embed"], swap_sincos=swap)
    embed_dirs, _ = get_embedder(cfg["multires_views"], cfg["i_embed"], swap_sincos=swap)
    points = grid_points(xs, ys, zs, swap_xz=mutation == "swap_xz").to(dtype)
    look = torch.tensor([0, 0, 1 if mutation == "plus_z" else -1], dtype=dtype)
    total = torch.zeros((points.shape[0], 3), dtype=dtype)
    for pose in poses.to(dtype):
        out = model(network_input(points, embed_pts, embed_dirs, pose[:3, :3] @ look, cfg["input_ch_cam"], bb_center.to(dtype),
                                  bb_scale.to(dtype)))
        colour = torch.sigmoid(out[:, :3])
        total = colour * len(poses) if mutation == "last_pose" else total + colour
    return torch.cat([total / len(poses), out[:, 3:4]], dim=1)


@torch.no_grad()
def view_table(state, cfg, poses, dtype=torch.float32):
    """c_p = W_d embed_dirs(d_p) + b of views_linears.0, (P, W / 2): the pose-dependent part of the hoisted head (camera part zero)."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    sd = {k[len("module."):] if k.startswith("module.") else k: v for k, v in state.items()}
    W = cfg["netwidth"]
    embeddirs_fn, ch = get_embedder(cfg["multires_views"], cfg["i_embed"])
    d = poses.to(dtype)[:, :3, :3] @ torch.tensor([0, 0, -1], dtype=dtype)
    wv = sd["views_linears.0.weight"].to(dtype)
    return embeddirs_fn(d) @ wv[:, W:W + ch].T + sd["views_linears.0.bias"].to(dtype)


@torch.no_grad()
def extract_hoisted(state, cfg, xs, ys, zs, bb_center, bb_scale, poses, dtype=torch.float32):
    """The formulation the kernels use: trunk once per point, g = W_f f, then per pose relu(g + c_p) through rgb_linear."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    sd = {k[len("module."):] if k.startswith("module.") else k: v.to(dtype) for k, v in state.items()}
    W = cfg["netwidth"]
    embed_fn, _ = get_embedder(cfg["multires"], cfg["i_embed"])
    p = (grid_points(xs, ys, zs).to(dtype) - bb_center.to(dtype)) * bb_scale.to(dtype)
    e = embed_fn(p)
    h = e
    for i in range(cfg["netdepth"]):
        h = F.relu(F.linear(h, sd[f"pts_linears.{i}.weight"], sd[f"pts_linears.{i}.bias"]))
        if i == 4:
            h = torch.cat([e, h], -1)
    sigma = F.linear(h, sd["alpha_linear.weight"], sd["alpha_linear.bias"])
    f = F.linear(h, sd["feature_linear.weight"], sd["feature_linear.bias"])
    g = f @ sd["views_linears.0.weight"][:, :W].T
    ctab = view_table(state, cfg, poses, dtype)
    acc = torch.zeros((p.shape[0], 3), dtype=dtype)
    for c in ctab:
        acc += torch.sigmoid(F.linear(F.relu(g + c), sd["rgb_linear.weight"], sd["rgb_linear.bias"]))
    return torch.cat([acc / len(ctab), sigma], dim=1)


# ----------------------------------------------------------------------------------------------------------------------
# scene bounds
# ----------------------------------------------------------------------------------------------------------------------
def far_points(H, W, intrinsic, c2w, far):
    """(H, W, 3) points at distance factor ``far`` along the ray of every pixel: camera direction [(u - cx) / fx, -(v - cy) / fy, -1]
    for column u and row v, rotated by R, from the camera position t (the assumed get_rays)."""
    fx, fy, cx, cy = intrinsic
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cam = torch.stack([(u - cx) / fx, -(v - cy) / fy, torch.full_like(u, -1.0)], -1)
    world = (cam[..., None, :] * c2w[:3, :3]).sum(-1)
    return c2w[:3, 3] + world * far


def scene_bounds(H, W, intrinsics, poses, far):
    """Scene normalisation of run_nerf.py:1063-1072 over every pixel of every training frame -> (bb_center, bb_scale, lo, hi): lo / hi
    the extremes of the far points, clamped as the reference's running min / max from +-1e6 are."""
    pts = torch.stack([far_points(H, W, k, p, far) for k, p in zip(torch.as_tensor(intrinsics), torch.as_tensor(poses))]).reshape(-1, 3)
    hi = pts.amax(0).clamp_min(-1e6)
    lo = pts.amin(0).clamp_max(1e6)
    return (hi + lo) / 2., 2. / (hi - lo).max(), lo, hi


# ----------------------------------------------------------------------------------------------------------------------
# the shared cases
# ----------------------------------------------------------------------------------------------------------------------
def make_poses(seed, n):
    """n camera-to-world matrices (n, 4, 4) float32: random rotations, positions inside a room."""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.linalg.det(q))[:, None, None]
    poses = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    poses[:, :3, :3] = q
    poses[:, :3, 3] = torch.rand(n, 3, generator=g, dtype=torch.float64) * torch.tensor([4.0, 3.0, 1.5]) + torch.tensor([-2.0, -1.5, 0.5])
    return poses.float()


def bbox_for(extent, lo=(-1.7, -1.3, 0.1)):
    """A two-instance bbox json whose scene box is lo .. lo + extent."""
    lo = np.asarray(lo, dtype=np.float64)
    hi = lo + np.asarray(extent, dtype=np.float64)
    mid = (lo + hi) / 2
    return {"instances": [{"min_pt": lo.tolist(), "max_pt": mid.tolist()}, {"min_pt": (lo + 0.25 * (hi - lo)).tolist(), "max_pt": hi.tolist()}]}


# name, bbox extent (res = round(extent / max * max_res)), max_res, expected resolution, poses, family, cfg overrides
CASES = [
    dict(name="odd_7x6x5", extent=(3.5, 3.0, 2.5), max_res=7, res=[7, 6, 5], P=5, family="a", cfg={}),
    dict(name="line_1x1x3", extent=(0.5, 0.5, 1.5), max_res=3, res=[1, 1, 3], P=1, family="b", cfg={}),
    dict(name="tiles_9x8x8", extent=(4.5, 4.0, 4.0), max_res=9, res=[9, 8, 8], P=70, family="b", cfg={}),
    dict(name="views_5x4x3", extent=(2.5, 2.0, 1.5), max_res=5, res=[5, 4, 3], P=3, family="a", cfg=dict(input_ch_cam=0, multires_views=2)),
    # 2.5 and 1.5 exactly: half to even gives 2 and 2 (half away from zero would give 3 and 2)
    dict(name="half_4x2x2", extent=(4.0, 2.5, 1.5), max_res=4, res=[4, 2, 2], P=2, family="a", cfg={}, lo=(0.0, 0.0, 0.0)),
]


def case_inputs(case, index=None):
    """Everything a case needs, regenerated: bbox json, cfg, state, axes, bounds, poses."""
    index = [c["name"] for c in CASES].index(case["name"]) if index is None else index
    cfg = dict(DEFAULT_CFG, **case["cfg"])
    bbox = bbox_for(case["extent"], case.get("lo", (-1.7, -1.3, 0.1)))
    min_xyz, max_xyz = scene_bounding_box(bbox)
    res, xs, ys, zs = grid_axes(min_xyz, max_xyz, case["max_res"])
    poses = make_poses(100 + index, case["P"])
    bb_center = ((max_xyz + min_xyz) / 2 + torch.tensor([0.11, -0.07, 0.05])).float()
    bb_scale = (2.0 / ((max_xyz - min_xyz).max() * 1.25)).float()
    state = make_state(10 + index, case["family"], cfg)
    return SimpleNamespace(name=case["name"], cfg=cfg, bbox=bbox, min_xyz=min_xyz, max_xyz=max_xyz, res=res, xs=xs, ys=ys, zs=zs,
                           poses=poses, bb_center=bb_center, bb_scale=bb_scale, state=state, max_res=case["max_res"])


def write_bbox_json(path, bbox):
    with open(path, "w") as f:
        json.dump(bbox, f)


# ----------------------------------------------------------------------------------------------------------------------
# the kernels' order of operations, emulated (csrc/nerfgrid.hip)
# ----------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, one rounding to float64 and one to float32 follow."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _mfma_gemm(x, w):
    """x [N, K] times w [out, K]^T as the trunk's chain of v_mfma_f32_32x32x2_f32: within a group of 8 k, step j adds k = 8 kg + j, then
    k = 8 kg + 4 + j."""
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for kg in range(x.shape[1] // 8):
        for j in range(4):
            for h in range(2):
                k = 8 * kg + 4 * h + j
                acc = _fma32(x[:, k:k + 1], w[None, :, k], acc)
    return acc


def extract_kernel_order(state, cfg, xs, ys, zs, bb_center, bb_scale, poses):
    """The float32 arithmetic of the HIP kernels in their order (host sin / cos / exp in place of the device's): 64-column zero-padded
    encoding, k-permuted fmaf chains, alpha_linear as one chain in k order, the head's 128-term chains and the pose-ordered sum."""
    cfg = dict(DEFAULT_CFG, **(cfg or {}))
    sd = {(k[len("module."):] if k.startswith("module.") else k): v.numpy() for k, v in state.items()}
    ch = 3 + 6 * cfg["multires"]
    pts = ((grid_points(xs, ys, zs) - bb_center) * bb_scale).numpy()
    e = [pts]
    for l in range(cfg["multires"]):
        a = pts * np.float32(2.0 ** l)
        e += [np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)]
    e = np.concatenate(e + [np.zeros((len(pts), 64 - ch), np.float32)], 1)

    def pad(w):
        return np.concatenate([w[:, :ch], np.zeros((w.shape[0], 64 - ch), np.float32), w[:, ch:]], 1)
    h = None
    for i in range(8):
        w, b = sd[f"pts_linears.{i}.weight"], sd[f"pts_linears.{i}.bias"]
        acc = _mfma_gemm(e, pad(w)) if i == 0 else _mfma_gemm(np.concatenate([e, h], 1), pad(w)) if i == 5 else _mfma_gemm(h, w)
        h = np.maximum(acc + b, np.float32(0))
    sigma = np.zeros(len(h), np.float32)
    for k in range(256):
        sigma = _fma32(h[:, k], np.broadcast_to(sd["alpha_linear.weight"][0, k], sigma.shape), sigma)
    sigma = sigma + sd["alpha_linear.bias"][0]
    f = _mfma_gemm(h, sd["feature_linear.weight"]) + sd["feature_linear.bias"]
    g = _mfma_gemm(f, sd["views_linears.0.weight"][:, :256])
    acc = np.zeros((len(h), 3), np.float32)
    one = np.float32(1)
    for c in view_table(state, cfg, poses).numpy():
        v = np.maximum(g + c, np.float32(0))
        r = np.zeros((len(h), 3), np.float32)
        for j in range(128):
            r = _fma32(sd["rgb_linear.weight"][None, :, j], v[:, j:j + 1], r)
        acc = acc + one / (one + np.exp(-(r + sd["rgb_linear.bias"])).astype(np.float32))
    return np.concatenate([acc / np.float32(len(poses)), sigma[:, None]], 1)


# ----------------------------------------------------------------------------------------------------------------------
# shared by tests/test_nerf_extract_host.py and tests/test_gpu_nerf_extract.py
# ----------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden_npz():
    return dict(np.load(os.path.join(GOLDEN, "nerf_extract.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(GOLDEN, "nerf_extract_bounds.json")) as f:
        return json.load(f)["cases"]


def write_run(tmp_path, c, layout="flat", prefix="module.", bounds_from_rays=None):
    """A checkpoint directory, bbox json and transforms json for case inputs ``c`` -> (argv of nerf_extract, paths)."""
    tmp = str(tmp_path)
    exp = os.path.join(tmp, "ckpt", "run1")
    os.makedirs(exp)
    with open(os.path.join(exp, "args.json"), "w") as f:
        json.dump(dict(c.cfg, expname="run1", lrate=5e-4, scene_id="scene0000_00"), f)
    state = {prefix + k: v for k, v in c.state.items()}
    torch.save({"global_step": 1, "network_fn_state_dict": {k: torch.zeros_like(v) for k, v in state.items()}},
               os.path.join(exp, "100000.tar"))
    torch.save({"global_step": 2, "network_fn_state_dict": state}, os.path.join(exp, "200000.tar"))
    torch.save({"global_step": 3, "network_fn_state_dict": {}}, os.path.join(exp, "200500.tar"))       # not a *000.tar name
    bbox_json = os.path.join(tmp, "bbox.json")
    write_bbox_json(bbox_json, c.bbox)
    scene = os.path.join(tmp, "data", "scene0000_00")
    os.makedirs(scene)
    frames = [{"transform_matrix": p.tolist(), "fx": 580.0 + k, "fy": 585.0, "cx": 319.5, "cy": 239.5} for k, p in enumerate(c.poses)]
    with open(os.path.join(scene, "transforms_train.json"), "w") as f:
        json.dump({"frames": frames, "far": 4.5}, f)
    argv = ["--expname", "run1", "--ckpt_dir", os.path.join(tmp, "ckpt"), "--data_dir", os.path.join(tmp, "data"), "--scene_id",
            "scene0000_00", "--max_res", str(c.max_res), "--extract_dir", os.path.join(tmp, "out"), "--bbox_json", bbox_json,
            "--layout", layout]
    if bounds_from_rays:
        argv += ["--image_hw", *map(str, bounds_from_rays)]
    else:
        argv += ["--bb_center", *(repr(float(v)) for v in c.bb_center), "--bb_scale", repr(float(c.bb_scale))]
    return argv, dict(exp=exp, bbox_json=bbox_json, scene=scene)
