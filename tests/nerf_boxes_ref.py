"""Checker of the NeRF render restricted to 3D boxes (ops.nerf_render_boxes, scripts/nerf_render_boxes.py):
tests/nerf_render_ref.py's render, in float32 and in float64, with the mask placed after each query.

A sample's world point is o + d z in the render's dtype (in float32: the product rounded, then the sum, what the kernels form).  It
is inside a box -- 8 doubles: centre, half extents, cos(theta), sin(theta), ops.nerf_box_table's rows -- if in float64
|R(-theta)(p - c)| <= the half extent on each axis.  It counts if it is inside at least one box (keep) or none (remove); the four
raw values of every other sample are +0 after the query of each pass, so the second list is drawn from the masked raw1 and masked
again.  A sample is *undecided* if its float64 distance to a face of a box is below 1e-5 of that box's smallest extent: there an ulp
of the float32 point can change the answer, and a ray with such a sample is left out of every comparison.  Host-only torch / numpy.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nerf_extract_ref as R
import nerf_render_ref as V

MUTATIONS = ("theta_sign", "full_extents", "pass2_unmasked", "draw_unmasked", "swap_modes")
MODES = ("keep", "remove")
TENSORS = ("rgb_map", "depth_map", "acc_map", "disp_map", "depth_std", "raw1", "z2")
UNDECIDED = 1e-5          # of a box's smallest extent
MAX_LEFT_OUT = 0.10       # of a case's rays
TILE = 64
FACTOR = 8.0              # tests/nerf_train_ref.FACTOR, the project's factor on the float32 checker's deviation


# ----------------------------------------------------------------------------------------------------------------------
# boxes
# ----------------------------------------------------------------------------------------------------------------------
def box_table(boxes):
    """The same 8 doubles per box the op hands the kernels."""
    from nerf_rpn_amd import ops
    return ops.nerf_box_table(boxes)


def _local(p, b, mutation=None):
    """p [..., 3] float64, one table row -> |R(-theta)(p - c)| per axis and the half extents."""
    c, h, cs, sn = b[:3], b[3:6], b[6], b[7]
    if mutation == "theta_sign":
        sn = -sn
    if mutation == "full_extents":
        h = 2.0 * h
    dx, dy, dz = p[..., 0] - c[0], p[..., 1] - c[1], p[..., 2] - c[2]
    u, v = cs * dx + sn * dy, cs * dy - sn * dx
    return np.stack([np.abs(u), np.abs(v), np.abs(dz)], -1), h


def inside(points, table, mutation=None):
    """points [..., 3] (any float dtype, widened) -> bool [...]: inside at least one box of table [K, 8], closed faces, float64."""
    p = np.asarray(points, dtype=np.float64)
    out = np.zeros(p.shape[:-1], dtype=bool)
    for b in np.asarray(table, dtype=np.float64).reshape(-1, 8):
        q, h = _local(p, b, mutation)
        out |= (q <= h).all(-1)
    return out


def counted(points, table, mode, mutation=None):
    assert mode in MODES
    ins = inside(points, table, mutation)
    keep = (mode == "keep") != (mutation == "swap_modes")
    return ins if keep else ~ins


def undecided(points, table):
    """bool [...]: within UNDECIDED x the smallest extent of a face of some box (the face itself, not its plane far from the box)."""
    p = np.asarray(points, dtype=np.float64)
    out = np.zeros(p.shape[:-1], dtype=bool)
    for b in np.asarray(table, dtype=np.float64).reshape(-1, 8):
        q, h = _local(p, b)
        tol = UNDECIDED * 2.0 * h.min()
        out |= (np.abs(q - h) < tol).any(-1) & (q <= h + tol).all(-1)
    return out


def face_margin(points, table):
    """The smallest distance of a point to a face of a box, in units of that box's smallest extent (inf without boxes)."""
    p = np.asarray(points, dtype=np.float64)
    best = np.inf
    for b in np.asarray(table, dtype=np.float64).reshape(-1, 8):
        q, h = _local(p, b)
        near = (q <= h + 0.05 * h.min()).all(-1)
        d = np.abs(q - h).min(-1) / (2.0 * h.min())
        if near.any():
            best = min(best, d[near].min())
    return best


def tiles_counted(mask, chunk=None):
    """mask bool [R, S] of one pass -> the 64-point tiles, ray-major per chunk of rays, that hold a counted point."""
    n = mask.shape[0]
    chunk = n if chunk is None else min(chunk, n)
    total = 0
    for r0 in range(0, n, chunk):
        flat = mask[r0:r0 + chunk].reshape(-1)
        flat = np.concatenate([flat, np.zeros(-len(flat) % TILE, dtype=bool)])
        total += int(flat.reshape(-1, TILE).any(1).sum())
    return total


def tiles_total(n, s, chunk=None):
    chunk = n if chunk is None else min(chunk, n)
    return sum(-(-min(chunk, n - r0) * s // TILE) for r0 in range(0, n, chunk))


# ----------------------------------------------------------------------------------------------------------------------
# the render: tests/nerf_render_ref.render with the mask after each query
# ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def render(c, table, mode, dtype=torch.float32, mutation=None):
    """Case inputs ``c`` (below) -> nerf_render_ref.render's dict of ``dtype`` for the boxes ``table`` [K, 8] and ``mode``, plus counted1
    / counted2 (bool numpy [R, S]) and pts1 / pts2 (the sample points, float64 numpy [R, S, 3])."""
    assert mutation is None or mutation in MUTATIONS
    cfg = dict(R.DEFAULT_CFG, **(c.cfg or {}))
    model = R.build_model(c.state, cfg, dtype)
    embed_fn, _ = R.get_embedder(cfg["multires"], cfg["i_embed"])
    embeddirs_fn, _ = R.get_embedder(cfg["multires_views"], cfg["i_embed"])
    bb_center, bb_scale = torch.as_tensor(c.bb_center).to(dtype), torch.as_tensor(c.bb_scale).to(dtype)
    cam = torch.zeros(cfg["input_ch_cam"], dtype=dtype)
    if c.rays is None:
        rays_o, rays_d = V.get_rays(c.H, c.W, torch.as_tensor(c.intrinsic), torch.as_tensor(c.c2w).to(dtype))
    else:
        rays_o, rays_d = torch.as_tensor(c.rays)[:, :3].to(dtype), torch.as_tensor(c.rays)[:, 3:6].to(dtype)
    rays_o, rays_d = torch.reshape(rays_o, [-1, 3]), torch.reshape(rays_d, [-1, 3])
    viewdirs = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    near, far = float(np.float32(c.near)), float(np.float32(c.far))
    near_t, far_t = near * torch.ones_like(rays_d[..., :1]), far * torch.ones_like(rays_d[..., :1])
    N_rays = rays_o.shape[0]
    out = {"rays_o": rays_o, "rays_d": rays_d}

    def query(z_vals, tag):
        pts = rays_o[..., None, :] + rays_d[..., None, :] * z_vals[..., :, None]
        flat = (torch.reshape(pts, [-1, 3]) - bb_center) * bb_scale
        dirs = embeddirs_fn(torch.reshape(viewdirs[:, None].expand(pts.shape), [-1, 3]))
        embedded = torch.cat([embed_fn(flat), dirs, cam.unsqueeze(0).expand(dirs.shape[0], cam.shape[0])], -1)
        raw = torch.reshape(model(embedded), list(pts.shape[:-1]) + [4])
        p64 = pts.double().numpy()
        m = counted(p64, table, mode, mutation)
        out["pts" + tag], out["counted" + tag] = p64, m
        return raw

    def masked(raw, tag):
        return torch.where(torch.from_numpy(out["counted" + tag])[..., None], raw, torch.zeros_like(raw))

    if c.z_samples is not None:
        zs = torch.as_tensor(c.z_samples).to(dtype)
        N_half = zs.shape[0]
        z_vals = zs.unsqueeze(0).expand((N_rays, N_half))
        raw_plain = query(z_vals, "1")
        raw = masked(raw_plain, "1")
        z_vals_2 = V.samples_around_depth(raw_plain if mutation == "draw_unmasked" else raw, z_vals, rays_d, N_half, zs[-1] - zs[-2],
                                          near_t[0, 0], far_t[0, 0])
        out["raw1"], out["z2"] = raw, z_vals_2
        raw_2 = query(z_vals_2, "2")
        if mutation != "pass2_unmasked":
            raw_2 = masked(raw_2, "2")
        z_vals = torch.cat((z_vals, z_vals_2), -1)
        raw = torch.cat((raw, raw_2), 1)
        z_vals, indices = z_vals.sort()
        raw = torch.gather(raw, 1, indices.unsqueeze(-1).expand_as(raw))
    else:
        t_vals = torch.linspace(0., 1., steps=c.n_samples, dtype=dtype)
        z_vals = near_t * (1. - t_vals) + far_t * (t_vals)
        raw = masked(query(z_vals, "1"), "1")
        out["raw1"] = raw
    rgb_map, disp_map, acc_map, weights, depth_map = V.raw2outputs(raw, z_vals, rays_d)
    depth_var = ((z_vals - depth_map.unsqueeze(-1)).pow(2) * weights).sum(-1)
    out.update(rgb_map=rgb_map, disp_map=disp_map, acc_map=acc_map, depth_map=depth_map, z_vals=z_vals, weights=weights,
               depth_std=depth_var.clamp(0., 1.).sqrt())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
# 6 x 8 frames at 8 samples per pass: an image row is exactly one 64-point tile.  The rays-only case: tiles straddle rays and the last
# tile of a pass is partial (130 * 13 = 26 * 64 + 26).
CASES = [
    dict(name="plain_6x8", H=6, W=8, N=8, near=0.1, far=4.0, plain=True, seed=91),
    dict(name="two_pass_6x8", H=6, W=8, N=16, near=0.1, far=4.0, seed=92),
    dict(name="rays_130x13", H=10, W=13, N=26, near=0.1, far=4.0, seed=93, as_rays=True),
]
NAMES = [c["name"] for c in CASES]
BOXES = ("rotated", "rows", "overlap", "origin", "all", "none", "k0", "aabb6")


def case_inputs(case):
    """nerf_render_ref.case_inputs for the frames above, regenerated from seeds; as_rays: the float32 rays of the frame, given as rays."""
    cfg = dict(R.DEFAULT_CFG)
    H, W, seed = case["H"], case["W"], case["seed"]
    focal = 1.2 * max(H, W, 3)
    intrinsic = torch.tensor([focal, focal * 1.03, (W - 1) / 2 + 0.25, (H - 1) / 2 - 0.125], dtype=torch.float32)
    c2w = R.make_poses(300 + seed, 1)[0]
    plain = case.get("plain", False)
    z_samples = None if plain else V.precompute_quadratic_samples(case["near"], case["far"], case["N"] // 2)
    o, d = V.get_rays(H, W, intrinsic, c2w)
    rays32 = torch.cat([o.reshape(-1, 3), d.reshape(-1, 3)], 1).contiguous()
    return SimpleNamespace(name=case["name"], cfg=cfg, H=H, W=W, intrinsic=intrinsic, c2w=c2w, near=case["near"], far=case["far"],
                           bb_center=torch.tensor([0.11, -0.07, 0.9]), bb_scale=torch.tensor(2.0 / 13.0),
                           state=V.make_state(seed, cfg, V.SIGMA_SCALE), z_samples=z_samples, n_samples=case["N"], plain=plain, lindisp=False, embedded_cam=None,
                           rays=rays32 if case.get("as_rays") else None, rays32=rays32, n_rays=H * W,
                           s1=case["N"] if plain else case["N"] // 2)


def first_pass_points(c):
    """float64 [H, W, S1, 3]: the float32 first-pass sample points of the case, widened."""
    if c.plain:
        t = torch.linspace(0., 1., steps=c.n_samples)
        z = np.float32(c.near) * (1. - t) + np.float32(c.far) * t
    else:
        z = c.z_samples
    o, d = c.rays32[:, :3], c.rays32[:, 3:]
    return (o[:, None, :] + d[:, None, :] * z[None, :, None]).double().numpy().reshape(c.H, c.W, -1, 3)


def _around(points, theta=0.0, grow=1.25):
    """(cx, cy, cz, w, l, h, theta): the box of rotation theta about the points' mean that holds them, its extents grown by ``grow``."""
    p = points.reshape(-1, 3)
    centre = p.mean(0)
    cs, sn = np.cos(theta), np.sin(theta)
    q = p - centre
    loc = np.stack([cs * q[:, 0] + sn * q[:, 1], cs * q[:, 1] - sn * q[:, 0], q[:, 2]], 1)
    lo, hi = loc.min(0), loc.max(0)
    mid = (lo + hi) / 2
    centre = centre + np.array([cs * mid[0] - sn * mid[1], sn * mid[0] + cs * mid[1], mid[2]])
    ext = np.maximum((hi - lo) * grow, 0.2)
    return np.concatenate([centre, ext, [theta]])


def case_boxes(c, which):
    """The boxes of a case, placed on its own sample points (a function of the seeds only) -> array [K, 7] or [K, 6]."""
    P = first_pass_points(c)
    H, W, S = P.shape[:3]
    o = c.rays32[0, :3].double().numpy()
    mid = slice(S // 3, S // 3 + max(2, S // 4))                    # a few samples in the middle of a ray
    if which == "rotated":          # neither 0 nor a multiple of pi / 2; rays cross it between samples
        return _around(P[H // 3:H // 3 + 2, W // 4:W // 4 + 4, mid], theta=0.6)[None]
    if which == "rows":             # around part of one image row: whole rows stay outside, its own tiles are partly inside
        return _around(P[1:2, 2:W - 2, mid], theta=-0.35, grow=1.1)[None]
    if which == "overlap":
        a = _around(P[H // 3:H // 3 + 2, W // 4:W // 4 + 4, mid], theta=0.6)
        b = a.copy()
        b[:3] += 0.3 * a[3:6] * np.array([1.0, -1.0, 0.5])
        b[6] = -1.1
        return np.stack([a, b])
    if which == "origin":           # holds the camera and the first samples of every ray
        return np.concatenate([o + np.array([0.05, -0.08, 0.03]), [1.7, 1.5, 1.9], [0.25]])[None]
    if which == "all":
        return np.concatenate([o, [40.0, 40.0, 40.0], [1.0]])[None]
    if which == "none":
        return np.concatenate([o + 100.0, [1.0, 2.0, 3.0], [0.5]])[None]
    if which == "k0":
        return np.zeros((0, 7))
    if which == "aabb6":            # [K, 6] = (min, max): two boxes, theta 0 on the host
        a = P[H // 2:, :W // 2, mid].reshape(-1, 3)
        b = P[:H // 2, W // 2:, S // 2:].reshape(-1, 3)
        return np.stack([np.concatenate([p.min(0) - 0.07, p.max(0) + 0.07]) for p in (a, b)])
    raise KeyError(which)


def left_out(f64, table):
    """bool [R]: the rays of a float64 checker result that hold an undecided sample."""
    out = undecided(f64["pts1"], table).any(1)
    if "pts2" in f64:
        out |= undecided(f64["pts2"], table).any(1)
    return out


def bound_of(f32, f64, key, keep):
    """The bound of one tensor over the rays ``keep``: FACTOR x the float32 checker's deviation from the float64 checker, floored at
    one float32 ulp of the largest magnitude -> (bound, float32 checker's error)."""
    a, b = np.asarray(f32[key], dtype=np.float64)[keep], np.asarray(f64[key], dtype=np.float64)[keep]
    ok = ~np.isnan(b)
    err = float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0
    top = float(np.abs(b[ok]).max()) if ok.any() else 0.0
    return max(FACTOR * err, float(np.spacing(np.float32(top)))), err


def error_of(got, f64, key, keep):
    """(largest |got - f64| over the rays ``keep`` where f64 is a number, whether the NaN positions are equal)."""
    a, b = np.asarray(got[key], dtype=np.float64)[keep], np.asarray(f64[key], dtype=np.float64)[keep]
    ok = ~np.isnan(b)
    same = bool(np.array_equal(np.isnan(a), np.isnan(b)))
    return (float(np.abs(a[ok] - b[ok]).max()) if ok.any() and same else 0.0 if same else float("inf")), same


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


_CASES, _REFS = {}, {}


def refs_of(name, which, mode):
    """(case name, boxes name, mode) -> (inputs, boxes, table, float32 checker, float64 checker, left-out rays): computed once per
    process and shared by every test, results read-only numpy."""
    key = (name, which, mode)
    if key not in _REFS:
        if name not in _CASES:
            _CASES[name] = case_inputs(CASES[NAMES.index(name)])
        c = _CASES[name]
        boxes = case_boxes(c, which)
        table = box_table(boxes)
        both, threads = [], torch.get_num_threads()
        torch.set_num_threads(1)             # the float32 checker's sums, and so the bounds, do not depend on the machine
        for dt in (torch.float32, torch.float64):
            o = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in render(c, table, mode, dt).items()}
            for v in o.values():
                v.setflags(write=False)
            both.append(o)
        torch.set_num_threads(threads)
        _REFS[key] = (c, boxes, table, both[0], both[1], left_out(both[1], table))
    return _REFS[key]


@pytest.fixture(scope="session")
def box_refs():
    return refs_of


def recorded_bounds():
    with open(os.path.join(GOLDEN, "nerf_boxes_bounds.json")) as f:
        return json.load(f)
