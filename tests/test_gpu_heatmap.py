"""Proposal heatmap kernels (csrc/heatmap.hip) on the MI355X: splat and gaussian filter bit-equal to the reference's numpy / scipy
(tests/golden/heatmap.npz), standardisation within 1e-5 and run-to-run identical, the MIP render against a plain-Python restatement of its
definition (include/nerfrpn.h, nrpn_render_mip), and the CLI end to end."""
import json
import math
import os

import numpy as np
import pytest
import torch

from nerf_rpn_amd import ops
from nerf_rpn_amd.scripts import render_heatmap as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heatmap.npz")
TAN_HALF_FOV = 0.57735026918962576451


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN, allow_pickle=False))


def _case(g, name):
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(name + "/")}


def test_splat_is_bit_equal_to_the_reference(g, dev):
    for name in g["cases"]:
        c = _case(g, str(name))
        out = ops.heatmap_splat(c["aabbs"], tuple(c["shape"]), str(c["kernel_type"]), dev).cpu().numpy()
        assert out.dtype == np.float32 and np.array_equal(out, c["pre"]), name


def test_gaussian_filter_is_bit_equal_to_scipy(g, dev):
    sigmas = set()
    for name in g["cases"]:
        c = _case(g, str(name))
        out = ops.gaussian_filter3d(torch.from_numpy(c["pre"]).to(dev), float(c["sigma"])).cpu().numpy()
        assert np.array_equal(out, c["filtered"]), (name, np.abs(out - c["filtered"]).max())
        sigmas.add(float(c["sigma"]))
    assert sigmas == {5.0, 2.0}


def test_standardize_within_tolerance_and_deterministic(g, dev):
    for name in g["cases"]:
        c = _case(g, str(name))
        x = torch.from_numpy(c["filtered"]).to(dev)
        a, ms = ops.standardize(x)
        b, _ = ops.standardize(x)
        assert torch.equal(a.cpu(), b.cpu()), name
        a, ref = a.cpu().numpy(), c["heatmap"]
        assert np.all(np.abs(a - ref) <= 1e-5 * np.maximum(1.0, np.abs(ref))), (name, np.abs(a - ref).max())
        mean, std = ms.tolist()
        assert abs(mean - float(c["filtered"].mean())) <= 1e-6 * max(1.0, abs(mean)) and std > 0


# ----------------------------------------------------------------------------------------------------------------------
# the render against a restatement of its definition
# ----------------------------------------------------------------------------------------------------------------------
def _basis(cam, W, H):
    o = [float(v) for v in cam[:3]]
    fx, fy, fz = cam[3] - o[0], cam[4] - o[1], cam[5] - o[2]
    fn = math.sqrt(fx * fx + fy * fy + fz * fz)
    fx, fy, fz = fx / fn, fy / fn, fz / fn
    rx, ry = fy, -fx
    rn = math.sqrt(rx * rx + ry * ry)
    rx, ry = rx / rn, ry / rn
    ux, uy, uz = ry * fz, -(rx * fz), rx * fy - ry * fx
    return o, (fx, fy, fz), (rx, ry), (ux, uy, uz)


def _ray(cam, W, H, px, py):
    o, (fx, fy, fz), (rx, ry), (ux, uy, uz) = _basis(cam, W, H)
    sx = (2.0 * (px + 0.5) / W - 1.0) * TAN_HALF_FOV * (W / H)
    sy = (1.0 - 2.0 * (py + 0.5) / H) * TAN_HALF_FOV
    return o, (fx + sx * rx + sy * ux, fy + sx * ry + sy * uy, fz + sy * uz)


def _ray_max(V, o, d):
    """Max of V over the cells the ray o + s d (s > 0) crosses with positive length: every face crossing inside the volume splits the
    ray into intervals, each interval's midpoint names its cell.  Also returns the distance of the ray to the nearest cell edge."""
    n = V.shape
    t0, t1 = 0.0, math.inf
    for a in range(3):
        if d[a] == 0.0:
            if o[a] < 0.0 or o[a] >= n[a]:
                return None, 0.0
        else:
            ta, tb = (0.0 - o[a]) / d[a], (n[a] - o[a]) / d[a]
            t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    if not t0 < t1:
        return None, 0.0
    ts = [t0, t1]
    for a in range(3):
        if d[a] != 0.0:
            ts += [t for t in ((k - o[a]) / d[a] for k in range(n[a] + 1)) if t0 < t < t1]
    ts = sorted(ts)
    m, edge = -math.inf, math.inf
    for ta, tb in zip(ts[:-1], ts[1:]):
        if tb <= ta:
            continue
        p = [o[a] + 0.5 * (ta + tb) * d[a] for a in range(3)]
        cell = [min(max(int(math.floor(p[a])), 0), n[a] - 1) for a in range(3)]
        m = max(m, float(V[cell[0], cell[1], cell[2]]))
    for t in ts:          # how close the ray passes to an edge (two coordinates on integers at once)
        q = [o[a] + t * d[a] for a in range(3)]
        dist = sorted(abs(v - round(v)) for v in q)
        edge = min(edge, dist[1])
    return m, edge


def _restated_render(h, d, scale, cam, W, H, jet):
    V = h[::d, ::d, ::d] * np.float32(scale)
    lo, hi = float(V.min()), float(V.max())
    m = np.full((H, W), -np.inf, dtype=np.float32)
    edge = np.full((H, W), np.inf)
    hit = np.zeros((H, W), dtype=bool)
    for py in range(H):
        for px in range(W):
            o, dr = _ray(cam, W, H, px, py)
            mm, e = _ray_max(V, o, dr)
            if mm is not None:
                m[py, px], edge[py, px], hit[py, px] = mm, e, True
    return V, m, edge, hit, lo, hi


def _colour(m, hit, lo, hi, jet):
    t = np.clip((m.astype(np.float32) - np.float32(lo)) / (np.float32(hi) - np.float32(lo)), np.float32(0), np.float32(1)) if hi > lo \
        else np.zeros_like(m)
    t = np.where(hit, t, np.float32(0)).astype(np.float32)
    idx = np.minimum((t * np.float32(256)).astype(np.int64), 255)
    rgb = np.rint(255.0 * jet[idx] * t.astype(np.float64)[..., None]).astype(np.uint8)
    return np.where(hit[..., None], rgb, 0)


def _check_render(h, d, scale, cams, W, H, dev):
    jet = ops.jet_table()
    rgb, mip = ops.render_mip(torch.from_numpy(h).to(dev), cams, d, scale, W, H, with_mip=True)
    rgb, mip = rgb.cpu().numpy(), mip.cpu().numpy()
    for f, cam in enumerate(np.asarray(cams, dtype=np.float64).reshape(-1, 6)):
        V, m, edge, hit, lo, hi = _restated_render(h, d, scale, cam, W, H, jet)
        same = (mip[f] == m) | (~hit & np.isneginf(mip[f]))
        assert same.mean() >= 0.99, (f, same.mean())
        assert np.all(edge[~same] <= 1e-4), (f, edge[~same].max())
        # RGB follows from m on every pixel
        assert np.array_equal(rgb[f], _colour(mip[f], ~np.isneginf(mip[f]), lo, hi, jet)), f
        assert np.all(rgb[f][~hit & same] == 0)
    return rgb, mip


def test_render_matches_the_restated_definition(g, dev):
    c = _case(g, "b_gauss_s5_t")
    h = c["heatmap"].astype(np.float32)
    X, Y, Z = (v / 2 for v in h.shape)
    outside = [[-8.0, -6.0, 9.0, X / 2, Y / 2, Z / 3], [X + 9.0, Y / 2, Z / 2, X / 2, Y / 2 + 1.0, Z / 2]]
    inside = np.concatenate([c["cam_pos_d2"], c["cam_focal_d2"]], axis=1)        # cameras of the frames (in the room)
    cams = np.concatenate([outside, inside], axis=0)
    _check_render(h, 2, 20.0, cams, 64, 48, dev)
    # a camera well inside the volume: every ray starts in a cell
    _, mip = _check_render(h, 2, 20.0, [[X / 2, Y / 2, Z / 2, X / 2 + 3.0, Y / 2 - 1.0, Z / 2 + 0.5]], 64, 48, dev)
    assert np.all(np.isfinite(mip))


def test_render_hot_cell_lands_on_the_pinhole_pixel_and_misses_are_black(dev):
    h = np.zeros((16, 12, 10), dtype=np.float32)
    h[9, 4, 6] = 1.0
    W, H = 64, 48
    cam = np.array([-20.0, -7.0, 13.0, 8.0, 6.0, 3.0])
    rgb, mip = ops.render_mip(torch.from_numpy(h).to(dev), cam, 1, 1.0, W, H, with_mip=True)
    rgb, mip = rgb.cpu().numpy()[0], mip.cpu().numpy()[0]
    o, f, (rx, ry), u = _basis(cam, W, H)
    p = np.array([9.5, 4.5, 6.5]) - np.array(o)
    pf, pr, pu = p @ np.array(f), p @ np.array([rx, ry, 0.0]), p @ np.array(u)
    x = (pr / pf / (TAN_HALF_FOV * W / H) + 1.0) * W / 2 - 0.5
    y = (1.0 - pu / pf / TAN_HALF_FOV) * H / 2 - 0.5
    hot = np.argwhere(mip == 1.0)
    assert len(hot) >= 1
    assert np.all(np.abs(hot[:, 1] - x) <= 2.0) and np.all(np.abs(hot[:, 0] - y) <= 2.0), (hot, x, y)
    assert np.hypot(hot[:, 1] - x, hot[:, 0] - y).min() <= 0.75, (hot, x, y)
    assert np.all(rgb[hot[:, 0], hot[:, 1]] == [128, 0, 0])                  # t = 1: jet's top colour (0.5, 0, 0)
    miss = np.isneginf(mip)
    assert miss.any() and np.all(rgb[miss] == 0)
    assert np.all(rgb[(mip == 0.0)] == 0)                                    # t = 0 on the cold cells: black too
    # a camera looking away from the volume sees nothing
    away = ops.render_mip(torch.from_numpy(h).to(dev), [-20.0, -7.0, 13.0, -30.0, -9.0, 14.0], 1, 1.0, W, H).cpu().numpy()
    assert not away.any()


def test_edge_cases(dev):
    shape = (11, 9, 7)
    zero = ops.heatmap_splat(np.zeros((0, 6), np.int64), shape, "gaussian", dev)
    assert not zero.any().item()
    _, ms = ops.standardize(ops.gaussian_filter3d(zero, 5.0))
    assert ms.tolist() == [0.0, 0.0]
    flat = ops.heatmap_splat(np.array([[3, 2, 1, 3, 5, 4], [1, 1, 1, 4, 1, 6]]), shape, "gaussian", dev)      # zero extent: no effect
    assert not flat.any().item()
    whole = ops.heatmap_splat(np.array([[0, 0, 0, 11, 9, 7]]), shape, "gaussian", dev).cpu().numpy()
    gx, gy, gz = ops.gkern_factors(11), ops.gkern_factors(9), ops.gkern_factors(7)
    ref = np.zeros(shape, np.float32)
    ref += np.outer(np.outer(gx, gy), gz).reshape(shape)
    assert np.array_equal(whole, ref)
    boxes = ops.heatmap_splat(np.array([[0, 0, 0, 11, 9, 7], [2, 3, 1, 5, 9, 2]]), shape, "box", dev).cpu().numpy()
    ref = np.ones(shape, np.float32)
    ref[2:5, 3:9, 1:2] += 1
    assert np.array_equal(boxes, ref)
    # d = 3 on sizes that 3 does not divide: V is heatmap[::3, ::3, ::3]
    rng = np.random.default_rng(4)
    h = rng.standard_normal((25, 20, 17)).astype(np.float32)
    V = h[::3, ::3, ::3]
    cams = [[-4.0, -3.0, 8.0, V.shape[0] / 2, V.shape[1] / 2, V.shape[2] / 2], [4.0, 3.5, 3.0, 8.0, 1.0, 2.5]]
    _check_render(h, 3, 2.5, cams, 32, 24, dev)


def _dataset(root, shot_size=(160, 120)):
    from PIL import Image
    rng = np.random.default_rng(11)
    for d in ("feat", "props", "gt", "ds/s0/train", "ds/s0/val/screenshots"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    shape = (24, 20, 16)
    np.savez(os.path.join(root, "feat", "s0.npz"), rgbsigma=rng.uniform(-2, 2, shape + (4,)).astype(np.float32),
             resolution=np.array([16, 24, 20]))
    props = np.concatenate([rng.uniform(2, 14, (12, 3)), rng.uniform(2, 8, (12, 3)), rng.uniform(-1, 1, (12, 1))], axis=1)
    np.savez(os.path.join(root, "props", "s0.npz"), proposal=props.astype(np.float32), score=np.linspace(1, 0.1, 12))
    np.save(os.path.join(root, "gt", "s0.npy"), props[:3].astype(np.float32))
    room = [[-1.0, -1.0, 0.0], [3.8, 3.0, 2.5]]
    with open(os.path.join(root, "ds/s0/train/transforms.json"), "w") as f:
        json.dump({"room_bbox": room, "frames": []}, f)
    frames = []
    for k, (pos, look) in enumerate((([0.2, 0.1, 1.6], [2.0, 1.5, 1.0]), ([3.5, 2.7, 1.9], [1.0, 1.0, 0.8]))):
        fwd = np.array(look) - np.array(pos)
        fwd /= np.linalg.norm(fwd)
        r = np.cross(fwd, [0, 0, 1.0])
        r /= np.linalg.norm(r)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, np.cross(r, fwd), -fwd, pos
        frames.append({"file_path": f"images/f{k}.jpg", "transform_matrix": m.tolist()})
        Image.fromarray(rng.integers(0, 255, (shot_size[1], shot_size[0], 3), dtype=np.uint8)).save(
            os.path.join(root, "ds/s0/val/screenshots", f"f{k}.jpg"))
    with open(os.path.join(root, "ds/s0/val/val_transforms.json"), "w") as f:
        json.dump({"fl_x": 120.0, "fl_y": 120.0, "cx": 80.0, "cy": 60.0, "frames": frames}, f)


def test_cli_end_to_end(tmp_path, dev):
    from PIL import Image
    _dataset(str(tmp_path))
    base = ["--dataset_dir", str(tmp_path / "ds"), "--feature_dir", str(tmp_path / "feat"), "--proposal_dir", str(tmp_path / "props"),
            "--boxes_dir", str(tmp_path / "gt")]
    for extra, size in (([], (640, 480)), (["--concat_img"], (480, 120)), (["--use_gt", "--concat_img"], (480, 120)),
                        (["--use_gt", "--kernel_type", "box", "--downsample", "3"], (640, 480))):
        out = tmp_path / ("out" + "".join(extra).replace("-", "_"))
        written = R.main(base + ["--output_dir", str(out)] + extra)
        assert sorted(os.path.basename(p) for p in written) == ["f0_hmp.png", "f1_hmp.png"], extra
        for p in written:
            assert p.startswith(str(out / "s0"))
            im = Image.open(p)
            assert im.size == size and im.mode == "RGB", (extra, im.size)
            assert np.asarray(im).any(), extra
