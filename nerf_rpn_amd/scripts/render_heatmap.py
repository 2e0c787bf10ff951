"""Proposal heatmaps rendered from a scene's validation cameras (reference nerf_rpn/scripts/render_heatmap.py).

Run as ``python -m nerf_rpn_amd.scripts.render_heatmap`` with the reference's flags (same names, defaults and choices) plus ``--width`` /
``--height`` (640 x 480).  For every scene of ``--proposal_dir``: the first ``top_n`` proposals become integer AABBs of the feature grid,
each splats a separable Gaussian (or a box of ones), the volume goes through scipy's ``gaussian_filter`` and is standardised -- all on the
GPU, bit-identical to numpy / scipy except the standardisation (float64 sums, ~1e-6 relative) -- and the volume is rendered by maximum
intensity from every frame of ``val/val_transforms.json`` into ``<output_dir>/<scene>/<frame>_hmp.png``.  The render replaces the
reference's VTK volume render (``add_volume(cmap='jet', opacity='linear', blending='maximum')``) with the definition in
include/nerfrpn.h (nrpn_render_mip): the reference's look, not VTK's pixels.

``--concat_img`` writes three panels side by side: the frame's screenshot (``val/screenshots/<frame>.jpg``), the heatmap resized to it
(box filter) and the screenshot with the wireframes of the boxes.  The reference projects them with a module that is not part of it, so
the projection here uses the renderer's camera convention: the camera looks down -z of the frame's ``transform_matrix`` with the
transforms file's ``fl_x, fl_y, cx, cy``; an edge is drawn when both its ends are in front of the camera.

Deliberate differences from the reference:
  * all scenes are processed (the reference stops after the first: ``scene_list[:1]``);
  * a box that still lies outside the array after the reference's clip, or an unclipped ``--use_gt`` box, is clamped to the array
    (the reference raises);
  * axis-aligned proposals [K,6] are used as they are (the reference fails on them);
  * the heatmap is float32 even for uint8 feature files (the reference's numpy promotion gives float16 there);
  * a heatmap with zero standard deviation (no boxes) is skipped with a warning instead of rendering NaNs;
  * ``--interactive`` exits with a message: there is no display;
  * a transforms file without ``room_bbox`` fails with a message naming the file.
"""
import argparse
import json
import os
import sys
import warnings

import numpy as np

_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--dataset_dir", type=str, help="path to dataset directory")
    p.add_argument("--feature_dir", type=str, help="path to feature directory")
    p.add_argument("--proposal_dir", type=str, help="path to proposal directory")
    p.add_argument("--output_dir", type=str, help="path to output directory")
    p.add_argument("--boxes_dir", type=str, help="path to boxes directory")
    p.add_argument("--transpose_yz", action="store_true", help="transpose y and z")
    p.add_argument("--top_n", type=int, default=100, help="top n proposals to be used for heatmap.")
    p.add_argument("--use_gt", action="store_true", help="use ground truth boxes")
    p.add_argument("--kernel_type", type=str, default="gaussian", choices=["gaussian", "box"], help="type of heatmap to be generated")
    p.add_argument("--value_scale", type=float, default=20, help="value scaling for heatmap")
    p.add_argument("--downsample", type=int, default=2, help="downsample factor for heatmap")
    p.add_argument("--gaussian_sigma", type=float, default=5, help="sigma for gaussian kernel")
    p.add_argument("--concat_img", action="store_true", help="concatenate heatmap with NeRF image")
    p.add_argument("--interactive", action="store_true", help="interactive mode (not supported: there is no display)")
    p.add_argument("--width", type=int, default=640, help="rendered image width")
    p.add_argument("--height", type=int, default=480, help="rendered image height")
    return p


# ----------------------------------------------------------------------------------------------------------------------
# boxes and cameras (host, numpy)
# ----------------------------------------------------------------------------------------------------------------------
def obb2hbb(obb):
    """[..., 7] (x, y, z, w, l, h, theta) -> the smallest AABB [..., 6] containing the rotated box."""
    xy, z, w, l, h, theta = np.split(obb, [2, 3, 4, 5, 6], axis=-1)
    c, s = np.cos(theta), np.sin(theta)
    half = np.concatenate([np.abs(w / 2 * c) + np.abs(l / 2 * s), np.abs(w / 2 * s) + np.abs(l / 2 * c)], axis=-1)
    return np.concatenate([xy - half, z - h / 2, xy + half, z + h / 2], axis=-1)


def obb_corners(obb):
    """[N,7] -> [N,8,3]: bottom face (z - h/2) corners 0-3 in cyclic order, then the top face in the same order."""
    x, y, z, w, l, h, theta = np.split(obb, [1, 2, 3, 4, 5, 6], axis=-1)
    c, s = np.cos(theta), np.sin(theta)
    dx1, dx2 = w / 2 * c - l / 2 * s, w / 2 * c + l / 2 * s
    dy1, dy2 = w / 2 * s + l / 2 * c, w / 2 * s - l / 2 * c
    xy = [(x + dx1, y + dy1), (x + dx2, y + dy2), (x - dx1, y - dy1), (x - dx2, y - dy2)]
    rows = [np.concatenate([px, py, zz], axis=-1) for zz in (z - h / 2, z + h / 2) for px, py in xy]
    return np.stack(rows, axis=1)


def aabb_corners(aabb):
    """[N,6] -> [N,8,3] in the order of obb_corners."""
    x1, y1, z1, x2, y2, z2 = (aabb[:, i:i + 1].astype(np.float64) for i in range(6))
    xy = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    return np.stack([np.concatenate([px, py, zz], axis=-1) for zz in (z1, z2) for px, py in xy], axis=1)


def world2grid(points, room_bbox, res, downsample=1):
    p = np.array(points, dtype=np.float64)
    p -= room_bbox[:3]
    p /= np.max(room_bbox[3:] - room_bbox[:3])
    p *= np.max(res)
    return p / downsample


def grid2world(points, room_bbox, res):
    p = np.array(points, dtype=np.float64)
    p /= np.max(res)
    p *= np.max(room_bbox[3:] - room_bbox[:3])
    p += room_bbox[:3]
    return p


def frame2config(frames, room_bbox, res, downsample=1):
    """Frame list of a transforms file -> (names, camera positions [F,3], focal points [F,3], poses [F,4,4]) in grid units / downsample.
    The focal point is one world unit down -z of the camera: c2w @ (0, 0, -1, 1), written as the column difference (exact: the other
    products are zeros and ones)."""
    names, pos, foc, poses = [], [], [], []
    for fr in frames:
        names.append(fr["file_path"].split("/")[-1].split(".")[0])
        c2w = np.array(fr["transform_matrix"], dtype=np.float64)
        poses.append(c2w)
        pos.append(world2grid(c2w[:3, 3], room_bbox, res, downsample))
        hom = c2w[:, 3] - c2w[:, 2]
        foc.append(world2grid(hom[:3] / hom[3], room_bbox, res, downsample))
    return names, np.array(pos).reshape(-1, 3), np.array(foc).reshape(-1, 3), poses


def load_scene(feature_path, proposal_path, json_path, transpose_yz, top_n):
    """-> (heatmap shape, proposals [<=top_n, 6|7], room_bbox [6], res) as the reference's load_alpha_and_proposals gives them."""
    feat = np.load(feature_path)
    shape = tuple(int(v) for v in feat["rgbsigma"].shape[:3])
    res = feat["resolution"]
    with open(json_path) as f:
        meta = json.load(f)
    if "room_bbox" not in meta:
        raise SystemExit(f"render_heatmap: no room_bbox in {json_path}")
    room_bbox = np.array(meta["room_bbox"]).flatten()
    if transpose_yz:
        shape = (shape[0], shape[2], shape[1])
        res = [res[2], res[0], res[1]]
    else:
        res = [res[1], res[2], res[0]]
    props = np.load(proposal_path)
    if "proposals" in props:
        proposals = props["proposals"]
    elif "proposal" in props:
        proposals = props["proposal"]
    else:
        raise ValueError("proposals and proposal are not found in npz.")
    return shape, proposals[:top_n], room_bbox, res


def clip_aabbs(boxes, res):
    """Boxes [K,6|7] -> integer AABBs [K,6]: obb2hbb (OBBs), truncation towards zero, axis i clipped to [0, res[i] - 1]."""
    a = (obb2hbb(boxes) if boxes.shape[-1] == 7 else boxes).astype(int).reshape(-1, 6)
    for i in range(3):
        a[:, [i, i + 3]] = np.clip(a[:, [i, i + 3]], a_min=0, a_max=res[i] - 1)
    return a


def clamp_to_array(aabbs, shape):
    a = np.array(aabbs, dtype=np.int64).reshape(-1, 6)
    for i in range(3):
        a[:, [i, i + 3]] = np.clip(a[:, [i, i + 3]], 0, shape[i])
    return a


def scene_boxes(proposals, res, shape, room_bbox, gt=None):
    """-> (AABBs [K,6] clamped to the array, world-space corners [K,8,3]) of the proposals, or of the gt boxes when given (unclipped)."""
    src = proposals if gt is None else gt
    src = np.asarray(src).reshape(-1, np.asarray(src).shape[-1] if np.asarray(src).size else 7)
    if gt is None:
        aabbs = clip_aabbs(src, res)
    else:
        aabbs = (obb2hbb(src) if src.shape[-1] == 7 else src).astype(int).reshape(-1, 6)
    corners = obb_corners(src) if src.shape[-1] == 7 else aabb_corners(src)
    return clamp_to_array(aabbs, shape), grid2world(corners, room_bbox, res)


# ----------------------------------------------------------------------------------------------------------------------
# GPU part
# ----------------------------------------------------------------------------------------------------------------------
def generate_heatmap(aabbs, shape, kernel_type="gaussian", sigma=5.0, device="cuda"):
    """splat -> gaussian_filter -> standardise on the device -> (heatmap float32 [X,Y,Z], mean, std)."""
    from nerf_rpn_amd import ops
    h = ops.heatmap_splat(aabbs, shape, kernel_type, device)
    h = ops.gaussian_filter3d(h, sigma)
    h, ms = ops.standardize(h)
    mean, std = ms.tolist()
    return h, mean, std


def project_wireframes(img, corners_world, c2w, fl_x, fl_y, cx, cy, colour=(0, 255, 0)):
    """Draw the 12 edges of every box (corners [K,8,3] in world units) on a PIL image, camera looking down -z of c2w."""
    from PIL import ImageDraw
    draw = ImageDraw.Draw(img)
    w2c = np.linalg.inv(c2w)
    for box in np.asarray(corners_world).reshape(-1, 8, 3):
        cam = (w2c[:3, :3] @ box.T).T + w2c[:3, 3]
        front = cam[:, 2] < 0
        depth = np.where(front, -cam[:, 2], 1.0)
        u = fl_x * cam[:, 0] / depth + cx
        v = cy - fl_y * cam[:, 1] / depth
        for a, b in _EDGES:
            if front[a] and front[b]:
                draw.line([(float(u[a]), float(v[a])), (float(u[b]), float(v[b]))], fill=colour, width=2)
    return img


def render_scene(heatmap, val_meta, room_bbox, res, out_dir, args, corners_world):
    from PIL import Image
    from nerf_rpn_amd import ops
    names, pos, foc, poses = frame2config(val_meta["frames"], room_bbox, res, args.downsample)
    if not names:
        return []
    cams = np.concatenate([pos, foc], axis=1)
    rgb = ops.render_mip(heatmap, cams, args.downsample, args.value_scale, args.width, args.height).cpu().numpy()
    written = []
    for name, img, pose in zip(names, rgb, poses):
        path = os.path.join(out_dir, name + "_hmp.png")
        out = Image.fromarray(img)
        if args.concat_img:
            shot = Image.open(os.path.join(args.dataset_dir, args.scene_name, "val", "screenshots", name + ".jpg")).convert("RGB")
            hmp = out.resize(shot.size, Image.BOX)
            boxes = project_wireframes(shot.copy(), corners_world, pose, val_meta["fl_x"], val_meta["fl_y"], val_meta["cx"], val_meta["cy"])
            out = Image.new("RGB", (3 * shot.size[0], shot.size[1]))
            for k, panel in enumerate((shot, hmp, boxes)):
                out.paste(panel, (k * shot.size[0], 0))
        out.save(path)
        written.append(path)
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.interactive:
        raise SystemExit("render_heatmap: --interactive is not supported (there is no display); the frames are written as PNG files")
    import torch
    scenes = [x.split(".")[0] for x in sorted(os.listdir(args.proposal_dir))]
    written = []
    for scene in scenes:
        args.scene_name = scene
        feature_path = os.path.join(args.feature_dir, scene + ".npz")
        proposal_path = os.path.join(args.proposal_dir, scene + ".npz")
        train_json = os.path.join(args.dataset_dir, scene, "train", "transforms.json")
        val_json = os.path.join(args.dataset_dir, scene, "val", "val_transforms.json")
        for what, path in (("feature file", feature_path), ("proposal file", proposal_path), ("train json file", train_json),
                           ("val json file", val_json)):
            if not os.path.isfile(path):
                raise SystemExit(f"render_heatmap: {what} not found: {path}")
        shape, proposals, room_bbox, res = load_scene(feature_path, proposal_path, train_json, args.transpose_yz, args.top_n)
        gt = np.load(os.path.join(args.boxes_dir, scene + ".npy")) if args.use_gt else None
        aabbs, corners = scene_boxes(proposals, res, shape, room_bbox, gt)
        heatmap, mean, std = generate_heatmap(aabbs, shape, args.kernel_type, args.gaussian_sigma, torch.device("cuda", 0))
        if not (std > 0 and np.isfinite(std)):
            warnings.warn(f"render_heatmap: scene {scene}: the heatmap has zero standard deviation (no boxes?); skipped")
            continue
        out_dir = os.path.join(args.output_dir, scene)
        os.makedirs(out_dir, exist_ok=True)
        with open(val_json) as f:
            val_meta = json.load(f)
        written += render_scene(heatmap, val_meta, room_bbox, res, out_dir, args, corners)
    print(f"Done: {len(written)} images.")
    return written


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
