"""Extract the rgb-sigma grid of a trained Dense-Depth-Priors NeRF (reference data/scannet/run_nerf.py, task ``extract``).

Run as ``python -m nerf_rpn_amd.scripts.nerf_extract --expname NAME --ckpt_dir DIR --data_dir DIR --scene_id SCENE --extract_dir DIR
--bbox_json FILE [--max_res 256] [--layout flat|wlh] [--dtype fp32|bf16x3]`` -- the reference's extract flags, and the arithmetic of
the MLP trunk.  ``<ckpt_dir>/<expname>/args.json`` gives the
network options, the last sorted checkpoint whose name contains ``000.tar`` gives ``network_fn_state_dict`` (load_checkpoint,
run_nerf.py:333-342), ``--bbox_json`` (what scannet_generate_bbox writes) gives the grid's box (get_scene_bounding_box, :1197-1210) and
the grid is min .. max in round(extent / largest extent * max_res) steps per axis (:1160-1168).  Every grid point goes through the MLP
on the GPU (ops.nerf_grid_query); ``<extract_dir>/<scene_id>.npz`` holds the reference's keys with its dtypes: rgbsigma, resolution,
bbox_min, bbox_max, scale=1.0, offset=0.0, from_mitsuba=False, from_ddp_nerf=True (:1147-1154).

``--layout flat`` (default) stores the reference's (N, 4) array; ``--layout wlh`` stores (res_x, res_y, res_z, 4), the grid
datasets.py reads, which is the README's reshape(res[2], res[1], res[0], -1).transpose(2, 1, 0, 3) of it.

Assumptions.  The reference imports NeRF, get_embedder, get_rays and load_scene from the Dense-Depth-Priors code,
which is not part of it.  The model is taken to be the nerf-pytorch MLP with a camera embedding (key list in DESIGN.md).  Poses and
scene bounds are defined here, not read from load_scene: ``--transforms`` (default ``<data_dir>/<scene_id>/transforms_train.json``)
holds ``frames[*].transform_matrix`` and ``fx, fy, cx, cy`` per frame or at the top level -- the keys data/scannet/visualize_bbox.py
reads.  The scene normalisation is either given (``--bb_center X Y Z --bb_scale S``) or computed as run_nerf.py:1063-1072 does from
``--image_hw H W`` and ``--far`` (default: the json's ``far``), with rays_d = [(i - cx) / fx, -(j - cy) / fy, -1] R^T and rays_o = t.
o + far d is affine in the pixel and, what counts in float32, every operation on the way is monotone in the pixel's row and column,
so the extremes are taken over the four corner pixels of every frame.
"""
import argparse
import json
import os

import numpy as np
import torch


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--expname', type=str, default=None)
    p.add_argument('--ckpt_dir', type=str, default="")
    p.add_argument('--data_dir', type=str, default="")
    p.add_argument('--scene_id', type=str, default="scene0710_00")
    p.add_argument('--max_res', type=int, default=256)
    p.add_argument('--extract_dir', type=str, default="")
    p.add_argument('--bbox_json', type=str, default="")
    p.add_argument('--transforms', type=str, default=None, help='poses and intrinsics (default <data_dir>/<scene_id>/transforms_train.json)')
    p.add_argument('--bb_center', type=float, nargs=3, default=None, metavar=('X', 'Y', 'Z'))
    p.add_argument('--bb_scale', type=float, default=None)
    p.add_argument('--image_hw', type=int, nargs=2, default=None, metavar=('H', 'W'))
    p.add_argument('--far', type=float, default=None)
    p.add_argument('--layout', choices=('flat', 'wlh'), default='flat')
    p.add_argument('--dtype', choices=('fp32', 'bf16x3'), default='fp32',
                   help='arithmetic of the MLP trunk: exact fp32, or three bf16 MFMA products of split operands (DESIGN.md 3.23)')
    return p


def load_checkpoint(ckpt_dir, expname):
    """-> (args.json as a dict, network_fn_state_dict, checkpoint path).  The checkpoint is the last, in sorted order, of the files of
    ``<ckpt_dir>/<expname>`` whose name contains ``000.tar`` (run_nerf.py:333-342, 1038-1041)."""
    run_dir = os.path.join(ckpt_dir, expname)
    with open(os.path.join(run_dir, 'args.json')) as f:
        cfg = json.load(f)
    names = sorted(n for n in os.listdir(run_dir) if '000.tar' in n)
    if not names:
        raise SystemExit(f'{run_dir}: no checkpoint whose name contains 000.tar')
    newest = os.path.join(run_dir, names[-1])
    return cfg, torch.load(newest, map_location='cpu')['network_fn_state_dict'], newest


def scene_bounding_box(bbox_json):
    """Float32 corner-wise min and max over the instances of the json scannet_generate_bbox writes (get_scene_bounding_box,
    run_nerf.py:1197-1210)."""
    with open(bbox_json) as f:
        instances = json.load(f)['instances']
    lo = torch.tensor([inst['min_pt'] for inst in instances]).amin(0)
    hi = torch.tensor([inst['max_pt'] for inst in instances]).amax(0)
    return lo, hi


def grid_axes(lo, hi, max_res):
    """[res_x, res_y, res_z] = round(extent / largest extent * max_res) (torch.round: half to even) and the three float32 linspace
    arrays (run_nerf.py:1160-1168)."""
    extent = hi - lo
    res = torch.round(extent / extent.max() * max_res).int().tolist()
    return (res, *(torch.linspace(lo[a], hi[a], res[a]) for a in range(3)))


def load_transforms(path, with_meta=False):
    """-> (poses float32 [P, 4, 4], intrinsics float32 [P, 4] = fx, fy, cx, cy, far or None); with_meta adds the parsed json."""
    with open(path) as f:
        meta = json.load(f)
    frames = meta['frames']
    if not frames:
        raise SystemExit(f'{path}: no frames')
    poses = torch.tensor([fr['transform_matrix'] for fr in frames], dtype=torch.float32)
    intr = torch.tensor([[fr.get(k, meta.get(k)) for k in ('fx', 'fy', 'cx', 'cy')] for fr in frames], dtype=torch.float32)
    return (poses, intr, meta.get('far'), meta) if with_meta else (poses, intr, meta.get('far'))


def corner_bounds(H, W, intrinsics, poses, far):
    """Scene normalisation of run_nerf.py:1063-1072 from the four corner pixels of every frame -> (bb_center, bb_scale, lo, hi).
    Every float32 operation between a pixel and its far point is monotone in the pixel's column and in its row (rounding is monotone,
    and so are subtraction, division and multiplication by a fixed number and the three-term sum), so the corners carry the extremes
    of the full image exactly; exact affinity is not needed.  lo / hi are clamped as the reference's running min / max from +-1e6 are."""
    u = torch.tensor([[0., W - 1.], [0., W - 1.]])
    v = torch.tensor([[0., 0.], [H - 1., H - 1.]])
    pts = []
    for (fx, fy, cx, cy), c2w in zip(intrinsics, poses):
        cam = torch.stack([(u - cx) / fx, -(v - cy) / fy, torch.full_like(u, -1.0)], -1)
        world = (cam[..., None, :] * c2w[:3, :3]).sum(-1)
        pts.append(c2w[:3, 3] + world * far)
    pts = torch.stack(pts).reshape(-1, 3)
    hi = pts.amax(0).clamp_min(-1e6)
    lo = pts.amin(0).clamp_max(1e6)
    return (hi + lo) / 2., 2. / (hi - lo).max(), lo, hi


def extract(cfg, state_dict, poses, bbox_json, max_res, bb_center, bb_scale, layout='flat', chunk=None, dtype='fp32'):
    """extract_nerf -> (rgbsigma numpy float32, resolution list, bbox_min, bbox_max numpy float32)."""
    from nerf_rpn_amd import ops
    lo, hi = scene_bounding_box(bbox_json)
    res, xs, ys, zs = grid_axes(lo, hi, max_res)
    print(f'nerf_extract: grid {res[0]} x {res[1]} x {res[2]} over {lo.tolist()} .. {hi.tolist()}, {len(poses)} poses')
    # the op takes the arithmetic from packed weights; a state dict is packed by the op itself, in fp32
    net = state_dict if dtype == 'fp32' else ops.nerf_grid_pack(state_dict, cfg, dtype)
    out = ops.nerf_grid_query(net, cfg, xs, ys, zs, bb_center, bb_scale, poses, layout=layout, chunk=chunk)
    return out.cpu().numpy(), res, lo.numpy(), hi.numpy()


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.expname is None:
        raise SystemExit('nerf_extract: --expname is required')
    from nerf_rpn_amd import ops
    cfg, state_dict, ckpt_path = load_checkpoint(args.ckpt_dir, args.expname)
    ops.nerf_grid_config(cfg)            # unsupported options stop here, before any file is read
    print(f'nerf_extract: weights from {ckpt_path}')
    transforms = args.transforms or os.path.join(args.data_dir, args.scene_id, 'transforms_train.json')
    poses, intrinsics, far = load_transforms(transforms)
    if (args.bb_center is None) != (args.bb_scale is None):
        raise SystemExit('--bb_center and --bb_scale go together')
    if args.bb_center is not None:
        bb_center, bb_scale = torch.tensor(args.bb_center, dtype=torch.float32), torch.tensor(args.bb_scale, dtype=torch.float32)
    else:
        far = args.far if args.far is not None else far
        if args.image_hw is None or far is None:
            raise SystemExit('scene bounds: give --bb_center and --bb_scale, or --image_hw H W and --far (or "far" in the transforms json)')
        bb_center, bb_scale, lo, hi = corner_bounds(args.image_hw[0], args.image_hw[1], intrinsics, poses, far)
        print(f'nerf_extract: scene bounds from the corner rays: {lo.tolist()} .. {hi.tolist()}')
    rgbsigma, res, bbox_min, bbox_max = extract(cfg, state_dict, poses, args.bbox_json, args.max_res, bb_center, bb_scale, args.layout, dtype=args.dtype)
    os.makedirs(args.extract_dir or '.', exist_ok=True)
    path = os.path.join(args.extract_dir, f'{args.scene_id}.npz')
    np.savez_compressed(path, rgbsigma=rgbsigma, resolution=res, bbox_min=bbox_min, bbox_max=bbox_max, scale=1.0, offset=0.0,
                        from_mitsuba=False, from_ddp_nerf=True)
    return path


if __name__ == '__main__':
    main()
