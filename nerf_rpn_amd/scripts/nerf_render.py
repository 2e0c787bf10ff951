"""Render views of a trained Dense-Depth-Priors NeRF: rgb, depth and depth-std frames (reference data/scannet/run_nerf.py, what its
tasks ``video``, ``test`` and ``render_train_depth`` do through render -> render_rays).

Run as ``python -m nerf_rpn_amd.scripts.nerf_render --expname NAME --ckpt_dir DIR --data_dir DIR --scene_id SCENE --image_hw H W
--output_dir DIR [--frames 0 5 9] [--near X] [--far X] [--N_samples N] [--depth_loss_weight W] [--lindisp] [--dtype fp32|bf16x3]``.  The
checkpoint and the
network options are found as nerf_extract finds them; N_samples, depth_loss_weight and lindisp default to the training run's
``args.json`` (else 256, 0.004, off -- config_parser's defaults, run_nerf.py:955-984).  depth_loss_weight > 0 selects the two-pass
path of render_rays (:595-600): the N_samples / 2 precomputed quadratic samples (:1076-1077), then as many around the depth they
predict; 0 selects the plain path (:602-614).  ``--transforms`` (default ``<data_dir>/<scene_id>/transforms_test.json``) holds the
poses and intrinsics of the frames to render, with nerf_extract's keys, and optionally ``near`` / ``far``.  The scene normalisation is
``--bb_center X Y Z --bb_scale S`` or, as in nerf_extract, computed from the corner rays of the training frames
(``--bounds_transforms``, default ``<data_dir>/<scene_id>/transforms_train.json``).

Per selected frame i the output directory gets ``<i>_rgb.png`` (8-bit, to8b = uint8(255 * clip(x, 0, 1)), written with PIL) and
``<i>.npz`` with float32 ``depth``, ``depth_std`` and ``acc`` (H, W).

Assumptions: get_rays, sample_pdf, precompute_quadratic_samples and to8b live in the Dense-Depth-Priors code,
which is not part of the reference; their assumed definitions are restated in DESIGN.md.  Only this command line depends on the
quadratic formula: ops.nerf_render takes the samples as data.
"""
import argparse
import os

import numpy as np
import torch

from .nerf_extract import corner_bounds, load_checkpoint, load_transforms


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--expname', type=str, default=None)
    p.add_argument('--ckpt_dir', type=str, default="")
    p.add_argument('--data_dir', type=str, default="")
    p.add_argument('--scene_id', type=str, default="scene0710_00")
    p.add_argument('--transforms', type=str, default=None, help='poses and intrinsics to render (default <data_dir>/<scene_id>/transforms_test.json)')
    p.add_argument('--bounds_transforms', type=str, default=None,
                   help='training poses for the scene bounds (default <data_dir>/<scene_id>/transforms_train.json)')
    p.add_argument('--bb_center', type=float, nargs=3, default=None, metavar=('X', 'Y', 'Z'))
    p.add_argument('--bb_scale', type=float, default=None)
    p.add_argument('--image_hw', type=int, nargs=2, default=None, metavar=('H', 'W'))
    p.add_argument('--near', type=float, default=None)
    p.add_argument('--far', type=float, default=None)
    p.add_argument('--N_samples', type=int, default=None)
    p.add_argument('--depth_loss_weight', type=float, default=None)
    p.add_argument('--lindisp', action='store_true', default=None)
    p.add_argument('--frames', type=int, nargs='*', default=None, help='indices into the transforms json (default: all)')
    p.add_argument('--chunk', type=int, default=None, help='rays per launch group')
    p.add_argument('--output_dir', type=str, default="")
    p.add_argument('--dtype', choices=('fp32', 'bf16x3'), default='fp32',
                   help='arithmetic of the MLP trunk: exact fp32, or three bf16 MFMA products of split operands (DESIGN.md 3.23)')
    return p


def precompute_quadratic_samples(near, far, num_samples):
    """The assumed definition of the fork's function: a parabola a x^2 + b x + near over x = linspace(0, 1) with b = 0.2 a, reaching
    far at x = 1 -- samples dense near the camera."""
    start = 0.1
    x = torch.linspace(0, 1, num_samples)
    a = (far - near) / (1. + 2. * start)
    b = 2. * start * a
    return a * x.pow(2) + b * x + near


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def render_options(args, cfg):
    """Command line over args.json over config_parser's defaults -> (N_samples, two_pass, lindisp)."""
    n = args.N_samples if args.N_samples is not None else int(cfg.get('N_samples', 256))
    dlw = args.depth_loss_weight if args.depth_loss_weight is not None else float(cfg.get('depth_loss_weight', 0.004))
    lindisp = args.lindisp if args.lindisp is not None else bool(cfg.get('lindisp', False))
    if n < 1 or (dlw > 0. and n // 2 < 3):
        raise SystemExit(f'nerf_render: N_samples {n}')
    return n, dlw > 0., lindisp


def write_frame(output_dir, index, result):
    """result: dict of numpy (H, W[, 3]) arrays with rgb_map, depth_map, depth_std, acc_map -> (png path, npz path)."""
    from PIL import Image
    png = os.path.join(output_dir, f'{index}_rgb.png')
    Image.fromarray(to8b(result['rgb_map'])).save(png)
    npz = os.path.join(output_dir, f'{index}.npz')
    np.savez_compressed(npz, depth=result['depth_map'].astype(np.float32), depth_std=result['depth_std'].astype(np.float32),
                        acc=result['acc_map'].astype(np.float32))
    return png, npz


def prepare(args, tool='nerf_render', transforms_name='transforms_test.json'):
    """What nerf_render and nerf_test share between the parsed flags and the frame loop: the checkpoint and its options, the poses and
    intrinsics of ``--transforms`` (default ``<data_dir>/<scene_id>/<transforms_name>``), near / far, the scene bounds, the frame
    selection, the first-pass samples and the packed weights -> namespace."""
    from types import SimpleNamespace
    if args.expname is None:
        raise SystemExit(f'{tool}: --expname is required')
    if args.image_hw is None:
        raise SystemExit(f'{tool}: --image_hw H W is required')
    from nerf_rpn_amd import ops
    cfg, state_dict, ckpt_path = load_checkpoint(args.ckpt_dir, args.expname)
    ops.nerf_grid_config(cfg)            # unsupported options stop here, before any file is read
    n_samples, two_pass, lindisp = render_options(args, cfg)
    print(f'{tool}: weights from {ckpt_path}')
    H, W = args.image_hw
    scene = os.path.join(args.data_dir, args.scene_id)
    transforms = args.transforms or os.path.join(scene, transforms_name)
    poses, intrinsics, meta_far, meta = load_transforms(transforms, with_meta=True)
    near = args.near if args.near is not None else meta.get('near')
    far = args.far if args.far is not None else meta_far
    if near is None or far is None:
        raise SystemExit(f'{tool}: give --near and --far (or "near" / "far" in the transforms json)')
    if (args.bb_center is None) != (args.bb_scale is None):
        raise SystemExit('--bb_center and --bb_scale go together')
    if args.bb_center is not None:
        bb_center, bb_scale = torch.tensor(args.bb_center, dtype=torch.float32), torch.tensor(args.bb_scale, dtype=torch.float32)
    else:
        t_poses, t_intr, _ = load_transforms(args.bounds_transforms or os.path.join(scene, 'transforms_train.json'))
        bb_center, bb_scale, lo, hi = corner_bounds(H, W, t_intr, t_poses, far)
        print(f'{tool}: scene bounds from the corner rays: {lo.tolist()} .. {hi.tolist()}')
    frames = list(range(len(poses))) if args.frames is None else args.frames
    for i in frames:
        if not 0 <= i < len(poses):
            raise SystemExit(f'{tool}: frame {i} of {len(poses)}')
    z_samples = precompute_quadratic_samples(near, far, n_samples // 2) if two_pass else None
    weights = ops.nerf_grid_pack(state_dict, cfg, getattr(args, 'dtype', 'fp32'))
    return SimpleNamespace(cfg=cfg, weights=weights, H=H, W=W, poses=poses, intrinsics=intrinsics, near=near, far=far, meta=meta,
                           transforms=transforms, bb_center=bb_center, bb_scale=bb_scale, frames=frames, z_samples=z_samples,
                           n_samples=n_samples, lindisp=lindisp)


def frame_kwargs(run, i):
    """What selects frame i of a prepared run, as ops.nerf_render and ops.nerf_camopt_prepare take it."""
    return dict(H=run.H, W=run.W, intrinsic=run.intrinsics[i], c2w=run.poses[i][:3, :4], near=run.near, far=run.far,
                bb_center=run.bb_center, bb_scale=run.bb_scale, z_samples=run.z_samples, n_samples=run.n_samples, lindisp=run.lindisp)


def render_frame(run, i, chunk=None, embedded_cam=None):
    """ops.nerf_render of frame i of a prepared run (embedded_cam None: the zero embedding)."""
    from nerf_rpn_amd import ops
    return ops.nerf_render(run.weights, run.cfg, chunk=chunk, embedded_cam=embedded_cam, **frame_kwargs(run, i))


def main(argv=None):
    args = build_parser().parse_args(argv)
    run = prepare(args)
    H, W, frames = run.H, run.W, run.frames
    os.makedirs(args.output_dir or '.', exist_ok=True)
    written = []
    for i in frames:
        out = render_frame(run, i, args.chunk)
        written.append(write_frame(args.output_dir, i, {k: v.cpu().numpy() for k, v in out.items()}))
    print(f'nerf_render: {len(written)} frames of {H} x {W} in {args.output_dir or "."}')
    return written


if __name__ == '__main__':
    main()
