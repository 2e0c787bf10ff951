"""Train a Dense-Depth-Priors NeRF on one scene (reference data/scannet/run_nerf.py, its task ``train``: run_nerf :1012-1094,
train_nerf :755-922), on one GPU through the HIP operations of nerf_rpn_amd.nerf_train.

Run as ``python -m nerf_rpn_amd.scripts.nerf_train --expname NAME --ckpt_dir DIR --data_dir DIR --scene_id SCENE --image_hw H W``
plus the flags of config_parser (:924-1008) that the train task reads, with its defaults: ``--N_rand --lrate --start_decay_lrate
--end_decay_lrate --no_reload --depth_loss_weight --N_samples --perturb --multires_views --input_ch_cam --raw_noise_std --lindisp
--i_print --i_weights --chunk``; ``--near --far --bb_center --bb_scale`` as in nerf_render; ``--N_iters`` (default 500001, which the
reference hard-codes), ``--depth_std`` (metres) and ``--dtype fp32|bf16x3`` (default fp32: the arithmetic of the MLP trunk in every step
and in the evaluation at the end; it is written to args.json, the checkpoints are float32 with the same keys either
way) and ``--backward_dtype fp32|bf16x3`` (default fp32: the arithmetic of the backward's own matrix products, DESIGN.md 3.24;
bf16x3 is refused without ``--dtype bf16x3``; written to args.json too).  An option ops.nerf_grid_config rejects (netdepth, netwidth, multires, i_embed,
N_importance, use_viewdirs) raises as in every NeRF tool here.

Data: ``<data_dir>/<scene_id>/transforms_train.json`` with nerf_extract's keys; the images and depths of its frames as nerf_test
reads them, uploaded once.  The depth prior is what the json names: ``depth_file_path`` is the depth (16-bit PNG / the json's
``depth_scaling_factor``; valid where the raw value is > 0, depth 0 elsewhere, so that such a ray is sampled around its predicted
depth); an optional ``depth_std_file_path`` in the same encoding is its standard deviation, otherwise ``--depth_std`` is required when
depth_loss_weight > 0.  The scene normalisation is ``--bb_center --bb_scale`` or the corner rays of the training frames.

Output: ``<ckpt_dir>/<expname>/args.json`` (:1019-1025) and ``{:06d}.tar`` every i_weights steps and after the last step, with the
reference's keys (global_step, network_fn_state_dict with ``module.`` prefixes, optimizer_state_dict) plus embedcam_state_dict.
Without ``--no_reload`` the newest ``.tar`` of the run is resumed.  nerf_render, nerf_test and nerf_extract read a run's newest
checkpoint whose name contains ``000.tar``, as the reference does (:335): a checkpoint at any other step count -- the last one of a
run whose ``N_iters - 1`` is no multiple of 1000 -- serves resuming only, and saving it warns so.  After the last step the views of
``transforms_test.json``, if the scene has one, are evaluated as nerf_test does, into ``test_images_<scene_id>/`` (:910-919).

Not covered: depth completion (complete_depth needs the fork's network and weights: the depth prior is read, not
predicted), tensorboard, the ``--i_img`` images, LPIPS, N_importance > 0, more than one GPU, a fused clip + Adam.
"""
import argparse
import datetime
import os
import time

import numpy as np
import torch

from . import nerf_render as NR
from . import nerf_test as NT
from .nerf_extract import corner_bounds, load_transforms

# config_parser's defaults (:929-1003) of the flags the train task reads
TRAIN_FLAGS = dict(N_rand=32 * 32, lrate=5e-4, start_decay_lrate=400000, end_decay_lrate=500000, depth_loss_weight=0.004, N_samples=256,
                   perturb=1., multires_views=0, input_ch_cam=4, raw_noise_std=0., i_print=1000, i_weights=100000, chunk=1024 * 32)
FIXED = dict(netdepth=8, netwidth=256, multires=9, i_embed=0, N_importance=0, use_viewdirs=True)      # what the kernels are built for


def build_parser():
    p = argparse.ArgumentParser()
    for name in ('expname', 'ckpt_dir', 'data_dir', 'scene_id', 'bb_center', 'bb_scale', 'image_hw', 'near', 'far'):
        src = next(a for a in NR.build_parser()._actions if a.dest == name)
        p.add_argument(*src.option_strings, type=src.type, default=src.default, nargs=src.nargs, metavar=src.metavar)
    for name, default in TRAIN_FLAGS.items():
        p.add_argument('--' + name, type=type(default), default=default)
    for name, default in FIXED.items():
        if name != 'use_viewdirs':
            p.add_argument('--' + name, type=int, default=default)
    p.add_argument('--use_viewdirs', action='store_true', default=True)
    p.add_argument('--no_reload', action='store_true')
    p.add_argument('--lindisp', action='store_true', default=False)
    p.add_argument('--N_iters', type=int, default=500001, help='the loop runs steps 1 .. N_iters - 1')
    p.add_argument('--depth_std', type=float, default=None, help='standard deviation of the depth prior in metres, without a std file')
    p.add_argument('--dtype', choices=('fp32', 'bf16x3'), default='fp32',
                   help='arithmetic of the MLP trunk: exact fp32, or three bf16 MFMA products of split operands (DESIGN.md 3.23)')
    p.add_argument('--backward_dtype', choices=('fp32', 'bf16x3'), default='fp32',
                   help='arithmetic of the dgrad and weight-gradient products of the trunk; bf16x3 needs --dtype bf16x3 (DESIGN.md 3.24)')
    return p


def load_depth_png(scene_dir, rel, H, W, scale):
    from PIL import Image
    if scale is None:
        raise SystemExit('nerf_train: the transforms json has depth files but no "depth_scaling_factor"')
    raw = np.asarray(Image.open(os.path.join(scene_dir, rel)))
    if raw.shape != (H, W) or raw.dtype.kind not in 'ui':
        raise SystemExit(f'nerf_train: {rel} is not a {H} x {W} integer depth image')
    return (raw.astype(np.float64) / float(scale)).astype(np.float32), raw > 0


def load_scene(args):
    """The training views -> the namespace nerf_train.train takes."""
    from types import SimpleNamespace
    if args.image_hw is None:
        raise SystemExit('nerf_train: --image_hw H W is required')
    H, W = args.image_hw
    scene = os.path.join(args.data_dir, args.scene_id)
    path = os.path.join(scene, 'transforms_train.json')
    poses, intrinsics, meta_far, meta = load_transforms(path, with_meta=True)
    near = args.near if args.near is not None else meta.get('near')
    far = args.far if args.far is not None else meta_far
    if near is None or far is None:
        raise SystemExit('nerf_train: give --near and --far (or "near" / "far" in the transforms json)')
    if (args.bb_center is None) != (args.bb_scale is None):
        raise SystemExit('--bb_center and --bb_scale go together')
    if args.bb_center is not None:
        bb_center, bb_scale = torch.tensor(args.bb_center, dtype=torch.float32), torch.tensor(args.bb_scale, dtype=torch.float32)
    else:
        bb_center, bb_scale, lo, hi = corner_bounds(H, W, intrinsics, poses, far)
        print(f'nerf_train: scene bounds from the corner rays: {lo.tolist()} .. {hi.tolist()}')
    images, depths, valids = [], [], []
    scale = meta.get('depth_scaling_factor')
    for fr in meta['frames']:
        image, depth, valid = NT.load_targets(scene, fr, H, W, scale)
        images.append(image)
        if args.depth_loss_weight > 0.:
            if depth is None:
                raise SystemExit('nerf_train: depth_loss_weight > 0 needs a "depth_file_path" for every training frame')
            if fr.get('depth_std_file_path'):
                std, _ = load_depth_png(scene, fr['depth_std_file_path'], H, W, scale)
            elif args.depth_std is not None:
                std = np.full((H, W), args.depth_std, np.float32)
            else:
                raise SystemExit('nerf_train: give --depth_std, or a "depth_std_file_path" for every training frame')
            depth, std = np.where(valid, depth, np.float32(0)), np.where(valid, std, np.float32(0))
            depths.append(np.stack([depth, std], -1).astype(np.float32))
            valids.append(valid)
    return SimpleNamespace(images=torch.from_numpy(np.stack(images)), depths=torch.from_numpy(np.stack(depths)) if depths else None,
                           valid_depths=torch.from_numpy(np.stack(valids)) if valids else None, poses=poses, intrinsics=intrinsics,
                           near=float(near), far=float(far), bb_center=bb_center, bb_scale=bb_scale, H=H, W=W, scene=scene)


def main(argv=None):
    from nerf_rpn_amd import nerf_train, ops
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.backward_dtype == 'bf16x3' and args.dtype != 'bf16x3':
        parser.error('--backward_dtype bf16x3 needs --dtype bf16x3')
    ops.nerf_grid_config(args)           # unsupported options stop here, before any file is read
    if args.expname is None:             # run_nerf :1020-1021
        args.expname = '{}_{}'.format(datetime.datetime.fromtimestamp(time.time()).strftime('%Y%m%d_%H%M%S'), args.scene_id)
    run = load_scene(args)
    args.near, args.far = run.near, run.far
    args.bb_center, args.bb_scale = [float(v) for v in run.bb_center], float(run.bb_scale)
    nerf_train.write_args(args)
    result = nerf_train.train(run, args)
    test_json = os.path.join(run.scene, 'transforms_test.json')
    if os.path.exists(test_json) and result.step + 1 == args.N_iters:
        targs = NT.build_parser().parse_args(['--expname', args.expname, '--ckpt_dir', args.ckpt_dir, '--data_dir', args.data_dir,
                                              '--scene_id', args.scene_id, '--image_hw', str(run.H), str(run.W)])
        targs.near, targs.far, targs.bb_center, targs.bb_scale = run.near, run.far, args.bb_center, args.bb_scale
        targs.dtype = args.dtype
        trun = test_run(targs, run, args, result.model)
        NT.run_frames(targs, trun, NT.result_dir(targs), tool='nerf_train')
    return result


def test_run(targs, run, args, model):
    """NR.prepare's namespace for the held-out views with the weights just trained (whatever the checkpoint's step number)."""
    from types import SimpleNamespace
    from nerf_rpn_amd import ops
    cfg = dict(vars(args))
    transforms = os.path.join(run.scene, 'transforms_test.json')
    poses, intrinsics, _, meta = load_transforms(transforms, with_meta=True)
    n_samples, two_pass, lindisp = NR.render_options(targs, cfg)
    z_samples = NR.precompute_quadratic_samples(run.near, run.far, n_samples // 2) if two_pass else None
    weights = ops.nerf_grid_pack({k: v.detach() for k, v in model.state_dict().items()}, cfg, getattr(args, 'dtype', 'fp32'))
    return SimpleNamespace(cfg=cfg, weights=weights, H=run.H, W=run.W, poses=poses, intrinsics=intrinsics, near=run.near, far=run.far,
                           meta=meta, transforms=transforms, bb_center=run.bb_center, bb_scale=run.bb_scale,
                           frames=list(range(len(poses))), z_samples=z_samples, n_samples=n_samples, lindisp=lindisp)


if __name__ == '__main__':
    main()
