"""Evaluate a trained Dense-Depth-Priors NeRF on held-out views with the camera embedding fitted to each view first: the ``test_opt``
task of the reference's data/scannet/run_nerf.py (optimize_camera_embedding :193-229, called from render_images_with_metrics :265-269,
dispatched at :1103-1119, written by write_images_with_metrics :313-331).

Run as ``python -m nerf_rpn_amd.scripts.nerf_test_opt --expname NAME --ckpt_dir DIR --data_dir DIR --scene_id SCENE --image_hw H W
[--N_rand N] [--opt_steps K] [--opt_seed S] [--opt_cache_gib G] [--output_dir DIR]`` plus every flag of nerf_render.  It is
nerf_test's ``test`` task -- the same frames of ``transforms_test.json``, targets, metrics, images and ``metrics.txt`` (its functions
are used as they are) -- with one step in front of each frame's render: ``--opt_steps`` (100) Adam steps over all pixels, in batches
of 2 ``--N_rand`` (args.json's, else 1024) drawn once per frame from a CPU generator seeded with ``--opt_seed`` (0).  Everything
that does not depend on the embedding is computed once per frame (ops.nerf_camopt_prepare; ``--opt_cache_gib`` caps the trunk outputs
kept on the device, default half of the free memory), each step is one ops.nerf_camopt_eval, the loop is camopt.optimize_embedding.
The fitted embedding is written to ``<ckpt_dir>/<expname>/test_latent_codes_<scene_id>/<frame index>.txt`` (np.savetxt, :267-269), the
frame is rendered with it, and the results go to ``<ckpt_dir>/<expname>/test_images_with_optimization_<scene_id>/`` (:316) or
``--output_dir``.  A model without a camera embedding (input_ch_cam 0) is refused.

nerf_test itself keeps its two tasks and its output byte for byte; this task is an entry point of its own.  Two quirks of the
reference are recorded, not copied: it builds its pixel grid with ``half_W = W`` (the whole image, as here), and on a GPU it hands Adam
the non-leaf ``torch.zeros(..., requires_grad=True).to(device)``.  Assumptions: those of nerf_test and
create_random_subsets (3.19).  LPIPS and ``rgb0`` (N_importance is 0) are not covered.
"""
import os

import numpy as np
import torch

from . import nerf_render as NR
from . import nerf_test as NT

TRANSFORMS, RESULT_PREFIX, LATENT_PREFIX = 'transforms_test.json', 'test_images_with_optimization_', 'test_latent_codes_'


def build_parser():
    p = NR.build_parser()
    p.add_argument('--N_rand', type=int, default=None, help='half the rays of a batch (default: args.json, else 1024)')
    p.add_argument('--opt_steps', type=int, default=100, help='Adam steps per frame')
    p.add_argument('--opt_seed', type=int, default=0, help='seed of the CPU generator that draws the batches')
    p.add_argument('--opt_cache_gib', type=float, default=None, help='GiB of trunk outputs kept on the device')
    p.set_defaults(output_dir=None)
    return p


def result_dir(args):
    """write_images_with_metrics :314-318 with test-time optimisation."""
    return args.output_dir or os.path.join(args.ckpt_dir, args.expname, RESULT_PREFIX + args.scene_id)


def latent_code_dir(args):
    """:267."""
    return os.path.join(args.ckpt_dir, args.expname, LATENT_PREFIX + args.scene_id)


def optimize_frame(run, i, image, args):
    """optimize_camera_embedding (:193-229) for frame i against its target image -> the fitted embedding, float32 [input_ch_cam]."""
    from nerf_rpn_amd import camopt, ops
    n = run.H * run.W
    n_rand = args.N_rand if args.N_rand is not None else int(run.cfg.get('N_rand', 1024))
    if n_rand < 1 or args.opt_steps < 0:
        raise SystemExit(f'nerf_test_opt: --N_rand {n_rand}, --opt_steps {args.opt_steps}')
    batches = camopt.random_subsets(n, 2 * n_rand, torch.Generator().manual_seed(args.opt_seed))
    cache = None if args.opt_cache_gib is None else int(args.opt_cache_gib * 2 ** 30)
    state = ops.nerf_camopt_prepare(run.weights, run.cfg, torch.from_numpy(image), chunk=args.chunk,
                                    ray_weight=camopt.ray_weights(batches, n), cache_bytes=cache, **NR.frame_kwargs(run, i))

    def value_and_grad(cam):
        loss, grad = ops.nerf_camopt_eval(state, cam)
        return loss / len(batches), grad
    return camopt.optimize_embedding(value_and_grad, ops.nerf_grid_config(run.cfg)['input_ch_cam'], steps=args.opt_steps)


def main(argv=None):
    args = build_parser().parse_args(argv)
    run = NR.prepare(args, tool='nerf_test_opt', transforms_name=TRANSFORMS)
    from nerf_rpn_amd import ops
    if ops.nerf_grid_config(run.cfg)['input_ch_cam'] == 0:
        raise SystemExit('nerf_test_opt: the model has no camera embedding to optimise (input_ch_cam is 0)')
    os.makedirs(latent_code_dir(args), exist_ok=True)

    def embedding(run, i, image):
        cam = optimize_frame(run, i, image, args)
        np.savetxt(os.path.join(latent_code_dir(args), f'{i}.txt'), cam.numpy())
        return cam
    return NT.run_frames(args, run, result_dir(args), tool='nerf_test_opt', embedding=embedding)


if __name__ == '__main__':
    main()
