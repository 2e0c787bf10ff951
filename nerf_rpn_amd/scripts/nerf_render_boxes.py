"""Render a trained Dense-Depth-Priors NeRF inside or outside 3D boxes: the proposals of run_rpn / run_fcos, or the ground-truth
boxes of scannet_generate_bbox, seen in the NeRF they came from (the counterpart, for the scenes of nerf_train / nerf_extract, of the
crop boxes the reference's nerf_rpn/scripts/proposals2ngp.py writes for the instant-ngp viewer).

Run as ``python -m nerf_rpn_amd.scripts.nerf_render_boxes <the flags of nerf_render>`` plus one source of boxes,

  ``--proposals FILE.npz --features FILE.npz [--threshold 0.5] [--top_k 30]``: ``proposal`` [K, 6 | 7] and ``score`` [K] in grid
      coordinates, filtered and ordered as proposals2ngp.process_scene does (score > threshold, best first, top_k), and taken to world
      coordinates with the feature file's resolution / bbox_min / bbox_max (ops.nerf_boxes_to_world: from_ddp_nerf files only), or
  ``--boxes_json FILE``: an instance json of scannet_generate_bbox, whose instances carry ``obb`` in world coordinates,

and ``--mode keep|remove`` (the scene inside the boxes only, or without them), ``--each`` (one output set per box under
``<output_dir>/box_<k>/`` instead of all boxes together) and ``--background R G B`` (default 0 0 0: ``rgb + (1 - acc) * bg`` before
quantising).  Per frame i an output set gets what nerf_render writes, ``<i>_rgb.png`` and ``<i>.npz``; the share of the 64-point
tiles whose MLP ran is printed per frame.
"""
import json
import os

import numpy as np

from . import nerf_render as NR


def build_parser():
    p = NR.build_parser()
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--proposals', type=str, default=None, help='proposal file of run_rpn / run_fcos (grid coordinates); needs --features')
    src.add_argument('--boxes_json', type=str, default=None, help='instance json of scannet_generate_bbox (obb, world coordinates)')
    p.add_argument('--features', type=str, default=None, help='the feature file the proposals were made on')
    p.add_argument('--threshold', type=float, default=0.5, help='the threshold for the proposal scores')
    p.add_argument('--top_k', type=int, default=30, help='the number of proposals to render')
    p.add_argument('--mode', choices=('keep', 'remove'), default='keep')
    p.add_argument('--each', action='store_true', help='one output set per box under box_<k>/')
    p.add_argument('--background', type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=('R', 'G', 'B'))
    return p


def load_boxes(args):
    """The boxes of the command line in world coordinates -> float64 [K, 6 | 7]."""
    from nerf_rpn_amd import ops
    if args.proposals is not None:
        if args.features is None:
            raise SystemExit('nerf_render_boxes: --proposals needs --features')
        with np.load(args.proposals) as p:
            scores, proposals = p['score'], p['proposal']
        keep = scores > args.threshold
        scores, proposals = scores[keep], proposals[keep]
        order = np.argsort(scores)[::-1]
        proposals = proposals[order][:args.top_k]
        with np.load(args.features) as f:
            return ops.nerf_boxes_to_world(proposals, {k: f[k] for k in f.files})
    with open(args.boxes_json) as f:
        scene = json.load(f)
    for inst in scene['instances']:
        if 'obb' not in inst:
            raise SystemExit(f'nerf_render_boxes: instance {inst.get("obj_id")!r} of {args.boxes_json} has no obb')
    return np.array([inst['obb'] for inst in scene['instances']], dtype=np.float64).reshape(-1, 7)


def over_background(result, background):
    """rgb + (1 - acc) * bg on the float32 maps."""
    bg = np.asarray(background, dtype=np.float32)
    return dict(result, rgb_map=result['rgb_map'] + (np.float32(1.0) - result['acc_map'])[..., None] * bg)


def main(argv=None):
    args = build_parser().parse_args(argv)
    from nerf_rpn_amd import ops
    boxes = load_boxes(args)
    ops.nerf_box_table(boxes)            # a bad box stops here, before the checkpoint is read
    run = NR.prepare(args, tool='nerf_render_boxes')
    sets = [(os.path.join(args.output_dir, f'box_{k}'), boxes[k:k + 1]) for k in range(len(boxes))] if args.each else [(args.output_dir, boxes)]
    written = []
    for out_dir, b in sets:
        os.makedirs(out_dir or '.', exist_ok=True)
        for i in run.frames:
            out = ops.nerf_render_boxes(run.weights, run.cfg, b, args.mode, chunk=args.chunk, **NR.frame_kwargs(run, i))
            ran, total = int(out.pop('tiles_run').sum()), int(out.pop('tiles_total').sum())
            print(f'nerf_render_boxes: frame {i}, {len(b)} boxes ({args.mode}): {ran} of {total} tiles run ({100.0 * ran / total:.1f} %)')
            written.append(NR.write_frame(out_dir, i, over_background({k: v.cpu().numpy() for k, v in out.items()}, args.background)))
    print(f'nerf_render_boxes: {len(written)} frames of {run.H} x {run.W} in {args.output_dir or "."}')
    return written


if __name__ == '__main__':
    main()
