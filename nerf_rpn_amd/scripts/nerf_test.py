"""Evaluate a trained Dense-Depth-Priors NeRF on held-out views: image MSE, PSNR, SSIM and depth RMSE against the ground truth
(reference data/scannet/run_nerf.py, its tasks ``test`` and ``render_train_depth``: render_images_with_metrics :231-311,
write_images_with_metrics :313-331, dispatched at :1102-1138).

Run as ``python -m nerf_rpn_amd.scripts.nerf_test --expname NAME --ckpt_dir DIR --data_dir DIR --scene_id SCENE --image_hw H W
[--task test|render_train_depth] [--output_dir DIR]`` plus every flag of nerf_render.  ``--task test`` (the default) reads
``<data_dir>/<scene_id>/transforms_test.json`` and writes to ``<ckpt_dir>/<expname>/test_images_<scene_id>/``; ``render_train_depth``
reads ``transforms_train.json`` and writes to ``<ckpt_dir>/<expname>/train_depth_<scene_id>/`` -- the same code over the training
views.  ``--transforms`` and ``--output_dir`` override either.

Per selected frame, in json order and numbered n = 0, 1, .. as the reference numbers what it rendered: the frame is rendered
(ops.nerf_render), its metrics and its 8- / 16-bit images are computed on the GPU (ops.nerf_view_metrics), ``<n>_rgb.jpg`` (PIL, quality
95) and ``<n>_d.png`` (16-bit, to16b(depth / far)) are written.  Then ``metrics.txt`` gets one ``key: value`` line each for img_loss,
psnr, ssim and depth_rmse -- the means over the frames; depth_rmse over the frames that have one, and no line if none has -- and the
same lines are printed.

Targets: each frame's ``file_path`` (relative to the json; image / 255 as float32) and, if present, ``depth_file_path`` (16-bit PNG /
the json's ``depth_scaling_factor`` as float32, valid where the raw value is > 0).  A frame without a depth file has no depth metric.

Assumptions: the loader, img2mse, mse2psnr, compute_rmse, to16b and MeanTracker's output format live in the
Dense-Depth-Priors code, which is not part of the reference; their assumed definitions are restated in DESIGN.md.  LPIPS, the
test-time optimisation of the camera embedding (``test_opt``) and ``rgb0`` (N_importance is 0) are not covered.
"""
import os

import numpy as np
import torch

from . import nerf_render as NR

TASKS = {'test': ('transforms_test.json', 'test_images_'), 'render_train_depth': ('transforms_train.json', 'train_depth_')}
KEYS = ('img_loss', 'psnr', 'ssim', 'depth_rmse')


def build_parser():
    p = NR.build_parser()
    p.add_argument('--task', type=str, default='test', choices=sorted(TASKS))
    p.set_defaults(output_dir=None)
    return p


def result_dir(args):
    """write_images_with_metrics :314-318."""
    if args.output_dir:
        return args.output_dir
    return os.path.join(args.ckpt_dir, args.expname, TASKS[args.task][1] + args.scene_id)


def load_targets(scene_dir, frame, H, W, depth_scaling_factor):
    """-> (image float32 [H, W, 3] in [0, 1], depth float32 [H, W] or None, valid bool [H, W] or None) of one frame of the json."""
    from PIL import Image
    if 'file_path' not in frame:
        raise SystemExit('nerf_test: a frame of the transforms json has no "file_path"')
    img = np.asarray(Image.open(os.path.join(scene_dir, frame['file_path'])).convert('RGB'))
    if img.shape != (H, W, 3):
        raise SystemExit(f'nerf_test: {frame["file_path"]} is {img.shape[0]} x {img.shape[1]}, --image_hw is {H} x {W}')
    image = (img / 255.).astype(np.float32)
    if not frame.get('depth_file_path'):
        return image, None, None
    if depth_scaling_factor is None:
        raise SystemExit('nerf_test: the transforms json has depth files but no "depth_scaling_factor"')
    raw = np.asarray(Image.open(os.path.join(scene_dir, frame['depth_file_path'])))
    if raw.shape != (H, W) or raw.dtype.kind not in 'ui':
        raise SystemExit(f'nerf_test: {frame["depth_file_path"]} is not a {H} x {W} integer depth image')
    depth = (raw.astype(np.float64) / float(depth_scaling_factor)).astype(np.float32)
    return image, depth, raw > 0


def mean_metrics(frames):
    """The reference's two trackers (:251-252, :309-310): depth_rmse is tracked apart because not every frame has one -> dict in
    metrics.txt's order, without depth_rmse if no frame has it."""
    out = {}
    for k in KEYS:
        vals = [m[k] for m in frames if m.get(k) is not None]
        if vals:
            out[k] = sum(vals) / float(len(vals))
    return out


def format_metrics(means):
    """MeanTracker.print's lines."""
    return ''.join('{}: {}\n'.format(k, v) for k, v in means.items())


def write_images(out_dir, n, rgb8, depth16):
    """write_images_with_metrics :321-327 -> (jpg path, png path).  The reference hands cv2 the frame as BGR, so the file holds RGB."""
    from PIL import Image
    jpg, png = os.path.join(out_dir, f'{n}_rgb.jpg'), os.path.join(out_dir, f'{n}_d.png')
    Image.fromarray(rgb8).save(jpg, quality=95)
    Image.fromarray(depth16).save(png)
    return jpg, png


def run_frames(args, run, out_dir, tool='nerf_test', embedding=None):
    """The frame loop of every task: targets, render, metrics, images, then the means and metrics.txt -> main's result.
    ``embedding(run, i, image)``, if given, returns the camera embedding frame i is rendered with (None: the zero embedding)."""
    from nerf_rpn_amd import ops
    H, W = run.H, run.W
    scene_dir = os.path.dirname(os.path.abspath(run.transforms))
    os.makedirs(out_dir, exist_ok=True)
    per_frame = []
    for n, i in enumerate(run.frames):
        image, depth, valid = load_targets(scene_dir, run.meta['frames'][i], H, W, run.meta.get('depth_scaling_factor'))
        if depth is None:      # no depth metric for this frame; the rendered depth is still written
            depth, valid = np.zeros((H, W), np.float32), np.zeros((H, W), bool)
        out = NR.render_frame(run, i, args.chunk, embedding(run, i, image) if embedding else None)
        m = ops.nerf_view_metrics(out['rgb_map'], torch.from_numpy(image), out['depth_map'], torch.from_numpy(depth),
                                  torch.from_numpy(valid), far=run.far, return_images=True)
        write_images(out_dir, n, m.pop('rgb8').cpu().numpy(), m.pop('depth16').cpu().numpy())
        per_frame.append(m)
        print('{}: frame {} ({}/{}): PSNR {}'.format(tool, i, n + 1, len(run.frames), m['psnr']))
    means = mean_metrics(per_frame)
    text = format_metrics(means)
    with open(os.path.join(out_dir, 'metrics.txt'), 'w') as f:
        f.write(text)
    print(text, end='')
    print(f'{tool}: {len(per_frame)} frames of {H} x {W} in {out_dir}')
    return {'dir': out_dir, 'frames': per_frame, 'mean': means}


def main(argv=None):
    args = build_parser().parse_args(argv)
    run = NR.prepare(args, tool='nerf_test', transforms_name=TASKS[args.task][0])
    return run_frames(args, run, result_dir(args))


if __name__ == '__main__':
    main()
