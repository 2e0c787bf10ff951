"""Rescale ScanNet boxes to grid units and drop small or excluded ones (reference data/scannet/filter_bbox.py).

Run as ``python -m nerf_rpn_amd.scripts.scannet_filter_bbox --feature_dir DIR --obj_json_dir DIR --npy_output_dir DIR
--json_output_dir DIR [--min_size 8] [--excluded_labels FILE]``.  For every ``<scene>.npz`` of ``--feature_dir`` (its ``resolution`` is
read) and the ``<scene>.json`` that scannet_generate_bbox wrote, the OBBs are mapped from the mesh frame into the feature grid -- the
scene box is the min / max over all instances' corners -- and an instance is dropped when its label is excluded or its smallest
extent is below ``--min_size`` grid cells.  ``<npy_output_dir>/<scene>.npy`` holds the kept float64 [N, 7] boxes (what datasets.py
reads as OBB ground truth) and ``<json_output_dir>/<scene>.json`` the kept instances.  Host-only numpy, the reference's arithmetic in
the reference's order: for the same inputs the ``.npy`` has the same bytes.

Deliberate difference: the reference carries its list of excluded labels in its source.  Here it is data: ``--excluded_labels`` names
a JSON list of label names; without the flag no label is excluded, and the tool says so.
"""
import argparse
import json
import os

import numpy as np


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--feature_dir', type=str, required=True)
    p.add_argument('--obj_json_dir', type=str, required=True)
    p.add_argument('--npy_output_dir', type=str, required=True)
    p.add_argument('--json_output_dir', type=str, required=True)
    p.add_argument('--min_size', type=int, default=8)
    p.add_argument('--excluded_labels', type=str, default=None, help='JSON list of label names to drop (default: none)')
    return p


def filter_scene(feature_path, obj_json_path, npy_output_path, json_output_path, min_size, excluded=()):
    """One scene; returns the keep mask over the input instances."""
    res = np.load(feature_path)['resolution']
    with open(obj_json_path) as f:
        scene = json.load(f)
    inst = scene['instances']
    obb = np.array([x['obb'] for x in inst])
    lo = np.min(np.array([x['min_pt'] for x in inst]), axis=0)
    hi = np.max(np.array([x['max_pt'] for x in inst]), axis=0)
    obb[:, 3:6] = obb[:, 3:6] / (hi - lo) * res
    obb[:, :3] = (obb[:, :3] - lo) / (hi - lo) * res
    excluded = set(excluded)
    keep = np.array([x['label'] not in excluded and not np.min(obb[i, 3:6]) < min_size for i, x in enumerate(inst)], dtype=bool)
    np.save(npy_output_path, obb[keep])
    scene['instances'] = [x for x, k in zip(inst, keep) if k]
    with open(json_output_path, 'w') as f:
        json.dump(scene, f, indent=2)
    return keep


def main(argv=None):
    args = build_parser().parse_args(argv)
    excluded = ()
    if args.excluded_labels is None:
        print('scannet_filter_bbox: no --excluded_labels file given: no label is excluded')
    else:
        with open(args.excluded_labels) as f:
            excluded = json.load(f)
        if not isinstance(excluded, list) or not all(isinstance(x, str) for x in excluded):
            raise SystemExit(f'{args.excluded_labels}: expected a JSON list of label names')
    os.makedirs(args.npy_output_dir, exist_ok=True)
    os.makedirs(args.json_output_dir, exist_ok=True)
    written = []
    for scene in sorted(os.listdir(args.feature_dir)):
        name = scene.split('.')[0]
        filter_scene(os.path.join(args.feature_dir, f'{name}.npz'), os.path.join(args.obj_json_dir, f'{name}.json'),
                     os.path.join(args.npy_output_dir, f'{name}.npy'), os.path.join(args.json_output_dir, f'{name}.json'),
                     args.min_size, excluded)
        written.append(os.path.join(args.npy_output_dir, f'{name}.npy'))
    return written


if __name__ == '__main__':
    main()
