"""Ground-truth boxes of ScanNet-style scans (reference data/scannet/generate_bbox.py with MinimumBoundingBox.py).

Run as ``python -m nerf_rpn_amd.scripts.scannet_generate_bbox --scene_path DIR --output_path DIR`` (the reference's flags).  DIR holds
one directory per scene; of ``<scene>/`` it reads ``<scene>_vh_clean.aggregation.json`` (instances: objectId, label, segments), the
segments file that names (``scannet.`` stripped; segIndices = segment of every vertex), ``<scene>_vh_clean_2.ply`` (vertex x / y / z)
and the ``axisAlignment`` line of ``<scene>.txt``, and writes ``<output_path>/<scene>.json``: ``scene_name`` and ``instances`` with
``obj_id``, ``label``, ``min_pt``, ``max_pt``, ``obb`` in the reference's layout (``indent=2``).

Per instance: the float32 min / max corner of its vertices and ``obb = (cx, cy, cz, length_parallel, length_orthogonal, dz, angle)``,
the minimum-area rectangle over the convex hull's edges of the xy projection with the z extent -- HIP kernels (csrc/scanbox.hip), all
instances of a scene in one batch.  The xy numbers are float64 of the float32 coordinates, which is what the reference computes under
its pinned numpy 1.x (``np.float32 / float`` widens there); under numpy 2 the same reference code stays in float32 and lands 1e-7 to
1e-6 relative away.  cz and dz follow the reference's float32 arithmetic.

As in the reference, the axis alignment is parsed (a scene without it is refused) and NOT applied: the boxes are "not aligned", in
the mesh's own frame.

Deliberate differences from the reference:
  * hull edges are enumerated counter-clockwise from the lexicographically smallest (x, y) hull vertex and the first edge of minimum
    area wins, so a box depends only on the set of vertices; the reference starts where Qhull does and may choose another edge of
    exactly equal area (a triangle's three edges, a square's four);
  * an instance with fewer than three vertices, or whose vertices are all collinear or coincident in xy, has no rectangle: the
    reference dies with a ValueError, a Qhull error or numpy's empty-min error.  Here the scene's JSON is not written, the remaining
    scenes are processed, and the program ends with a non-zero exit and one line per such instance (scene, obj_id, label);
  * the PLY file is read with numpy (``read_ply_vertices``: ascii and binary_little_endian, scalar vertex properties); plyfile is
    not needed;
  * scenes are processed one after another on one GPU, in sorted order (the reference uses a pool of 16 processes).
"""
import argparse
import json
import os

import numpy as np

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}
STATUS_TEXT = {1: 'fewer than three vertices', 2: 'all vertices collinear or coincident in xy'}


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('--scene_path', type=str, required=True)
    p.add_argument('--output_path', type=str, required=True)
    return p


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def read_ply_vertices(path):
    """The vertex element of a PLY file as a numpy structured array (one field per scalar property, in the header's order and types).
    Formats ascii and binary_little_endian; elements after the vertices (faces) are not read."""
    with open(path, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError(f'{path}: not a PLY file')
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f'{path}: no end_header')
            tok = line.decode('ascii', 'replace').split()
            if not tok or tok[0] in ('comment', 'obj_info'):
                continue
            if tok[0] == 'format':
                fmt = tok[1]
            elif tok[0] == 'element':
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == 'property':
                if not elements:
                    raise ValueError(f'{path}: property before the first element')
                elements[-1][2].append(tok[1:])
            elif tok[0] == 'end_header':
                break
        if fmt not in ('ascii', 'binary_little_endian'):
            raise ValueError(f'{path}: format {fmt!r} is not supported (ascii, binary_little_endian)')
        if not elements or elements[0][0] != 'vertex':
            raise ValueError(f'{path}: the first element must be the vertices')
        _, count, props = elements[0]
        fields = []
        for p in props:
            if p[0] == 'list' or p[0] not in _PLY_TYPES:
                raise ValueError(f'{path}: vertex property {" ".join(p)!r} is not a scalar')
            fields.append((p[1], '<' + _PLY_TYPES[p[0]]))
        dtype = np.dtype(fields)
        if fmt == 'binary_little_endian':
            data = np.frombuffer(f.read(count * dtype.itemsize), dtype=dtype)
            if data.shape[0] != count:
                raise ValueError(f'{path}: {data.shape[0]} of {count} vertices')
            return data
        out = np.empty(count, dtype=dtype)
        for i in range(count):
            tok = f.readline().split()
            if len(tok) != len(fields):
                raise ValueError(f'{path}: vertex row {i} has {len(tok)} values, {len(fields)} expected')
            out[i] = tuple(float(t) if np.dtype(ft).kind == 'f' else int(t) for t, (_, ft) in zip(tok, fields))
        return out


def load_vertices(path):
    """float32 [V, 3] = x, y, z of the PLY file's vertices."""
    data = read_ply_vertices(path)
    vertices = np.zeros((data.shape[0], 3), dtype=np.float32)
    for k, name in enumerate('xyz'):
        vertices[:, k] = data[name]
    return vertices


def axis_alignment(path):
    """The 4 x 4 axisAlignment matrix of <scene>.txt (parsed as the reference parses it; not applied)."""
    with open(path, 'r') as f:
        lines = [x for x in f.readlines() if 'axisAlignment' in x]
    if not lines:
        raise ValueError(f'{path}: no axisAlignment line')
    return np.array([float(x) for x in lines[0].split('=', 1)[1].split()]).reshape(4, 4)


def load_scene(scene_path):
    """(scene name, [(obj_id, label, segments)], seg_of_vertex int32 [V], vertices float32 [V, 3])."""
    name = os.path.basename(os.path.normpath(scene_path))
    axis_alignment(os.path.join(scene_path, f'{name}.txt'))
    with open(os.path.join(scene_path, f'{name}_vh_clean.aggregation.json'), 'r') as f:
        aggregation = json.load(f)
    instances = [(g['objectId'], g['label'], g['segments']) for g in aggregation['segGroups']]
    with open(os.path.join(scene_path, aggregation['segmentsFile'].replace('scannet.', '')), 'r') as f:
        seg = np.asarray(json.load(f)['segIndices'], dtype=np.int64)
    vertices = load_vertices(os.path.join(scene_path, f'{name}_vh_clean_2.ply'))
    if seg.shape != (vertices.shape[0],):
        raise ValueError(f'{scene_path}: {seg.shape[0]} segment indices for {vertices.shape[0]} vertices')
    if seg.size and (seg.min() < -2 ** 31 or seg.max() >= 2 ** 31):
        raise ValueError(f'{scene_path}: segment indices do not fit int32')
    return name, instances, seg.astype(np.int32), vertices


# ----------------------------------------------------------------------------------------------------------------------
# one scene
# ----------------------------------------------------------------------------------------------------------------------
def scene_dict(name, instances, min_pt, max_pt, obb):
    """The reference's JSON structure (key order as Instance.to_dict)."""
    return {'scene_name': name,
            'instances': [{'obj_id': oid, 'label': label, 'min_pt': min_pt[i].tolist(), 'max_pt': max_pt[i].tolist(), 'obb': obb[i].tolist()}
                          for i, (oid, label, _) in enumerate(instances)]}


def write_scene_json(d, path):
    with open(path, 'w') as f:
        json.dump(d, f, indent=2)


def process_scene(scene_path, output_path, device='cuda'):
    """Write <output_path>/<scene>.json; returns (its path, []) or (None, [one message per degenerate instance])."""
    import torch
    from nerf_rpn_amd import ops
    name, instances, seg, vertices = load_scene(scene_path)
    if not instances:
        return None, [f'{name}: no instances']
    min_pt, max_pt, obb, status, _ = ops.scannet_instance_boxes(torch.from_numpy(vertices).to(device), torch.from_numpy(seg).to(device),
                                                                [s for _, _, s in instances])
    status = status.cpu().numpy()
    bad = [f'{name}: obj_id {instances[i][0]} ({instances[i][1]!r}): {STATUS_TEXT[int(status[i])]}' for i in np.flatnonzero(status)]
    if bad:
        return None, bad
    path = os.path.join(output_path, f'{name}.json')
    write_scene_json(scene_dict(name, instances, min_pt.cpu().numpy(), max_pt.cpu().numpy(), obb.cpu().numpy()), path)
    return path, []


def main(argv=None):
    args = build_parser().parse_args(argv)
    os.makedirs(args.output_path, exist_ok=True)
    written, failed = [], []
    for scene in sorted(os.listdir(args.scene_path)):
        path, bad = process_scene(os.path.join(args.scene_path, scene), args.output_path)
        if path:
            written.append(path)
        failed += bad
    if failed:
        raise SystemExit('no box for:\n  ' + '\n  '.join(failed))
    return written


if __name__ == '__main__':
    main()
