"""Timing record of scannet_generate_bbox on one synthetic ScanNet-sized scene (recorded, not gated: profiles/scannet_bbox_scene.json).

The scene has 150 000 vertices and 40 instances in the real ScanNet file layout; one instance is a 5 000-vertex ring (every vertex a
hull vertex: the case that stalls the reference's quadratic rectangle search for minutes), the others are boxes, blobs and discs.

    python tools/scannet_profile_scene.py --out profiles/scannet_bbox_scene.json       end-to-end CLI path + kernel times (HIP events)
    python tools/scannet_profile_scene.py --kernels-only                               the kernels alone, e.g. under a kernel-trace profiler
    python tools/scannet_profile_scene.py --out FILE --reference-seconds 123.4         also record the reference's CPU time for this scene
                                                                                       (tests/golden/make_scannet_golden.py --time)
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

IDENTITY = "1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1"


def write_scene_dir(root, name, vertices, seg_of_vertex, groups, faces=((0, 1, 2), (2, 3, 0)), seed=0):
    """A scene directory <root>/<name>/ in ScanNet's layout: <name>.txt (axisAlignment), <name>_vh_clean.aggregation.json (groups =
    [(objectId, label, [segments])]), <name>_vh_clean_2.0.010000.segs.json, <name>_vh_clean_2.ply (binary little-endian, x y z red green
    blue alpha, a few faces).  Returns the directory."""
    d = os.path.join(root, name)
    os.makedirs(d, exist_ok=True)
    segs_file = f"{name}_vh_clean_2.0.010000.segs.json"
    with open(os.path.join(d, f"{name}.txt"), "w") as f:
        f.write(f"axisAlignment = {IDENTITY}\ncolorHeight = 968\nnumDepthFrames = 1\nsceneType = Synthetic\n")
    with open(os.path.join(d, f"{name}_vh_clean.aggregation.json"), "w") as f:
        json.dump({"sceneId": f"scannet.{name}", "appId": "synthetic",
                   "segGroups": [{"id": i, "objectId": oid, "segments": [int(s) for s in segs], "label": label}
                                 for i, (oid, label, segs) in enumerate(groups)],
                   "segmentsFile": f"scannet.{segs_file}"}, f)
    with open(os.path.join(d, segs_file), "w") as f:
        json.dump({"sceneId": name, "segIndices": [int(s) for s in seg_of_vertex]}, f)
    v = np.asarray(vertices, dtype=np.float32)
    rec = np.zeros(len(v), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    rgb = np.random.default_rng(seed).integers(0, 256, (len(v), 3))
    rec["red"], rec["green"], rec["blue"], rec["alpha"] = rgb[:, 0], rgb[:, 1], rgb[:, 2], 255
    header = ("ply\nformat binary_little_endian 1.0\ncomment synthetic scene\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
              f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(os.path.join(d, f"{name}_vh_clean_2.ply"), "wb") as f:
        f.write(header.encode())
        f.write(rec.tobytes())
        for tri in faces:
            f.write(struct.pack("<B3i", 3, *tri))
    return d


def profile_scene(root, name="scene9000_00", num_vertices=150_000, num_instances=40, ring=5_000, seed=20261018):
    """Write the timing scene; returns its directory."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(800, 4000, num_instances - 1)
    parts, seg, groups = [], [], []
    t = np.sort(rng.uniform(0, 2 * np.pi, ring))
    parts.append(np.stack([2.0 + 0.6 * np.cos(t), -1.0 + 0.6 * np.sin(t), rng.uniform(0.7, 0.75, ring)], axis=1))
    seg += [1] * ring
    groups.append((0, "round table", [1]))
    for g, n in enumerate(sizes, start=1):
        c = rng.uniform(-4, 4, 3) * np.array([1, 1, 0.2])
        a = rng.uniform(0, np.pi)
        rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        kind = g % 3
        if kind == 0:
            xy = rng.uniform(-0.5, 0.5, (n, 2)) * rng.uniform(0.3, 1.5, 2)
        elif kind == 1:
            xy = rng.normal(0, 1, (n, 2)) * rng.uniform(0.1, 0.5, 2)
        else:
            r, th = 0.5 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
            xy = np.stack([r * np.cos(th), 0.6 * r * np.sin(th)], axis=1)
        parts.append(np.concatenate([xy @ rot.T + c[:2], c[2] + rng.uniform(0, 0.8, (n, 1))], axis=1))
        half = int(n) // 2
        seg += [2 * g] * half + [2 * g + 1] * (int(n) - half)
        groups.append((g, f"object {g}", [2 * g, 2 * g + 1]))
    rest = num_vertices - sum(len(p) for p in parts)       # floor and walls: vertices of no instance
    parts.append(np.concatenate([rng.uniform(-5, 5, (rest, 2)), np.zeros((rest, 1))], axis=1))
    seg += [0] * rest
    order = rng.permutation(num_vertices)
    return write_scene_dir(root, name, np.concatenate(parts)[order], np.array(seg)[order], groups, seed=seed)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--kernels-only", action="store_true", help="run the kernels 3 times on the loaded scene and exit")
    ap.add_argument("--reference-seconds", type=float, default=None, help="CPU time of the reference on the same scene, measured elsewhere")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    import torch
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.scripts import scannet_generate_bbox as S
    with tempfile.TemporaryDirectory() as tmp:
        scenes, out = os.path.join(tmp, "scans"), os.path.join(tmp, "out")
        d = profile_scene(scenes)
        name, instances, seg, vertices = S.load_scene(d)
        dv, ds = torch.from_numpy(vertices).cuda(), torch.from_numpy(seg).cuda()
        segs = [s for _, _, s in instances]
        for _ in range(3):
            res = ops.scannet_instance_boxes(dv, ds, segs)
        torch.cuda.synchronize()
        if args.kernels_only:
            return None
        ev = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = ops.scannet_instance_boxes(dv, ds, segs)
            b.record()
            torch.cuda.synchronize()
            ev.append(a.elapsed_time(b))
        cli = []
        for _ in range(3):
            t0 = time.perf_counter()
            S.main(["--scene_path", scenes, "--output_path", out])
            cli.append(time.perf_counter() - t0)
        rec = {"scene": {"vertices": int(vertices.shape[0]), "instances": len(instances), "ring_vertices": 5000,
                         "largest_instance": int(res[4].max().item())},
               "device": torch.cuda.get_device_name(0),
               "boxes_ms": {"what": "ops.scannet_instance_boxes, inputs on the device: three C calls, two read-backs (HIP events)",
                            "runs": [round(x, 3) for x in ev], "median": round(float(np.median(ev)), 3)},
               "cli_seconds": {"what": "scannet_generate_bbox.main on the scene directory: JSON + PLY parsing, upload, kernels, JSON write",
                               "runs": [round(x, 3) for x in cli], "median": round(float(np.median(cli)), 3)},
               "reference_cpu_seconds": args.reference_seconds,
               "note": "recorded, not gated; the reference figure is interpreted Python on one CPU core of the build machine"}
    text = json.dumps(rec, indent=2)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return rec


if __name__ == "__main__":
    main()
