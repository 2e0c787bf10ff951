"""Generate tests/golden/scannet.npz and scannet_excluded_labels.json from the REFERENCE's data/scannet/MinimumBoundingBox.py,
generate_bbox.py and filter_bbox.py (build container only: it reads the reference tree).

The three modules are imported from the read-only tree with stand-ins in sys.modules for what they import and this machine lacks or
does not need: empty ``cv2`` and ``tqdm.contrib.concurrent`` modules, and a ``plyfile`` whose PlyData.read is the project's own
numpy reader.  Only inputs and recorded results are stored; no reference text.

Per case (one instance, float32 vertices v32 [n, 3]) the file holds
  <case>/vertices   the input
  <case>/obb_run    find_minimum_bounding_box(v32) as it runs here -- its z numbers (cz, dz: float32 arithmetic) are the golden ones; its
                    xy numbers are float32-contaminated under numpy 2 (np.float32 / float no longer widens) and are NOT used
  <case>/xy64       MinimumBoundingBox(v32[:, :2].astype(float64)): (area, length_parallel, length_orthogonal, cx, cy, angle) -- the float64
                    computation the reference's pinned numpy 1.x performs
  <case>/margin     (second-smallest edge-rectangle area / smallest) - 1 from tests/scannet_ref.py; below 1e-6 the winning edge is not
                    unique enough to compare numbers (triangles, lattices: exact ties) and only the properties of a minimum rectangle
                    are tested.  At most a third of the cases may be of that kind (asserted here).
The scene is one synthetic scan directory in ScanNet's layout (about 6 000 vertices, 12 instances, two of them sharing a segment):
its four files' bytes, the JSON of the reference's process_scene -- run with MinimumBoundingBox's input widened to float64, for
the same reason -- per-instance xy64 and margin, and the reference's filter_bbox outputs (.npy bytes, JSON text) at two --min_size.

    python tests/golden/make_scannet_golden.py            rewrites both files; the same bytes on every run
    python tests/golden/make_scannet_golden.py --time     times the reference's process_scene on the scene of
                                                          tools/scannet_profile_scene.py (minutes: its 5 000-vertex ring)
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True       # the reference tree is read-only

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_DIR = "/root/reference/data/scannet"
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import scannet_ref as R                                           # noqa: E402
from scannet_profile_scene import profile_scene, write_scene_dir  # noqa: E402
from nerf_rpn_amd.scripts.scannet_generate_bbox import read_ply_vertices  # noqa: E402

MARGIN_MIN = 1e-6
LDS_FREE_NGON = 1200
SCENE = "scene0000_00"
MIN_SIZES = (8, 3)
RESOLUTION = np.array([160, 140, 60], dtype=np.int64)


def reference_modules():
    class _Element:
        def __init__(self, data):
            self.data, self.count = data, len(data)

    class PlyData(dict):
        @staticmethod
        def read(path):
            return PlyData(vertex=_Element(read_ply_vertices(path)))
    sys.modules["cv2"] = types.ModuleType("cv2")
    conc = types.ModuleType("tqdm.contrib.concurrent")
    conc.process_map = None
    sys.modules["tqdm.contrib.concurrent"] = conc
    ply = types.ModuleType("plyfile")
    ply.PlyData, ply.PlyElement = PlyData, _Element
    sys.modules["plyfile"] = ply
    sys.path.insert(0, REF_DIR)
    import MinimumBoundingBox as M
    import generate_bbox as G
    import filter_bbox as F
    return M, G, F


# ----------------------------------------------------------------------------------------------------------------------
# single-instance cases
# ----------------------------------------------------------------------------------------------------------------------
def rot(a):
    return np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])


def with_z(rng, xy, z0=0.3, dz=1.1):
    return np.concatenate([xy, rng.uniform(z0, z0 + dz, (len(xy), 1))], axis=1).astype(np.float32)


def blob(seed, n, shift=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    xy = (rng.normal(0, 1, (n, 2)) * np.array([1.7, 0.45])) @ rot(rng.uniform(0.2, 1.3)).T + np.array([1.5, -2.0]) + np.array(shift)
    return with_z(rng, xy)


def uniform_rect(seed, n):
    rng = np.random.default_rng(seed)
    xy = (rng.uniform(-0.5, 0.5, (n, 2)) * np.array([2.2, 0.9])) @ rot(rng.uniform(0.2, 1.3)).T + np.array([-3.0, 4.0])
    return with_z(rng, xy)


def lattice():
    rng = np.random.default_rng(5)
    gx, gy = np.meshgrid(np.arange(9) * 0.25 + 1.0, np.arange(7) * 0.5 - 2.0, indexing="ij")
    return with_z(rng, np.stack([gx.ravel(), gy.ravel()], axis=1))


def duplicated():
    v = blob(77, 40)
    return np.concatenate([v, v[::2], v[:7], v[:7]])[np.random.default_rng(6).permutation(40 + 20 + 14)]


def collinear_plus_one():
    rng = np.random.default_rng(8)
    t = np.arange(20, dtype=np.float64)
    xy = np.stack([0.5 + 0.125 * t, -1.0 + 0.25 * t], axis=1)          # exactly representable: exactly collinear
    return with_z(rng, np.concatenate([xy, [[2.0, -2.5]]]))


def ellipse_ngon(n=LDS_FREE_NGON):
    rng = np.random.default_rng(17)      # seed picked by the recorded margin (1.6e-6; seeds 9 .. 16 give 1e-7 .. 9e-7)
    t = np.cumsum(rng.uniform(0.5, 1.5, n))
    t = t / t[-1] * 2 * np.pi
    xy = np.stack([3.0 * np.cos(t), 1.2 * np.sin(t)], axis=1) @ rot(0.7).T + np.array([10.0, -6.0])
    return with_z(rng, xy)[rng.permutation(n)]


def cases():
    out = [(f"blob_n{n}", blob(100 + n, n)) for n in (3, 4, 5, 63, 64, 65, 257, 4097)]
    out += [("rect_n300", uniform_rect(1, 300)), ("rect_n3000", uniform_rect(2, 3000))]
    out += [("lattice", lattice()), ("duplicated", duplicated()), ("collinear_plus_one", collinear_plus_one()), ("ellipse_ngon", ellipse_ngon())]
    out += [("blob_n257_shifted", blob(100 + 257, 257, shift=(500.0, -300.0)))]
    return out


def record_case(M, G, v32):
    run = np.asarray(G.find_minimum_bounding_box(v32), dtype=np.float64)
    b = M.MinimumBoundingBox(v32[:, :2].astype(np.float64))
    xy64 = np.array([b.area, b.length_parallel, b.length_orthogonal, b.rectangle_center[0], b.rectangle_center[1], b.unit_vector_angle],
                    dtype=np.float64)
    return dict(vertices=v32, obb_run=run, xy64=xy64, margin=np.array(R.min_rectangle(v32[:, :2].astype(np.float64))["margin"]))


# ----------------------------------------------------------------------------------------------------------------------
# the scene
# ----------------------------------------------------------------------------------------------------------------------
def golden_scene(root):
    """12 instances over 6 000 vertices; instance 11 lists segment 21 of instance 10 as well; segments 90.. belong to nobody."""
    rng = np.random.default_rng(20261018)
    labels = ["chair", "table", "wall", "sofa", "cabinet", "floor", "lamp", "bed", "desk", "mug", "shelf", "bookshelf"]
    parts, seg, groups = [], [], []
    for g, label in enumerate(labels):
        n = int(rng.integers(250, 600))
        size = np.array([0.12, 0.1]) if label == "lamp" else rng.uniform(0.4, 1.6, 2)       # the lamp is below --min_size 8 and 3
        if label == "desk":
            size = np.array([0.9, 0.25])                                                     # between the two --min_size values
        c = np.array([rng.uniform(-3, 3), rng.uniform(-2.5, 2.5)])
        kind = g % 3
        if kind == 0:
            xy = rng.normal(0, 0.3, (n, 2))
        elif kind == 1:
            r, th = 0.5 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
            xy = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
        else:
            xy = rng.uniform(-0.5, 0.5, (n, 2)) * np.array([1.0, 0.8]) + 0.1 * rng.normal(0, 1, (n, 2))
        xy = (xy * size) @ rot(rng.uniform(0.15, 1.4)).T + c
        z = rng.uniform(0.0, 0.4) + rng.uniform(0, 1, (n, 1)) * (0.2 if label == "desk" else rng.uniform(0.5, 1.5))
        parts.append(np.concatenate([xy, z], axis=1))
        a = n // 3
        seg += [2 * g + 1] * a + [2 * g + 2] * (n - a)
        groups.append((g + 1, label, [2 * g + 1, 2 * g + 2]))
    groups[11] = (12, labels[11], groups[11][2] + [21])
    rest = 6000 - sum(len(p) for p in parts)
    parts.append(np.concatenate([rng.uniform(-4, 4, (rest, 2)), rng.uniform(0, 2.5, (rest, 1))], axis=1))
    seg += list(rng.integers(90, 99, rest))
    order = rng.permutation(6000)
    return write_scene_dir(root, SCENE, np.concatenate(parts)[order], np.array(seg)[order], groups, seed=1)


def record_scene(M, G, F, out):
    with tempfile.TemporaryDirectory() as tmp:
        d = golden_scene(os.path.join(tmp, "scans"))
        for fn in sorted(os.listdir(d)):
            with open(os.path.join(d, fn), "rb") as f:
                out[f"scene/file/{fn}"] = np.frombuffer(f.read(), dtype=np.uint8)
        jdir = os.path.join(tmp, "json")
        os.makedirs(jdir)
        mbb = G.MinimumBoundingBox
        G.MinimumBoundingBox = lambda pts: mbb(np.asarray(pts, dtype=np.float64))      # numpy 1.x widened here; numpy 2 does not
        try:
            G.process_scene(d, jdir)
        finally:
            G.MinimumBoundingBox = mbb
        with open(os.path.join(jdir, f"{SCENE}.json")) as f:
            text = f.read()
        out["scene/json"] = np.array(text)
        inst = json.loads(text)["instances"]
        # per-instance float64 rectangle and margin, from the vertices the reference selected
        from nerf_rpn_amd.scripts.scannet_generate_bbox import load_scene
        _, groups, seg, vertices = load_scene(d)
        xy64, margins, counts = [], [], []
        for (_, _, segs), rec in zip(groups, inst):
            v = vertices[np.isin(seg, segs)]
            b = M.MinimumBoundingBox(v[:, :2].astype(np.float64))
            row = [b.area, b.length_parallel, b.length_orthogonal, b.rectangle_center[0], b.rectangle_center[1], b.unit_vector_angle]
            assert np.array_equal(np.array(rec["obb"])[[3, 4, 0, 1, 6]], np.array(row)[[1, 2, 3, 4, 5]]), rec["label"]
            xy64.append(row)
            margins.append(R.min_rectangle(v[:, :2].astype(np.float64))["margin"])
            counts.append(len(v))
        out["scene/xy64"], out["scene/margin"], out["scene/num_vertices"] = np.array(xy64), np.array(margins), np.array(counts, dtype=np.int64)
        assert min(margins) >= MARGIN_MIN, margins
        feat = os.path.join(tmp, "feat.npz")
        np.savez(feat, resolution=RESOLUTION)
        out["scene/resolution"] = RESOLUTION
        out["scene/min_sizes"] = np.array(MIN_SIZES)
        kept = []
        for ms in MIN_SIZES:
            npy, js = os.path.join(tmp, f"f{ms}.npy"), os.path.join(tmp, f"f{ms}.json")
            F.filter_bbox(feat, os.path.join(jdir, f"{SCENE}.json"), npy, js, ms)
            with open(npy, "rb") as f:
                out[f"scene/filter{ms}/npy"] = np.frombuffer(f.read(), dtype=np.uint8)
            with open(js) as f:
                out[f"scene/filter{ms}/json"] = np.array(f.read())
            kept.append(len(np.load(npy)))
        assert 0 < kept[0] < kept[1] < len(inst), kept       # both rules bite, and the two sizes differ


def save_stable(path, arrays):
    """np.savez_compressed with fixed zip timestamps: regenerating gives the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def time_reference(G):
    with tempfile.TemporaryDirectory() as tmp:
        d = profile_scene(os.path.join(tmp, "scans"))
        os.makedirs(os.path.join(tmp, "out"))
        t0 = time.perf_counter()
        G.process_scene(d, os.path.join(tmp, "out"))
        dt = time.perf_counter() - t0
    print(json.dumps({"reference_process_scene_seconds": round(dt, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    M, G, F = reference_modules()
    if args.time:
        return time_reference(G)
    out, names, loose = {}, [], 0
    for name, v32 in cases():
        t0 = time.perf_counter()
        rec = record_case(M, G, v32)
        names.append(name)
        loose += float(rec["margin"]) < MARGIN_MIN
        for k, v in rec.items():
            out[f"{name}/{k}"] = v
        print(f"{name}: n {len(v32)}, margin {float(rec['margin']):.3g}, {time.perf_counter() - t0:.1f} s")
    assert 3 * loose <= len(names), (loose, len(names))
    out["cases"] = np.array(names)
    record_scene(M, G, F, out)
    with open(os.path.join(HERE, "scannet_excluded_labels.json"), "w") as f:
        json.dump(list(F.exlcuded_labels), f, indent=0)
        f.write("\n")
    path = os.path.join(HERE, "scannet.npz")
    save_stable(path, out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB ({loose} of {len(names)} cases under margin {MARGIN_MIN})")


if __name__ == "__main__":
    main()
