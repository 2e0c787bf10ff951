"""Host side of the ScanNet box tools: the float64 checker (tests/scannet_ref.py) against the reference's recorded results
(tests/golden/scannet.npz, from tests/golden/make_scannet_golden.py), the PLY reader, scannet_filter_bbox against the reference's
outputs byte for byte, and the JSON writer.

Tolerance of the checker comparison: 1e-9 * scale, scale = the instance's largest |coordinate| (1 for the angle).  Both sides are
float64 evaluations of the same formula on the same hull; a float64 brute force agreed with the reference to 0.0 relative on blobs,
rectangles, a 6 000-gon and a lattice, so 1e-9 leaves about five orders over float64 rounding and is far below any change of winning
edge at margin >= 1e-6."""
import json
import os

import numpy as np
import pytest

import scannet_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN_MIN = 1e-6


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "scannet.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def scene_dir(g, tmp_path_factory):
    root = tmp_path_factory.mktemp("scans")
    return rebuild_scene(g, str(root))


def rebuild_scene(g, root):
    """The golden scene directory from the file bytes in scannet.npz; returns its path."""
    files = {k.split("/", 2)[2]: v for k, v in g.items() if k.startswith("scene/file/")}
    name = next(f for f in files if f.endswith(".txt"))[:-4]
    d = os.path.join(root, name)
    os.makedirs(d, exist_ok=True)
    for fn, data in files.items():
        with open(os.path.join(d, fn), "wb") as f:
            f.write(data.tobytes())
    return d


def case_names(g):
    return [str(n) for n in g["cases"]]


def test_checker_reproduces_the_reference(g):
    tight = 0
    for name in case_names(g):
        xy = g[f"{name}/vertices"][:, :2].astype(np.float64)
        area, len_p, len_o, cx, cy, angle = g[f"{name}/xy64"]
        m = R.min_rectangle(xy)
        scale = np.abs(xy).max()
        print(f"{name}: area diff {abs(m['area'] - area):.3g}, margin {m['margin']:.3g} (recorded {float(g[f'{name}/margin']):.3g})")
        assert abs(m["area"] - area) <= 1e-9 * area, name
        assert m["margin"] == float(g[f"{name}/margin"])
        if m["margin"] >= MARGIN_MIN:
            tight += 1
            got = np.array([m["length_parallel"], m["length_orthogonal"], m["cx"], m["cy"]])
            assert np.abs(got - np.array([len_p, len_o, cx, cy])).max() <= 1e-9 * scale, name
            assert abs(m["angle"] - angle) <= 1e-9, name
        # the reference's own rectangle contains every point and stands on a hull edge
        assert R.outside_distance(xy, cx, cy, len_p, len_o, angle) <= 1e-9 * scale
        assert R.parallel_error(angle, m["hull"]) <= 1e-9
    assert 3 * (len(case_names(g)) - tight) <= len(case_names(g))


def test_bound_rejects_the_second_best_edge(g):
    """The 1e-9 bound is sharp enough to tell the best edge from the runner-up of a case with margin >= 1e-3."""
    name = next(n for n in case_names(g) if float(g[f"{n}/margin"]) >= 1e-3 and len(g[f"{n}/vertices"]) >= 60)
    xy = g[f"{name}/vertices"][:, :2].astype(np.float64)
    m = R.min_rectangle(xy)
    r, e2 = m["rects"], m["second"]
    scale = np.abs(xy).max()
    golden = g[f"{name}/xy64"]
    wrong = np.array([r["area"][e2], r["length_parallel"][e2], r["length_orthogonal"][e2], r["cx"][e2], r["cy"][e2], r["angle"][e2]])
    assert wrong[0] > golden[0] * (1 + 1e-9)                               # the area property of the GPU test would fail
    assert np.abs(wrong[1:5] - golden[1:5]).max() > 1e-9 * scale or abs(wrong[5] - golden[5]) > 1e-9
    # and a rectangle that is too small is caught by containment
    assert R.outside_distance(xy, golden[3], golden[4], golden[1] * (1 - 1e-6), golden[2], golden[5]) > 1e-9 * scale


def test_hull_drops_duplicates_and_collinear_points(g):
    h = R.hull_ccw(g["lattice/vertices"][:, :2].astype(np.float64))
    assert len(h) == 4 and tuple(h[0]) == (1.0, -2.0)
    h = R.hull_ccw(g["collinear_plus_one/vertices"][:, :2].astype(np.float64))
    assert len(h) == 3
    d = g["duplicated/vertices"][:, :2].astype(np.float64)
    assert np.array_equal(R.hull_ccw(d), R.hull_ccw(np.unique(d, axis=0)))
    e = np.roll(h, -1, axis=0) - h
    assert (e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0] > 0).all()       # counter-clockwise


# ----------------------------------------------------------------------------------------------------------------------
# PLY reader
# ----------------------------------------------------------------------------------------------------------------------
def test_ply_reader_binary_and_ascii(g, scene_dir, tmp_path):
    from nerf_rpn_amd.scripts import scannet_generate_bbox as S
    name = os.path.basename(scene_dir)
    path = os.path.join(scene_dir, f"{name}_vh_clean_2.ply")
    data = S.read_ply_vertices(path)
    assert data.dtype.names == ("x", "y", "z", "red", "green", "blue", "alpha") and len(data) == 6000
    v = S.load_vertices(path)
    assert v.dtype == np.float32 and v.shape == (6000, 3)
    raw = open(path, "rb").read()
    body = raw[raw.index(b"end_header\n") + len(b"end_header\n"):]
    assert np.array_equal(v.reshape(-1), np.frombuffer(body[:6000 * 16], dtype=np.dtype([("p", "<f4", 3), ("c", "u1", 4)]))["p"].reshape(-1))
    # an ASCII rewrite (repr of float32 round-trips) gives the same arrays
    header = raw[:raw.index(b"end_header\n")].decode().replace("binary_little_endian", "ascii")
    with open(tmp_path / "a.ply", "w") as f:
        f.write(header + "end_header\n")
        for row in data:
            f.write(" ".join(repr(float(row[k])) if k in "xyz" else str(int(row[k])) for k in data.dtype.names) + "\n")
        f.write("3 0 1 2\n3 2 3 0\n")
    a = S.read_ply_vertices(str(tmp_path / "a.ply"))
    assert a.dtype == data.dtype and all(np.array_equal(a[k], data[k]) for k in data.dtype.names)
    assert np.array_equal(S.load_vertices(str(tmp_path / "a.ply")), v)


def test_ply_reader_other_property_order(tmp_path):
    from nerf_rpn_amd.scripts import scannet_generate_bbox as S
    rng = np.random.default_rng(3)
    rec = np.zeros(17, dtype=[("nx", "<f4"), ("z", "<f8"), ("quality", "<u2"), ("y", "<f4"), ("x", "<f4"), ("label", "i1")])
    for k in ("nx", "x", "y", "z"):
        rec[k] = rng.normal(0, 3, 17).astype(np.float32)
    rec["quality"], rec["label"] = rng.integers(0, 60000, 17), rng.integers(-100, 100, 17)
    header = ("ply\nformat binary_little_endian 1.0\ncomment made by a test\nobj_info none\nelement vertex 17\nproperty float nx\n"
              "property double z\nproperty ushort quality\nproperty float32 y\nproperty float x\nproperty char label\n"
              "element face 0\nproperty list uchar int vertex_indices\nend_header\n")
    with open(tmp_path / "b.ply", "wb") as f:
        f.write(header.encode() + rec.tobytes())
    v = S.load_vertices(str(tmp_path / "b.ply"))
    assert np.array_equal(v, np.stack([rec["x"], rec["y"], rec["z"].astype(np.float32)], axis=1))
    assert np.array_equal(S.read_ply_vertices(str(tmp_path / "b.ply"))["quality"], rec["quality"])
    with open(tmp_path / "c.ply", "wb") as f:
        f.write(header.replace("binary_little_endian", "binary_big_endian").encode() + rec.tobytes())
    with pytest.raises(ValueError):
        S.read_ply_vertices(str(tmp_path / "c.ply"))


def test_scene_loader_reads_the_reference_layout(g, scene_dir):
    from nerf_rpn_amd.scripts import scannet_generate_bbox as S
    name, instances, seg, vertices = S.load_scene(scene_dir)
    ref = json.loads(str(g["scene/json"]))
    assert name == ref["scene_name"] and seg.dtype == np.int32 and seg.shape == (6000,)
    assert [(i, l) for i, l, _ in instances] == [(x["obj_id"], x["label"]) for x in ref["instances"]]
    counts = [int(np.isin(seg, s).sum()) for _, _, s in instances]
    assert counts == g["scene/num_vertices"].tolist()
    assert set(instances[10][2]) & set(instances[11][2])             # two instances share a segment
    for (_, _, s), x in zip(instances, ref["instances"]):
        v = vertices[np.isin(seg, s)]
        assert v.min(axis=0).tolist() == x["min_pt"] and v.max(axis=0).tolist() == x["max_pt"]


# ----------------------------------------------------------------------------------------------------------------------
# filter_bbox and the JSON writer
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_filter_bbox_equals_the_reference(g, tmp_path, which, capsys):
    from nerf_rpn_amd.scripts import scannet_filter_bbox as F
    ms = int(g["scene/min_sizes"][which])
    ref = json.loads(str(g["scene/json"]))
    name = ref["scene_name"]
    for d in ("feat", "obj"):
        os.makedirs(tmp_path / d)
    np.savez(tmp_path / "feat" / f"{name}.npz", resolution=g["scene/resolution"])
    with open(tmp_path / "obj" / f"{name}.json", "w") as f:
        f.write(str(g["scene/json"]))
    args = ["--feature_dir", str(tmp_path / "feat"), "--obj_json_dir", str(tmp_path / "obj"), "--npy_output_dir", str(tmp_path / "npy"),
            "--json_output_dir", str(tmp_path / "json"), "--min_size", str(ms)]
    F.main(args + ["--excluded_labels", os.path.join(GOLDEN, "scannet_excluded_labels.json")])
    assert open(tmp_path / "npy" / f"{name}.npy", "rb").read() == g[f"scene/filter{ms}/npy"].tobytes()
    assert open(tmp_path / "json" / f"{name}.json").read() == str(g[f"scene/filter{ms}/json"])
    capsys.readouterr()
    # without the label file nothing is excluded by name, and the tool says so
    F.main(args)
    assert "no label is excluded" in capsys.readouterr().out
    kept = [x["label"] for x in json.load(open(tmp_path / "json" / f"{name}.json"))["instances"]]
    with_labels = [x["label"] for x in json.loads(str(g[f"scene/filter{ms}/json"]))["instances"]]
    assert set(with_labels) < set(kept) and {"wall", "floor"} & set(kept) and not {"wall", "floor"} & set(with_labels)


def test_filtered_boxes_load_as_obb_ground_truth(g):
    import io
    boxes = np.load(io.BytesIO(g["scene/filter8/npy"].tobytes()))
    assert boxes.dtype == np.float64 and boxes.ndim == 2 and boxes.shape[1] == 7 and len(boxes)
    res = g["scene/resolution"]
    assert (boxes[:, :3] >= 0).all() and (boxes[:, :3] <= res).all() and (boxes[:, 3:6].min(axis=1) >= 8).all()


def test_json_writer_equals_the_reference_file(g, tmp_path):
    from nerf_rpn_amd.scripts import scannet_generate_bbox as S
    text = str(g["scene/json"])
    ref = json.loads(text)
    inst = [(x["obj_id"], x["label"], []) for x in ref["instances"]]
    min_pt = np.array([x["min_pt"] for x in ref["instances"]]).astype(np.float32)
    max_pt = np.array([x["max_pt"] for x in ref["instances"]]).astype(np.float32)
    obb = np.array([x["obb"] for x in ref["instances"]], dtype=np.float64)
    S.write_scene_json(S.scene_dict(ref["scene_name"], inst, min_pt, max_pt, obb), str(tmp_path / "s.json"))
    got = open(tmp_path / "s.json").read()
    assert got == text
    assert list(json.loads(got)["instances"][0]) == ["obj_id", "label", "min_pt", "max_pt", "obb"] and got.startswith('{\n  "scene_name"')
