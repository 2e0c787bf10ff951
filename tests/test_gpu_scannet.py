"""ScanNet box kernels (csrc/scanbox.hip) on the MI355X, through ops.scannet_instance_boxes and the two command-line tools.

Golden numbers are the reference's (tests/golden/scannet.npz: find_minimum_bounding_box for z, MinimumBoundingBox on the float64-widened
xy for the rectangle); tests/scannet_ref.py is the float64 checker for everything else.  For every instance, ties included:
  (a) min_pt / max_pt bit-equal to numpy, cz / dz bit-equal to the reference's float32 arithmetic, num_vertices exact, the returned
      area <= the checker's minimum * (1 + 1e-9), every vertex inside the returned rectangle within 1e-9 * scale, one side parallel
      to a hull edge within 1e-9 rad;
and where the margin between the best and the second-best edge is >= 1e-6 (the winner is then the same edge on both sides):
  (b) all seven obb numbers within 1e-9 * scale of the reference (1e-9 rad for the angle; both traverse the hull counter-clockwise).
scale = the instance's largest |x| or |y|.  Float64 evaluations of the same formula on the same hull differ by rounding only (1e-16
relative per operation, amplified by at most the ratio scale / extent, ~1e-13 here), so 1e-9 leaves several orders of room and is
still far below the change a different winning edge makes at margin >= 1e-6."""
import io
import json
import os

import numpy as np
import pytest
import torch

import scannet_ref as R
from nerf_rpn_amd import lib, ops
from nerf_rpn_amd.scripts import scannet_filter_bbox as F
from nerf_rpn_amd.scripts import scannet_generate_bbox as S
from test_scannet_host import GOLDEN, MARGIN_MIN, case_names, rebuild_scene

pytestmark = pytest.mark.gpu

NUM_INSTANCES = 70          # more instances than one wave has lanes


@pytest.fixture(scope="module")
def g():
    return dict(np.load(os.path.join(GOLDEN, "scannet.npz"), allow_pickle=False))


def circle(n, seed):
    rng = np.random.default_rng(seed)
    t = (np.arange(n) + rng.uniform(-0.1, 0.1, n)) * (2 * np.pi / n)
    xy = np.stack([1.0 + 2.0 * np.cos(t), 1.0 + 1.9 * np.sin(t)], axis=1)
    return np.concatenate([xy, rng.uniform(0, 1, (n, 1))], axis=1).astype(np.float32)


def small_blob(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(6, 120))
    a = rng.uniform(0, np.pi)
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    xy = (rng.normal(0, 1, (n, 2)) * rng.uniform(0.1, 2.0, 2)) @ rot.T + rng.uniform(-20, 20, 2)
    return np.concatenate([xy, rng.uniform(-1, 3, (n, 1))], axis=1).astype(np.float32)


def run(dev, vertices, seg, instance_segments):
    out = ops.scannet_instance_boxes(torch.from_numpy(vertices).to(dev), torch.from_numpy(seg).to(dev), instance_segments)
    return tuple(t.cpu().numpy() for t in out)


@pytest.fixture(scope="module")
def batch(g, dev):
    """One call with every family: instance name -> (vertices or None, expected status); the golden cases first."""
    cap = lib.query("scanbox_lds_points")
    clouds = [(n, g[f"{n}/vertices"]) for n in case_names(g)]
    clouds += [("circle_at_capacity", circle(cap, 1)), ("circle_over_capacity", circle(cap + 1, 2))]
    line = np.stack([np.arange(9) * 0.5, 2.0 - np.arange(9) * 0.25, np.linspace(0, 1, 9)], axis=1).astype(np.float32)
    clouds += [("two_vertices", small_blob(900)[:2]), ("collinear", line), ("coincident", np.repeat(small_blob(901)[:1], 5, axis=0))]
    k = 0
    while len(clouds) < NUM_INSTANCES - 2:        # - 2: the empty instance and the one that shares segments
        clouds.append((f"pad{k}", small_blob(1000 + k)))
        k += 1
    parts, seg, names, segments, expect = [], [], [], [], {}
    for i, (name, v) in enumerate(clouds):
        half = len(v) // 2
        parts.append(v)
        seg += [10 + 2 * i] * half + [11 + 2 * i] * (len(v) - half)
        names.append(name)
        segments.append([10 + 2 * i, 11 + 2 * i])
        expect[name] = v
    ia, ib = names.index("blob_n63"), names.index("pad0")
    names += ["shared", "empty"]
    segments += [[11 + 2 * ia, 10 + 2 * ib, 11 + 2 * ib], [5, 7]]       # half of one cloud and all of another; segments no vertex has
    expect["shared"] = np.concatenate([clouds[ia][1][len(clouds[ia][1]) // 2:], clouds[ib][1]])
    expect["empty"] = np.zeros((0, 3), np.float32)
    vertices, seg = np.concatenate(parts), np.array(seg, dtype=np.int32)
    extra = small_blob(5)                                                 # vertices of segments that belong to nobody
    vertices, seg = np.concatenate([vertices, extra]), np.concatenate([seg, np.full(len(extra), 3, np.int32)])
    order = np.random.default_rng(0).permutation(len(vertices))
    vertices, seg = np.ascontiguousarray(vertices[order]), np.ascontiguousarray(seg[order])
    assert len(names) == NUM_INSTANCES
    out = run(dev, vertices, seg, segments)
    return dict(names=names, expect=expect, vertices=vertices, seg=seg, segments=segments, out=out)


STATUS = {"two_vertices": 1, "empty": 1, "collinear": 2, "coincident": 2}


def check_a(name, v, min_pt, max_pt, obb, count, zref=None):
    """The properties that hold for every non-degenerate instance; returns (checker result, scale)."""
    assert count == len(v), name
    assert min_pt.tobytes() == v.min(axis=0).tobytes() and max_pt.tobytes() == v.max(axis=0).tobytes(), name
    mn, mx = v[:, 2].min(), v[:, 2].max()
    cz, dz = (np.float64((mn + mx) / np.float32(2)), np.float64(mx - mn)) if zref is None else zref
    assert obb[2] == cz and obb[5] == dz, (name, obb[2], cz, obb[5], dz)
    xy = v[:, :2].astype(np.float64)
    m = R.min_rectangle(xy)
    scale = np.abs(xy).max()
    area = obb[3] * obb[4]
    out = R.outside_distance(xy, obb[0], obb[1], obb[3], obb[4], obb[6])
    par = R.parallel_error(obb[6], m["hull"])
    print(f"{name}: n {len(v)}, hull {len(m['hull'])}, margin {m['margin']:.3g}, area / min - 1 = {area / m['area'] - 1:.3g}, "
          f"outside {out / scale:.3g} * scale, parallel {par:.3g} rad")
    assert area <= m["area"] * (1 + 1e-9), name
    assert out <= 1e-9 * scale, name
    assert par <= 1e-9, name
    return m, scale


def check_b(name, obb, want, scale):
    d = np.abs(obb - want)
    print(f"{name}: |obb - reference| / scale = {(d[:6] / scale).max():.3g}, angle {d[6]:.3g}")
    assert (d[:6] <= 1e-9 * scale).all() and d[6] <= 1e-9, (name, obb, want)


def golden_obb(g, name):
    _, len_p, len_o, cx, cy, angle = g[f"{name}/xy64"]
    run_ = g[f"{name}/obb_run"]
    return np.array([cx, cy, run_[2], len_p, len_o, run_[5], angle])


def test_golden_cases(g, batch):
    min_pt, max_pt, obb, status, count = batch["out"]
    loose = 0
    for name in case_names(g):
        i = batch["names"].index(name)
        assert status[i] == 0, name
        want = golden_obb(g, name)
        m, scale = check_a(name, g[f"{name}/vertices"], min_pt[i], max_pt[i], obb[i], count[i], zref=(want[2], want[5]))
        if float(g[f"{name}/margin"]) >= MARGIN_MIN:
            check_b(name, obb[i], want, scale)
        else:
            loose += 1
    assert 3 * loose <= len(case_names(g))


def test_every_other_instance_against_the_checker(g, batch):
    """Circles at and one past the LDS capacity (the second sorts and chains in global memory), the instance that shares segments,
    the padding blobs: properties (a), and the checker's own winner where the margin allows."""
    min_pt, max_pt, obb, status, count = batch["out"]
    cap = lib.query("scanbox_lds_points")
    assert len(batch["expect"]["circle_over_capacity"]) == cap + 1
    seen = 0
    for i, name in enumerate(batch["names"]):
        if name in STATUS or name in case_names(g):
            continue
        assert status[i] == 0, name
        v = batch["expect"][name]
        m, scale = check_a(name, v, min_pt[i], max_pt[i], obb[i], count[i])
        if name.startswith("circle"):
            assert len(m["hull"]) == len(v)                   # nothing is discarded, every point is a hull vertex
        if m["margin"] >= MARGIN_MIN:
            check_b(name, obb[i], np.array([m["cx"], m["cy"], obb[i][2], m["length_parallel"], m["length_orthogonal"], obb[i][5], m["angle"]]), scale)
        seen += 1
    assert seen == NUM_INSTANCES - len(case_names(g)) - len(STATUS)


def test_degenerate_instances_are_flagged_and_isolated(batch):
    min_pt, max_pt, obb, status, count = batch["out"]
    for name, want in STATUS.items():
        i = batch["names"].index(name)
        v = batch["expect"][name]
        assert status[i] == want and count[i] == len(v), (name, status[i], count[i])
        assert np.isnan(obb[i]).all(), name
        if len(v):
            assert min_pt[i].tobytes() == v.min(axis=0).tobytes() and max_pt[i].tobytes() == v.max(axis=0).tobytes()
        else:
            assert np.isposinf(min_pt[i]).all() and np.isneginf(max_pt[i]).all()
    assert (status[[n not in STATUS for n in batch["names"]]] == 0).all()


def test_single_instance_call(g, dev):
    v = g["blob_n65/vertices"]
    min_pt, max_pt, obb, status, count = run(dev, v, np.full(len(v), 4, np.int32), [[4]])
    assert status.tolist() == [0] and obb.shape == (1, 7) and obb.dtype == np.float64 and count.dtype == np.int64
    want = golden_obb(g, "blob_n65")
    _, scale = check_a("blob_n65", v, min_pt[0], max_pt[0], obb[0], count[0], zref=(want[2], want[5]))
    check_b("blob_n65", obb[0], want, scale)


def test_translated_blob_follows_the_translation(g, batch):
    """The blob moved by (+500, -300): its golden is the reference on the moved float32 input; against the unmoved blob's box the
    difference is the float32 rounding of the moved coordinates (2^-24 * 500 = 3e-5 per coordinate)."""
    obb = batch["out"][2]
    a, b = obb[batch["names"].index("blob_n257")], obb[batch["names"].index("blob_n257_shifted")]
    scale = np.abs(g["blob_n257_shifted/vertices"][:, :2]).max()
    check_b("blob_n257_shifted", b, golden_obb(g, "blob_n257_shifted"), scale)
    assert np.abs(b[[0, 1]] - a[[0, 1]] - np.array([500.0, -300.0])).max() <= 1e-3 and np.abs(b[[3, 4]] - a[[3, 4]]).max() <= 1e-3


def test_runs_and_vertex_orders_give_identical_bits(batch, dev):
    again = run(dev, batch["vertices"], batch["seg"], batch["segments"])
    perm = np.random.default_rng(42).permutation(len(batch["vertices"]))
    permuted = run(dev, np.ascontiguousarray(batch["vertices"][perm]), np.ascontiguousarray(batch["seg"][perm]), batch["segments"])
    for k, (a, b, c) in enumerate(zip(batch["out"], again, permuted)):
        assert a.tobytes() == b.tobytes(), f"output {k} differs between two runs"
        assert a.tobytes() == c.tobytes(), f"output {k} differs after permuting the vertices"


def test_argument_checks(dev):
    v = torch.zeros(8, 3)
    s = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(lib.NrpnError):
        ops.scannet_instance_boxes(v, s, [[0]])                                  # CPU tensors
    with pytest.raises(lib.NrpnError):
        ops.scannet_instance_boxes(v.to(dev).double(), s.to(dev), [[0]])
    with pytest.raises(lib.NrpnError):
        ops.scannet_instance_boxes(v.to(dev), s.to(dev).long(), [[0]])
    with pytest.raises(lib.NrpnError):
        ops.scannet_instance_boxes(v.to(dev), s.to(dev), [])
    assert lib.query("scanbox_work_bytes", 1 << 24, 4096, 1 << 24) > 0 and lib.query("scanbox_work_bytes", -1, 1, 0) == -1


def test_cli_scene_and_filter(g, tmp_path, dev, capsys):
    scans = tmp_path / "scans"
    rebuild_scene(g, str(scans))
    written = S.main(["--scene_path", str(scans), "--output_path", str(tmp_path / "json")])
    ref = json.loads(str(g["scene/json"]))
    name = ref["scene_name"]
    assert [os.path.basename(p) for p in written] == [f"{name}.json"]
    text = open(written[0]).read()
    got = json.loads(text)
    assert list(got) == list(ref) and got["scene_name"] == name and len(got["instances"]) == len(ref["instances"]) == 12
    assert text.startswith('{\n  "scene_name"')
    _, instances, seg, vertices = S.load_scene(str(scans / name))
    for k, (a, b) in enumerate(zip(got["instances"], ref["instances"])):
        assert list(a) == list(b)
        assert (a["obj_id"], a["label"], a["min_pt"], a["max_pt"]) == (b["obj_id"], b["label"], b["min_pt"], b["max_pt"])
        v = vertices[np.isin(seg, instances[k][2])]
        obb, want = np.array(a["obb"]), np.array(b["obb"])
        _, scale = check_a(a["label"], v, np.array(a["min_pt"], np.float32), np.array(a["max_pt"], np.float32), obb,
                           int(g["scene/num_vertices"][k]), zref=(want[2], want[5]))
        assert float(g["scene/margin"][k]) >= MARGIN_MIN
        check_b(a["label"], obb, want, scale)
    # our JSON through the filter: the reference's kept set and boxes
    os.makedirs(tmp_path / "feat")
    np.savez(tmp_path / "feat" / f"{name}.npz", resolution=g["scene/resolution"])
    for ms in (int(x) for x in g["scene/min_sizes"]):
        F.main(["--feature_dir", str(tmp_path / "feat"), "--obj_json_dir", str(tmp_path / "json"), "--npy_output_dir", str(tmp_path / f"npy{ms}"),
                "--json_output_dir", str(tmp_path / f"fjson{ms}"), "--min_size", str(ms),
                "--excluded_labels", os.path.join(GOLDEN, "scannet_excluded_labels.json")])
        boxes, want = np.load(tmp_path / f"npy{ms}" / f"{name}.npy"), np.load(io.BytesIO(g[f"scene/filter{ms}/npy"].tobytes()))
        kept = [x["obj_id"] for x in json.load(open(tmp_path / f"fjson{ms}" / f"{name}.json"))["instances"]]
        assert kept == [x["obj_id"] for x in json.loads(str(g[f"scene/filter{ms}/json"]))["instances"]]
        assert boxes.shape == want.shape and boxes.dtype == np.float64
        scale = np.abs(want[:, :6]).max()
        d = np.abs(boxes - want)
        print(f"filter --min_size {ms}: {len(boxes)} boxes, |box - reference| / scale {(d[:, :6] / scale).max():.3g}, angle {d[:, 6].max():.3g}")
        assert (d[:, :6] <= 1e-9 * scale).all() and (d[:, 6] <= 1e-9).all()
    # what datasets.py reads as OBB ground truth
    assert np.load(tmp_path / "npy8" / f"{name}.npy").shape[1] == 7


def test_cli_refuses_a_scene_with_a_degenerate_instance(g, tmp_path, dev):
    scans = tmp_path / "scans"
    d = rebuild_scene(g, str(scans))
    name = os.path.basename(d)
    path = os.path.join(d, f"{name}_vh_clean.aggregation.json")
    agg = json.load(open(path))
    agg["segGroups"].append({"id": 99, "objectId": 77, "segments": [123456], "label": "ghost"})
    json.dump(agg, open(path, "w"))
    with pytest.raises(SystemExit) as e:
        S.main(["--scene_path", str(scans), "--output_path", str(tmp_path / "json")])
    msg = str(e.value.code)
    assert e.value.code not in (0, None) and name in msg and "77" in msg and "ghost" in msg
    assert os.listdir(tmp_path / "json") == []
