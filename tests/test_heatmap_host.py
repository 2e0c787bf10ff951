"""scripts/render_heatmap.py, host side: box preparation, gkern factor tables, cameras, CLI flags and the jet table against what the
reference computes (tests/golden/heatmap.npz, tests/golden/make_heatmap_golden.py), and the C layer's argument checks (no GPU needed)."""
import json
import os

import numpy as np
import pytest

from nerf_rpn_amd import lib, ops
from nerf_rpn_amd.scripts import render_heatmap as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heatmap.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN, allow_pickle=False))


def _case(g, name):
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(name + "/")}


def test_aabbs_factor_tables_and_cameras_equal_the_reference(g):
    for name in g["cases"]:
        c = _case(g, str(name))
        res = [int(v) for v in c["res"]]
        aabbs = R.clip_aabbs(c["proposals"], res)
        assert np.array_equal(aabbs, c["aabbs"]), name
        assert np.array_equal(R.clamp_to_array(aabbs, tuple(c["shape"])), aabbs), name     # the reference succeeded: nothing to clamp
        frames = json.loads(str(c["frames"]))
        for d in (1, 2):
            _, pos, foc, _ = R.frame2config(frames, c["room_bbox"].flatten(), res, d)
            assert np.array_equal(pos, c[f"cam_pos_d{d}"]) and np.array_equal(foc, c[f"cam_focal_d{d}"]), (name, d)
    # the 3-D gkern_3d kernel is the outer product (gx[i] * gy[j]) * gz[k] of the host's factor tables, bit for bit
    at = 0
    for w, l, h in g["kernel_shapes"]:
        f, off = ops.heatmap_factor_tables(np.array([[0, 0, 0, w, l, h]]))
        assert off.tolist() == [0] and f.size == w + l + h
        k = (f[:w][:, None, None] * f[w:w + l][None, :, None]) * f[w + l:][None, None, :]
        assert np.array_equal(k.reshape(-1), g["kernels"][at:at + w * l * h]), (w, l, h)
        at += w * l * h
    assert at == g["kernels"].size


def test_aabb_proposals_and_gt_boxes_are_clamped_to_the_array():
    shape, res = (10, 8, 6), [10, 8, 6]
    room = np.array([0., 0, 0, 2, 2, 2])
    aabb, _ = R.scene_boxes(np.array([[1.7, 2.2, -3.0, 4.9, 9.5, 3.1]]), res, shape, room)
    assert aabb.tolist() == [[1, 2, 0, 4, 7, 3]]
    gt = np.array([[-2.0, 3.0, 2.0, 6.0, 30.0, 2.0, 0.0]])
    aabb, corners = R.scene_boxes(np.zeros((0, 7)), res, shape, room, gt=gt)
    assert aabb.tolist() == [[0, 0, 1, 1, 8, 3]] and corners.shape == (1, 8, 3)


def test_cli_flags_match_the_reference(g):
    ref = json.loads(str(g["cli_flags"]))
    ours = [dict(options=a.option_strings, dest=a.dest, default=a.default, choices=list(a.choices) if a.choices else None,
                 type=a.type.__name__ if a.type else None, action=type(a).__name__)
            for a in R.build_parser()._actions if a.option_strings and a.dest != "help"]
    by_dest = {f["dest"]: f for f in ours}
    for f in ref:
        assert by_dest.get(f["dest"]) == f, f
    extra = sorted(set(by_dest) - {f["dest"] for f in ref})
    assert extra == ["height", "width"] and by_dest["width"]["default"] == 640 and by_dest["height"]["default"] == 480


def test_gaussian_weights_are_scipys():
    nd = pytest.importorskip("scipy.ndimage")
    from scipy.ndimage import _filters
    for s in (5.0, 2.0, 0.7, 3.3):
        r, w = ops.gaussian_weights(s)
        assert r == int(4.0 * s + 0.5) and np.array_equal(w, _filters._gaussian_kernel1d(s, 0, r))
    assert nd is not None


def test_jet_table_matches_matplotlib():
    cm = pytest.importorskip("matplotlib.cm")
    ref = np.asarray(cm.jet(np.arange(256)))[:, :3]
    assert np.abs(ops.jet_table() - ref).max() <= 1e-7


def test_interactive_exits_with_a_message(tmp_path):
    with pytest.raises(SystemExit, match="--interactive is not supported"):
        R.main(["--interactive", "--proposal_dir", str(tmp_path)])


def test_missing_room_bbox_names_the_file(tmp_path):
    for d in ("feat", "props", "ds/s0/train", "ds/s0/val"):
        os.makedirs(tmp_path / d)
    np.savez(tmp_path / "feat" / "s0.npz", rgbsigma=np.zeros((4, 4, 4, 4), np.float32), resolution=np.array([4, 4, 4]))
    np.savez(tmp_path / "props" / "s0.npz", proposals=np.zeros((1, 7), np.float32))
    train = tmp_path / "ds" / "s0" / "train" / "transforms.json"
    train.write_text(json.dumps({"frames": []}))
    (tmp_path / "ds" / "s0" / "val" / "val_transforms.json").write_text(json.dumps({"frames": []}))
    with pytest.raises(SystemExit, match="no room_bbox in " + str(train)):
        R.main(["--dataset_dir", str(tmp_path / "ds"), "--feature_dir", str(tmp_path / "feat"), "--proposal_dir", str(tmp_path / "props"),
                "--output_dir", str(tmp_path / "out")])


def test_argument_errors_are_reported_not_fatal():
    if not os.path.exists(lib.SO_PATH):
        lib.build()
    cases = [
        ("heatmap_splat", (0, 1, 0, 0, 0, 0, 4, 4, 0, 0), "bad dims"),
        ("heatmap_splat", (0, -1, 0, 0, 0, 4, 4, 4, 0, 0), "K < 0"),
        ("heatmap_splat", (0, 0, 0, 0, 7, 4, 4, 4, 0, 0), "kernel_type"),
        ("gaussian_filter3d", (0, 4, -4, 4, 1.0, 4, 0, 0, 0, 0), "bad dims"),
        ("gaussian_filter3d", (0, 4, 4, 4, -1.0, 0, 0, 0, 0, 0), "bad sigma"),
        ("gaussian_filter3d", (0, 4, 4, 4, float("nan"), 0, 0, 0, 0, 0), "bad sigma"),
        ("heatmap_standardize", (0, 0, 0, 0, 0, 0), "element count"),
        ("render_mip", (0, 4, 4, 4, 0, 1.0, 0, 1, 0, 64, 48, 0, 0, 0, 0), "d < 1"),
        ("render_mip", (0, 4, 4, 4, 2, 1.0, 0, 1, 0, 0, 48, 0, 0, 0, 0), "image size"),
        ("render_mip", (0, 4, 0, 4, 2, 1.0, 0, 1, 0, 64, 48, 0, 0, 0, 0), "bad dims"),
    ]
    for name, args, msg in cases:
        with pytest.raises(lib.NrpnError, match=msg):
            lib.call(name, *args)
    assert lib.query("heatmap_work_doubles") > 0
