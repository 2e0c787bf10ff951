"""PLY export kernels (csrc/plyexport.hip) on the MI355X: the cubic zoom and the score grid bit-equal to scipy / the reference, whole PLY
files byte-equal to the reference's visualize_scene (tests/golden/visualize.npz, from the reference's own functions), run-to-run
identical bytes, the CLI end to end on voxel-score files written by the RPN, and a full-size 200x200x130 scene."""
import os

import numpy as np
import pytest
import torch

from nerf_rpn_amd import ops
from nerf_rpn_amd.scripts import visualize_rpn_input as V

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visualize.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN, allow_pickle=False))


def _case(g, name):
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(name + "/")}


def _obj_cases(g):
    return [str(n) for n in g["cases"] if str(_case(g, str(n))["objectness"])]


def _layout(root, name, c, reference_names=True):
    """The reference's inputs of one golden case under root: features/, boxes/, objectness/."""
    for d in ("features", "boxes", "objectness", "out"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    np.savez(os.path.join(root, "features", name + ".npz"), rgbsigma=c["rgbsigma"], resolution=c["resolution"])
    if "boxes" in c:
        np.save(os.path.join(root, "boxes", name + ".npy"), c["boxes"])
    if str(c["objectness"]):
        lv = {str(k): c[f"level{k}"] for k in range(4)}
        if reference_names:      # the reference's name and [1, w, l, h] levels
            np.savez(os.path.join(root, "objectness", name + "_objectness.npz"), **{k: v[None] for k, v in lv.items()})
        else:                    # what run_rpn.py / run_fcos.py --output_voxel_scores write
            np.savez(os.path.join(root, "objectness", name + ".npz"), **lv)


def test_zoom_is_bit_equal_to_scipy(g, dev):
    n = 0
    for name in _obj_cases(g):
        c = _case(g, name)
        shape = tuple(int(v) for v in c["shape"])
        for k in range(4):
            lv = c[f"level{k}"]
            assert ops.zoom_output_shape(lv.shape, shape) == shape
            out = ops.zoom_cubic3d(torch.from_numpy(lv).to(dev), shape).cpu().numpy()
            assert out.dtype == np.float32 and np.array_equal(out, c[f"zoom{k}"]), (name, k, np.abs(out - c[f"zoom{k}"]).max())
            n += 1
    assert n == 8


def test_score_grid_equals_reference(g, dev):
    for name in _obj_cases(g):
        c = _case(g, name)
        levels = [torch.from_numpy(c[f"level{k}"]).to(dev) for k in range(4)]
        score = ops.objectness_grid(levels, c["resolution"]).cpu().numpy()
        assert score.dtype == np.float64 and np.array_equal(score, c["score"]), (name, np.abs(score - c["score"]).max())


@pytest.mark.parametrize("name", ["rgb_obb", "rgb_aabb", "rgb_nobox", "obj_rpn", "obj_fcos", "empty"])
def test_ply_is_byte_equal_to_reference(g, name, tmp_path, dev):
    c = _case(g, name)
    _layout(str(tmp_path), name, c)
    kw = dict(box_dir=str(tmp_path / "boxes") if "boxes" in c else None, box_format=str(c["box_format"]) or "obb",
              objectness_dir=str(tmp_path / "objectness") if str(c["objectness"]) else None, alpha_threshold=float(c["alpha_threshold"]))
    path = V.visualize_scene(name, str(tmp_path / "out"), str(tmp_path / "features"), device=dev, **kw)
    got = open(path, "rb").read()
    ref = c["ply"].tobytes()
    if got != ref:
        i = next(k for k in range(min(len(got), len(ref))) if got[k] != ref[k]) if got[:len(ref)] != ref[:len(got)] else min(len(got), len(ref))
        pytest.fail(f"{name}: first difference at byte {i} of {len(ref)} (got {len(got)}): {got[max(0, i - 60):i + 60]!r} vs "
                    f"{ref[max(0, i - 60):i + 60]!r}")


def test_two_runs_give_identical_bytes(g, dev):
    c = _case(g, "obj_rpn")
    levels = [torch.from_numpy(c[f"level{k}"]).to(dev) for k in range(4)]
    rs = torch.from_numpy(c["rgbsigma"]).to(dev)
    outs = []
    for _ in range(2):
        s = ops.objectness_grid(levels, c["resolution"])
        outs.append((s.cpu().numpy().tobytes(), ops.ply_points(rs, c["resolution"], float(c["alpha_threshold"]), s)[1].cpu().numpy().tobytes()))
    assert outs[0] == outs[1]


def test_resolution_order_and_argument_checks(g, dev):
    c = _case(g, "rgb_nobox")
    rs = torch.from_numpy(c["rgbsigma"]).to(dev)
    # coordinates follow the resolution and the colours the grid's own axes (the reference's construct_grid vs transpose)
    res = c["resolution"][[1, 2, 0]]
    count, rows = ops.ply_points(rs, res, float(c["alpha_threshold"]))
    lines = rows.cpu().numpy().tobytes().decode().splitlines()
    ref = c["ply"].tobytes().decode().split("end_header\n\n", 1)[1].splitlines()
    assert count == len(lines) == len(ref) == int(c["num_points"])
    assert [l.split()[3:] for l in lines] == [l.split()[3:] for l in ref]
    pts = np.transpose(c["rgbsigma"], (2, 1, 0, 3)).reshape(-1, 4)
    keep = np.flatnonzero(np.clip(1.0 - np.exp(-np.exp(pts[:, 3]) / 100.0), 0.0, 1.0) > np.float32(c["alpha_threshold"]))
    ix, iy, iz = keep % res[0], keep // res[0] % res[1], keep // (res[0] * res[1])
    first = [float(v) for v in lines[0].split()[:3]]
    m = res.max()
    want = [np.linspace(0, n, n)[i] / m + 0.5 * (1.0 / m) for n, i in zip(res, (ix[0], iy[0], iz[0]))]
    assert np.allclose(first, want, atol=1e-6)
    with pytest.raises(ops.lib.NrpnError):
        ops.ply_points(rs, (1, 2, 3), 0.01)
    with pytest.raises(ops.lib.NrpnError):
        ops.objectness_grid([], (10, 10, 10))
    with pytest.raises(ops.lib.NrpnError):
        ops.objectness_grid([torch.zeros(3, 3, 3, dtype=torch.float64, device=dev)], (10, 10, 10))


def test_cli_end_to_end_on_rpn_voxel_scores(g, tmp_path, dev):
    """A golden case with the voxel-score naming of this repository's writers (3-D levels, <scene>.npz) and a scene whose voxel scores
    come from the RPN's objectness_output_paths (run_rpn.py --output_voxel_scores), all through main()."""
    from test_gpu_e2e import build, scene
    root = str(tmp_path)
    c = _case(g, "obj_rpn")
    _layout(root, "obj_rpn", c, reference_names=False)
    shape = (48, 40, 32)
    x = scene(shape, 9)
    m = build(True, 160, dev).eval()
    with torch.no_grad():
        m([x.to(dev)], objectness_output_paths=[os.path.join(root, "objectness", "rpn_scene.npz")])
    rgbsigma = np.ascontiguousarray(x.permute(1, 2, 3, 0).numpy()).astype(np.float32)
    rgbsigma[..., 3] = rgbsigma[..., 3] * 4 - 1
    np.savez(os.path.join(root, "features", "rpn_scene.npz"), rgbsigma=rgbsigma, resolution=np.array(shape))
    boxes = np.array([[10, 12, 8, 8, 6, 5, 0.3], [30, 20, 16, 12, 10, 8, -0.5]], np.float32)
    np.save(os.path.join(root, "boxes", "rpn_scene.npy"), boxes)
    np.save(os.path.join(root, "boxes", "obj_rpn.npy"), c["boxes"])
    written = V.main(["-o", root + "/out", "-f", root + "/features", "-b", root + "/boxes", "--objectness_dir", root + "/objectness", "-tr"])
    assert sorted(os.path.basename(p) for p in written) == ["obj_rpn.ply", "rpn_scene.ply"]
    assert open(os.path.join(root, "out", "obj_rpn.ply"), "rb").read() == c["ply"].tobytes()
    text = open(os.path.join(root, "out", "rpn_scene.ply")).read()
    head, body = text.split("end_header\n\n")
    nv = int(head.split("element vertex ")[1].split()[0])
    rows, edges = body.split("\n\n")
    rows = rows.splitlines()
    pts = np.transpose(rgbsigma, (2, 1, 0, 3)).reshape(-1, 4)
    kept = int((np.clip(1.0 - np.exp(-np.exp(pts[:, 3]) / 100.0), 0.0, 1.0) > np.float32(0.01)).sum())
    assert nv == len(rows) == 24 + kept and len(edges.splitlines()) == 36
    turbo = {tuple(int(v) for v in t) for t in ops.turbo_table()} | {(0, 0, 0)}
    assert all(tuple(int(v) for v in r.split()[3:]) in turbo for r in rows[24:])
    z = np.load(os.path.join(root, "objectness", "rpn_scene.npz"))
    score = ops.objectness_grid([torch.from_numpy(z[str(k)]).to(dev) for k in range(4)], shape).cpu().numpy()
    assert score.max() == 1.0


def test_full_size_scene_with_four_levels(dev):
    shape = (200, 200, 130)
    rng = np.random.default_rng(11)
    lshapes = [tuple(int(v) for v in np.ceil(np.array(shape) / 2 ** (k + 2))) for k in range(4)]
    levels = [rng.normal(-3, 2, s).astype(np.float32) for s in lshapes]
    dl = [torch.from_numpy(v).to(dev) for v in levels]
    score = ops.objectness_grid(dl, shape)
    rgbsigma = rng.uniform(-2, 1, shape + (4,)).astype(np.float32)
    count, rows = ops.ply_points(torch.from_numpy(rgbsigma).to(dev), shape, 0.01, score)
    pts = rgbsigma.reshape(-1, 4)[:, 3]
    assert count == int((np.clip(1.0 - np.exp(-np.exp(pts) / 100.0), 0.0, 1.0) > np.float32(0.01)).sum())
    b = rows.cpu().numpy().tobytes()
    assert b.count(b"\n") == count and b.endswith(b"\n")
    s = score.cpu().numpy()
    assert np.nanmax(s) == 1.0 and s.shape == (200 * 200 * 130,)
    try:
        import scipy.ndimage
    except ImportError:
        return
    acc = np.zeros(shape)
    for k, lv in enumerate(levels):
        ref = scipy.ndimage.zoom(lv, np.array(shape) / np.array(lv.shape), order=3)
        got = ops.zoom_cubic3d(dl[k], shape).cpu().numpy()
        assert np.array_equal(got, ref), (k, np.abs(got - ref).max())
        acc += ref
    acc = np.transpose(acc, (2, 1, 0)).reshape(-1)
    acc /= acc.max()
    assert np.array_equal(s, acc)
