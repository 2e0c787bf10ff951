"""Host side of scripts/visualize_rpn_input.py (no GPU): flags, the host-written PLY rows, the row rules the kernels implement (restated
in Python and held to the reference's bytes), the packaged turbo table and the input checks.  Fixture: tests/golden/visualize.npz
(make_visualize_golden.py, from the reference's own functions)."""
import json
import os

import numpy as np
import pytest

from nerf_rpn_amd import ops
from nerf_rpn_amd.scripts import visualize_rpn_input as V

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "visualize.npz"))
CASES = [str(c) for c in G["cases"]]


def _case(name):
    return {k.split("/", 1)[1]: G[k] for k in G.files if k.startswith(name + "/")}


def test_parser_matches_reference_flags():
    ref = json.loads(str(G["cli"]))
    p = V.build_parser()
    assert p.description == ref["description"]
    mine = [dict(options=a.option_strings, dest=a.dest, default=a.default, type=a.type.__name__ if a.type else None,
                 action=type(a).__name__, required=a.required, help=a.help)
            for a in p._actions if a.option_strings and a.dest != "help"]
    assert mine == ref["flags"]
    a = p.parse_args(["-o", "out", "-f", "feat", "-b", "boxes", "-bf", "aabb", "-tr"])
    assert (a.output_dir, a.feature_dir, a.box_dir, a.box_format, a.transpose_yz) == ("out", "feat", "boxes", "aabb", True)
    assert a.objectness_dir is None and a.alpha_threshold == 0.01


def _host_parts(c):
    res = c["resolution"]
    boxes = c["boxes"].copy() if "boxes" in c else None
    k = None if boxes is None else boxes.shape[0]
    head = V.header(int(c["num_points"]), k)
    if boxes is not None:
        head += V.box_vertex_rows(res, boxes, str(c["box_format"]))
    tail = V.edge_rows(k) if boxes is not None else ""
    return head.encode(), tail.encode()


@pytest.mark.parametrize("name", CASES)
def test_host_rows_equal_reference_bytes(name):
    c = _case(name)
    ply = c["ply"].tobytes()
    head, tail = _host_parts(c)
    assert ply.startswith(head)
    assert ply.endswith(tail)
    middle = ply[len(head):len(ply) - len(tail)]
    assert middle.count(b"\n") == int(c["num_points"])


def fixed6(v):
    """'%.6f' of a float by integer arithmetic: the exact binary value times 10^6, rounded half-even (the kernel's rule)."""
    bits = int(np.float64(v).view(np.uint64))
    neg, ex, m = bits >> 63, (bits >> 52) & 0x7FF, bits & ((1 << 52) - 1)
    if ex == 0:
        ex = 1
    else:
        m |= 1 << 52
    e = ex - 1075
    p = m * 1000000
    if e >= 0:
        q = p << e
    else:
        q, rem = p >> -e, p & ((1 << -e) - 1)
        half = 1 << (-e - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
    return ("-" if neg else "") + f"{q // 1000000}.{q % 1000000:06d}"


def test_fixed6_matches_python_format():
    rng = np.random.default_rng(5)
    vals = list(rng.uniform(0, 2, 20000)) + list(rng.uniform(-3, 3, 2000)) + list(10.0 ** rng.uniform(-12, 6, 2000))
    vals += [k / 2 ** 7 for k in range(0, 600)] + [k / 2 ** 8 + 1 for k in range(256)]     # exact ties at the 7th decimal
    vals += [0.0, -0.0, 0.0078125, 0.5e-6, 1.5e-6, 2.5e-6, 1e-7, 5e-324, 1.0, 0.9999995, 0.99999949999999997]
    for v in vals:
        assert fixed6(v) == f"{v:4f}" == f"{np.float64(v):4f}", v
    assert fixed6(0.0078125) == "0.007812"


def _restated_rows(c):
    """The grid rows by the kernel's rules, in numpy."""
    rgbsigma, res, thr = c["rgbsigma"], c["resolution"], float(c["alpha_threshold"])
    pts = np.transpose(rgbsigma, (2, 1, 0, 3)).reshape(-1, 4)
    alpha = np.clip(1.0 - np.exp(-np.exp(pts[:, 3]) / 100.0), 0.0, 1.0)
    keep = alpha > np.float32(thr)
    axes = []
    for n in res:
        n = int(n)
        lv = np.array([0.0 if n == 1 else (float(n) if k == n - 1 else k * (n / (n - 1))) for k in range(n)])
        axes.append(lv / float(res.max()) + 0.5 * (1.0 / float(res.max())))
    iz, iy, ix = np.meshgrid(np.arange(res[2]), np.arange(res[1]), np.arange(res[0]), indexing="ij")
    xyz = np.stack([axes[0][ix.reshape(-1)], axes[1][iy.reshape(-1)], axes[2][iz.reshape(-1)]], axis=1)
    if "score" in c:
        s = c["score"]
        idx = np.where(s * 256 >= 256, 255, np.where(s < 0, 0, np.floor(np.clip(s * 256, 0, 255)))).astype(int)
        rgb = ops.turbo_table()[idx]
        rgb[np.isnan(s)] = 0
    else:
        rgb = (np.clip(pts[:, :3], 0, 1) * 255).astype(np.uint8)
    return "".join(f"{fixed6(p[0])} {fixed6(p[1])} {fixed6(p[2])} {r[0]} {r[1]} {r[2]}\n"
                   for p, r in zip(xyz[keep], rgb[keep])).encode(), int(keep.sum())


@pytest.mark.parametrize("name", CASES)
def test_restated_grid_rows_equal_reference_bytes(name):
    c = _case(name)
    head, tail = _host_parts(c)
    rows, count = _restated_rows(c)
    assert count == int(c["num_points"])
    assert head + rows + tail == c["ply"].tobytes()


def test_linspace_restatement():
    for n in list(range(1, 300)) + [511, 1000]:
        ref = np.linspace(0, n, n)
        mine = np.array([0.0 if n == 1 else (float(n) if k == n - 1 else k * (n / (n - 1))) for k in range(n)])
        assert np.array_equal(ref, mine), n


def test_turbo_table_matches_matplotlib():
    mpl = pytest.importorskip("matplotlib")
    cmap = mpl.colormaps["turbo"]
    t = ops.turbo_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    s = np.linspace(0, 1, 1001)
    assert np.array_equal((cmap(np.arange(256) / 256.0) * 255).astype(np.uint8)[:, :3], t)
    ref = (cmap(np.concatenate([s, [-0.5, 1.5, np.nan]])) * 255).astype(np.uint8)[:, :3]
    idx = np.minimum((s * 256).astype(int), 255)
    assert np.array_equal(ref[:-3], t[idx])
    assert np.array_equal(ref[-3:], np.stack([t[0], t[255], [0, 0, 0]]))


def test_input_checks(tmp_path):
    f = tmp_path / "s.npz"
    np.savez(f, rgbsigma=np.zeros((3, 4, 5, 4), np.float64), resolution=np.array([3, 4, 5]))
    with pytest.raises(ValueError, match="float32"):
        V.load_feature(str(f))
    np.savez(f, rgbsigma=np.zeros((3, 4, 5, 4), np.float32), resolution=np.array([3, 4, 6]))
    with pytest.raises(ValueError, match="resolution"):
        V.load_feature(str(f))
    np.savez(f, rgbsigma=np.zeros((3, 4, 5, 4), np.float32), resolution=np.array([5, 4, 3]))
    res, rgbsigma = V.load_feature(str(f))
    assert res.tolist() == [5, 4, 3] and rgbsigma.shape == (3, 4, 5, 4)
    # objectness: <scene>_objectness.npz first, then <scene>.npz; 3-D levels as they are, 4-D levels with [0]
    lv = [np.full((2 + k, 2, 1), k, np.float32) for k in range(4)]
    np.savez(tmp_path / "s.npz", **{str(k): v for k, v in enumerate(lv)})
    assert V.objectness_path(str(tmp_path), "s") == str(tmp_path / "s.npz")
    assert all(np.array_equal(a, b) for a, b in zip(V.load_levels(V.objectness_path(str(tmp_path), "s")), lv))
    np.savez(tmp_path / "s_objectness.npz", **{str(k): v[None] for k, v in enumerate(lv)})
    assert V.objectness_path(str(tmp_path), "s") == str(tmp_path / "s_objectness.npz")
    assert all(np.array_equal(a, b) for a, b in zip(V.load_levels(V.objectness_path(str(tmp_path), "s")), lv))
    np.savez(tmp_path / "s_objectness.npz", **{str(k): v.astype(np.float64) for k, v in enumerate(lv)})
    with pytest.raises(ValueError, match="float32"):
        V.load_levels(str(tmp_path / "s_objectness.npz"))


def test_edge_rows_layout():
    e = V.edge_rows(1).splitlines()
    assert e[0] == "" and len(e) == 25 and e[1:4] == ["0 1", "4 5", "0 4"]
    assert e[10:13] == ["0 3", "4 7", "3 7"] and e[13] == "8 9" and e[-3:] == ["8 11", "12 15", "11 15"]
