"""Generate tests/golden/visualize.npz from the REFERENCE's visualize_rpn_input.py (build container only: it reads the reference tree).

The reference script imports tqdm's process_map at module level and runs its pool under ``__main__``, so the functions this fixture
needs are taken out of its source with ``ast`` and executed with numpy, os, matplotlib's cm and scipy's zoom in their namespace.  The
zoom and get_objectness_grid are wrapped to record their inputs and outputs; visualize_scene writes each case's PLY file into a
temporary directory.  Only the recorded arrays and the PLY bytes are stored.

    python tests/golden/make_visualize_golden.py            (rewrites visualize.npz; the same bytes on every run)
"""
import os

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")      # as tests/conftest.py: the OBB corners go through a small matmul

import argparse       # noqa: E402
import ast            # noqa: E402
import io             # noqa: E402
import json           # noqa: E402
import tempfile       # noqa: E402
import zipfile        # noqa: E402

import matplotlib     # noqa: E402
import matplotlib.cm  # noqa: E402
import numpy as np    # noqa: E402
import scipy.ndimage  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SCRIPT = "/root/reference/nerf_rpn/scripts/visualize_rpn_input.py"
FUNCS = ("density_to_alpha", "construct_grid", "write_box_vertex_to_ply", "get_obb_corners", "write_obb_vertex_to_ply",
         "write_box_edge_to_ply", "write_objectness_heatmap_to_ply", "write_rgb_to_ply", "get_objectness_grid", "visualize_scene",
         "parse_args")
ULP_MARGIN = 8        # no voxel's float32 alpha within this many ulp of the threshold: device expf cannot flip a keep decision


class _Recorder:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *a, **kw):
        y = self.fn(*a, **kw)
        self.calls.append((np.array(a[0], copy=True) if isinstance(a[0], np.ndarray) else None, np.array(y, copy=True)))
        return y


class _Parser(argparse.ArgumentParser):
    def parse_args(self, *a, **k):        # the reference's parse_args() returns what its parser would parse: keep the parser instead
        return self


def _cm():
    cm = matplotlib.cm
    if not hasattr(cm, "get_cmap"):       # removed from matplotlib.cm in newer releases
        import types
        cm = types.SimpleNamespace(get_cmap=lambda name: matplotlib.colormaps[name])
    return cm


def reference_namespace():
    tree = ast.parse(open(REF_SCRIPT).read())
    ns = {"np": np, "os": os, "cm": _cm(), "argparse": argparse, "zoom": _Recorder(scipy.ndimage.zoom)}
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(f.name for f in fns) == sorted(FUNCS), [f.name for f in fns]
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF_SCRIPT, "exec"), ns)
    ns["get_objectness_grid"] = _Recorder(ns["get_objectness_grid"])     # visualize_scene looks it up in this namespace
    ns["argparse"] = type("argparse", (), {"ArgumentParser": _Parser})
    return ns


def cli_flags(ns):
    parser = ns["parse_args"]()
    return dict(description=parser.description,
                flags=[dict(options=a.option_strings, dest=a.dest, default=a.default, type=a.type.__name__ if a.type else None,
                            action=type(a).__name__, required=a.required, help=a.help)
                       for a in parser._actions if a.option_strings and a.dest != "help"])


# (name, grid shape (W, L, H), boxes None / 'obb' / 'aabb', objectness None / 'rpn' / 'fcos', alpha threshold, density range)
# every level grid is ceil(n / 2^(level + 2)) per axis, as the voxel-score writers crop them: sizes 1 and 2 occur at levels 2 and 3
CASES = [("rgb_obb", (13, 11, 7), "obb", None, 0.01, (-3.0, 6.0)),
         ("rgb_aabb", (9, 14, 5), "aabb", None, 0.01, (-3.0, 6.0)),
         ("rgb_nobox", (15, 6, 9), None, None, 0.3, (-3.0, 8.0)),
         ("obj_rpn", (64, 9, 7), "obb", "rpn", 0.01, (-3.0, 6.0)),
         ("obj_fcos", (12, 19, 10), None, "fcos", 0.05, (-3.0, 6.0)),
         ("empty", (11, 7, 13), "aabb", None, 0.9, (-4.0, 2.0))]


def level_shapes(shape):
    return [tuple(int(v) for v in np.ceil(np.array(shape) / 2 ** (lvl + 2))) for lvl in range(4)]


def densities(rng, shape, lo, hi, thr):
    """Seeded densities whose float32 alphas keep ULP_MARGIN ulp away from float32(thr)."""
    t = np.float32(thr)
    band = ULP_MARGIN * np.spacing(t)
    d = rng.uniform(lo, hi, shape).astype(np.float32)
    for _ in range(100):
        a = np.clip(1.0 - np.exp(-np.exp(d) / 100.0), 0.0, 1.0)
        near = np.abs(a - t) <= band
        if not near.any():
            return d
        d[near] = rng.uniform(lo, hi, int(near.sum())).astype(np.float32)
    raise AssertionError("could not keep the alphas away from the threshold")


def boxes_for(rng, shape, fmt, n=5):
    d = np.array(shape, dtype=np.float64)
    if fmt == "obb":
        c = rng.uniform(0.1, 0.9, (n, 3)) * d
        s = rng.uniform(0.1, 0.5, (n, 3)) * d
        t = rng.uniform(-np.pi, np.pi, (n, 1))
        return np.concatenate([c, s, t], axis=1).astype(np.float32)
    lo = rng.uniform(0, 0.6, (n, 3)) * d
    hi = lo + rng.uniform(0.1, 0.4, (n, 3)) * d
    return np.concatenate([lo, hi], axis=1).astype(np.float32)


def run_case(ns, rng, tmp, name, shape, box_fmt, obj, thr, drange):
    feat, box_dir, obj_dir, out = (os.path.join(tmp, name, d) for d in ("features", "boxes", "objectness", "out"))
    for d in (feat, box_dir, obj_dir, out):
        os.makedirs(d)
    rgb = rng.uniform(0, 1, shape + (3,)).astype(np.float32)
    rgb.reshape(-1, 3)[:7] = np.array([0, 1, 0.5], dtype=np.float32)        # exact ends of the rgb range
    sigma = densities(rng, shape, drange[0], drange[1], thr)
    rgbsigma = np.concatenate([rgb, sigma[..., None]], axis=3)
    res = np.array(shape, dtype=np.int64)
    np.savez(os.path.join(feat, "scene.npz"), rgbsigma=rgbsigma, resolution=res)
    rec = dict(shape=np.array(shape), resolution=res, rgbsigma=rgbsigma, alpha_threshold=np.array(thr), box_format=np.array(box_fmt or ""),
               objectness=np.array(obj or ""))
    boxes = None
    if box_fmt:
        boxes = boxes_for(rng, shape, box_fmt)
        np.save(os.path.join(box_dir, "scene.npy"), boxes)
        rec["boxes"] = boxes.copy()
    levels = None
    if obj:
        if obj == "rpn":       # max-over-anchors logits: mostly negative (the 'under' colour after the normalisation), one positive blob
            levels = [rng.normal(-4.0, 1.5, s).astype(np.float32) for s in level_shapes(shape)]
            for lv in levels:
                lv.reshape(-1)[:3] = 6.0
        else:                  # sigmoid scores in [0, 1]
            levels = [rng.uniform(0, 1, s).astype(np.float32) ** 3 for s in level_shapes(shape)]
        # the reference reads <scene>_objectness.npz and takes [0] of every level: store them with a leading axis
        np.savez(os.path.join(obj_dir, "scene_objectness.npz"), **{str(k): lv[None] for k, lv in enumerate(levels)})
        for k, lv in enumerate(levels):
            rec[f"level{k}"] = lv
    zoom, grid = ns["zoom"], ns["get_objectness_grid"]
    zoom.calls.clear()
    grid.calls.clear()
    ns["visualize_scene"]("scene", out, feat, box_dir=box_dir if boxes is not None else None, box_format=box_fmt or "obb",
                          objectness_dir=obj_dir if obj else None, alpha_threshold=thr)
    with open(os.path.join(out, "scene.ply"), "rb") as f:
        rec["ply"] = np.frombuffer(f.read(), dtype=np.uint8)
    if obj:
        assert len(zoom.calls) == 4 and len(grid.calls) == 1
        for k, (x, y) in enumerate(zoom.calls):
            assert np.array_equal(x, levels[k]) and x.dtype == np.float32 and y.dtype == np.float32 and y.shape == shape
            rec[f"zoom{k}"] = y
        rec["score"] = grid.calls[0][1]
    a = ns["density_to_alpha"](rgbsigma.reshape(-1, 4)[:, 3])
    rec["num_points"] = np.array(int((a > thr).sum()))
    return rec


def save_stable(path, arrays):
    """np.savez_compressed with fixed zip timestamps: regenerating gives the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    ns = reference_namespace()
    rng = np.random.default_rng(20261016)
    out = {"cli": np.array(json.dumps(cli_flags(ns))), "cases": np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        for name, shape, box_fmt, obj, thr, drange in CASES:
            for k, v in run_case(ns, rng, tmp, name, shape, box_fmt, obj, thr, drange).items():
                out[f"{name}/{k}"] = v
    path = os.path.join(HERE, "visualize.npz")
    save_stable(path, out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
