"""Generate tests/golden/heatmap.npz from the REFERENCE's render_heatmap.py (build container only: it reads the reference tree).

The reference script imports pyvista, plotly, svglib, reportlab and cv2 at module level, so it cannot be imported here.  The functions
this fixture needs are taken out of its source with ``ast`` and executed with numpy, copy and scipy in their namespace; scipy's
``gaussian_filter`` is wrapped to record its input and output.  Only the recorded arrays are stored.

    python tests/golden/make_heatmap_golden.py            (rewrites heatmap.npz; the same bytes on every run)
"""
import argparse
import ast
import copy
import io
import json
import os
import tempfile
import types
import zipfile

import numpy as np
import scipy.ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
REF_SCRIPT = "/root/reference/nerf_rpn/scripts/render_heatmap.py"
FUNCS = ("density_to_alpha", "gkern_3d", "obb2hbb", "obb2point8", "world2grid", "grid2world", "generate_heatmap", "frame2config",
         "load_alpha_and_proposals", "parse_args")


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, x, sigma, **kw):
        y = scipy.ndimage.gaussian_filter(x, sigma, **kw)
        self.calls.append((x.copy(), y.copy()))
        return y


class _Parser(argparse.ArgumentParser):
    def parse_args(self, *a, **k):        # the reference's parse_args() returns what its parser would parse: keep the parser instead
        return self


def reference_namespace():
    tree = ast.parse(open(REF_SCRIPT).read())
    ns = {"np": np, "copy": copy, "json": json, "os": os, "ArgumentParser": _Parser, "gaussian_filter": _Recorder()}
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in FUNCS]
    assert sorted(f.name for f in fns) == sorted(FUNCS), [f.name for f in fns]
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF_SCRIPT, "exec"), ns)
    # the box preparation of __main__ (obb2hbb -> astype(int) -> clip of axis i to res[i] - 1), taken from the reference too
    main = next(n for n in tree.body if isinstance(n, ast.If) and "__main__" in ast.dump(n.test))
    loop = next(n for n in main.body if isinstance(n, ast.For))
    prep = []
    for st in loop.body:
        if isinstance(st, ast.Assign) and ast.unparse(st.targets[0]) == "aabbs":
            prep.append(st)
        if isinstance(st, ast.For) and prep:
            prep.append(st)
            break
    assert len(prep) == 2, ast.unparse(loop)
    ns["_prepare"] = compile(ast.Module(body=prep, type_ignores=[]), REF_SCRIPT, "exec")
    return ns


def cli_flags(ns):
    parser = ns["parse_args"]()
    return [dict(options=a.option_strings, dest=a.dest, default=a.default, choices=list(a.choices) if a.choices else None,
                 type=a.type.__name__ if a.type else None, action=type(a).__name__)
            for a in parser._actions if a.option_strings and a.dest != "help"]


def proposals(rng, dims, n=30):
    """Seeded OBBs (x, y, z, w, l, h, theta) in grid units: some cross the faces, some are 0 or 1 voxel thick, some overlap."""
    d = np.array(dims, dtype=np.float64)
    c = rng.uniform(-0.1, 1.1, (n, 3)) * d
    s = rng.uniform(0.08, 0.5, (n, 3)) * d
    t = rng.uniform(-np.pi, np.pi, (n, 1))
    b = np.concatenate([c, s, t], axis=1)
    b[3:6, 6] = 0.0
    b[3, 5], b[3, 2] = 0.2, 5.3            # zero extent in z after truncation
    b[4, 3], b[4, 0] = 0.3, 7.6            # one voxel in x (theta 0)
    b[5, 4], b[5, 1] = 0.0, 4.5            # zero-width in y
    b[6:9, :3] = b[9, :3] + rng.uniform(-1, 1, (3, 3))    # overlapping with box 9
    b[10, :3], b[10, 3:6] = d / 2, d * 1.5                 # covers the whole grid
    return b.astype(np.float32)


def frames(rng, count=3):
    out = []
    for k in range(count):
        a, e = rng.uniform(-np.pi, np.pi), rng.uniform(-0.6, 0.2)
        f = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
        r = np.cross(f, [0, 0, 1.0])
        r /= np.linalg.norm(r)
        u = np.cross(r, f)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2] = r, u, -f
        m[:3, 3] = rng.uniform([-0.5, -0.3, 0.4], [2.8, 2.4, 2.0])
        out.append({"file_path": f"./images/{k:04d}.jpg", "transform_matrix": m.tolist()})
    return out


ROOM = [[-1.2, -0.8, 0.0], [3.4, 2.9, 2.6]]
# (name, alpha shape (W, L, H), kernel_type, sigma, transpose_yz): every axis of the small grids is shorter than 2r at sigma 5 (r = 20)
CASES = [("a_gauss_s5", (36, 30, 22), "gaussian", 5.0, False),
         ("a_box_s2_t", (36, 30, 22), "box", 2.0, True),
         ("b_gauss_s5_t", (24, 20, 16), "gaussian", 5.0, True),
         ("b_box_s5", (24, 20, 16), "box", 5.0, False),
         ("b_gauss_s2", (24, 20, 16), "gaussian", 2.0, False),
         ("b_box_s2_t", (24, 20, 16), "box", 2.0, True)]
KERNEL_SHAPES = [(0, 3, 2), (1, 1, 1), (1, 4, 2), (2, 3, 5), (5, 1, 7), (6, 6, 6), (7, 9, 4), (10, 3, 12)]


def run_case(ns, rng, tmp, shape, kernel_type, sigma, transpose_yz):
    W, L, H = shape
    # the feature file's resolution is chosen so that the reference's res permutation matches the alpha grid it loads
    if transpose_yz:
        rgbsigma = rng.uniform(-2, 2, (W, H, L, 4)).astype(np.float32)
        resolution = np.array([L, H, W])
    else:
        rgbsigma = rng.uniform(-2, 2, (W, L, H, 4)).astype(np.float32)
        resolution = np.array([H, W, L])
    props = proposals(rng, shape)
    np.savez(os.path.join(tmp, "f.npz"), rgbsigma=rgbsigma, resolution=resolution)
    np.savez(os.path.join(tmp, "p.npz"), proposals=props)
    with open(os.path.join(tmp, "t.json"), "w") as f:
        json.dump({"room_bbox": ROOM}, f)
    args = types.SimpleNamespace(transpose_yz=transpose_yz, top_n=100, kernel_type=kernel_type, gaussian_sigma=sigma)
    alpha, proposals_, room_bbox, res = ns["load_alpha_and_proposals"](os.path.join(tmp, "f.npz"), os.path.join(tmp, "p.npz"),
                                                                       os.path.join(tmp, "t.json"), args)
    assert alpha.shape == tuple(shape) and alpha.dtype == np.float32, (alpha.shape, alpha.dtype)
    loc = dict(ns, proposals=proposals_, res=res)
    exec(ns["_prepare"], loc)
    aabbs = loc["aabbs"]
    rec = ns["gaussian_filter"]
    rec.calls.clear()
    heat = ns["generate_heatmap"](alpha, aabbs, args)
    (pre, filt), = rec.calls
    fr = frames(rng)
    cams = {}
    for d in (1, 2):
        names, pos, foc, _ = ns["frame2config"](fr, room_bbox, res, d)
        cams[d] = (np.array(pos), np.array(foc))
    return dict(shape=np.array(shape), resolution=resolution, transpose_yz=np.array(transpose_yz), sigma=np.array(sigma),
                kernel_type=np.array(kernel_type), proposals=props, aabbs=aabbs.astype(np.int64), res=np.array(res, dtype=np.int64),
                pre=pre, filtered=filt, heatmap=heat, frames=np.array(json.dumps(fr)), room_bbox=np.array(ROOM),
                cam_pos_d1=cams[1][0], cam_focal_d1=cams[1][1], cam_pos_d2=cams[2][0], cam_focal_d2=cams[2][1])


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
    out = {"cli_flags": np.array(json.dumps(cli_flags(ns))), "cases": np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        for name, shape, kt, sigma, tyz in CASES:
            for k, v in run_case(ns, rng, tmp, shape, kt, sigma, tyz).items():
                out[f"{name}/{k}"] = v
    out["kernel_shapes"] = np.array(KERNEL_SHAPES, dtype=np.int64)
    out["kernels"] = np.concatenate([ns["gkern_3d"](w=w, l=l, h=h).reshape(-1) for w, l, h in KERNEL_SHAPES])
    path = os.path.join(HERE, "heatmap.npz")
    save_stable(path, out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
