"""NeRF test-view metrics (csrc/nerfmetrics.hip) on the MI355X, through ops.nerf_view_metrics and the nerf_test command line.

The reference is tests/nerf_eval_ref.py in float64, in the valid-window form whose rounding the derived bounds count
(ssim_pixel_bound and the functions after it: functions of 2^-53, 49, C1 and C2, never typed in).  The kernel and the checker are two
float64 evaluations, each within the bound of the exact value, so they must lie within twice it of each other.  The sizes are placed
around the kernel's tile edge T (lib.query("nerfmetrics_tile")): one window row and column, a partial tile, exactly one tile of
windows over four tiles of pixels, one window more than a tile, and a frame of several tiles.  The command line is compared with what
the reference's own test task recorded (tests/golden/nerf_eval.npz) within 8 x the float32 checker's error of that case
(nerf_eval_bounds.json).  Every figure is printed before it is asserted."""
import math
import os

import numpy as np
import pytest
import torch

import nerf_eval_ref as E
from nerf_eval_ref import bounds, evals, golden_npz  # noqa: F401  (fixtures)
from nerf_rpn_amd import lib, ops
from nerf_rpn_amd.scripts import nerf_test as X

pytestmark = pytest.mark.gpu

# in units of the tile edge T
SIZES = {"7x7": lambda T: (7, 7), "7x40": lambda T: (7, 40), "13x9": lambda T: (13, 9), "T+6": lambda T: (T + 6, T + 6),
         "T+7x2T+5": lambda T: (T + 7, 2 * T + 5), "96x130": lambda T: (96, 130)}
_REFS = {}


def frame_and_ref(H, W, noise):
    """The seeded frame and its float64 reference, computed once per (size, noise) and shared."""
    key = (H, W, noise)
    if key not in _REFS:
        f = E.synth_frame(H, W, noise)
        _REFS[key] = (f, E.frame_ref(f, torch.float64, form="windows"))
    return _REFS[key]


def metrics(f, depth=True, **kw):
    d = dict(depth=f.depth, target_depth=f.target_depth, valid_depth=f.valid) if depth and f.depth is not None else {}
    return ops.nerf_view_metrics(f.rgb, f.target, far=f.far, **d, **kw)


@pytest.mark.parametrize("noise", E.NOISES)
@pytest.mark.parametrize("size", list(SIZES))
def test_metrics_within_the_derived_bound_of_fp64(dev, size, noise):
    T = lib.query("nerfmetrics_tile")
    assert T >= 8
    H, W = SIZES[size](T)
    f, ref = frame_and_ref(H, W, noise)
    got = metrics(f)
    E.check_against_fp64(got, ref, H, W, name=f"{H}x{W} noise {noise}")
    if noise == 0.0:
        assert got["img_loss"] == 0.0 and got["psnr"] == math.inf and abs(got["ssim"] - 1.0) <= E.ssim_bound((H - 6) * (W - 6))


def test_depth_selection(dev):
    T = lib.query("nerfmetrics_tile")
    H, W = T + 7, 2 * T + 5
    f, ref = frame_and_ref(H, W, 0.02)
    plain = metrics(f, depth=False)
    assert plain["depth_rmse"] is None and plain["n_valid"] == 0

    def run(valid, target_depth=None):
        td = f.target_depth if target_depth is None else target_depth
        got = ops.nerf_view_metrics(f.rgb, f.target, f.depth, td, valid)
        want = E.frame_metrics(f.rgb, f.target, f.depth, td, valid, dtype=torch.float64, form="windows")
        E.check_against_fp64(got, want, H, W, name=f"{int(valid.sum())} valid")
        for k in ("img_loss", "psnr", "ssim"):           # the depth arguments leave the colour metrics bit-equal
            assert got[k] == plain[k], k
        return got
    none = run(torch.zeros(H, W, dtype=torch.bool))
    assert none["depth_rmse"] is None and none["n_valid"] == 0
    one = torch.zeros(H, W, dtype=torch.bool)
    one[H - 1, W - 1] = True                              # the last pixel of the last, partial tile
    got = run(one)
    assert got["n_valid"] == 1 and got["depth_rmse"] == abs(float(f.depth[-1, -1].double() - f.target_depth[-1, -1].double()))
    assert run(torch.ones(H, W, dtype=torch.bool))["n_valid"] == H * W
    # NaN / inf under the mask are never read
    bad = torch.where(f.valid, f.target_depth, torch.where(torch.arange(H * W).reshape(H, W) % 2 == 0, float("nan"), float("inf")))
    assert not torch.isfinite(bad[~f.valid]).any()
    poisoned, clean = run(f.valid, bad), run(f.valid)
    assert poisoned["depth_rmse"] == clean["depth_rmse"] and math.isfinite(poisoned["depth_rmse"]) and poisoned["n_valid"] == ref["n_valid"]
    u8 = ops.nerf_view_metrics(f.rgb, f.target, f.depth, bad, f.valid.to(torch.uint8))
    assert u8["depth_rmse"] == clean["depth_rmse"]


def test_quantisers_equal_numpy(dev):
    table = E.quantiser_table()
    W = 9
    rows = -(-len(table) // W)
    x = np.resize(table, rows * W).reshape(rows, W)
    assert rows >= 7
    far = 4.0                                             # a power of two: depth / far gives the table's values back exactly
    rgb = torch.from_numpy(np.stack([x, x[::-1], np.roll(x, 1, 1)], -1).copy())
    depth = torch.from_numpy(x * np.float32(far))
    zeros = torch.zeros(rows, W)
    out = ops.nerf_view_metrics(rgb, rgb.clamp(0, 1), depth, zeros, zeros.bool(), far=far, return_images=True)
    assert out["rgb8"].dtype == torch.uint8 and out["depth16"].dtype == torch.uint16
    assert np.array_equal(out["rgb8"].cpu().numpy(), E.to8b(rgb.numpy()))
    assert np.array_equal(out["depth16"].cpu().numpy(), E.to16b(x))
    # an arbitrary far: float32 division, as numpy's
    f, _ = frame_and_ref(13, 9, 0.2)
    for far in (4.0, 3.7, 0.9):
        out = ops.nerf_view_metrics(f.rgb, f.target, f.depth, f.target_depth, f.valid, far=far, return_images=True)
        a, b = E.frame_images(f.rgb, f.depth, float(np.float32(far)))
        assert np.array_equal(out["rgb8"].cpu().numpy(), a) and np.array_equal(out["depth16"].cpu().numpy(), b), far
        assert (a == 0).any() and (a == 255).any()
    assert sorted(ops.nerf_view_metrics(f.rgb, f.target, return_images=True)) == ["depth_rmse", "img_loss", "n_valid", "psnr", "rgb8", "ssim"]


def test_repeated_runs_are_bit_equal(dev):
    T = lib.query("nerfmetrics_tile")
    f, _ = frame_and_ref(T + 7, 2 * T + 5, 0.2)
    a = metrics(f, return_images=True)
    for _ in range(3):
        b = metrics(f, return_images=True)
        assert {k: v for k, v in a.items() if not torch.is_tensor(v)} == {k: v for k, v in b.items() if not torch.is_tensor(v)}
        assert torch.equal(a["rgb8"], b["rgb8"]) and torch.equal(a["depth16"], b["depth16"])


def test_small_frames_and_mismatches_raise(dev):
    f, _ = frame_and_ref(13, 9, 0.02)
    for shape in ((6, 9), (9, 6)):
        with pytest.raises(ValueError, match="7 x 7"):
            ops.nerf_view_metrics(torch.zeros(*shape, 3), torch.zeros(*shape, 3))
    with pytest.raises(lib.NrpnError, match="target_rgb has shape"):
        ops.nerf_view_metrics(f.rgb, f.target[:, :8])
    with pytest.raises(lib.NrpnError, match="torch.float64"):
        ops.nerf_view_metrics(f.rgb.double(), f.target)
    with pytest.raises(lib.NrpnError, match="go together"):
        ops.nerf_view_metrics(f.rgb, f.target, depth=f.depth)
    with pytest.raises(lib.NrpnError, match="valid_depth is"):
        ops.nerf_view_metrics(f.rgb, f.target, f.depth, f.target_depth, f.valid.float())
    with pytest.raises(lib.NrpnError, match="far"):
        ops.nerf_view_metrics(f.rgb, f.target, f.depth, f.target_depth, f.valid, return_images=True)
    assert lib.query("nerfmetrics_work_bytes", 6, 9) == -1


@pytest.mark.parametrize("name, task", [("two_pass_9x8", "test"), ("plain_no_depth_7x10", "render_train_depth")])
def test_cli_end_to_end_against_the_reference(dev, evals, golden_npz, bounds, tmp_path, name, task):
    from PIL import Image
    c, _, f32, _ = evals(name)
    transforms = X.TASKS[task][0]
    argv = E.write_run(tmp_path, c, golden_npz[f"{name}/target_rgb8"], golden_npz[f"{name}/target_depth16"], transforms=transforms)
    res = X.main(argv + ["--task", task])
    out_dir = os.path.join(str(tmp_path), "ckpt", "run1", X.TASKS[task][1] + "scene0000_00")
    assert res["dir"] == out_dir
    want = sorted([f"{n}_rgb.jpg" for n in range(c.frames)] + [f"{n}_d.png" for n in range(c.frames)] + ["metrics.txt"])
    assert sorted(os.listdir(out_dir)) == want == sorted(os.path.basename(p) for p in golden_npz[f"{name}/files"])
    for n in range(c.frames):
        d = np.asarray(Image.open(os.path.join(out_dir, f"{n}_d.png")))
        assert d.dtype == np.uint16 and d.shape == (c.H, c.W)
        assert np.abs(d.astype(np.int64) - golden_npz[f"{name}/depth16"][n]).max() <= 1      # the render differs in its last float32 bits
        img = Image.open(os.path.join(out_dir, f"{n}_rgb.jpg"))
        assert img.format == "JPEG" and img.size == (c.W, c.H)
    with open(os.path.join(out_dir, "metrics.txt")) as f:
        lines = f.read().splitlines()
    parsed = {ln.split(": ")[0]: float(ln.split(": ")[1]) for ln in lines}
    assert list(parsed) == [ln.split(":")[0] for ln in golden_npz[f"{name}/metrics_txt"]] and parsed == res["mean"]
    b, bad = bounds["cases"][name], []
    rows = [(f"frame {n}", m, golden_npz[f"{name}/frame_metrics"][n]) for n, m in enumerate(res["frames"])]
    for label, got, recorded in rows + [("mean", parsed, golden_npz[f"{name}/mean_metrics"])]:
        for k, want_v in zip(E.METRICS, recorded):
            if np.isnan(want_v):
                assert got.get(k) is None, (label, k)
                continue
            err = abs(got[k] - want_v)
            print(f"{name} {label}: {k} {got[k]!r} vs the reference's {want_v!r}: error {err:.3g} (bound {b[k]['bound']:.3g}, float32 checker {b[k]['fp32_error']:.3g})")
            if not err <= b[k]["bound"]:
                bad.append((label, k, err, b[k]["bound"]))
    assert not bad, bad
