"""NeRF grid kernels (csrc/nerfgrid.hip) on the MI355X, through ops.nerf_grid_query and the nerf_extract command line.

The reference is tests/nerf_extract_ref.py in float64 (extract_nerf in the reference's order, on the float32 grid coordinates, weights
and poses).  Every element of every case, in both layouts, must lie within the case's bound of it: 8 x the largest |float32 checker
in reference order - float64 checker| of that case and channel group (tests/golden/nerf_extract_bounds.json, written by
make_nerf_extract_golden.py, never typed in).  The factor covers the 313-term skip product split into 64 + 256, the MFMA's k order
and the device's sinf / cosf / expf.  The weights are regenerated from seeds; the float64 reference is computed once per case and
shared."""
import numpy as np
import pytest
import torch

import nerf_extract_ref as R
from nerf_rpn_amd import ops
from nerf_rpn_amd.scripts import nerf_extract as X
from nerf_extract_ref import bounds, golden_npz, write_run  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in R.CASES]


@pytest.fixture(scope="module")
def refs():
    """case name -> (inputs, float64 (N, 4) reference); filled on first use."""
    cache = {}

    def get(name):
        if name not in cache:
            c = R.case_inputs(R.CASES[NAMES.index(name)])
            f64 = R.extract(c.state, c.cfg, c.xs, c.ys, c.zs, c.bb_center, c.bb_scale, c.poses, dtype=torch.float64).numpy()
            f64.setflags(write=False)
            cache[name] = (c, f64)
        return cache[name]
    return get


def query(c, layout="flat", chunk=None, state=None):
    return ops.nerf_grid_query(state or c.state, c.cfg, c.xs, c.ys, c.zs, c.bb_center, c.bb_scale, c.poses, layout=layout,
                               chunk=chunk).cpu().numpy()


def check(name, got, ref, b):
    err = np.abs(got.astype(np.float64) - ref)
    e_rgb, e_sigma = err[..., :3].max(), err[..., 3].max()
    print(f"{name}: rgb error {e_rgb:.3g} (bound {b['rgb']:.3g}), sigma error {e_sigma:.3g} (bound {b['sigma']:.3g})")
    assert np.isfinite(got).all()
    assert e_rgb <= b["rgb"], (name, e_rgb, b["rgb"])
    assert e_sigma <= b["sigma"], (name, e_sigma, b["sigma"])


@pytest.mark.parametrize("layout", ["flat", "wlh"])
@pytest.mark.parametrize("name", NAMES)
def test_every_element_within_bound_of_fp64(dev, refs, bounds, name, layout):
    c, f64 = refs(name)
    got = query(c, layout)
    assert got.dtype == np.float32
    ref = f64 if layout == "flat" else R.flat_to_wlh(f64, c.res)
    assert got.shape == ref.shape == ((len(f64), 4) if layout == "flat" else (*c.res, 4))
    check(f"{name}/{layout}", got, ref, bounds[name])


@pytest.mark.parametrize("name", ["odd_7x6x5", "line_1x1x3"])
def test_coordinates_through_a_zero_weight_network(dev, refs, name):
    """All weights zero, alpha_linear.bias and rgb_linear.bias set: the exact output is bias and sigmoid(bias) at every point whatever
    the coordinates; with pts_linears.0 reading one encoding column it is the coordinate itself."""
    c, _ = refs(name)
    zero = {k: torch.zeros_like(v) for k, v in c.state.items()}
    zero["alpha_linear.bias"] = torch.tensor([0.625])
    zero["rgb_linear.bias"] = torch.tensor([-1.5, 0.25, 2.0])
    got = query(c, state=zero)
    assert (got[:, 3] == np.float32(0.625)).all()
    want = torch.sigmoid(zero["rgb_linear.bias"].double()).numpy()
    # expf within 2 ulp, the two divisions and the P - 1 = 4 additions half an ulp each: 5 ulp of a value below 1 = 2.5 eps
    assert np.abs(got[:, :3] - want).max() <= 4 * np.finfo(np.float32).eps
    # sigma = relu chain of p[a] + 4 >= 0 through identity-like weights: column a of the encoding reaches alpha_linear unchanged
    pts = ((R.grid_points(c.xs, c.ys, c.zs) - c.bb_center) * c.bb_scale).numpy()
    for a in range(3):
        st = {k: v.clone() for k, v in zero.items()}
        st["pts_linears.0.weight"][0, a] = 1.0
        st["pts_linears.0.bias"][0] = 4.0
        for i in range(1, 8):
            st[f"pts_linears.{i}.weight"][0, 57 if i == 5 else 0] = 1.0
        st["alpha_linear.weight"][0, 0] = 1.0
        st["alpha_linear.bias"][0] = 0.0
        got = query(c, state=st)
        assert np.array_equal(got[:, 3], pts[:, a] + np.float32(4.0)), a


def test_chunk_of_one_tile_is_bit_equal(dev, refs):
    c, _ = refs("tiles_9x8x8")
    for layout in ("flat", "wlh"):
        assert np.array_equal(query(c, layout), query(c, layout, chunk=64))
    c, _ = refs("odd_7x6x5")
    assert np.array_equal(query(c), query(c, chunk=1))
    assert np.array_equal(query(c), query(c, chunk=130))


def test_two_runs_are_bit_equal(dev, refs):
    c, _ = refs("tiles_9x8x8")
    assert np.array_equal(query(c), query(c))


def test_module_prefix_and_unsupported(dev, refs):
    c, _ = refs("half_4x2x2")
    assert np.array_equal(query(c), query(c, state={"module." + k: v for k, v in c.state.items()}))
    with pytest.raises(NotImplementedError, match="netwidth"):
        ops.nerf_grid_query(c.state, dict(c.cfg, netwidth=128), c.xs, c.ys, c.zs, c.bb_center, c.bb_scale, c.poses)


def test_cli_end_to_end(dev, refs, bounds, golden_npz, tmp_path):
    c, f64 = refs("odd_7x6x5")
    argv, _ = write_run(tmp_path, c)
    path = X.main(argv)
    assert path == str(tmp_path / "out" / "scene0000_00.npz")
    with np.load(path) as f:
        got = {k: f[k] for k in f.files}
    assert got["rgbsigma"].dtype == np.float32 and got["rgbsigma"].shape == (210, 4)
    check("cli", got["rgbsigma"], f64, bounds["odd_7x6x5"])
    gold = golden_npz["odd_7x6x5/rgbsigma"].astype(np.float64)
    b = bounds["odd_7x6x5"]
    err = np.abs(got["rgbsigma"] - gold)
    print(f"cli against the reference golden: rgb {err[:, :3].max():.3g}, sigma {err[:, 3].max():.3g}")
    assert err[:, :3].max() <= b["rgb"] and err[:, 3].max() <= b["sigma"]
    assert np.array_equal(got["resolution"], golden_npz["odd_7x6x5/resolution"])
    assert got["bbox_min"].dtype == np.float32 and np.array_equal(got["bbox_min"], golden_npz["odd_7x6x5/bbox_min"])
    assert np.array_equal(got["bbox_max"], golden_npz["odd_7x6x5/bbox_max"])
    assert got["scale"] == 1.0 and got["offset"] == 0.0 and not got["from_mitsuba"] and got["from_ddp_nerf"]
