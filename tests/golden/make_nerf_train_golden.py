"""Generate tests/golden/nerf_train.npz and nerf_train_bounds.json from the REFERENCE's data/scannet/run_nerf.py (build container
only: it reads the reference tree).

run_nerf.py is imported as make_nerf_render_golden.py imports it.  get_rays, sample_pdf and select_coordinates come from the fork; the
checker's definitions (tests/nerf_train_ref.py, tests/nerf_render_ref.py; the assumptions of DESIGN.md 3.16 and 3.22) are set as the
module's globals, and recorded numbers stand in for torch.rand_like (perturb_z_vals) and for sample_pdf's torch.rand.  For every case
the reference's own get_ray_batch_from_one_image, perturb_z_vals and render -> render_rays with depth columns and perturb = 1 run on
the CPU, around a query function that returns the case's recorded raw for the first list and a pointwise linear function of the points
for the second -- compute_samples_around_depth, sample_3sigma, raw2depth, forward_with_additonal_samples and raw2outputs are the
reference's code.  raw_noise_std is 0: the noise enters after the stage under test.  Only recorded results are
stored; no reference text.

nerf_train.npz          <case>/rays, viewdirs, target_s, target_d, target_vd, depth_range, z1, z2, z_vals, weights, rgb_map, depth_map
nerf_train_bounds.json  per case and tensor: 8 x the largest |float32 checker - float64 checker|, floored at one float32 ulp of the
                        tensor's largest magnitude, with the measured error; "rejected": the rays left out of the z2 comparison (a
                        sample of the float64 run in a bin of non-zero width whose cdf difference is between 1e-6 and 1e-4), asserted
                        to be at most 10 % of the case's rays; "loop": the eight losses of the float64 host loop and the bound on each;
                        "cli_defaults": config_parser's defaults (:924-1008) of the flags the train task reads.

The float32 checker must equal the reference bit for bit in every stored array (asserted) or nothing is written.

    python tests/golden/make_nerf_train_golden.py       rewrites both files; the same bytes on every run
"""
import json
import os
import sys

os.environ.setdefault("MKL_CBWR", "COMPATIBLE")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.dont_write_bytecode = True       # the reference tree is read-only

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import nerf_render_ref as V                                 # noqa: E402
import nerf_train_ref as T                                  # noqa: E402
from argparse import Namespace                              # noqa: E402
from make_nerf_extract_golden import reference_module       # noqa: E402
from make_scannet_golden import save_stable                 # noqa: E402


def reference_case(RN, c):
    """The reference's batch, perturbation and render_rays on one case -> dict of numpy arrays over T.STORED."""
    T.select_coordinates.pix = c.pix
    args = Namespace(N_rand=c.R, depth_loss_weight=0.004)
    np.random.seed(0)
    batch_rays, target_s, target_d, target_vd, img_i = RN.get_ray_batch_from_one_image(
        T.H, T.W, np.array([0]), c.image[None], c.depth[None], c.valid[None], c.c2w[None], c.intrinsic[None], args)
    out = {"rays": torch.cat([batch_rays[0], batch_rays[1]], -1), "target_s": target_s, "target_d": target_d, "target_vd": target_vd,
           "depth_range": batch_rays[2]}
    saved = torch.rand_like
    torch.rand_like = lambda x, **kw: c.t_rand
    try:
        out["z1"] = RN.perturb_z_vals(c.z.unsqueeze(0).expand(c.R, c.S), False)
        valid = batch_rays[2][:, 0] >= c.near
        T.sample_pdf.feed = [c.u[~valid], c.u[valid]]
        drawn, calls = [], []

        def recording_pdf(*a, **k):
            drawn.append(T.sample_pdf(*a, **k))
            return drawn[-1]

        def query(pts, viewdirs, embedded_cam, network_fn):
            calls.append(viewdirs)
            return c.raw1 if len(calls) == 1 else T.point_raw(pts, c.A)
        RN.sample_pdf = recording_pdf
        rgb, _, _, extras = RN.render(T.H, T.W, None, chunk=1 << 20, rays=batch_rays, near=c.near, far=c.far, use_viewdirs=True,
                                      network_fn=None, network_query_fn=query, N_samples=2 * c.S, precomputed_z_samples=c.z, perturb=1.,
                                      raw_noise_std=0.)
    finally:
        torch.rand_like = saved
        RN.sample_pdf = T.sample_pdf
    assert len(calls) == 2 and len(drawn) == 2 and not T.sample_pdf.feed, c.name
    z2 = torch.empty(c.R, c.S)
    z2[~valid], z2[valid] = drawn[0], drawn[1]
    out.update(viewdirs=calls[0], z2=z2, z_vals=extras["z_vals"], weights=extras["weights"], rgb_map=rgb, depth_map=extras["depth_map"])
    return {k: out[k].detach().numpy() for k in T.STORED}


def main():
    torch.set_num_threads(1)
    RN = reference_module()
    RN.get_rays = V.get_rays
    RN.sample_pdf = T.sample_pdf
    RN.select_coordinates = T.select_coordinates
    out, cases = {}, {}
    for case in T.CASES:
        c = T.case_inputs(case)
        ref = reference_case(RN, c)
        o32, o64 = T.run_case(c, torch.float32), T.run_case(c, torch.float64)
        for k in T.STORED:
            mine = o32[k].numpy()
            assert mine.dtype == ref[k].dtype and np.array_equal(mine, ref[k], equal_nan=False), f"{c.name}/{k}: checker != reference"
        assert all(torch.isfinite(o64[k]).all() for k in T.STORED if k != "target_vd"), c.name
        norm = o64["rays"][:, 3:].norm(dim=-1)
        assert 0.5 < norm.min() and norm.max() < 2.0, (c.name, float(norm.min()), float(norm.max()))
        rejected = o64["rejected"].numpy()
        assert rejected.sum() <= T.REJECT_CAP * c.R, (c.name, int(rejected.sum()))
        b = {"num_rays": c.R, "rejected": [int(i) for i in np.nonzero(rejected)[0]]}
        for k in T.STORED:
            if k == "target_vd":
                continue
            err = C_max_error(T.kept(o32, k, rejected), T.kept(o64, k, rejected))
            b[k] = {"bound": T.bound_of(err, T.kept(o64, k, rejected)), "fp32_error": err}
        cases[c.name] = b
        for k in T.STORED:
            out[f"{c.name}/{k}"] = ref[k]
        print(f"{c.name}: rejected {b['rejected']}, fp32 errors " + ", ".join(f"{k} {b[k]['fp32_error']:.2g}" for k in ("z1", "z2", "weights")))
    L = T.loop_inputs()
    l64, l32 = T.train_loop_host(L, torch.float64), T.train_loop_host(L, torch.float32)
    assert l64[-1] < l64[0], l64
    loop = {"fp64": l64, "fp32_error": [abs(a - b) for a, b in zip(l32, l64)]}
    loop["bound"] = [max(T.FACTOR * e, float(np.spacing(np.float32(abs(v))))) for e, v in zip(loop["fp32_error"], l64)]
    print("loop:", ", ".join(f"{v:.4g} (+-{b:.2g})" for v, b in zip(l64, loop["bound"])))
    parser = RN.config_parser()
    cli = {a.dest: a.default for a in parser._actions if a.dest in T.CLI_FLAGS}
    assert sorted(cli) == sorted(T.CLI_FLAGS), sorted(set(T.CLI_FLAGS) - set(cli))
    out["cases"] = np.array(T.NAMES)
    path = os.path.join(HERE, "nerf_train.npz")
    save_stable(path, out)
    with open(os.path.join(HERE, "nerf_train_bounds.json"), "w") as f:
        json.dump({"factor": T.FACTOR, "reject_cap": T.REJECT_CAP, "cases": cases, "loop": loop, "cli_defaults": cli}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")


def C_max_error(a, b):
    return T.C.max_error(a, b)


if __name__ == "__main__":
    main()
