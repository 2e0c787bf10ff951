"""Generate tests/golden/nerf_composite_golden.npz and nerf_composite_bounds.json from the REFERENCE's data/scannet/run_nerf.py
(build container only: it reads the reference tree).

run_nerf.py is imported as make_nerf_extract_golden.py imports it.  For every case of tests/nerf_composite_ref.py the reference's own
forward_with_additonal_samples (two lists) or raw2outputs (one list) runs on the case's raw and z without noise, and its
compute_weights on the merged samples with the case's noise; autograd of the seeded cotangent through them gives draw1 and draw2.
The checker must reproduce them: in float64 to 1e-12 of each tensor's largest magnitude, in float32 bit for bit with 1 and with 16
threads.  compute_depth_loss is not in the reference tree: the checker's depth loss is compared with torch.nn.GaussianNLLLoss(eps=
0.001) over boolean masks composed here as DESIGN.md 3.21 states them.  Only recorded results are stored; no reference text.

nerf_composite_golden.npz    per case and tensor <case>/<tensor>: [sum, absolute sum, 16 entries at seeded positions] of the
                             float64 checker (nerf_query_ref.summary), after the comparisons above.
nerf_composite_bounds.json   per case: tau per decision = 8 x the float32 checker's largest error in the quantity decided on over a
                             seeded pool of 256 candidate rays, the candidates and the rejected among them, what the rays cover, and
                             per tensor the bound (8 x the float32 checker's error, floored at a float32 ulp of the largest
                             magnitude; 0 for an exactly zero tensor) with the measured error; "train": as in nerf_query_bounds.json.

    python tests/golden/make_nerf_composite_golden.py       rewrites both files; the same bytes on every run
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

import nerf_composite_ref as C                              # noqa: E402
import nerf_query_ref as Q                                  # noqa: E402
from make_nerf_extract_golden import reference_module       # noqa: E402
from make_scannet_golden import save_stable                 # noqa: E402


def reference_stage(RN, c, dtype, noise):
    """The reference's functions on the case -> dict of tensors.  Without noise: forward_with_additonal_samples / raw2outputs, every
    output and the gradient of the seeded cotangent; with noise: compute_weights on the merged samples."""
    def f(x):
        return None if x is None else x.to(dtype)
    raw1 = f(c.raw1).clone().requires_grad_(True)
    raw2 = None if c.raw2 is None else f(c.raw2).clone().requires_grad_(True)
    z1 = f(c.z1).expand(raw1.shape[0], -1) if c.z1.dim() == 1 else f(c.z1)
    rays_d = f(c.rays_d)
    if noise:
        raw, z, nz = C.merge(raw1, z1, raw2, f(c.z2), f(c.noise))
        return {"weights": RN.compute_weights(raw, z, rays_d, nz).detach()}
    if raw2 is None:
        out = dict(zip(C.OUTPUTS, (*RN.raw2outputs(raw1, z1, rays_d, 0.), z1)))
    else:
        out = RN.forward_with_additonal_samples(z1, raw1, f(c.z2), torch.zeros_like(rays_d), rays_d, None, None, None,
                                                lambda *a: raw2, 0., False)
    wrt = [raw1] + ([] if raw2 is None else [raw2])
    res = {k: out[k].detach() for k in C.OUTPUTS}
    res.update(zip(["draw1", "draw2"], torch.autograd.grad(C.cot_sum(out, c, dtype), wrt)))
    return res


def composed_depth_loss(o, c, dtype):
    """GaussianNLLLoss(eps=0.001) over the boolean masks of DESIGN.md 3.21, on the checker's outputs."""
    m, z, w = (torch.as_tensor(o[k]) for k in ("depth_map", "z_vals", "weights"))
    t, s, vd = c.target_d[:, 0].to(dtype), c.target_d[:, 1].to(dtype), c.target_vd
    v = ((z - m[:, None]) ** 2 * w).sum(-1) + 1e-5
    applied = vd & (((m - t).abs() - s > 0) | (s ** 2 < v))
    if not applied.any():
        return torch.zeros((), dtype=dtype)
    return float(applied.sum()) / float(len(vd)) * torch.nn.GaussianNLLLoss(eps=0.001)(m[applied], t[applied], v[applied])


def main():
    torch.set_num_threads(1)
    RN = reference_module()
    out, cases = {}, {}
    f32_equal = True
    below = above = 0
    for index, case in enumerate(C.CASES):
        pool = C.pool_errors(case)
        tau = {k: C.FACTOR * v for k, v in pool.items()}
        c = C.case_inputs(case, tau)
        share = c.info["rejected"] / c.info["candidates"]
        assert share <= 0.10, (c.name, share)
        plain = C.SimpleNamespace(**dict(vars(c), noise=None))
        o64, o32 = C.check_case(c, torch.float64), C.check_case(c, torch.float32)
        for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 0.0)):
            for threads in ((1,) if tol else (1, 16)):
                torch.set_num_threads(threads)
                pairs = []
                if case["S1"] + case["S2"] > 1:       # the reference's compute_weights cannot take a single sample (:423)
                    pairs.append((reference_stage(RN, c, dtype, False), C.check_case(plain, dtype)))
                if c.noise is not None:
                    pairs.append((reference_stage(RN, c, dtype, True), C.check_case(c, dtype)))
                for ref, chk in pairs:
                    for k, v in ref.items():
                        if tol:
                            assert C.max_error(chk[k], v) <= tol * C.top_of(v), (c.name, k)
                        else:
                            f32_equal &= bool(np.array_equal(chk[k].numpy(), v.numpy(), equal_nan=True))
                chk = C.check_case(c, dtype)
                want = composed_depth_loss(chk, c, dtype)
                if tol:
                    assert abs(float(chk["depth_loss"]) - float(want)) <= tol * max(abs(float(want)), 1.0), (c.name, "depth_loss")
                else:
                    f32_equal &= bool(torch.equal(chk["depth_loss"], want))
        torch.set_num_threads(1)
        man = C.manual(c)
        q, _, aux = C.margins(c)
        kinds = C.ray_kinds(case, torch.arange(case["R"]))
        cover = dict(empty_rays=int((kinds == 1).sum()), opaque_rays=int((kinds == 2).sum()), thin_rays=int((kinds == 3).sum()), valid=int(c.target_vd.sum()),
                     applied=int(aux["applied"].sum()), applied_v_below=int((aux["applied"] & (aux["v"] < 1e-3)).sum()),
                     applied_v_above=int((aux["applied"] & (aux["v"] > 1e-3)).sum()),
                     zero_weight_samples=int((torch.as_tensor(man["weights"]) == 0).sum()),
                     norm_min=float(c.rays_d.norm(dim=-1).min()), norm_max=float(c.rays_d.norm(dim=-1).max()))
        assert float(o64["acc_map"][kinds == 1].abs().max() if cover["empty_rays"] else 0.) == 0.
        below += cover["applied_v_below"]
        above += cover["applied_v_above"]
        b = dict(tau=tau, pool_error=pool, candidates=c.info["candidates"], rejected=c.info["rejected"], cover=cover, tensors={})
        for k in C.tensor_names(case):
            assert C.max_error(man[k], o64[k]) <= 1e-12 * max(C.top_of(o64[k]), 1e-300), (c.name, k, "manual")
            err = C.max_error(o32[k], o64[k])
            b["tensors"][k] = {"bound": C.bound_of(err, o64[k]), "fp32_error": err, "top": C.top_of(o64[k])}
            out[f"{c.name}/{k}"] = Q.summary(k, index, o64[k])
        cases[c.name] = b
        worst = max(b["tensors"].items(), key=lambda kv: kv[1]["fp32_error"] / max(kv[1]["top"], 1e-300))
        print(f"{c.name}: rejected {c.info['rejected']} of {c.info['candidates']} ({100 * share:.1f} %), cover {cover}, largest relative "
              f"fp32 error {worst[1]['fp32_error'] / max(worst[1]['top'], 1e-300):.3g} ({worst[0]})")
    assert below >= 1 and above >= 1, (below, above)
    tc = Q.case_inputs(Q.CASES[Q.NAMES.index(Q.TRAIN_CASE)], json.load(open(os.path.join(HERE, "nerf_query_bounds.json")))["cases"][Q.TRAIN_CASE]["tau"])
    l32, l64 = C.train_loop_host(tc, torch.float32), C.train_loop_host(tc, torch.float64)
    dev = [abs(a - b) for a, b in zip(l32, l64)]
    assert l64[-1] < l64[0], l64
    train = dict(case=Q.TRAIN_CASE, depth_loss_weight=C.DEPTH_LOSS_WEIGHT, losses_fp64=l64, deviation=dev, bound=C.FACTOR * max(dev))
    print(f"train: losses {l64[0]:.6g} -> {l64[-1]:.6g}, largest fp32 deviation {max(dev):.3g}")
    out["cases"] = np.array(C.NAMES)
    path = os.path.join(HERE, "nerf_composite_golden.npz")
    save_stable(path, out)
    with open(os.path.join(HERE, "nerf_composite_bounds.json"), "w") as f:
        json.dump({"factor": C.FACTOR, "f32_bit_equal": bool(f32_equal), "cases": cases, "train": train}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB; float32 checker bit-equal to the reference: {f32_equal}")


if __name__ == "__main__":
    main()
