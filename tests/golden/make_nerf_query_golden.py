"""Generate tests/golden/nerf_query.npz and nerf_query_bounds.json from the REFERENCE's data/scannet/run_nerf.py (build container
only: it reads the reference tree).

run_nerf.py is imported as make_nerf_extract_golden.py imports it.  For every case of tests/nerf_query_ref.py the reference's own
run_network runs on the checker model in float64; loss = sum(raw * cot) and torch autograd give the 24 gradients and dcam.  Only
recorded results are stored; no reference text.

nerf_query.npz          <case>/raw, and per gradient <case>/<tensor>: [sum, absolute sum, 16 entries at seeded positions], float64.
                        <case>/f32/...: the same of a float32 run of the reference, stored if the float32 checker equals it bit for
                        bit with 1 and with 16 threads (asserted here; "f32_bit_equal" in the bounds file says which).
nerf_query_bounds.json  per case: tau = 8 x the float32 checker's largest pre-activation error over a seeded pool of 1024 candidates,
                        the candidates and the rejected among them, and per tensor 8 x max |float32 checker - float64 checker| with
                        the measured error next to it; "train": per step of the eight-step Adam loop the deviation of the float32
                        from the float64 host run and 8 x the largest of them.

    python tests/golden/make_nerf_query_golden.py       rewrites both files; the same bytes on every run
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

import nerf_extract_ref as R                                # noqa: E402
import nerf_query_ref as Q                                  # noqa: E402
from make_nerf_extract_golden import reference_module       # noqa: E402
from make_scannet_golden import save_stable                 # noqa: E402

BOUND_FACTOR = 8.0


def reference_query(RN, c, dtype):
    """The reference's run_network on the checker model, and autograd of sum(raw * cot) -> {name: tensor} over raw, gradients, dcam."""
    model = R.build_model(c.state, c.cfg, dtype)
    embed_fn, _ = R.get_embedder(c.cfg["multires"], c.cfg["i_embed"])
    embeddirs_fn, _ = R.get_embedder(c.cfg["multires_views"], c.cfg["i_embed"])
    cam = (torch.zeros(0) if c.cam is None else c.cam).to(dtype).clone().requires_grad_(c.cam is not None)
    raw = RN.run_network(c.pts.to(dtype), c.viewdirs.to(dtype), cam, model, embed_fn, embeddirs_fn, torch.tensor(c.bb_center).to(dtype),
                         torch.tensor(c.bb_scale).to(dtype))
    params = dict(model.named_parameters())
    wrt = [params[k] for k in Q.PARAMS] + ([cam] if c.cam is not None else [])
    g = torch.autograd.grad((raw * c.cot.to(dtype)).sum(), wrt)
    out = dict(zip(Q.PARAMS, g), raw=raw.detach())
    if c.cam is not None:
        out["dcam"] = g[-1]
    return out


def main():
    torch.set_num_threads(1)
    RN = reference_module()
    out, cases = {}, {}
    f32_equal = True
    inputs = {}
    for index, case in enumerate(Q.CASES):
        pre_error = Q.pool_error(case)
        tau = BOUND_FACTOR * pre_error
        c = Q.case_inputs(case, tau)
        inputs[c.name] = c
        share = c.info["rejected"] / c.info["candidates"]
        assert share <= 0.10, (c.name, share)
        ref64 = reference_query(RN, c, torch.float64)
        o64, o32 = Q.check_case(c, torch.float64), Q.check_case(c, torch.float32)
        names = Q.tensor_names(c.cfg)
        b = dict(tau=tau, pre_error=pre_error, candidates=c.info["candidates"], rejected=c.info["rejected"], tensors={})
        for k in names:
            top = float(ref64[k].abs().max())
            assert float((o64[k] - ref64[k]).abs().max()) <= 1e-12 * top, (c.name, k)
            err = float((o32[k].double() - o64[k]).abs().max())
            b["tensors"][k] = {"bound": BOUND_FACTOR * err, "fp32_error": err}
            out[f"{c.name}/{k}"] = ref64[k].numpy() if k == "raw" else Q.summary(k, index, ref64[k])
        for threads in (1, 16):
            torch.set_num_threads(threads)
            ref32, chk32 = reference_query(RN, c, torch.float32), Q.check_case(c, torch.float32)
            f32_equal &= all(torch.equal(ref32[k], chk32[k]) for k in names)
        torch.set_num_threads(1)
        ref32 = reference_query(RN, c, torch.float32)
        for k in names:
            out[f"{c.name}/f32/{k}"] = ref32[k].numpy() if k == "raw" else Q.summary(k, index, ref32[k])
        cases[c.name] = b
        worst = max(b["tensors"].items(), key=lambda kv: kv[1]["fp32_error"])
        print(f"{c.name}: tau {tau:.3g}, rejected {c.info['rejected']} of {c.info['candidates']} ({100 * share:.1f} %), largest fp32 "
              f"error {worst[1]['fp32_error']:.3g} ({worst[0]})")
    if not f32_equal:
        print("the float32 checker does NOT reproduce the reference's float32 run bit for bit: nothing of it is stored")
        out = {k: v for k, v in out.items() if "/f32/" not in k}
    c = inputs[Q.TRAIN_CASE]
    l32, l64 = Q.train_loop_host(c, torch.float32), Q.train_loop_host(c, torch.float64)
    dev = [abs(a - b) for a, b in zip(l32, l64)]
    assert l64[-1] < l64[0], l64
    train = dict(case=Q.TRAIN_CASE, losses_fp64=l64, deviation=dev, bound=BOUND_FACTOR * max(dev))
    print(f"train: losses {l64[0]:.6g} -> {l64[-1]:.6g}, largest fp32 deviation {max(dev):.3g}")
    out["cases"] = np.array(Q.NAMES)
    path = os.path.join(HERE, "nerf_query.npz")
    save_stable(path, out)
    with open(os.path.join(HERE, "nerf_query_bounds.json"), "w") as f:
        json.dump({"factor": BOUND_FACTOR, "f32_bit_equal": bool(f32_equal), "cases": cases, "train": train}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB; float32 checker bit-equal to the reference: {f32_equal}")


if __name__ == "__main__":
    main()
