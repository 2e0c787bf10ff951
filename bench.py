#!/usr/bin/env python
"""Throughput bench of the RPN hot path on MI355X.

  python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run, one rank per GPU)
  python bench.py ... --full                           (also every secondary measurement, see below)
  python bench.py ... --dump-outputs DIR               (also write what the last timed step computed, DIR/<name>.npy)

One "step" = one full training pass of the hot path over one synthetic scene per rank: 160^3 x 4 rgb-sigma grid ->
VGG19-3D + FPN + RPN head forward, target assignment, sampled losses, backward, bucketed RCCL gradient all-reduce,
fused clip + AdamW.  Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line with the
BASELINE.json metric (scenes/sec) and `ms_per_step`.  A plain run sets up, warms up, times K steps and prints that line.
With --full it also carries a `roofline` object for the dominant kernel (HIP events inside the timed region), the host
enqueue figures, the secondary measurements (`--no-extras` drops them), the comm-only exchange table (N > 1) and a
`cpu_baseline` object (the oracle, timed on the host cores on a bounded sample; `--no-cpu-baseline` drops it).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # the host driver only supports dmabuf IPC (RCCL between the ranks of a node)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

GRID = 160
NUM_GT = 16
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}      # dense peaks, /opt/skills/guides/MI355X_MICROARCH.md


def synthetic_scene(seed, device):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(4, GRID, GRID, GRID, generator=g)
    g1 = torch.Generator().manual_seed(seed + 1000)
    ctr = torch.rand(NUM_GT, 3, generator=g1) * 120 + 20
    size = torch.rand(NUM_GT, 3, generator=g1) * 40 + 8
    theta = (torch.rand(NUM_GT, 1, generator=g1) - 0.5) * math.pi
    return x.to(device), torch.cat([ctr, size, theta], dim=1).to(device)


def build_backbone(kind):
    from nerf_rpn_amd.model import VGG_FPN, ResNet_FPN_256, Bottleneck, SwinTransformer_FPN
    if kind == "vgg":
        return VGG_FPN("EF", 4, True, GRID)
    if kind == "resnet":
        return ResNet_FPN_256(Bottleneck, [3, 4, 6, 3], input_dim=4, is_max_pool=True)
    return SwinTransformer_FPN(patch_size=[4, 4, 4], embed_dim=96, depths=[2, 2, 18, 2], num_heads=[3, 6, 12, 24], window_size=[4, 4, 4],
                               stochastic_depth_prob=0.1 if kind == "swin" else 0.0, expand_dim=True)


def build_fcos(dtype, device, backbone):
    """Secondary workload (not the BASELINE metric): train_fcos.sh configuration, Swin-S + FCOS head, OBB."""
    from nerf_rpn_amd.model.fcos import FCOSOverNeRF
    torch.manual_seed(0)
    a = argparse.Namespace(num_convs=4, norm_reg_targets=True, centerness_on_reg=True, rotated_bbox=True, pre_nms_thresh=0.0,
                           pre_nms_top_n=2500, nms_thresh=0.3, fpn_post_nms_top_n=2500, min_size=0.0, center_sampling_radius=1.5,
                           iou_loss_type="iou", use_additional_l1_loss=False, proj2d_loss_weight=0.0)
    return FCOSOverNeRF(a, build_backbone(backbone), [4, 8, 16, 32], compute_dtype=dtype).to(device).train()


def build_model(dtype, device, backbone="vgg"):
    from nerf_rpn_amd import ops
    from nerf_rpn_amd.model import RPNHead, NeRFRegionProposalNetwork, AnchorGenerator3D
    torch.manual_seed(0)
    bb = build_backbone(backbone)
    hd = RPNHead(256, 13, 4, rotate=True)
    model = NeRFRegionProposalNetwork(bb, AnchorGenerator3D(ops.ANCHOR_SIZES, ops.ASPECT_RATIOS), hd, rpn_pre_nms_top_n_train=2500,
                                      rpn_pre_nms_top_n_test=2500, rpn_post_nms_top_n_train=2500, rpn_post_nms_top_n_test=2500,
                                      rpn_nms_thresh=0.3, rpn_fg_iou_thresh=0.35, rpn_bg_iou_thresh=0.2, rpn_batch_size_per_mesh=256,
                                      rpn_positive_fraction=0.5, rotated_bbox=True, reg_loss_type="smooth_l1", compute_dtype=dtype)
    model.rpn.loss_2d_requires_grad = False     # reg_loss_weight_2d = 0 (run_rpn.py default); the value is still computed
    return model.to(device).train()


class ConvProbe:
    """HIP-event timing of every conv launch on the stream it is enqueued on (torch's current stream == the stream handed to
    the C ABI).  Used for the `roofline` object: algorithmic FLOPs of a launch / its measured duration."""

    def __init__(self):
        from nerf_rpn_amd import lib
        self.lib = lib
        self.records = []
        self.breakdown = None     # records of the untimed breakdown pass (every heavy launch class), see main()
        self.only = None          # (call, shape): restrict the events of the TIMED region to the dominant kernel's launches
        self.enabled = False
        self._orig = lib.call

    def install(self):
        orig = self._orig

        def call(name, *args):
            if not self.enabled or name not in ("conv3d_fwd", "conv3d_fwd_ex", "conv3d_fwd_stats", "conv3d_wgrad"):
                return orig(name, *args)
            called, name = name, ("conv3d_fwd" if name in ("conv3d_fwd_stats", "conv3d_fwd_ex") else name)     # same kernels, same leading arguments
            n_, gx_, gy_, gz_, cin_, _, wrows_, k_ = args[4:12]
            if 2.0 * n_ * gx_ * gy_ * gz_ * cin_ * wrows_ * (k_ ** 3) < 1e10:     # only the heavy launches (>= 10 GFLOP) are timed
                return orig(called, *args)
            if self.only is not None and ((name, (n_ * gx_ * gy_ * gz_, cin_, wrows_, k_)) != self.only or self.ops.IN_BACKWARD[0]):
                # timed region: forward-pass launches of the dominant kernel only; its
                # dgrad launches share the GPU with the weight-gradient side stream, so their wall time is not a kernel duration
                return orig(called, *args)
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            rc = orig(called, *args)
            b.record()
            if name == "conv3d_fwd":
                n, gx, gy, gz, cin, cout, wrows, k = args[4:12]
            else:
                n, gx, gy, gz, cin, cout, wrows, k = args[4:12]
            flops = 2.0 * n * gx * gy * gz * cin * wrows * (k ** 3)
            self.records.append((name, (n * gx * gy * gz, cin, wrows, k), flops, a, b))
            return rc
        self.lib.call = call
        import nerf_rpn_amd.ops as ops
        ops.call = call
        self.ops = ops

    def summary(self, dtype_name):
        def group(records):
            by = {}
            for name, shape, flops, a, b in records:
                e = by.setdefault((name, shape), [0, 0.0, flops])
                e[0] += 1
                e[1] += a.elapsed_time(b)
            return sorted(((k, v) for k, v in by.items()), key=lambda kv: -kv[1][1])
        timed = group(self.records)
        if not timed:
            return None, []
        rows = group(self.breakdown) if self.breakdown else timed
        (name, shape), (cnt, ms, flops) = timed[0]      # the dominant kernel: its events were recorded inside the timed region
        avg_ms = ms / cnt
        achieved = flops / (avg_ms * 1e-3) / 1e12
        peak = MFMA_PEAK_TFLOPS[dtype_name]
        total_ms = sum(v[1] for _, v in rows)
        total_fl = sum(v[0] * v[2] for _, v in rows)
        vox, cin_, cout_, _k = shape
        code = self.lib.BF16 if dtype_name == "bf16" else self.lib.F32
        if name == "conv3d_fwd":     # ask the library which kernel launch_conv selects for this shape
            g = round(vox ** (1.0 / 3.0))
            dims = (g, g, g) if g ** 3 == vox else (vox, 1, 1)        # the bench grids are cubes: the plan depends on the grid, not only on M
            plan = self.lib.query("conv3d_fwd_plan", 1, *dims, cin_, cout_, _k, code)
            kernel = {0: "conv_igemm_kernel", 1: "conv_igemm_big_kernel", 2: "conv_igemm_big_kernel (K slices)",
                      3: "conv_igemm_kernel (K slices)", 4: "conv_igemm_ws_kernel", 5: "conv_igemm_big4_kernel", 6: "conv_igemm_big4_kernel (K slices)",
                      7: "conv_halo_kernel"}[plan]
        else:
            kernel = "conv_wgrad_big_kernel" if self.lib.query("conv3d_wgrad_plan", 1, vox, 1, 1, cin_, cout_, cout_, _k, code) else "conv_wgrad_kernel"
        es = 2 if dtype_name == "bf16" else 4
        algo_bytes = vox * cin_ * es + vox * cout_ * es + (_k ** 3) * cin_ * cout_ * es      # x + y + w, each once
        traffic, note = None, "no PMC collection for this kernel in profiles/ (null = not measured)"
        for pmc_name in ("r06_pmc_conv_256x256_40c.json", "r05_pmc_conv_256x256_40c.json", "r04_pmc_conv_256x256_40c.json", "r03_pmc_conv_256x256_40c.json",
                         "r02_pmc_conv_256x256_40c.json"):
            pmc = os.path.join(ROOT, "profiles", pmc_name)
            if not (os.path.exists(pmc) and shape == (64000, 256, 256, 3)):
                continue
            d = json.load(open(pmc))
            base = kernel.split(" ")[0]          # the counter file keys carry template arguments ("conv_halo_kernel<0>")
            cands = [(name, v) for name, v in d.get("kernels", {}).items() if name.split("<")[0] == base]
            # several instantiations of the halo kernel are profiled (K orders, fp32 rows): the one this shape runs by default pairs taps
            # across chunk boundaries (Cin >= 256) and stores bf16 rows = conv_halo_kernel<0, true, false>
            prod = [v for name, v in cands if name.replace(" ", "").endswith("<0,true,false>")]
            k = prod[0] if prod else (cands[0][1] if cands else None)
            if not (k and k.get("hbm_bytes") is not None):
                continue
            # the counters describe the kernel SOURCE they were collected on: a newer conv3d.hip makes them stale, and stale is null
            if d.get("conv_source_sha16") == conv_source_hash():
                traffic, note = k["hbm_bytes"], f"{pmc_name} (conv3d.hip sha16 {d['conv_source_sha16']}): " + d.get("method", "")
            else:
                note = (f"{pmc_name} was collected on conv3d.hip sha16 {d.get('conv_source_sha16', 'unrecorded')}, the tree runs "
                        f"{conv_source_hash()}: stale counters are not reported (null)")
            break
        roof = {"bound": "mfma", "kernel": kernel,
                "shape": {"voxels": shape[0], "cin": shape[1], "cout": shape[2], "k": shape[3]}, "launches": cnt,
                "avg_ms": round(avg_ms, 4), "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_note": note, "algorithmic_bytes": algo_bytes,
                "timed_heavy_launches": {"tflops": round(total_fl / (total_ms * 1e-3) / 1e12, 2), "ms_per_step": None}}
        # per (call, shape) breakdown of every timed conv launch class: launches per step are filled in by main()
        roof["conv_breakdown"] = [{"call": k[0], "voxels": k[1][0], "cin": k[1][1], "cout": k[1][2], "k": k[1][3], "launches": v[0],
                                   "avg_us": round(1e3 * v[1] / v[0], 1), "tflops": round(v[2] / (v[1] / v[0] * 1e-3) / 1e12, 1)} for k, v in rows]
        return roof, rows


# Algorithmic work of one 160^3 scene: FLOPs = 2 * MACs of every conv; bytes = each activation read
# once per consumer and written once, weights once, BN/ReLU fused.
FWD_VGG_FPN_GFLOP = 1713.2
FWD_VGG_FPN_GB = {"bf16": 0.974, "f32": 1.947}
STEP_GFLOP = 8168.0
HBM_PEAK_GBS = 8000.0
BREAKDOWN_STEPS = 3


def forward_only(model, x, dtype_name, iters=10):
    """VGG19-3D + FPN forward alone (north_star's forward roofline): eval-mode backbone on the resident scene, HIP events."""
    was = model.training
    model.eval()
    with torch.no_grad():
        for _ in range(3):
            model.backbone(x.unsqueeze(0))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            model.backbone(x.unsqueeze(0))
        b.record()
        torch.cuda.synchronize()
    model.train(was)
    ms = a.elapsed_time(b) / iters
    tf = FWD_VGG_FPN_GFLOP / ms            # GFLOP / ms = TFLOP/s
    gbs = FWD_VGG_FPN_GB[dtype_name] / (ms * 1e-3)
    return {"ms": round(ms, 3), "scenes_per_s": round(1e3 / ms, 2), "gflop": FWD_VGG_FPN_GFLOP, "tflops": round(tf, 1),
            "mfma_frac": round(tf / MFMA_PEAK_TFLOPS[dtype_name], 4), "algorithmic_gb": FWD_VGG_FPN_GB[dtype_name],
            "hbm_gbs": round(gbs, 1), "hbm_frac": round(gbs / HBM_PEAK_GBS, 4),
            "hbm_frac_ceiling": 0.18 if dtype_name == "bf16" else None,
            "note": "MFMA-bound (1760 FLOP/B bf16 >> ridge 310): the whole-forward HBM fraction cannot exceed ~18 % even at 100 % "
                    "of the dense MFMA peak (SURVEY 8d); eval-mode BatchNorm (running statistics)"}


def hbm_stages(dtype, dev):
    """Achieved HBM GB/s of the HBM-bound kernels of the step, each on its largest shape in the 160^3 VGG19 configuration (fresh
    buffers, 20 back-to-back launches between HIP events; bytes = algorithmic: every operand read / written once)."""
    from nerf_rpn_amd import lib, ops
    es = 2 if dtype == torch.bfloat16 else 4
    out = []

    def timed(name, shape, nbytes, fn, iters=20):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = 1e3 * a.elapsed_time(b) / iters
        gbs = nbytes / (us * 1e-6) / 1e9
        out.append({"kernel": name, "shape": shape, "bytes": int(nbytes), "avg_us": round(us, 1), "gbs": round(gbs, 1),
                    "frac": round(gbs / HBM_PEAK_GBS, 4)})

    def P(t):
        return t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    for rows, c in ((80 ** 3, 64), (40 ** 3, 256)):
        x = torch.randn(rows, c, device=dev).to(dtype)
        y, dy, dx = torch.empty_like(x), torch.randn(rows, c, device=dev).to(dtype), torch.empty_like(x)
        mean, var = torch.empty(c, device=dev), torch.empty(c, device=dev)
        g, bta = torch.ones(c, device=dev), torch.zeros(c, device=dev)
        dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
        ws = torch.empty(lib.query("bn_workspace_bytes", rows, c), dtype=torch.uint8, device=dev)
        code = ops._dt(x)
        timed("bn_stats", f"{c}@{rows}", rows * c * es, lambda: lib.call("bn_stats", P(x), rows, c, code, P(mean), P(var), 0, 0, 0.1, P(ws), st))
        timed("bn_apply+relu", f"{c}@{rows}", 2 * rows * c * es,
              lambda: lib.call("bn_apply", P(x), P(y), rows, c, code, P(mean), P(var), P(g), P(bta), 1e-5, 1, st))
        timed("bn_backward", f"{c}@{rows}", 5 * rows * c * es,
              lambda: lib.call("bn_backward", P(x), 0, P(dy), P(dx), rows, c, code, P(mean), P(var), P(g), P(bta), 1e-5, 1, P(dg), P(db), 0, 0,
                               P(ws), st))
    for (gx, c, k, s_, p_, ceil) in ((80, 64, 3, 2, 1, 0), (40, 256, 2, 2, 0, 1)):
        x = torch.randn(1, gx, gx, gx, c, device=dev).to(dtype)
        o = lib.query("pool_out_size", gx, k, s_, p_, ceil)
        y = torch.empty(1, o, o, o, c, device=dev, dtype=dtype)
        arg = torch.empty(y.shape, dtype=torch.int8, device=dev)
        dx = torch.empty_like(x)
        code = ops._dt(x)
        timed("maxpool3d_fwd", f"{c}@{gx}^3 k{k}s{s_}", x.numel() * es + y.numel() * (es + 1),
              lambda: lib.call("maxpool3d_fwd", P(x), P(y), P(arg), 1, gx, gx, gx, c, k, s_, p_, ceil, code, st))
        timed("maxpool3d_bwd", f"{c}@{gx}^3 k{k}s{s_}", x.numel() * es + y.numel() * (es + 1),
              lambda: lib.call("maxpool3d_bwd", P(y), P(arg), P(dx), 1, gx, gx, gx, c, k, s_, p_, ceil, code, st))
    fine = torch.randn(1, 40, 40, 40, 256, device=dev).to(dtype)
    coarse = torch.randn(1, 20, 20, 20, 256, device=dev).to(dtype)
    code = ops._dt(fine)
    timed("upsample_add_fwd", "256@40^3 += 256@20^3", 2 * fine.numel() * es + coarse.numel() * es,
          lambda: lib.call("upsample_add_fwd", P(fine), P(coarse), 1, 40, 40, 40, 20, 20, 20, 256, code, st))
    timed("upsample_add_bwd", "256@40^3 -> 256@20^3", fine.numel() * es + coarse.numel() * es,
          lambda: lib.call("upsample_add_bwd", P(fine), P(coarse), 1, 40, 40, 40, 20, 20, 20, 256, code, 0, st))
    n = 74_815_925
    pa, ga, m, v = (torch.zeros(n, device=dev) for _ in range(4))
    ga.normal_()
    ss = torch.zeros(lib.query("grad_sumsq_floats"), device=dev)
    timed("grad_sumsq", f"{n} f32", 4 * n, lambda: ops.grad_sumsq(ga, ss, 1.0))
    timed("adamw_step", f"{n} f32 (p,m,v rw + g r)", 28 * n, lambda: ops.adamw_step(pa, ga, m, v, ss, 0.1, 1e-4, (0.9, 0.999), 1e-8, 0.01, 1))
    slices = lib.query("conv3d_wgrad_slices", 1, 40, 40, 40, 256, 256, 256, 3, ops._dt(fine))
    gwp = torch.randn(slices, 27, 256, 256, device=dev)
    gw = torch.zeros(256, 256, 27, device=dev)
    timed("unpack_conv_wgrad", f"256x256x27, {slices} slices -> arena (+=)", (slices + 2) * 27 * 256 * 256 * 4,
          lambda: lib.call("unpack_conv_wgrad", P(gwp), 256, 256, 27, 256, 0, P(gw), 1, slices, st))
    return out


def cpu_baseline(budget_s=60.0):
    """The oracle (CPU restatement of the reference, torch fp32 on the host cores): fwd+bwd of the same 160^3 scene.  Bounded sample: with
    every host core, warm-up passes then up to three timed passes inside ``budget_s`` (always at least one warm-up + one timed pass);
    then the same with 8 threads (the reference was timed on 8 cores in the build container: 19.1 s) -- one warm-up + up to
    two timed passes inside the same budget."""
    from oracle import nets as ON, rpn as OR
    torch.manual_seed(0)
    bb, hd = ON.VGGFPN("EF", 4, GRID), ON.RPNHead(256, 13, 4, True)
    det = OR.Detector(bb, OR.RPN(hd, rotated=True))
    bb.train()
    x, gt = synthetic_scene(0, "cpu")

    def one():
        for p in list(bb.parameters()) + list(hd.parameters()):
            p.grad = None
        t0 = time.time()
        _, losses, _, _ = det([x], [gt], training=True)
        (losses["loss_objectness"] + 5.0 * losses["loss_rpn_box_reg"]).backward()
        return time.time() - t0

    def run(threads, warm_max, timed_max):
        torch.set_num_threads(threads)
        start, warm, timed = time.time(), [one()], []
        while len(warm) < warm_max and time.time() - start + 2 * warm[-1] < budget_s / 2:
            warm.append(one())
        timed.append(one())
        while len(timed) < timed_max and time.time() - start + timed[-1] < budget_s:
            timed.append(one())
        return warm, timed

    all_cores = torch.get_num_threads()
    runs = {}
    for threads, warm_max, timed_max in ((all_cores, 2, 3), (32, 1, 2), (8, 1, 2)):
        if threads > all_cores or threads in runs:
            continue
        warm, timed = run(threads, warm_max, timed_max)
        runs[threads] = {"value": round(len(timed) / sum(timed), 5), "unit": "scenes/sec", "cores": threads, "warmup_s": [round(t, 2) for t in warm],
                         "passes_s": [round(t, 2) for t in timed]}
    torch.set_num_threads(all_cores)
    best = max(runs.values(), key=lambda r: r["value"])      # the oracle's best thread count on this host (oversubscription hurts torch's CPU convs)
    return {"value": best["value"], "unit": "scenes/sec", "cores": best["cores"], "kind": "port",
            "sample": f"fwd+bwd of one {GRID}^3x4 scene (VGG19-EF+FPN+RPN, OBB, fp32, no optimiser step): per thread count 1-2 warm-up + 2-3 timed "
                      f"passes, mean, each bounded to ~{budget_s:.0f} s; value = the best thread count ({best['cores']} of {all_cores} host threads)",
            "by_threads": {str(k): v for k, v in sorted(runs.items())}}


def eval_forward_protocol(dtype_name, dev, iters=20, warm=3):
    """The reference's own benchmark protocol (run_rpn.py:594-617, --mode benchmark): eval forwards of VGG19-EF + FPN + RPN on a
    200 x 200 x 130 grid INCLUDING decode / top-k / filter / NMS (random-init weights; the reference runs 300, here ``iters`` after
    ``warm`` warm-ups).  Host wall time per forward (the proposal count is read back every forward, as in the product path)."""
    dtype = torch.bfloat16 if dtype_name == "bf16" else torch.float32
    model = build_model(dtype, dev).eval()
    x = torch.randn(4, 200, 200, 130, generator=torch.Generator().manual_seed(0)).to(dev)        # the reference feeds randn
    with torch.no_grad():
        for _ in range(warm):
            model([x])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            (_, props, _), _, _ = model([x])
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / iters
    return {"shape": [200, 200, 130], "dtype": dtype_name, "iters": iters, "ms": round(ms, 3), "proposals": int(props[0].shape[0]),
            "note": "eval forward incl. decode / top-k / NMS at the reference's benchmark shape (run_rpn.py:594-617)"}


def make_step_for(model_, trainer_, xs_, gts_, fcos):
    def step():
        _, losses, _ = model_(xs_, gts_)
        if fcos:
            loss = losses["loss_cls"] + losses["loss_reg"] + losses["loss_centerness"]
        else:
            loss = losses["loss_objectness"] + 5.0 * losses["loss_rpn_box_reg"] + 0.0 * losses["loss_rpn_box_reg_2d"]
        loss.backward()
        trainer_.step()
        return loss
    return step


def secondary_workloads(dtype, dev, xs, gts, make, steps=12):
    """The other BASELINE.json configurations on the same 160^3 scene, in the same invocation (bounded: ``steps`` timed steps each, after the
    headline's timed region): ResNet-50 + RPN (configs[2] / [4]), Swin-S + RPN, Swin-S + FCOS (configs[3]).  Trunk graphs as `--graph auto`
    chooses them (Swin-S: captured; ResNet-50: eager).  Not the BASELINE metric."""
    from nerf_rpn_amd import ops as _o
    from nerf_rpn_amd.engine import FlatTrainer
    out = {}
    def measure(m, tr, g, fcos, warm):
        st = make(m, tr, xs, g, fcos)
        for _ in range(warm):                  # eager: 3 warm-ups; graph: 2 eager warm-ups + the capture + replays
            st()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            loss = st()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t1) / steps
        cnt = [0]
        orig = _o.call

        def counting(nm, *a):
            cnt[0] += 1
            return orig(nm, *a)
        _o.call = counting
        enq = []
        for _ in range(4):
            torch.cuda.synchronize()
            th = time.perf_counter()
            st()
            enq.append(time.perf_counter() - th)
        torch.cuda.synchronize()
        _o.call = orig
        enq.sort()
        return {"ms_per_step": round(ms, 3), "scenes_per_s": round(1e3 / ms, 2), "steps": steps, "trunk_hip_graph": bool(m.use_graph),
                "host_enqueue_ms_per_step": round(1e3 * enq[len(enq) // 2], 3), "c_abi_calls_per_step": round(cnt[0] / 4, 1),
                "final_loss": round(float(loss.detach()), 5)}

    for name in ("resnet_rpn", "swin_rpn", "swin_fcos"):
        backbone, head = name.split("_")
        fcos = head == "fcos"
        try:
            m = build_fcos(dtype, dev, "swin0" if backbone == "swin" else backbone) if fcos else build_model(dtype, dev, backbone)
            m.use_graph = backbone == "swin"
            tr = FlatTrainer(m, lr=1e-4, weight_decay=0.01, clip_grad_norm=0.1, total_steps=4 * steps + 64)
            g = gts           # host tensors, as the reference's loader yields them (both model families upload them on their target stream)
            res = measure(m, tr, g, fcos, 5 if m.use_graph else 3)
            if not m.use_graph and res["host_enqueue_ms_per_step"] >= 0.9 * res["ms_per_step"]:
                # the eager step sits on the host's enqueue rate on this box (ResNet-50: ~500 C-ABI calls per step): the trunk as captured HIP
                # graphs (bit-identical, graphs.py) is the configuration for such a host -- both are reported, `ms_per_step` is the better one
                m.use_graph = True
                captured = measure(m, tr, g, fcos, 5)
                res = {**(captured if captured["ms_per_step"] < res["ms_per_step"] else res), "eager": res, "captured_trunk": captured,
                       "note": "eager step host-bound on this box (enqueue >= 0.9 x step): also measured with the trunk as captured HIP graphs"}
            out[name] = res
            del m, tr
        except Exception as e:                  # a secondary workload must never take the headline line down with it
            out[name] = {"error": f"{type(e).__name__}: {str(e)[:300]}"}
        torch.cuda.empty_cache()
    return out


def measured_ceiling():
    """What the MFMA array sustains at the part's power cap on the operands the conv layers multiply (tools/mfma_peak_probe.py: a
    register-only v_mfma_f32_32x32x16_bf16 loop, post-ReLU activations x small weights) -- profiles/r04_mfma_ceiling.json."""
    path = os.path.join(ROOT, "profiles", "r06_mfma_ceiling.json")      # re-measured in round 6 (tools/mfma_peak_probe.py); round 4's otherwise
    if not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", "r04_mfma_ceiling.json")
    if not os.path.exists(path):
        return None
    rows = json.load(open(path)).get("rows", [])
    pick = [r for r in rows if r.get("operands") == "relu_randn_x_w0.05" and r.get("waves_per_simd") == 2]
    if not pick:
        return None
    r = pick[0]
    return {"tflops": r["tflops"], "power_w": r["power_w"], "sclk_mhz": r["sclk_mhz"], "source": "profiles/" + os.path.basename(path)}


def conv_source_hash():
    import hashlib
    h = hashlib.sha256()
    for f in ("conv3d.hip", "conv_halo.hip", "conv_common.cuh", "common.h"):
        h.update(open(os.path.join(ROOT, "nerf_rpn_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


DUMP_SAMPLE = 1 << 21      # elements kept of an array larger than this (a fixed, seeded sample): < 64 MB for all files together


def dump_outputs(path, last, trainer):
    """What the last timed step handed back to its caller -> ``path/<name>.npy`` (float32): the loss and each loss term, the FPN
    feature maps (logical NCDHW order) and the parameters after the optimiser step (logical order, ``FlatTrainer.flat_params``).
    Arrays above DUMP_SAMPLE elements are sampled at indices drawn from a generator seeded by the array's name and size, so two
    runs (or two builds) with the same arguments write the same elements of the same inputs."""
    import zlib
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {"loss": last["loss"]}
    arrays.update({k: v for k, v in last["losses"].items() if isinstance(v, torch.Tensor)})
    feats = last["outs"][0] if isinstance(last["outs"], (list, tuple)) and last["outs"] else None
    if isinstance(feats, (list, tuple)):
        arrays.update({f"features_{i}": f for i, f in enumerate(feats) if isinstance(f, torch.Tensor)})
    arrays["params"] = trainer.flat_params()
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        if flat.numel() > DUMP_SAMPLE:
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + flat.numel())
            idx = torch.randint(0, flat.numel(), (DUMP_SAMPLE,), generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        np.save(os.path.join(path, name + ".npy"), flat.float().cpu().numpy())


def _compact(obj):
    """The JSON line without its prose: every "note" is dropped (DESIGN.md section 4 says what each field is; --notes keeps them) and the
    traffic note is cut to its first clause.  VERDICT r5: the driver's record of the line lost `host` / `rpn_head_cone` to the length."""
    if isinstance(obj, dict):
        return {k: (v[:140] if k == "traffic_note" and isinstance(v, str) else (v.split(" (")[0] if k == "mode_chosen_by" else _compact(v)))
                for k, v in obj.items() if k not in ("note", "what")}
    if isinstance(obj, list):
        return [_compact(v) for v in obj]
    return obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)      # ~1.2 s of timed region (10 steps were 0.12 s: invisible to a GPU-busy sampler)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--full", action="store_true",
                    help="run every measurement beyond the headline too: conv launch timing + roofline, host enqueue, secondary measurements, "
                         "the comm-only exchange table (N > 1) and the CPU baseline (the --no-* options below drop parts of it)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (losses, FPN features, updated parameters; a fixed "
                         "seeded sample of the larger arrays) as DIR/<name>.npy, float32, rank 0")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-probe", action="store_true", help="disable per-launch HIP-event timing of the conv kernels")
    ap.add_argument("--no-extras", action="store_true", help="skip the secondary measurements (fp32 step, eval protocol, 2 scenes per GPU)")
    ap.add_argument("--notes", action="store_true", help="keep the explanatory 'note' strings in the JSON line (dropped by default: DESIGN.md section 4)")
    ap.add_argument("--scenes-per-gpu", type=int, default=1, help="per-rank batch of the TIMED region (1 = the BASELINE metric; 2 = the reference's train.sh setting)")
    ap.add_argument("--exchange", default=None, choices=["auto", "allreduce", "rs_ag", "a2a_bf16"],
                    help="gradient exchange of the trainer (N > 1); default auto = the fastest fp32 mode of the comm-only measurement at start-up")
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off", "fwd"],
                    help="backbone + FPN forward / backward as captured HIP graphs (nerf_rpn_amd/graphs.py): auto = for the Swin-S and ResNet-50 backbones, "
                         "whose eager steps are bound by the host's enqueue rate; the VGG19 step (the BASELINE metric) is GPU-bound and stays eager")
    ap.add_argument("--model", default="vgg_rpn", choices=["vgg_rpn", "resnet_rpn", "swin_rpn", "swin_fcos", "vgg_fcos"],
                    help="vgg_rpn = the BASELINE.json metric (default); the others are secondary workloads for profiling")
    args = ap.parse_args()
    if not args.full:       # a plain run measures the headline figure and nothing else
        args.no_probe = args.no_extras = args.no_cpu_baseline = True

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start N ranks (one per GPU) over RCCL ourselves
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from nerf_rpn_amd.affinity import pin_rank
    pin = pin_rank(local, int(os.environ.get("LOCAL_WORLD_SIZE", world)))      # ranks > 1: own cores next to the GPU's NUMA node (NRPN_PIN=0: off)
    # NRPN_FORCE_EXCHANGE=1: a one-rank RCCL process group with the trainer's exchange machinery switched on -- the multi-GPU code path
    # of this file and of engine.FlatTrainer (buckets, launch stream, collectives, the prints) on a single-GPU box (tests only)
    dist_on = world > 1 or os.environ.get("NRPN_FORCE_EXCHANGE") == "1"
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(sk.getsockname()[1]))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=dev)
    from nerf_rpn_amd import lib
    from nerf_rpn_amd.engine import FlatTrainer
    lib.call("check_device", local)
    # tuning experiments (not part of the measured configuration unless stated in the output): kernel-selection knobs from the environment
    knobs = {}
    for env, fn in (("NRPN_CONV_TILE_M", "set_conv_tile_m"), ("NRPN_CONV_BIG_SPLIT", "set_conv_big_split"), ("NRPN_WGRAD_BIG", "set_wgrad_big_tile"),
                    ("NRPN_CONV_STAGGER", "set_conv_stagger"), ("NRPN_ROWS_BIG", "set_rows_big_tile"), ("NRPN_ROWS_TAIL", "set_rows_tail_split"), ("NRPN_BN_FAST", "set_bn_fast"),
                    ("NRPN_WGRAD_PACK2", "set_wgrad_pack2"), ("NRPN_POOL_FAST", "set_pool_fast"), ("NRPN_GN_FAST", "set_gn_fast"),
                    ("NRPN_HALO_AUTO", "set_conv_halo_auto")):      # tools-only process defaults (A/B runs); the measured configuration sets none
        if env in os.environ:
            lib.call(fn, int(os.environ[env]))
            knobs[env] = int(os.environ[env])

    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    backbone, head = args.model.split("_")
    fcos = head == "fcos"
    model = build_fcos(dtype, dev, "swin0" if backbone == "swin" else backbone) if fcos else build_model(dtype, dev, backbone)
    # auto: the backbones whose eager step sits on the host's enqueue rate (round 5, same box: ResNet-50+RPN 13.0 ms eager with 13.1 ms of
    # enqueue -> 10.6 ms captured; Swin-S 23.6 -> 15-16 ms); the VGG19 step is GPU-bound and 4-6 % SLOWER captured (9.17 / 9.47 vs 9.73 / 9.83)
    use_graph = args.graph == "on" or (args.graph == "auto" and backbone in ("swin", "resnet"))
    if args.graph == "fwd":
        use_graph = "fwd"       # forward captured, backward eager (graphs.GraphedBackbone backward="eager")
    if os.environ.get("NRPN_GRAPH") in ("0", "1"):
        use_graph = os.environ["NRPN_GRAPH"] == "1"
    model.use_graph = use_graph
    trainer = FlatTrainer(model, lr=1e-4, weight_decay=0.01, clip_grad_norm=0.1, total_steps=args.steps + args.warmup + 1 + 64,
                          exchange=args.exchange)
    spg = max(1, args.scenes_per_gpu)
    scenes = [synthetic_scene(rank * spg + i, dev) for i in range(spg)]       # every rank (and every scene of a rank) its own grid
    xs = [sc[0] for sc in scenes]
    x, gt = scenes[0]
    probe = ConvProbe()
    if not args.no_probe:
        probe.install()
        if backbone == "vgg" and spg == 1:
            # inside the timed region only the dominant kernel's launches carry HIP events (two event records per launch cost ~8 us of
            # stream time: on all ~60 heavy launches of a step that was 0.5 ms of the step being measured); the per-class table of all
            # heavy launches comes from BREAKDOWN_STEPS extra, untimed steps afterwards
            probe.only = ("conv3d_fwd", (64000, 256, 256, 3))

    # the scene grids are resident in HBM; the ground-truth boxes (NUM_GT x 7 floats) are handed over as host tensors, as the reference's
    # loader does -- the RPN uploads them on its target-preparation stream (nerf_rpn.py forward)
    gts = [sc[1].cpu() for sc in scenes]

    keep = [None]       # --dump-outputs: a dict here makes the next step leave what it computed in it

    def make_step(model_, trainer_, xs_, gts_):
        def step():
            outs, losses, _ = model_(xs_, gts_)
            if fcos:
                loss = losses["loss_cls"] + losses["loss_reg"] + losses["loss_centerness"]
            else:
                loss = losses["loss_objectness"] + 5.0 * losses["loss_rpn_box_reg"] + 0.0 * losses["loss_rpn_box_reg_2d"]
            loss.backward()
            trainer_.step()
            if keep[0] is not None:
                keep[0].update(outs=outs, losses=losses, loss=loss)
            return loss
        return step
    step = make_step(model, trainer, xs, gts)

    for _ in range(args.warmup):
        step()
    if dist_on:
        dist.barrier()
        if args.full:
            trainer.exchange_events = []
    torch.cuda.synchronize()
    probe.enabled = not args.no_probe
    from nerf_rpn_amd import ops as _ops0
    side_stream = _ops0._WGRAD_SIDE["enabled"]
    packs0 = _ops0.PACK_COUNT["conv"] + _ops0.PACK_COUNT["stem"]
    last = {}
    t0 = time.perf_counter()
    for i in range(args.steps):
        if args.dump_outputs and i == args.steps - 1:
            keep[0] = last
        loss = step()
    keep[0] = None
    torch.cuda.synchronize()
    own_elapsed = time.perf_counter() - t0          # this rank's own K steps (before the closing barrier)
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    probe.enabled = False
    from nerf_rpn_amd import ops as _ops
    packs_per_step = (_ops.PACK_COUNT["conv"] + _ops.PACK_COUNT["stem"] - packs0) / args.steps
    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    per_rank_ms, exch = [round(1e3 * own_elapsed / args.steps, 3)], None
    if dist_on:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ev = trainer.exchange_events or []      # recorded by --full runs only
        wait_ms = sum(a.elapsed_time(b) for a, b in ev) / max(1, len(ev))
        trainer.exchange_events = None
        mine = torch.tensor([1e3 * own_elapsed / args.steps, wait_ms], device=dev, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank_ms = [round(v[0].item(), 3) for v in allr]
        if args.full:
            # comm-only arm: every exchange mode x bucket size on the real arena with no compute in flight (the start-up measurement of
            # exchange='auto', or taken here when a mode was forced), next to the wait the training steps actually saw
            startup = dict(trainer.exchange_table) if trainer.exchange_table else None
            table = trainer.measure_exchange()       # the full table (every mode x bucket size); start-up times only the candidates of 'auto'
            exch = {"mode": trainer.exchange, "mode_chosen_by": "comm-only measurement at start-up (fastest of the fp32 modes x 16/32/64 MiB; pin with NRPN_GRAD_EXCHANGE / NRPN_GRAD_BUCKET_MIB)" if startup else "--exchange / NRPN_GRAD_EXCHANGE",
                    **({"startup_comm_only_ms": {f"{m}@{mib}MiB": v for (m, mib), v in sorted(startup.items())}} if startup else {}),
                    "comm_only_ms": {f"{m}@{mib}MiB": v for (m, mib), v in sorted(table.items())},
                    "buckets": len(trainer.buckets), "bucket_mib": [round((e - s_) * 4 / 2 ** 20, 1) for s_, e in trainer.buckets],
                    "bytes_per_step_per_rank": int(trainer.g_arena.numel() * 4),
                    "wait_after_backward_ms_per_rank": [round(v[1].item(), 3) for v in allr],
                    "note": "wait = main-stream time between the end of the enqueued backward and the arrival of the last reduced bucket "
                            "(HIP events around FlatTrainer.sync_gradients): the part of the exchange NOT hidden behind backward"}
    elapsed = t.item()
    final_loss = loss.item()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last, trainer)
    last.clear()
    if probe.only is not None:
        timed_records, probe.records, probe.only, probe.enabled = probe.records, [], None, True
        _ops0.set_wgrad_stream(False)       # per-class durations: one kernel at a time (no overlap with the weight-gradient stream)
        for _ in range(BREAKDOWN_STEPS):
            step()
        torch.cuda.synchronize()
        _ops0.set_wgrad_stream(side_stream)
        probe.enabled = False
        probe.breakdown, probe.records = probe.records, timed_records

    # host side of a step (never part of `value`): C-ABI crossings per step and the time the host needs to enqueue one step when the GPU is
    # idle at its start (synchronise, then time until step() returns) -- the step is host-bound once this exceeds the GPU time
    # (every rank runs these steps -- a step holds the gradient exchange's collectives -- rank 0 reports its own figures)
    host = None
    if args.full:
        from nerf_rpn_amd import ops as _opsh
        cnt = [0]
        orig_call = _opsh.call

        def counting(name, *a):
            cnt[0] += 1
            return orig_call(name, *a)
        _opsh.call = counting
        enq = []
        for _ in range(6):
            torch.cuda.synchronize()
            if dist_on:
                dist.barrier()
            th = time.perf_counter()
            step()
            enq.append(time.perf_counter() - th)
        torch.cuda.synchronize()
        _opsh.call = orig_call
        enq.sort()
        host = {"c_abi_calls_per_step": round(cnt[0] / 6, 1), "enqueue_ms_per_step": round(1e3 * enq[len(enq) // 2], 3),
                "note": "median of 6 steps, each started on an idle GPU: time until step() has enqueued forward + backward + optimiser",
                "host_cores": os.cpu_count(), "pinning": pin}
        if dist_on:
            mine_enq = torch.tensor([1e3 * enq[len(enq) // 2]], device=dev, dtype=torch.float64)
            all_enq = [torch.zeros_like(mine_enq) for _ in range(world)]
            dist.all_gather(all_enq, mine_enq)
            host["enqueue_ms_per_step_per_rank"] = [round(v.item(), 3) for v in all_enq]
    cone = getattr(getattr(model, "rpn", None), "last_cone", None)

    extras = {}
    if not args.no_extras and args.model == "vgg_rpn" and spg == 1:
        # (a) two scenes per GPU, the reference's train.sh setting (batch_size 2 per rank): same trainer, batch of two grids
        sc2 = [synthetic_scene(1000 + rank * 2 + i, dev) for i in range(2)]
        step2 = make_step(model, trainer, [a for a, _ in sc2], [b.cpu() for _, b in sc2])
        for _ in range(3):
            step2()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n2 = max(5, args.steps // 5)
        for _ in range(n2):
            step2()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        t2 = torch.tensor([time.perf_counter() - t1], device=dev, dtype=torch.float64)
        if dist_on:
            dist.all_reduce(t2, op=dist.ReduceOp.MAX)
        extras["scenes_per_gpu_2"] = {"steps": n2, "ms_per_step": round(1e3 * t2.item() / n2, 3), "scenes_per_s": round(2 * world * n2 / t2.item(), 3)}
    if not args.no_extras and args.model == "vgg_rpn" and spg == 1:
        # (a') the dense head: the same step with the RPN head evaluated on every voxel (NRPN_CONE=0), as the reference computes it
        model.rpn.use_cone = False
        for _ in range(3):
            step()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        nd = max(5, args.steps // 5)
        for _ in range(nd):
            step()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        td = torch.tensor([time.perf_counter() - t1], device=dev, dtype=torch.float64)
        if dist_on:
            dist.all_reduce(td, op=dist.ReduceOp.MAX)
        extras["dense_head_ms_per_step"] = round(1e3 * td.item() / nd, 3)
        model.rpn.use_cone = True
        step()
        torch.cuda.synchronize()
    if rank == 0 and not args.no_extras and args.model == "vgg_rpn" and world == 1 and spg == 1:
        # (b) the parity mode: the same step in fp32 (exact fp32 MFMA chains); (c) the reference's own eval benchmark protocol
        del step
        m32 = build_model(torch.float32, dev)
        tr32 = FlatTrainer(m32, lr=1e-4, weight_decay=0.01, clip_grad_norm=0.1, total_steps=32)
        s32 = make_step(m32, tr32, xs, gts)
        for _ in range(2):
            s32()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(5):
            s32()
        torch.cuda.synchronize()
        extras["fp32_ms_per_step"] = round(1e3 * (time.perf_counter() - t1) / 5, 3)
        # (b') the parity-grade FAST mode: the same fp32 model, 3x3x3 convolutions on split-bf16 operands (ops.SPLIT3)
        from nerf_rpn_amd import ops as _o3
        _o3.SPLIT3[0] = True
        try:
            for _ in range(2):
                s32()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(8):
                l3 = s32()
            torch.cuda.synchronize()
            extras["bf16x3_ms_per_step"] = round(1e3 * (time.perf_counter() - t1) / 8, 3)
            extras["bf16x3_final_loss"] = round(float(l3.detach()), 5)
        finally:
            _o3.SPLIT3[0] = False
        del m32, tr32, s32
        torch.cuda.empty_cache()
        extras["eval_forward_protocol"] = eval_forward_protocol(args.dtype, dev)
        extras["secondary"] = secondary_workloads(dtype, dev, xs, gts, make_step_for)

    if rank == 0:
        roof, rows = probe.summary(args.dtype) if not args.no_probe else (None, [])
        if roof is not None:
            conv_ms = sum(v[1] for _, v in rows) / (BREAKDOWN_STEPS if probe.breakdown else args.steps)
            roof["timed_heavy_launches"]["ms_per_step"] = round(conv_ms, 3)
            ceil = measured_ceiling()
            if ceil is not None:
                roof["measured_ceiling"] = ceil
                roof["frac_of_measured_ceiling"] = round(roof["achieved"] / ceil["tflops"], 4)
            if args.model == "vgg_rpn":
                # FLOPs of the step: the reference's dense algorithm and what this engine executes -- in training the RPN head
                # runs on the sampled-anchor cones only (ops.ConeHeadFn), so its convolutions cost rows x 2 * 256 * 256 * 27 instead of voxels x ...
                executed = spg * STEP_GFLOP
                if cone is not None:
                    r, V = cone["rows"], cone["total_voxels"]
                    per_row = 2.0 * 256 * 256 * 27 / 1e9
                    dense_head = 4 * 3 * V * per_row
                    done = sum((2 * r[3 - i] + (r[4 - i] if i > 0 else V)) * per_row for i in range(4)) if len(r) == 4 else dense_head
                    executed = spg * STEP_GFLOP - dense_head + done
                step_tf = executed / (1e3 * elapsed / args.steps)
                roof["step"] = {"gflop": round(executed, 1), "gflop_dense_algorithm": spg * STEP_GFLOP, "tflops": round(step_tf, 1),
                                "mfma_frac": round(step_tf / MFMA_PEAK_TFLOPS[args.dtype], 4),
                                "note": "whole training step (fwd + dgrad + wgrad + everything else), EXECUTED FLOPs against the dense MFMA peak; "
                                        "gflop_dense_algorithm = the same step with the head evaluated on every voxel, as the reference does"}
                roof["forward_vgg19_fpn"] = forward_only(model, x, args.dtype)
                roof["hbm_stages"] = hbm_stages(dtype, dev)
        out = {
            "metric": "scenes/sec (160^3x4 grids, VGG19-3D+FPN+RPN fwd+bwd)", "value": round(world * spg * args.steps / elapsed, 4),
            "unit": "scenes/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"configs[1]: {'one' if spg == 1 else spg} 160x160x160x4 rgb-sigma grid{'s' if spg > 1 else ''} per GPU, VGG19-EF 3D + FPN + "
                                   "anchor RPN (OBB, 16 GT boxes per scene), fwd+bwd+clip+AdamW, random-init weights", "scenes_per_gpu": spg,
                       "parallelism": f"dp{world}", "world_size_seen": world,
                       "backend": (dist.get_backend() if dist_on else "single process")},
            "per_rank_ms_per_step": per_rank_ms,
            **({"gradient_exchange": exch} if exch else {}),
            "weight_packs_per_step": packs_per_step, "wgrad_side_stream": side_stream, "trunk_hip_graph": (use_graph if isinstance(use_graph, str) else bool(use_graph)), **({"tuning_knobs": knobs} if knobs else {}),
            "final_loss": round(final_loss, 5),
            **({"host": host} if host else {}),
            **({"rpn_head_cone": {**cone, "note": "training: the RPN head is evaluated on the receptive-field cones of the sampled anchors only "
                                                  "(rows = |S_0| .. |S_3| of the last step, of total_voxels over the four levels); NRPN_CONE=0 "
                                                  "runs the dense head"}} if cone else {}),
            "roofline": roof,
            **extras,
        }
        if args.model != "vgg_rpn":
            out["metric"] = f"scenes/sec (160^3x4 grids, {args.model} fwd+bwd) -- secondary workload, not the BASELINE metric"
            out["config"]["workload"] = f"{args.model}: one 160x160x160x4 grid per GPU, 16 OBB GT boxes, fwd+bwd+clip+AdamW, random-init weights"
        if world == 1 and not args.no_cpu_baseline and args.model == "vgg_rpn":
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out if args.notes else _compact(out)))
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
