"""What the tools/nerf_*_profile.py timers share."""
import torch


def timed(fn, repeats):
    """HIP-event time in ms of one call of fn: the best of ``repeats`` after a warm-up call."""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def window_times(fn, repeats):
    """HIP-event times in ms of ``repeats`` calls of fn after a warm-up call, in the order measured."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def trunk_kernel(tile, arithmetic="fp32"):
    """The family (see kernel_times) of one instantiation of nerf_mlp.cuh's trunk_kernel<kSplit, Tile>, as the profiler spells it.
    tile: the consumer's Tile -- GridTile (nerfgrid.hip), RayTile (nerfrender.hip), PointTile or KeepTile (nerfquery.hip: the forward,
    and the backward's trunk that keeps its activations).  Neither the two arithmetics nor two tiles share a family."""
    return "trunk_kernel<%s, (anonymous namespace)::%s>" % ("true" if arithmetic == "bf16x3" else "false", tile)


def kernel_times(fn, kernels):
    """Device time in ms per kernel family (a substring of the kernel's name) of one call of fn, from torch.profiler; None if the
    profiler records nothing of the first family."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {k: 0.0 for k in kernels}
    for e in prof.key_averages():
        for k in kernels:
            if k in e.key:
                out[k] += getattr(e, "device_time_total", getattr(e, "cuda_time_total", 0.0)) / 1e3
    return out if out[kernels[0]] > 0 else None
