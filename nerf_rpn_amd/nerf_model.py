"""The NeRF MLP the reference's run_nerf.py trains (create_nerf, data/scannet/run_nerf.py:344-358; the assumed model of DESIGN.md 3.16)
as a module whose query runs in HIP, forward and backward (ops.nerf_query)."""
import torch.nn as nn

from . import ops


class NeRF(nn.Module):
    """The 24 parameters of the network under the names and shapes of a checkpoint's network_fn_state_dict (D = 8, W = 256, skips =
    [4], multires 9, view directions), initialised as torch initialises nn.Linear.  ``cfg`` is a training run's args.json (a dict or a
    namespace) and goes through ops.nerf_grid_config, which raises NotImplementedError for an unsupported option.  ``dtype`` is the
    arithmetic of the trunk's matrix products in query, forward and backward: "fp32" (exact, the default) or "bf16x3" (DESIGN.md 3.23);
    the parameters and gradients are float32 either way.  ``backward_dtype`` is the arithmetic of the backward's own products: "fp32"
    (the default) or, with dtype "bf16x3" only, "bf16x3" (DESIGN.md 3.24)."""

    def __init__(self, cfg=None, dtype="fp32", backward_dtype="fp32"):
        super().__init__()
        self.set_compute_dtype(dtype, backward_dtype)
        self.cfg = dict(cfg) if isinstance(cfg, dict) else ({} if cfg is None else cfg)
        c = ops.nerf_grid_config(self.cfg)
        W, input_ch, views_ch = 256, 3 + 6 * c["multires"], 3 + 6 * c["multires_views"]
        self.pts_linears = nn.ModuleList([nn.Linear(input_ch, W)]
                                         + [nn.Linear(W + input_ch if i == 4 else W, W) for i in range(7)])
        self.views_linears = nn.ModuleList([nn.Linear(views_ch + c["input_ch_cam"] + W, W // 2)])
        self.feature_linear = nn.Linear(W, W)
        self.alpha_linear = nn.Linear(W, 1)
        self.rgb_linear = nn.Linear(W // 2, 3)

    def set_compute_dtype(self, dtype, backward_dtype="fp32"):
        """"fp32" or "bf16x3", and the backward's "fp32" or (with "bf16x3") "bf16x3"; anything else raises ValueError."""
        self.compute_dtype = ops.nerf_check_dtype(dtype)
        self.backward_dtype = ops.nerf_check_backward_dtype(dtype, backward_dtype)
        return self

    def query(self, pts, viewdirs, embedded_cam=None, bb_center=(0., 0., 0.), bb_scale=1., chunk=None):
        """network_query_fn(pts, viewdirs, embedded_cam, self): raw [R, S, 4], differentiable in the parameters and embedded_cam."""
        return ops.nerf_query(dict(self.named_parameters()), self.cfg, pts, viewdirs, embedded_cam, bb_center, bb_scale, chunk,
                              self.compute_dtype, self.backward_dtype)

    def forward(self, pts, viewdirs, embedded_cam=None, bb_center=(0., 0., 0.), bb_scale=1., chunk=None):
        return self.query(pts, viewdirs, embedded_cam, bb_center, bb_scale, chunk)
