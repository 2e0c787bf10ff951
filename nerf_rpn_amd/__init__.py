"""nerf_rpn_amd -- MI355X-native (gfx950) engine for the 3D RPN-over-NeRF hot path of lyclyc52/NeRF_RPN.

Python host code mirrors the reference's model API (``nerf_rpn_amd.model.*``) and calls hand-written HIP kernels
through the C ABI in ``include/nerfrpn.h`` (``libnerfrpn_hip.so``).  No CPU fallback exists on the product path.
"""
from . import lib  # noqa: F401

__all__ = ["lib", "NeRF", "render_rays_train", "training_loss"]


def __getattr__(name):
    if name == "NeRF":          # the NeRF MLP module (nerf_model.py); imported on first use, with torch
        from .nerf_model import NeRF
        return NeRF
    if name in ("render_rays_train", "training_loss"):        # one training step's ray stage (nerf_train.py)
        from . import nerf_train
        return getattr(nerf_train, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
