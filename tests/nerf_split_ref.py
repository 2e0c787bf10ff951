"""Checker of the bf16x3 arithmetic of the NeRF trunk: a host emulation in torch float32.

Each of the trunk's ten matrix products -- pts_linears.0 .. 7, feature_linear and the feature columns W_f of views_linears.0 -- is
restated as ``x_hi @ w_hi.T + (x_hi @ w_lo.T + x_lo @ w_hi.T) + b`` with ``hi = x.bfloat16().float()`` and
``lo = (x - hi).bfloat16().float()``; the encoding, alpha_linear, the view and camera columns of views_linears.0 and rgb_linear are the
float32 checker's (tests/nerf_extract_ref.NeRF).  In the backward pass the split is the identity: a product's gradients are
``dY @ W`` and ``dY.T @ X`` on the float32 operands, which is what the kernels compute on the activations the forward kept.

The yardstick stays the float64 evaluation of the same float32 parameters and inputs; the emulation only says how far a correct
implementation of the arithmetic may be from it: ``bound = FACTOR x max|emulation - float64|``, floored at one float32 ulp of the
float64 result's largest magnitude.  MODES has the emulation's variants: the blocked summation order of the MFMA (K in blocks of 16,
the three products interleaved), the three mutations of the sharpness test, and the sanity form with exact residuals.

Also here: the cases, the bias nudging that keeps every relu of a gradient case a margin away from zero, and ``emulated()``, which lets
the other checkers (render, extract, the training loop) build the emulation in place of their float32 model.
"""
import contextlib
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf_extract_ref as R
import nerf_query_ref as Q

FACTOR = 8.0            # the convention of tests/nerf_train_ref.FACTOR
MARGIN = 64.0           # a gradient case keeps every relu pre-activation MARGIN x the emulation's deviation at that layer from zero
MODES = ("split", "blocked", "no_lohi", "no_hilo", "hihi", "exact_residuals")
MUTATIONS = ("no_lohi", "no_hilo", "hihi")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W = 256


def split(x):
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def split_product(x, w, mode="split"):
    """x [N, K] @ w [O, K].T in the arithmetic ``mode`` -> [N, O] float32."""
    assert x.dtype == torch.float32 and w.dtype == torch.float32 and mode in MODES
    xh, xl = split(x)
    wh, wl = split(w)
    if mode == "split":
        return xh @ wh.T + (xh @ wl.T + xl @ wh.T)
    if mode == "no_lohi":
        return xh @ wh.T + xh @ wl.T
    if mode == "no_hilo":
        return xh @ wh.T + xl @ wh.T
    if mode == "hihi":
        return xh @ wh.T
    if mode == "exact_residuals":       # the residuals unrounded, and their product too: hi hi + hi lo + lo hi + lo lo = x w
        xl, wl = x - xh, w - wh
        return xh @ wh.T + (xh @ wl.T + xl @ wh.T) + xl @ wl.T
    # "blocked": the order of the MFMA loop -- k in steps of 16 (zero-padded), per step hi hi, hi lo, lo hi into one accumulator
    pad = (-x.shape[1]) % 16
    xh, xl, wh, wl = (F.pad(t, (0, pad)) for t in (xh, xl, wh, wl))
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k in range(0, xh.shape[1], 16):
        s = slice(k, k + 16)
        acc = acc + xh[:, s] @ wh[:, s].T
        acc = acc + xh[:, s] @ wl[:, s].T
        acc = acc + xl[:, s] @ wh[:, s].T
    return acc


class SplitLinear(torch.autograd.Function):
    """y = split_product(x, w) + b; backward: the float32 Linear's, on the unsplit operands."""

    @staticmethod
    def forward(ctx, x, w, b, mode):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        y = split_product(x, w, mode)
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return dy @ w, dy.T @ x, (dy.sum(0) if ctx.has_bias else None), None


class SplitNeRF(R.NeRF):
    """The checker model with the trunk's products in the emulated arithmetic.  ``pre``: after a forward, the relu pre-activations of
    every row, [N, 8 x 256 + 128] (trunk layers 0 .. 7, then views_linears.0), detached."""
    mode = "split"

    def forward(self, x):
        assert self.use_viewdirs and x.dtype == torch.float32
        input_pts, input_views = torch.split(x, [self.input_ch, self.input_ch_views + self.input_ch_cam], dim=-1)
        h, pre = input_pts, []
        for i, l in enumerate(self.pts_linears):
            y = SplitLinear.apply(h, l.weight, l.bias, self.mode)
            pre.append(y.detach())
            h = F.relu(y)
            if i in self.skips:
                h = torch.cat([torch.zeros_like(input_pts) if self.drop_skip else input_pts, h], -1)
        alpha = self.alpha_linear(h)
        feature = SplitLinear.apply(h, self.feature_linear.weight, self.feature_linear.bias, self.mode)
        lv = self.views_linears[0]
        g = SplitLinear.apply(feature, lv.weight[:, :self.W], None, self.mode)
        y = g + F.linear(input_views, lv.weight[:, self.W:], lv.bias)
        pre.append(y.detach())
        rgb = self.rgb_linear(F.relu(y))
        self.pre = torch.cat(pre, -1)
        return torch.cat([rgb, alpha], -1)


def build_model(state, cfg=None, mode="split"):
    cfg = dict(R.DEFAULT_CFG, **(cfg or {}))
    state = {k[len("module."):] if k.startswith("module.") else k: v for k, v in state.items()}
    m = SplitNeRF(D=cfg["netdepth"], W=cfg["netwidth"], input_ch=3 + 6 * cfg["multires"], output_ch=4, skips=[4],
                  input_ch_views=3 + 6 * cfg["multires_views"], input_ch_cam=cfg["input_ch_cam"], use_viewdirs=True)
    m.load_state_dict(state)
    m.mode = mode
    return m.float().eval()


@contextlib.contextmanager
def emulated(mode="split"):
    """While active, the float32 model the other checkers build (R.build_model) is the emulation; their float64 model is untouched."""
    saved = R.build_model

    def build(state, cfg=None, dtype=torch.float32):
        return build_model(state, cfg, mode) if dtype == torch.float32 else saved(state, cfg, dtype)
    R.build_model = build
    try:
        yield
    finally:
        R.build_model = saved


def query(state, cfg, pts, viewdirs, cam=None, cot=None, mode="split", bb_center=Q.BB_CENTER, bb_scale=Q.BB_SCALE):
    """Q.query in the emulated arithmetic -> dict: raw, pre and, with ``cot``, grads (with dcam)."""
    cfg = dict(R.DEFAULT_CFG, **(cfg or {}))
    model = build_model(state, cfg, mode)
    embed_fn, _ = R.get_embedder(cfg["multires"], cfg["i_embed"])
    embeddirs_fn, _ = R.get_embedder(cfg["multires_views"], cfg["i_embed"])
    cam_t = (torch.zeros(cfg["input_ch_cam"]) if cam is None else torch.as_tensor(cam, dtype=torch.float32)).clone().requires_grad_(True)
    x = Q.network_rows(pts.float(), viewdirs.float(), cam_t, embed_fn, embeddirs_fn, torch.as_tensor(bb_center).float(),
                       torch.as_tensor(bb_scale).float())
    raw = model(x).reshape(*pts.shape[:2], 4)
    out = {"raw": raw.detach(), "pre": model.pre}
    if cot is not None:
        params = dict(model.named_parameters())
        wrt = [params[k] for k in Q.PARAMS] + ([cam_t] if cfg["input_ch_cam"] else [])
        g = torch.autograd.grad((raw * cot.float()).sum(), wrt)
        out["grads"] = dict(zip(Q.PARAMS, g[:len(Q.PARAMS)]))
        if cfg["input_ch_cam"]:
            out["grads"]["dcam"] = g[-1]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# bounds
# ----------------------------------------------------------------------------------------------------------------------
def as_np(x):
    return x.detach().double().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float64)


def deviation(x, x64):
    return float(np.abs(as_np(x) - as_np(x64)).max())


def bound_of(emulation, x64):
    """FACTOR x the emulation's deviation from the float64 result, floored at one float32 ulp of that result's largest magnitude."""
    top = float(np.abs(as_np(x64)).max())
    floor = float(np.spacing(np.float32(top))) if top > 0 else 0.0
    return max(FACTOR * deviation(emulation, x64), floor)


def assert_within(tag, got, emulation, x64):
    """Print the figures, then assert max|got - float64| <= bound_of(emulation, float64) -> (error, bound)."""
    err, bound = deviation(got, x64), bound_of(emulation, x64)
    print(f"{tag}: error {err:.3g}, emulation {deviation(emulation, x64):.3g}, bound {bound:.3g}, ratio {err / bound if bound else 0:.3g}")
    assert err <= bound, (tag, err, bound)
    return err, bound


# ----------------------------------------------------------------------------------------------------------------------
# the cases: 1, 63, 64, 65 and 130 points (a partial tile, an exact one, two and three tiles); multires_views 0 / 4, input_ch_cam 0 / 4
# ----------------------------------------------------------------------------------------------------------------------
CASES = [
    dict(name="p1", R=1, S=1, cfg=dict(multires_views=0, input_ch_cam=4), family="a", grads=True),
    dict(name="p63", R=7, S=9, cfg=dict(multires_views=4, input_ch_cam=4), family="b"),
    dict(name="p64", R=4, S=16, cfg=dict(multires_views=0, input_ch_cam=0), family="a"),
    dict(name="p65", R=5, S=13, cfg=dict(multires_views=4, input_ch_cam=0), family="a", grads=True),
    dict(name="p130", R=10, S=13, cfg=dict(multires_views=0, input_ch_cam=4), family="a", grads=True),
    # weights and activations with lo exactly 0 (bf16-representable values) and below bf16's normal range (subnormal float32)
    dict(name="p65_edge", R=5, S=13, cfg=dict(multires_views=0, input_ch_cam=4), family="a", edge=True),
]
NAMES = [c["name"] for c in CASES]
GRAD_NAMES = [c["name"] for c in CASES if c.get("grads")]


def case_inputs(case, nudged=False):
    """A case regenerated from seeds: the state as the query cases draw it (R.make_state), positions uniform in [-1, 1]^3 (2^8 p
    reaches 256 rad: all nine frequencies matter), unit view directions, a cotangent.  ``nudged``: the gradient form, biases moved by
    nudge_biases (info in .nudge)."""
    index = NAMES.index(case["name"])
    gen = torch.Generator().manual_seed(9500 + index)
    cfg = dict(R.DEFAULT_CFG, **case["cfg"])
    state = R.make_state(Q.STATE_SEED + index, case["family"], cfg)
    nr, ns = case["R"], case["S"]
    pts = Q.candidates(gen, nr * ns)
    viewdirs = Q.unit_dirs(gen, nr)
    if case.get("edge"):
        pts[0] = torch.tensor([0.0, 0.5, -0.25])                 # lo = 0 in p and in cos(0) = 1, sin(0) = 0
        pts[1] = torch.tensor([1e-40, -3e-39, 0.75])             # subnormal p, sin(2^l p)
        pts[64] = torch.tensor([-1.0, 2e-41, 0.015625])          # the same in the second tile
        w0 = state["pts_linears.0.weight"]
        w0[::2] = w0[::2].bfloat16().float()                      # every other row: lo = 0
        w0[1, :8] = torch.tensor([1e-40, -2e-40, 5e-39, 1e-41, -1e-45, 3e-39, 0.0, 1e-38])
        w3 = state["pts_linears.3.weight"]
        w3[:, ::3] = w3[:, ::3].bfloat16().float()
        w3[5, 10:14] = torch.tensor([4e-40, -6e-39, 1e-44, 9e-39])
        state["feature_linear.weight"][7, :4] = torch.tensor([2e-40, -2e-40, 7e-39, -1e-42])
    cam = torch.tensor(Q.CAM[:cfg["input_ch_cam"]], dtype=torch.float32) if cfg["input_ch_cam"] else None
    cot = torch.randn(nr, ns, 4, generator=gen)
    c = SimpleNamespace(name=case["name"], cfg=cfg, state=state, cam=cam, pts=pts.reshape(nr, ns, 3), viewdirs=viewdirs, cot=cot,
                        bb_center=Q.BB_CENTER, bb_scale=Q.BB_SCALE, nudge=None)
    if nudged:
        c.nudge = nudge_biases(c)
    return c


# ----------------------------------------------------------------------------------------------------------------------
# gradient cases: no relu within a margin of zero
# ----------------------------------------------------------------------------------------------------------------------
LAYERS = [(f"pts_linears.{i}.bias", slice(W * i, W * (i + 1))) for i in range(8)] + [("views_linears.0.bias", slice(8 * W, 8 * W + W // 2))]
SLACK = 1.5             # a nudge clears SLACK x the margin, so that the margin may drift while later passes move other layers
MAX_PASSES = 8


def layer_margins(c):
    """Per relu layer: (margin = MARGIN x the emulation's largest pre-activation deviation from float64 there, the float64
    pre-activations [N, units])."""
    p64 = Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, dtype=torch.float64)["pre"]
    pe = query(c.state, c.cfg, c.pts, c.viewdirs, c.cam)["pre"]
    return [(MARGIN * float((pe[:, s].double() - p64[:, s]).abs().max()), p64[:, s]) for _, s in LAYERS]


def smallest_shift(p, m):
    """p [N, U] float64, m > 0 -> d [U]: per column the d of smallest magnitude with |p + d| >= m in every row."""
    n, u = p.shape
    # the admissible d lie outside the open intervals (-p - m, -p + m); the nearest one to 0 is 0 or an end of an interval
    cand = torch.cat([torch.zeros(1, u, dtype=p.dtype), -p - m, -p + m], 0)                       # [1 + 2 N, U]
    ok = ((p[None, :, :] + cand[:, None, :]).abs() >= m * (1 - 1e-12)).all(1)                      # [1 + 2 N, U]
    cost = torch.where(ok, cand.abs(), torch.full_like(cand, float("inf")))
    return cand.gather(0, cost.argmin(0, keepdim=True))[0]


def nudge_biases(c):
    """Moves each hidden unit's bias (pts_linears.0 .. 7 and views_linears.0) by the smallest amount that leaves no point's float64
    pre-activation of that unit within the layer's margin of zero; the parameters stay float32 values; layer after layer, and again
    until a whole pass finds nothing to move.  Changes c.state in place -> info: passes, moved units, the largest move."""
    c.state = {k: v.clone() for k, v in c.state.items()}
    info = dict(passes=0, moved=0, largest=0.0)
    for _ in range(MAX_PASSES):
        info["passes"] += 1
        moved = 0
        for li, (name, _) in enumerate(LAYERS):
            m, p = layer_margins(c)[li]                  # after the earlier layers' moves of this pass
            if float(p.abs().min()) >= m:
                continue
            d = smallest_shift(p, SLACK * m)
            new = (c.state[name].double() + d).float()
            moved += int((new != c.state[name]).sum())
            info["largest"] = max(info["largest"], float(d.abs().max()))
            c.state[name] = new
        info["moved"] += moved
        if moved == 0:
            break
    info["holds"] = margins_hold(c)
    return info


def margins_hold(c):
    """The condition a gradient case is built for, on the float64 reference: at every relu layer min|pre| >= the layer's margin."""
    return all(float(p.abs().min()) >= m for m, p in layer_margins(c))


# ----------------------------------------------------------------------------------------------------------------------
# shared by tests/test_nerf_split_host.py and tests/test_gpu_nerf_split.py
# ----------------------------------------------------------------------------------------------------------------------
def tensors_of(o):
    return dict(o.get("grads", {}), raw=o["raw"])


@pytest.fixture(scope="module")
def refs():
    """(case name, nudged) -> (inputs, emulation, float64 checker): dicts over raw and, for a nudged case, the 24 gradients and dcam,
    as read-only numpy float64; filled on first use and shared."""
    cache = {}

    def get(name, nudged=False):
        if (name, nudged) not in cache:
            c = case_inputs(CASES[NAMES.index(name)], nudged)
            cot = c.cot if nudged else None
            both = []
            for o in (query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, cot), Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, cot, torch.float64)):
                o = {k: as_np(v) for k, v in tensors_of(o).items()}
                for v in o.values():
                    v.setflags(write=False)
                both.append(o)
            cache[(name, nudged)] = (c, *both)
        return cache[(name, nudged)]
    return get


@pytest.fixture(scope="module")
def records():
    with open(os.path.join(GOLDEN, "nerf_split_bounds.json")) as f:
        return json.load(f)
