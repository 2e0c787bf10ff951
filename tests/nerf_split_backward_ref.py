"""Checker of the bf16x3 arithmetic in the backward of the NeRF query (backward_dtype="bf16x3"): a host emulation in
torch float32 on top of tests/nerf_split_ref.py (the forward's emulation, ``S``).

With the switch on, every backward product that involves one of the trunk's ten matrices splits both operands as the forward does:
``dX = split_product(dY, W^T)`` (dgrad) and ``dW = split_product(dY^T, X^T)`` (wgrad, the summed index is the point); a bias gradient
is the float64 column sum of the unsplit dY.  ``SplitLinear`` here is S.SplitLinear with that backward; S.SplitNeRF looks its linear up
in its module at call time, so ``backward_emulated()`` substitutes it there and everything built on S -- S.query, S.emulated() for the
training loop -- runs the new arithmetic while it is active.  The head (rgb_linear, alpha_linear, the view and camera columns and the
bias of views_linears.0, dcam) is not touched: its gradients are S.query's, bit for bit.

MODES: "split" (the arithmetic, torch's summation order), "blocked" (the kernels' order: dgrad as the forward's blocked product; wgrad
with the points cut into the kernel's 64 slices of whole tiles, inside a slice 16 points at a time with hi hi, hi lo, lo hi added into
one float32 accumulator, then the slices in float64; the forward blocked too) and the mutations "no_lohi", "no_hilo", "hihi", applied to
the backward products only.  The yardstick stays the float64 evaluation, the bound S.bound_of.

Cases: S.GRAD_NAMES nudged; "p65x65", the nudged p65 repeated 65 times (4225 points, 67 tiles: slices of two tiles) under a fresh
cotangent; "p65_edgecot", p65 under a cotangent with two whole rays of zeros (one spans the tile boundary and leaves the second tile
without a cotangent), entries that are bf16 values (lo = 0) and subnormal entries.
"""
import contextlib
import math
from types import SimpleNamespace

import pytest
import torch

import nerf_query_ref as Q
import nerf_split_ref as S

MODES = ("split", "blocked", "no_lohi", "no_hilo", "hihi")
MUTATIONS = ("no_lohi", "no_hilo", "hihi")
TILE, SLICES = 64, 64           # of csrc/nerfquery.hip: points per tile, slices of a chunk's points in wgrad
CASE_NAMES = (*S.GRAD_NAMES, "p65x65", "p65_edgecot")
REPEATS = 65

# what the mode changes: the ten trunk matrices' gradients and the nine trunk biases' (through dY); and what it must leave alone
TOUCHED = tuple([f"pts_linears.{i}.weight" for i in range(8)] + ["feature_linear.weight", "views_linears.0.weight"]
                + [f"pts_linears.{i}.bias" for i in range(8)] + ["feature_linear.bias"])
UNTOUCHED = ("rgb_linear.weight", "rgb_linear.bias", "alpha_linear.weight", "alpha_linear.bias", "views_linears.0.bias", "dcam")


def wgrad_product(dy, x, mode="split"):
    """dY [P, N], X [P, K] -> dY^T X [N, K] float32 in the arithmetic ``mode``."""
    if mode != "blocked":
        return S.split_product(dy.T.contiguous(), x.T.contiguous(), mode)
    rows_per_slice = math.ceil(math.ceil(dy.shape[0] / TILE) / SLICES) * TILE
    acc = torch.zeros(dy.shape[1], x.shape[1], dtype=torch.float64)
    for p0 in range(0, dy.shape[0], rows_per_slice):
        sl = slice(p0, p0 + rows_per_slice)
        acc = acc + S.split_product(dy[sl].T.contiguous(), x[sl].T.contiguous(), "blocked").double()
    return acc.float()


def make_linear(mode):
    """S.SplitLinear with the backward in the arithmetic ``mode`` -> (dgrad product, wgrad product, float64 column sum of dY)."""
    assert mode in MODES

    class SplitLinear(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b, fwd_mode):
            ctx.save_for_backward(x, w)
            ctx.has_bias = b is not None
            y = S.split_product(x, w, fwd_mode)
            return y if b is None else y + b

        @staticmethod
        def backward(ctx, dy):
            x, w = ctx.saved_tensors
            dy = dy.contiguous()
            db = dy.double().sum(0).float() if ctx.has_bias else None
            return S.split_product(dy, w.T.contiguous(), mode), wgrad_product(dy, x, mode), db, None
    return SplitLinear


SplitLinear = make_linear("split")


@contextlib.contextmanager
def backward_emulated(mode="split"):
    """While active, S.SplitNeRF (and with S.emulated() every checker built on it) takes its gradients in the arithmetic ``mode``."""
    saved = S.SplitLinear
    S.SplitLinear = make_linear(mode)
    try:
        yield
    finally:
        S.SplitLinear = saved


def forward_mode(mode):
    return "blocked" if mode == "blocked" else "split"


def query(state, cfg, pts, viewdirs, cam=None, cot=None, mode="split", **kw):
    """S.query with the backward in the arithmetic ``mode`` (a mutation leaves the forward alone) -> dict: raw, pre, grads."""
    with backward_emulated(mode):
        return S.query(state, cfg, pts, viewdirs, cam, cot, mode=forward_mode(mode), **kw)


class SplitNeRF(S.SplitNeRF):
    """S.SplitNeRF that takes its gradients in ``backward_mode`` wherever it is called from."""
    backward_mode = "split"

    def forward(self, x):
        with backward_emulated(self.backward_mode):
            return super().forward(x)


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
def case_inputs(name):
    if name in S.GRAD_NAMES:
        return S.case_inputs(S.CASES[S.NAMES.index(name)], nudged=True)
    c = S.case_inputs(S.CASES[S.NAMES.index("p65")], nudged=True)
    c.name = name
    if name == "p65x65":
        # the same 5 rays x 13 points 65 times: the relu margins are p65's (nudging 4225 distinct points is out of reach)
        c.pts, c.viewdirs = c.pts.repeat(REPEATS, 1, 1), c.viewdirs.repeat(REPEATS, 1)
        c.cot = torch.randn(*c.pts.shape[:2], 4, generator=torch.Generator().manual_seed(9565))
    elif name == "p65_edgecot":
        cot = c.cot.clone()
        cot[1] = 0.                                                  # whole rays without a cotangent: one inside the first tile,
        cot[4] = 0.                                                  # one across the tile boundary (its point 12 is the second tile's
        #                                                              only point: dY of that tile is zero throughout)
        cot[2] = cot[2].bfloat16().float()                           # lo = 0
        cot[3, :4] = torch.tensor([[1e-40, -3e-39, 2e-41, 0.], [-1e-45, 5e-39, 1e-38, -2e-40], [4e-40, 0., -6e-39, 1e-44],
                                   [9e-39, -1e-42, 7e-39, 2e-40]])   # below bf16's and float32's normal range
        cot[3, 12] = torch.tensor([0.5, -2.0, 1e-40, 0.0078125])      # bf16 values and a subnormal in one row
        c.cot = cot
    else:
        raise KeyError(name)
    return c


def evaluate(c, mode):
    """-> the 24 gradients, dcam and raw of case ``c`` as read-only numpy float64: mode "f64" the yardstick, else the emulation's."""
    if mode == "f64":
        o = Q.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot, torch.float64)
    else:
        o = query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot, mode)
    o = {k: S.as_np(v) for k, v in S.tensors_of(o).items()}
    for v in o.values():
        v.setflags(write=False)
    return o


@pytest.fixture(scope="module")
def brefs():
    """case name -> SimpleNamespace(c, f64, split, old): the inputs, the float64 yardstick, the new emulation and S.query's; and
    .mode(name) for the other variants.  Filled on first use and shared, never changed."""
    cache = {}

    def get(name):
        if name not in cache:
            c = case_inputs(name)
            old = {k: S.as_np(v) for k, v in S.tensors_of(S.query(c.state, c.cfg, c.pts, c.viewdirs, c.cam, c.cot)).items()}
            variants = {}

            def mode(m, c=c, variants=variants):
                if m not in variants:
                    variants[m] = evaluate(c, m)
                return variants[m]
            cache[name] = SimpleNamespace(c=c, f64=mode("f64"), split=mode("split"), old=old, mode=mode)
        return cache[name]
    return get


def touched_names(cfg):
    return [k for k in Q.tensor_names(cfg) if k in TOUCHED]


def untouched_names(cfg):
    return [k for k in Q.tensor_names(cfg) if k in UNTOUCHED]
