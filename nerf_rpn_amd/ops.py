"""Tensor-level wrappers over the C ABI (``include/nerfrpn.h``).

PyTorch is used only for device memory, streams and autograd graph stitching: every function here hands raw device
pointers + the current HIP stream to ``libnerfrpn_hip.so``.  Activations are channels-last tensors of shape
``[N, X, Y, Z, C]`` (fp32 or bf16).  There is no CPU / eager fallback: non-CUDA tensors raise.
"""
import ctypes
import itertools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from . import lib
from .lib import BF16, CONV_BIAS, CONV_OUT_F32, CONV_RELU, F32, call

# Size / plan queries of the C ABI are pure functions of (arguments, process-wide tool knobs): a training step asks the same ~40 of them
# ~600 times, each a ctypes crossing with argument conversion (~3 us).  Memoised per (name, arguments) and dropped whenever a
# nrpn_set_* knob is touched (lib.KNOB_EPOCH).  Queries that take an nrpn_conv_opts pointer are keyed on the descriptor's plan fields.
_QCACHE = {"epoch": -1, "map": {}}


def query(name, *args):
    if _QCACHE["epoch"] != lib.KNOB_EPOCH[0]:
        _QCACHE["epoch"], _QCACHE["map"] = lib.KNOB_EPOCH[0], {}
    m = _QCACHE["map"]
    key = (name, args)
    v = m.get(key)
    if v is None:
        v = m[key] = lib.query(name, *args)
    return v


def _query_opts(name, opts, *args):
    """``query`` for the *_ex entry points: the nrpn_conv_opts descriptor is the last argument; its plan fields (not its address) key the cache."""
    if _QCACHE["epoch"] != lib.KNOB_EPOCH[0]:
        _QCACHE["epoch"], _QCACHE["map"] = lib.KNOB_EPOCH[0], {}
    m = _QCACHE["map"]
    key = (name, args, opts.tile, opts.lds_dma, opts.kstep_bytes, opts.stagger, opts.big_split, opts.debug, bool(opts.scale), bool(opts.relu_mask))
    v = m.get(key)
    if v is None:
        v = m[key] = lib.query(name, *args, opts.ptr())
    return v


import os as _os


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _s():
    """Raw handle of torch's current HIP stream on the current device (the stream every kernel of this module is enqueued on)."""
    if _raw_stream is not None:      # ~0.3 us; torch.cuda.current_stream() spends ~10 us in device-index / availability checks per call
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


# Weight-gradient side stream (_on_wgrad_stream; DESIGN.md 3.10, "Where a parameter gradient goes").  Consumers of the arena (optimiser
# step, bucket all-reduce) call wgrad_stream_join(); NRPN_WGRAD_STREAM=0 or set_wgrad_stream(False) keeps everything on the current stream.
# "keep": the tensors side-stream kernels of this backward pass read, referenced until the main stream has joined the side stream.
_WGRAD_SIDE = {"enabled": _os.environ.get("NRPN_WGRAD_STREAM", "1") != "0", "streams": {}, "dirty": False, "prefetch": False, "keep": []}


def set_wgrad_stream(enabled):
    _WGRAD_SIDE["enabled"] = bool(enabled)


def _wgrad_side_stream(device):
    if not _WGRAD_SIDE["enabled"] or device.type != "cuda":
        return None
    key = device.index if device.index is not None else torch.cuda.current_device()
    st = _WGRAD_SIDE["streams"].get(key)
    if st is None:
        # NRPN_WGRAD_PRIORITY: HIP stream priority of the weight-gradient stream (0 = default; positive = lower than the main stream's,
        # so the critical chain of the backward gets free workgroup slots first -- measured)
        prio = int(_os.environ.get("NRPN_WGRAD_PRIORITY", _WGRAD_SIDE.get("priority", 0)))
        st = _WGRAD_SIDE["streams"][key] = torch.cuda.Stream(device=device, priority=prio) if prio else torch.cuda.Stream(device=device)
    return st


def wgrad_stream_join():
    """Make the current stream wait for every weight-gradient kernel enqueued on the side stream so far."""
    if _WGRAD_SIDE["dirty"] or _WGRAD_SIDE["prefetch"]:      # wgrads of this backward pass / an operand refresh enqueued after the last step
        joined = True
        for st in _WGRAD_SIDE["streams"].values():
            cur = torch.cuda.current_stream(st.device)
            if cur == st:            # called from inside the side-stream context (a bucket completed by a wgrad): already ordered, but
                joined = False       # the main stream has not waited yet -- keep the flag for the next join
            else:
                cur.wait_stream(st)
        if joined:
            _WGRAD_SIDE["dirty"] = _WGRAD_SIDE["prefetch"] = False
            _WGRAD_SIDE["keep"] = []        # every later write of the main stream is ordered behind the side stream's reads now


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise lib.NrpnError("HIP op called with a non-CUDA tensor (the product path has no CPU fallback)")
        if not t.is_contiguous():
            raise lib.NrpnError(f"HIP op needs contiguous tensors, got strides {t.stride()} for shape {tuple(t.shape)}")


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise lib.NrpnError(f"unsupported dtype {t.dtype} (fp32 / bf16 only)")


def _f32(t):
    return t if t.dtype == torch.float32 else t.float()


# ======================================================================================================================
# rotated IoU / NMS / top-k
# ======================================================================================================================
def sort_vertices(vertices, mask, num_valid):
    """Drop-in for reference ``sort_vertices.sort_vertices_forward`` (cuda_op/sort_vert.cpp:6-33)."""
    vertices = vertices.float().contiguous()
    m8 = mask.to(torch.uint8).contiguous()
    nv = num_valid.to(torch.int32).contiguous()
    _chk(vertices, m8, nv)
    B, N, M = m8.shape
    out = torch.zeros((B, N, 9), dtype=torch.int32, device=vertices.device)
    call("sort_vertices_f32", _p(vertices), _p(m8), _p(nv), _p(out), B * N, M, _s())
    return out


def iou3d_pair(b1, b2):
    """Paired rotated 3D IoU, boxes [..., 7] -> [...] (reference cal_iou_3d)."""
    shape = b1.shape[:-1]
    a, b = _f32(b1).reshape(-1, 7).contiguous(), _f32(b2).reshape(-1, 7).contiguous()
    _chk(a, b)
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    call("iou3d_obb_pair_f32", _p(a), _p(b), _p(out), a.shape[0], _s())
    return out.reshape(shape)


_IOU_LOSS_MODES = {"iou": 0, "linear_iou": 1, "giou": 2, "diou": 3}


class RotatedIoULossFn(torch.autograd.Function):
    """Per-pair IoU-type regression loss of RotatedIOULoss (reference model/rpn.py:133-164, fcos/loss.py:137-173): pred, target
    [n,7] -> (loss [n], iou [n]).  Forward and the gradient w.r.t. ``pred`` come out of one kernel (dual numbers over the reference's
    arithmetic, csrc/geomloss.hip); ``target`` is a constant."""

    @staticmethod
    def forward(ctx, pred, target, mode):
        p, t = _f32(pred).reshape(-1, 7).contiguous(), _f32(target).detach().reshape(-1, 7).contiguous()
        _chk(p, t)
        n = p.shape[0]
        loss = torch.empty(n, dtype=torch.float32, device=p.device)
        iou = torch.empty(n, dtype=torch.float32, device=p.device)
        grad = torch.empty((n, 7), dtype=torch.float32, device=p.device)
        call("rotated_iou_loss_f32", _p(p), _p(t), n, _IOU_LOSS_MODES[mode], _p(loss), _p(grad), _p(iou), _s())
        ctx.save_for_backward(grad)
        ctx.shape = pred.shape
        ctx.mark_non_differentiable(iou)
        return loss.reshape(pred.shape[:-1]), iou.reshape(pred.shape[:-1])

    @staticmethod
    def backward(ctx, g_loss, _g_iou):
        (grad,) = ctx.saved_tensors
        return (grad * g_loss.reshape(-1, 1)).reshape(ctx.shape), None, None


def rotated_iou_loss(pred, target, mode):
    """-> (per-pair loss, per-pair IoU); differentiable in ``pred``."""
    return RotatedIoULossFn.apply(pred, target, mode)


_SAMPLE_WS = {}


def sample_pos_neg(labels, batch, max_pos, seed, extra_flags=None, before_readback=None):
    """Balanced sampler of every scene in ONE host read-back (reference BalancedPositiveNegativeSampler, model/utils.py:35-98).
    labels: list of [T] float32 device tensors; seed: python int (one draw per call; scene i uses seed + i).
    -> ([(pos_i, neg_i)], host list of ``extra_flags``): int64 ascending index tensors; ``extra_flags`` (a list of 0-dim device tensors)
    ride on the same device->host copy so that callers with their own pending checks do not synchronise a second time.
    ``before_readback(out_pos, out_neg, counts)``: optional; enqueues more work on the sampler's raw output (device int64 [n, max_pos],
    int64 [n, batch], int32 (kp, kn, err) per scene) and returns ``(int32 device vector, finish)``: the vector rides on the same copy and
    ``finish(host values)`` is called after it (the cone lists of the RPN head are built this way, ``cone_build``)."""
    n = len(labels)
    dev = labels[0].device
    for lab in labels:
        if lab.dtype != torch.float32 or lab.dim() != 1:
            raise TypeError("sample_pos_neg: labels must be 1-D float32")
        _chk(lab.contiguous())
    wsb = int(query("sample_workspace_bytes"))
    key = (str(dev), n, batch, max_pos, _s())
    if key not in _SAMPLE_WS:          # per-scene scratch of this stream, reused every step (stream-ordered)
        _SAMPLE_WS[key] = torch.empty((n, (wsb + 7) // 8), dtype=torch.int64, device=dev)
    ws = _SAMPLE_WS[key]
    out_pos = torch.empty((n, max(max_pos, 1)), dtype=torch.int64, device=dev)
    out_neg = torch.empty((n, max(batch, 1)), dtype=torch.int64, device=dev)
    nx = len(extra_flags) if extra_flags else 0
    counts = torch.empty(n * 3 + nx, dtype=torch.int32, device=dev)
    for i, lab in enumerate(labels):
        call("sample_pos_neg", _p(lab.contiguous()), lab.numel(), int(max_pos), int(batch), (int(seed) + i) & 0x7FFFFFFFFFFFFFFF, _p(ws[i]),
             _p(out_pos[i]), _p(out_neg[i]), _p(counts[3 * i:]), _s())
    if nx:
        counts[3 * n:] = torch.stack([f.reshape(()) for f in extra_flags]).to(torch.int32)
    finish = None
    if before_readback is not None:
        more, finish = before_readback(out_pos, out_neg, counts)
        host = torch.cat([counts, more.to(torch.int32).reshape(-1)]).cpu().tolist()      # the one synchronisation
        finish(host[3 * n + nx:])
        host = host[:3 * n + nx]
    else:
        host = counts.cpu().tolist()                  # the one synchronisation
    res = []
    for i in range(n):
        kp, kn, err = host[3 * i:3 * i + 3]
        if err:
            raise RuntimeError("sample_pos_neg: a key bin holds more candidates than the kernel's LDS sort (see nrpn_sample_pos_neg)")
        res.append((out_pos[i, :kp], out_neg[i, :kn]))
    return res, host[3 * n:]


def projection_loss(pred, target, views, intrinsics, beta, max_mesh_dim):
    """2-D projection smooth-L1 of the RPN (value only, no gradient): pred / target [n,6|7], views [4,4,4], intrinsics [3,3] -> scalar
    (reference rpn.py:37-102, 421-453)."""
    if pred.shape != target.shape or pred.shape[1] not in (6, 7):
        raise ValueError(f"projection_loss: pred {tuple(pred.shape)} and target {tuple(target.shape)} must both be [n,6] or [n,7]")
    pred, target = _f32(pred.detach()).contiguous(), _f32(target.detach()).contiguous()
    views, intrinsics = views.contiguous(), intrinsics.contiguous()
    _chk(pred, target, views, intrinsics)
    out = torch.empty(1, dtype=torch.float32, device=pred.device)
    call("projection_loss_f32", _p(pred), _p(target), pred.shape[0], pred.shape[1], _p(views), _p(intrinsics), float(beta), float(max_mesh_dim),
         _p(out), _s())
    return out[0]


def iou3d_matrix(a, b):
    """All-pairs IoU [n,w] x [m,w] -> [n,m], w = 6 (AABB) or 7 (OBB) (reference box_iou_3d)."""
    if a.shape[1] != b.shape[1] or a.shape[1] not in (6, 7):
        raise ValueError(f"The second dimension of boxes1 and boxes2 should be the same, both 6 or 7. But get {a.shape[1]} and {b.shape[1]}.")
    a, b = _f32(a).contiguous(), _f32(b).contiguous()
    _chk(a, b)
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    for i in range(0, a.shape[0], 32768):
        part = a[i:i + 32768]
        call("iou3d_matrix_f32", _p(part), _p(b), _p(out[i:]), part.shape[0], b.shape[0], a.shape[1], _s())
    return out


def nms3d_sorted(boxes, levels, thr, count=None):
    """Greedy NMS on boxes already score-descending inside each (non-decreasing) level run -> uint8 keep mask."""
    boxes = _f32(boxes).contiguous()
    _chk(boxes, levels, count)
    n = boxes.shape[0]
    keep = torch.empty(n, dtype=torch.uint8, device=boxes.device)
    if n == 0:
        return keep
    ws = torch.empty(query("nms3d_workspace_bytes", n), dtype=torch.uint8, device=boxes.device)
    call("nms3d", _p(boxes), _p(levels), _p(count), n, boxes.shape[1], float(thr), _p(keep), _p(ws), _s())
    return keep


def segmented_topk(scores, offsets, k):
    """Per-segment top-k in (score desc, index asc) order.  offsets: python list of nseg+1 ints."""
    scores = scores.contiguous()
    _chk(scores)
    nseg = len(offsets) - 1
    idx = torch.empty((nseg, k), dtype=torch.int32, device=scores.device)
    val = torch.empty((nseg, k), dtype=torch.float32, device=scores.device)
    host = (ctypes.c_int64 * (nseg + 1))(*[int(o) for o in offsets])
    nbytes = int(query("segmented_topk_workspace_bytes", nseg, int(k)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=scores.device)
    call("segmented_topk_f32_ws", _p(scores), ctypes.addressof(host), nseg, int(k), _p(idx), _p(val), _p(ws), nbytes, _s())
    return idx, val


def argsort_desc(scores):
    """(score desc, index asc) permutation of a 1-D tensor with n <= 16384 (deterministic argsort)."""
    n = scores.numel()
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=scores.device)
    if n > 16384:
        raise lib.NrpnError("argsort_desc supports at most 16384 elements")
    idx, _ = segmented_topk(_f32(scores).reshape(-1), [0, n], n)
    return idx[0].long()


# ======================================================================================================================
# anchors / coders
# ======================================================================================================================
ANCHOR_SIZES = ((8,), (16,), (32,), (64,))
ASPECT_RATIOS = (((1., 1., 1.), (1., 1., 2.), (1., 2., 2.), (1., 1., 3.), (1., 3., 3.)),) * 4


def unique_ratio_permutations(ratios):
    """The reference iterates ``set(itertools.permutations(r))`` per ratio (anchor.py:57-60); CPython's hash order of
    float tuples is deterministic, so the same expression reproduces the channel <-> anchor mapping of checkpoints."""
    out = []
    for r in ratios:
        out += list(set(itertools.permutations(r)))
    return out


def base_anchor_table(scales, ratios):
    """anchor.py:49-82 (is_normalized=False): [A,6] rounded half-to-even, on the host."""
    r = torch.tensor(unique_ratio_permutations(ratios), dtype=torch.float32)
    s = torch.as_tensor(scales, dtype=torch.float32)
    e = (r[:, None, :] * s[None, :, None]).reshape(-1, 3)
    return (torch.cat([-e, e], dim=1) / 2).round()


class AnchorTable:
    """Device-side description of the anchor pyramid (layout in nerfrpn.h); anchors are computed from flat indices."""

    def __init__(self, mesh_size, grids, sizes=ANCHOR_SIZES, ratios=ASPECT_RATIOS, device="cuda"):
        bases = [base_anchor_table(s, r) for s, r in zip(sizes, ratios)]
        self.A = bases[0].shape[0]
        if any(b.shape[0] != self.A for b in bases):
            raise lib.NrpnError("all pyramid levels must have the same number of anchors per cell")
        self.grids = [tuple(int(v) for v in g) for g in grids]
        self.strides = [tuple(int(mesh_size[i]) // g[i] for i in range(3)) for g in self.grids]
        self.cells = [g[0] * g[1] * g[2] for g in self.grids]
        self.counts = [c * self.A for c in self.cells]
        self.offsets = [0]
        for c in self.counts:
            self.offsets.append(self.offsets[-1] + c)
        self.total = self.offsets[-1]
        L = len(self.grids)
        words = torch.zeros(int(query("anchor_table_words", L, self.A)), dtype=torch.int32)
        words[0], words[1] = L, self.A
        for l, (g, s) in enumerate(zip(self.grids, self.strides)):
            first = self.offsets[l]
            lo = first & 0xFFFFFFFF
            lo = lo - (1 << 32) if lo >= (1 << 31) else lo
            words[2 + 8 * l: 2 + 8 * l + 8] = torch.tensor([g[0], g[1], g[2], s[0], s[1], s[2], lo, first >> 32], dtype=torch.int32)
        fl = torch.cat([b.reshape(-1) for b in bases]).view(torch.int32)
        words[2 + 8 * L:] = fl
        self.words = words.to(device)
        self.base = bases

    def level_of(self, device):
        return torch.cat([torch.full((c,), i, dtype=torch.int64, device=device) for i, c in enumerate(self.counts)])


def anchors(table, sel=None, count=None):
    count = table.total if sel is None else sel.numel()
    out = torch.empty((count, 6), dtype=torch.float32, device=table.words.device)
    _chk(sel)
    call("anchors_f32", _p(table.words), _p(sel), count, _p(out), _s())
    return out


def decode_boxes(table, deltas, sel, coder):
    """deltas [T, 6|8] (flat anchor order), sel int64 [K] or None -> boxes [K, 6|7]."""
    deltas = _f32(deltas).contiguous()
    _chk(deltas, sel)
    count = deltas.shape[0] if sel is None else sel.numel()
    out = torch.empty((count, 7 if coder else 6), dtype=torch.float32, device=deltas.device)
    call("decode_boxes_f32", _p(table.words), _p(deltas), _p(sel), count, int(coder), _p(out), _s())
    return out


def encode_boxes(table, gt, sel, coder):
    gt = _f32(gt).contiguous()
    _chk(gt, sel)
    count = gt.shape[0]
    out = torch.empty((count, 8 if coder else 6), dtype=torch.float32, device=gt.device)
    call("encode_boxes_f32", _p(table.words), _p(gt), _p(sel), count, int(coder), _p(out), _s())
    return out


def coder_pairs(inp, anchor_boxes, coder, encode):
    inp, anchor_boxes = _f32(inp).contiguous(), _f32(anchor_boxes).contiguous()
    _chk(inp, anchor_boxes)
    if inp.shape[0] != anchor_boxes.shape[0]:
        raise AssertionError("coder: row count mismatch")
    width = (8 if coder else 6) if encode else (7 if coder else 6)
    out = torch.empty((inp.shape[0], width), dtype=torch.float32, device=inp.device)
    call("coder_pairs_f32", _p(inp), _p(anchor_boxes), inp.shape[0], int(coder), int(bool(encode)), _p(out), _s())
    return out


def obb_to_aabb(obb):
    obb = _f32(obb).contiguous()
    _chk(obb)
    out = torch.empty((obb.shape[0], 6), dtype=torch.float32, device=obb.device)
    call("obb_to_aabb_f32", _p(obb), _p(out), obb.shape[0], _s())
    return out


# ======================================================================================================================
# proposal filter / target assignment / losses
# ======================================================================================================================
def filter_candidates(boxes, logits, levels, valid, grid_size, min_size, score_thresh, fix_obb_clip=False):
    _chk(boxes, logits, levels, valid)
    n, w = boxes.shape
    dev = boxes.device
    ob = torch.empty((n, w), dtype=torch.float32, device=dev)
    os_ = torch.empty(n, dtype=torch.float32, device=dev)
    ol = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(16, query("filter_workspace_bytes", n, w)), dtype=torch.uint8, device=dev)
    host = (ctypes.c_float * 3)(*[float(v) for v in grid_size])
    call("filter_candidates_f32", _p(boxes), _p(logits), _p(levels), _p(valid), n, w, ctypes.addressof(host), float(min_size),
         float(score_thresh), int(bool(fix_obb_clip)), _p(ob), _p(os_), _p(ol), _p(cnt), _p(ws), _s())
    return ob, os_, ol, cnt


def select_kept(boxes, scores, levels, keep, count, post_top_n):
    _chk(boxes, scores, levels, keep, count)
    n, w = boxes.shape
    dev = boxes.device
    ob = torch.empty((post_top_n, w), dtype=torch.float32, device=dev)
    os_ = torch.empty(post_top_n, dtype=torch.float32, device=dev)
    ol = torch.empty(post_top_n, dtype=torch.float32, device=dev)
    oc = torch.zeros(1, dtype=torch.int32, device=dev)
    call("select_kept_f32", _p(boxes), _p(scores), _p(levels), _p(keep), _p(count), n, w, int(post_top_n), _p(ob), _p(os_), _p(ol),
         _p(oc), _s())
    return ob, os_, ol, oc


def match_anchors(table, gt_aabb, fg, bg, ori_size=None):
    """labels f32 [T] in {1,0,-1} and clamped match index int32 [T] (reference assign_targets_to_anchors + Matcher)."""
    gt_aabb = _f32(gt_aabb).contiguous()
    _chk(gt_aabb)
    dev = gt_aabb.device
    labels = torch.empty(table.total, dtype=torch.float32, device=dev)
    matched = torch.empty(table.total, dtype=torch.int32, device=dev)
    ws = torch.empty(gt_aabb.shape[0], dtype=torch.float32, device=dev)
    host = None
    hp = 0
    if ori_size is not None:
        host = (ctypes.c_float * 3)(*[float(v) for v in ori_size])
        hp = ctypes.addressof(host)
    call("match_anchors_f32", _p(table.words), table.total, _p(gt_aabb), gt_aabb.shape[0], float(fg), float(bg), hp, _p(labels),
         _p(matched), _p(ws), _s())
    return labels, matched


class SampledLossFn(torch.autograd.Function):
    """BCE-with-logits (mean over pos+neg) and smooth-L1 (sum over pos / (|pos|+|neg|)) with fused backward
    (reference compute_loss, rpn.py:372-419).  logits [M], deltas [M,dw] flat over the batch."""

    @staticmethod
    def forward(ctx, logits, deltas, targets, pos, neg, beta):
        logits, deltas = logits.contiguous(), deltas.contiguous()
        targets = targets.contiguous()
        _chk(logits, deltas, targets, pos, neg)
        out = torch.empty(2, dtype=torch.float32, device=logits.device)
        g_logits = torch.zeros_like(logits)
        g_deltas = torch.zeros_like(deltas)
        call("rpn_sampled_loss_f32", _p(logits), _p(deltas), deltas.shape[-1], _p(targets), _p(pos), pos.numel(), _p(neg), neg.numel(),
             float(beta), _p(out), _p(g_logits), _p(g_deltas), _s())
        ctx.save_for_backward(g_logits, g_deltas)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_obj, g_reg):
        g_logits, g_deltas = ctx.saved_tensors
        return g_logits * g_obj, g_deltas * g_reg, None, None, None, None


class FlattenHeadFn(torch.autograd.Function):
    """Per-level head rows [N, cells_l, ld] -> logits [N, T], deltas [N, T, dw] in the reference's (level, x, y, z, a) order
    (concat_box_prediction_layers, rpn.py:105-130); backward scatters dense gradients back into the padded head rows."""

    @staticmethod
    def forward(ctx, A, dw, grad_dtype, *heads):
        n = heads[0].shape[0]
        cells = [h.shape[1] for h in heads]
        T = sum(cells) * A
        dev = heads[0].device
        logits = torch.empty((n, T), dtype=torch.float32, device=dev)
        deltas = torch.empty((n, T, dw), dtype=torch.float32, device=dev)
        off = 0
        for h, c in zip(heads, cells):
            _chk(h)
            for i in range(n):
                call("head_flatten_f32", _p(h[i]), c, h.shape[2], A, dw, _p(logits[i, off:]), _p(deltas[i, off:]), _s())
            off += c * A
        ctx.meta = (A, dw, cells, [h.shape[2] for h in heads], grad_dtype)
        return logits, deltas

    @staticmethod
    def backward(ctx, g_logits, g_deltas):
        A, dw, cells, lds, grad_dtype = ctx.meta
        g_logits, g_deltas = g_logits.contiguous(), g_deltas.contiguous()
        n = g_logits.shape[0]
        outs = []
        off = 0
        for c, ld in zip(cells, lds):
            d = torch.empty((n, c, ld), dtype=grad_dtype, device=g_logits.device)
            for i in range(n):
                call("head_unflatten", _p(g_logits[i, off:]), _p(g_deltas[i, off:]), c, ld, A, dw, 0, _p(d[i]), _dt(d), _s())
            outs.append(d)
            off += c * A
        return (None, None, None, *outs)


# ======================================================================================================================
# conv / norm / pool with autograd
# ======================================================================================================================
class GradSink:
    """Direct gradient destination of a parameter inside a flat gradient arena (set by engine.FlatTrainer as
    ``param._nrpn_sink``).  Backward kernels accumulate straight into ``slot`` and call ``notify()`` instead of returning a
    gradient tensor for autograd to add -- this removes one elementwise kernel per parameter per use.
    ``flat``: for weights the trainer keeps in the forward GEMM layout [taps][Cout][Cin], the contiguous 1-D arena range of the
    gradient in THAT layout (the sum of a wgrad's slice partials goes there without any layout shuffle); None otherwise."""
    __slots__ = ("slot", "notify", "flat")

    def __init__(self, slot, notify, flat=None):
        self.slot, self.notify, self.flat = slot, notify, flat


class ArenaWeights:
    """GEMM operands of the weights a trainer keeps in the forward GEMM layout inside its flat fp32 arena (engine.FlatTrainer).

    forward operand  = the master arena itself (fp32) or its bf16 shadow -- the same element order, written by the AdamW kernel as a
                       second output, so there is no per-step repack;
    dgrad operand    = [taps reversed][Cin][Cout] copies of ALL weights, refreshed by ONE batched launch per optimiser step.
    ``epoch`` counts parameter updates (optimiser steps, or torch-side writes noticed through tensor._version)."""

    def __init__(self, master):
        self.master = master
        self.entries = []             # (offset, taps, cout, cin, param)
        self.versions = []
        self.epoch = 0
        self.shadow = None            # bf16 [len(master)]
        self.shadow_epoch = -1
        self.trans = {}               # dtype -> [tensor, epoch]
        self.table = None
        self.launches = {"cast": 0, "transpose": 0}

    def add(self, param, offset, taps, cout, cin):
        param._nrpn_arena = (self, len(self.entries))
        self.entries.append((int(offset), int(taps), int(cout), int(cin), param))
        self.versions.append(param._version)
        self.table = None

    def bump(self, shadow_written=False):
        """The master arena was rewritten (optimiser step)."""
        self.epoch += 1
        if shadow_written and self.shadow is not None:
            self.shadow_epoch = self.epoch

    def _check(self, idx):
        if self.entries[idx][4]._version != self.versions[idx]:      # torch-side write (load_state_dict, manual init): everything is stale
            self.versions = [e[4]._version for e in self.entries]
            self.epoch += 1

    def shadow_ptr(self):
        """bf16 shadow for the AdamW kernel to refresh (None until a bf16 forward asked for it)."""
        return self.shadow

    def fwd(self, idx, dtype):
        self._check(idx)
        off, taps, cout, cin, _ = self.entries[idx]
        if dtype == torch.float32:
            return self.master[off:off + taps * cout * cin].view(taps, cout, cin)
        if self.shadow is None:
            self.shadow = torch.empty(self.master.numel(), dtype=torch.bfloat16, device=self.master.device)
        if self.shadow_epoch != self.epoch:
            call("cast", _p(self.master), _p(self.shadow), self.master.numel(), F32, BF16, _s())
            self.launches["cast"] += 1
            self.shadow_epoch = self.epoch
        return self.shadow[off:off + taps * cout * cin].view(taps, cout, cin)

    def dgrad(self, idx, dtype):
        self._check(idx)
        off, taps, cout, cin, _ = self.entries[idx]
        ent = self.trans.get(dtype)
        if ent is None:
            ent = [torch.empty(self.master.numel(), dtype=dtype, device=self.master.device), -1]
            self.trans[dtype] = ent
        if ent[1] != self.epoch:
            self._transpose(dtype)
        return ent[0][off:off + taps * cout * cin].view(taps, cin, cout)

    def _transpose(self, dtype):
        ent = self.trans[dtype]
        if self.table is None:
            rows, prefix = [], [0]
            for (o, t, co, ci, _) in self.entries:
                rows.append([o, t, co, ci])
                prefix.append(prefix[-1] + t * ((co + 63) // 64) * ((ci + 63) // 64))
            dev = self.master.device
            self.table = (torch.tensor(rows, dtype=torch.int64, device=dev), torch.tensor(prefix, dtype=torch.int32, device=dev), prefix[-1])
        tab, prefix, total = self.table
        call("transpose_weights", _p(self.master), _p(ent[0]), _p(tab), _p(prefix), len(self.entries), total, F32 if dtype == torch.float32 else BF16, _s())
        self.launches["transpose"] += 1
        ent[1] = self.epoch

    def prefetch_dgrad(self):
        """Called by the trainer right after an optimiser step: refresh the dgrad operands on the weight-gradient side stream, off the
        next forward's critical path (they are first read by the next BACKWARD, which waits for the event recorded here)."""
        side = _wgrad_side_stream(self.master.device)
        if side is None or not self.trans or self.table is None:
            return
        side.wait_stream(torch.cuda.current_stream(self.master.device))      # behind the AdamW kernel that rewrote the master arena
        with torch.cuda.stream(side):
            for dtype in list(self.trans):
                if self.trans[dtype][1] != self.epoch:
                    self._transpose(dtype)
            ev = torch.cuda.Event()
            ev.record(side)
        _DGRAD_READY["event"] = ev
        _DGRAD_READY["waited"] = set()
        _WGRAD_SIDE["prefetch"] = True   # a step() with no backward in between still joins the side stream before it rewrites the arena
                                         # (a flag of its own: "dirty" also decides whether a backward pass queues its end-of-pass join)


_DGRAD_READY = {"event": None, "waited": set()}


def _wait_dgrad_operands():
    """First dgrad of a stream after an optimiser step: wait for the operand refresh enqueued on the side stream."""
    ev = _DGRAD_READY["event"]
    if ev is not None and torch.cuda.is_current_stream_capturing():
        return      # graph capture (graphs.GraphedBackbone): the replay is ordered behind the refresh by an eager wait on the launching stream
    if ev is not None:
        sid = _s()
        if sid not in _DGRAD_READY["waited"]:
            torch.cuda.current_stream().wait_event(ev)
            _DGRAD_READY["waited"].add(sid)


def _sink(t):
    return getattr(t, "_nrpn_sink", None) if t is not None else None


def hand_in(sink, grad, copy=False):
    """A finished gradient goes into its sink (added to the slot, the sink notified; -> None) or, without one, back to autograd
    (-> ``grad``; ``copy``: it is a slice of a buffer shared with other gradients)."""
    if sink is None:
        return grad.clone() if copy else grad
    sink.slot.add_(grad)
    sink.notify()
    return None


def _sinks_cover(params, sinks):
    """Every parameter of a layer that exists (is not None) has a GradSink: the layer hands nothing back to autograd."""
    return all(s is not None for p, s in zip(params, sinks) if p is not None)


# Parameters can be rewritten behind autograd's back (engine.FlatTrainer updates its flat arena through the raw-pointer AdamW
# kernel, which never bumps tensor._version), so every GEMM-layout cache is also keyed on this epoch; whoever writes
# parameter memory outside torch calls ``weights_changed()``.
_weight_epoch = 0
PACK_COUNT = {"conv": 0, "stem": 0}      # pack launches so far (tests assert packs == modules x optimiser steps)


def a2a_reduce(recv, bucket, rank, world):
    """recv: bf16 [world * chunk] (chunk ``rank`` of every peer's bucket, peer-major), bucket: this rank's fp32 bucket [world * chunk] -> bf16
    [chunk] = sum over the ranks in ascending order in fp32, the own chunk read from the fp32 bucket (engine.FlatTrainer, a2a_bf16)."""
    chunk = bucket.numel() // world
    _chk(recv, bucket)
    out = torch.empty(chunk, dtype=torch.bfloat16, device=bucket.device)
    call("a2a_reduce_bf16", _p(recv), bucket.data_ptr() + rank * chunk * 4, rank, world, chunk, _p(out), _s())
    return out


def weights_changed():
    global _weight_epoch
    _weight_epoch += 1


class PackedWeight:
    """GEMM-layout copies of one or more reference-layout conv weights sharing a GEMM (rows_total rows), refreshed when
    the parameters change (tensor._version for torch-side writes, the module weight epoch for raw-pointer writes)."""

    def __init__(self):
        self.key = None
        self.fwd = None
        self.dgrad = None

    def get(self, weights, dtype, rows_total, need_dgrad, cin=None):
        cin = weights[0].shape[1] if cin is None else cin     # nn.Linear [out,in] and a flattened patch conv are taps == 1
        taps = weights[0][0].numel() // cin
        arena = getattr(weights[0], "_nrpn_arena", None) if len(weights) == 1 else None
        if arena is not None and rows_total == weights[0].shape[0] and arena[0].entries[arena[1]][1:4] == (taps, rows_total, cin):
            # master weights already live in the GEMM layout inside the trainer's arena: no packing at all
            aw, idx = arena
            return aw.fwd(idx, dtype), (aw.dgrad(idx, dtype) if need_dgrad else None)
        key = tuple((w.data_ptr(), w._version) for w in weights) + (dtype, rows_total, need_dgrad, _weight_epoch)
        if key == self.key:
            return self.fwd, self.dgrad
        PACK_COUNT["conv"] += 1
        dev = weights[0].device
        padded = rows_total != sum(w.shape[0] for w in weights)
        alloc = torch.zeros if padded else torch.empty
        fwd = alloc((taps, rows_total, cin), dtype=dtype, device=dev)
        dgrad = alloc((taps, cin, rows_total), dtype=dtype, device=dev) if need_dgrad else None
        row = 0
        for w in weights:
            wc = w.detach().contiguous()
            call("pack_conv_weight", _p(wc), w.shape[0], cin, taps, _dt(fwd), _p(fwd), _p(dgrad), rows_total, row, _s())
            row += w.shape[0]
        self.key, self.fwd, self.dgrad = key, fwd, dgrad
        return fwd, dgrad

    def fused_bias(self, biases, rows_total):
        """fp32 bias row of a fused multi-weight GEMM, zero-padded to rows_total: assembled once per parameter update, not once per
        pyramid level."""
        bkey = tuple((b.data_ptr(), b._version) for b in biases) + (rows_total, _weight_epoch)
        if getattr(self, "bias_key", None) != bkey:
            parts = [b.detach().float().reshape(-1) for b in biases]
            used = sum(p.numel() for p in parts)
            if used < rows_total:
                parts.append(parts[0].new_zeros(rows_total - used))
            self.bias, self.bias_key = torch.cat(parts), bkey
        return self.bias


# ======================================================================================================================
# bf16x3: the parity-grade fast mode (round 5).  fp32 activations / weights / gradients everywhere; the dense and row-list 3x3x3
# convolutions -- 95 % of the step's FLOPs -- multiply SPLIT operands (hi = bf16(x), lo = bf16(x - hi)) on the bf16 MFMA kernels:
# x * w ~ hi*whi + hi*wlo + lo*whi, fp32 accumulation, fp32 rows out (csrc/elementwise.hip: split_bf16x3_kernel).  The K axis is tripled,
# the kernels are the bf16 ones unchanged.  SPLIT3 decides HOW an fp32 convolution is computed, not what it returns (to fp32 accumulation
# error) -- in the spirit of torch.backends.cuda.matmul.allow_tf32.  A model raises it for the duration of its own forward pass
# (NeRFRegionProposalNetwork.set_compute_dtype("bf16x3"), run_rpn.py --dtype bf16x3; backward passes follow what their forward recorded);
# NRPN_BF16X3=1 turns it on for the whole process.
# ======================================================================================================================
SPLIT3 = [_os.environ.get("NRPN_BF16X3", "0") == "1"]
_ACT_I, _W_I = 0b100, 0b010          # interleaved [rows][3C]: activations (hi | hi | lo), weights (hi | lo | hi)
_X_P, _DY_P = 0b010, 0b100           # planes stacked on the batch axis: x (hi ; lo ; hi), dy (hi ; hi ; lo)


def split3(src, ipattern=None, nplanes=0, ppattern=0):
    """src f32 [..., C] -> (bf16 [..., 3C] interleaved or None, bf16 [nplanes, ..., C] planes or None); see nrpn_split_bf16x3."""
    src = src.contiguous()
    _chk(src)
    c = src.shape[-1]
    inter = torch.empty(tuple(src.shape[:-1]) + (3 * c,), dtype=torch.bfloat16, device=src.device) if ipattern is not None else None
    planes = torch.empty((nplanes,) + tuple(src.shape), dtype=torch.bfloat16, device=src.device) if nplanes else None
    call("split_bf16x3", _p(src), src.numel() // c, c, _p(inter), ipattern or 0, _p(planes), nplanes, ppattern, _s())
    return inter, planes


def _x3_ok(x, ksize, segs, rows_total, differentiable):
    # ragged voxel lists (the dense head over all pyramid levels) only when nothing is differentiated: their weight gradient has no batch
    # axis to stack on and the split dgrad launch knows no segments.  `differentiable` comes from the caller (hip_nn.conv3d: grad mode on AND
    # an operand that requires a gradient) -- inside autograd.Function.forward grad mode is always off and ctx.needs_input_grad mirrors
    # requires_grad even under torch.no_grad(), which sent every eval-mode ragged conv with trainable weights to the fp32 kernels
    return (SPLIT3[0] and x.dtype == torch.float32 and ksize == 3 and (segs is None or not differentiable)
            and x.shape[-1] % 32 == 0 and rows_total % 32 == 0)


def _x3_weights(pack, weights, wp, wpd):
    """Split forms of a conv's fp32 GEMM operands (forward [taps][rows][Cin] -> [taps][rows][3 Cin], dgrad [taps][Cin][rows] ->
    [taps][Cin][3 rows]), refreshed when the parameters change (the same epochs PackedWeight.get keys on)."""
    arena = getattr(weights[0], "_nrpn_arena", None) if len(weights) == 1 else None
    key = (wp.data_ptr(), wpd.data_ptr() if wpd is not None else 0, _weight_epoch, arena[0].epoch if arena is not None else pack.key)
    ent = pack.__dict__.get("x3")
    if ent is None or ent[0] != key:
        w3 = split3(wp, _W_I)[0]
        if wpd is not None:
            _wait_dgrad_operands()       # the trainer refreshes the dgrad operands on the weight-gradient stream (ArenaWeights.prefetch_dgrad): this
                                         # stream reads them here, in the FORWARD pass, before the first dgrad's own wait
        wd3 = split3(wpd, _W_I)[0] if wpd is not None else None
        ent = (key, w3, wd3)
        pack.__dict__["x3"] = ent
    return ent[1], ent[2]


def column_sum_f32(t, out=None, accumulate=False):
    """f32 [rows, C] -> f32 [C] column sums, deterministic; ``out`` += when ``accumulate``.  Shapes the BatchNorm statistics reduction takes
    (C % 4 == 0, C / 4 dividing 256: every conv width of the VGG / ResNet paths) go through its slab pass -- 4-channel lanes over ~1000 row
    slabs -- when they are large, and the slab sums it leaves in the workspace ([slabs][2][C]: sum, sum of squares) are added up in fp64
    here; the rest (e.g. C = 96) through nrpn_column_sum_f32.  Both: fp32 sums inside a slab, fp64 across slabs, one rounding of the total --
    on exactly summable data the sum itself.  (The first version returned bn_stats' mean * rows: two more roundings, an ulp off on about
    one column in eight.)  Measured on an MI355X, slab pass + fp64 finish / nrpn_column_sum_f32: 160^3 x 64: 209 / 490 us, 80^3 x 128:
    62 / 75 us, 40^3 x 256: 40 / 32 us, 20^3 x 512: 32 / 14 us -- hence the size threshold."""
    t = t.contiguous()
    rows, c = t.shape
    tile = min(c, 1024)
    if rows * c >= (1 << 25) and c % 4 == 0 and 256 % (tile // 4) == 0 and c % tile == 0:
        mean, var = torch.empty(c, dtype=torch.float32, device=t.device), torch.empty(c, dtype=torch.float32, device=t.device)
        ws = torch.empty(query("bn_workspace_bytes", rows, c), dtype=torch.uint8, device=t.device)
        call("bn_stats", _p(t), rows, c, F32, _p(mean), _p(var), 0, 0, 0.1, _p(ws), _s())
        res = ws.view(torch.float32).view(-1, 2, c)[:, 0].sum(0, dtype=torch.float64).float()
        if out is None:
            return res
        return out.add_(res) if accumulate else out.copy_(res)
    if out is None:
        out = torch.empty(c, dtype=torch.float32, device=t.device)
    ws = torch.empty(query("column_sum_workspace_bytes", rows, c), dtype=torch.uint8, device=t.device)
    call("column_sum_f32", _p(t), rows, c, _p(out), 1 if accumulate else 0, _p(ws), _s())
    return out


def _seg_dims(segs):
    import ctypes
    flat = [int(v) for d in segs for v in d]
    return (ctypes.c_int32 * len(flat))(*flat)


def _conv_fwd(x, wp, bias, cout, wrows, ksize, flags, out_dtype, segs=None, mask=None, stats=None, scale=None, tile=0, halo_pairing=0):
    """segs: None, or the (X, Y, Z) dims of the grids laid end to end in x = [1, sum(X*Y*Z), 1, 1, C] (ragged list).
    stats: None, or a dict that asks for BatchNorm statistics out of the conv epilogue: when the shape's kernel has them, the launch
    fills stats['partials'] = f32 [P, 2, cout] (see nrpn_conv3d_fwd_stats); otherwise the dict stays empty.
    scale: None or f32 [cout]: y = acc * scale + bias (eval-mode BatchNorm folded into the conv, nrpn_conv_opts.scale).
    tile: per-call kernel selection (lib.TILE_*; 0 = the library's choice for the shape); halo_pairing: nrpn_conv_opts.halo_pairing (0 = default,
    1 = taps paired across chunk boundaries, 2 = 14 K-steps per chunk)."""
    import ctypes
    n, gx, gy, gz, cin = x.shape
    y = torch.empty((n, gx, gy, gz, cout), dtype=out_dtype, device=x.device)
    if out_dtype == torch.float32 and x.dtype == torch.bfloat16:
        flags |= CONV_OUT_F32
    if bias is not None:
        flags |= CONV_BIAS
    if segs is not None and ksize != 1:
        if scale is not None or mask is not None or tile:
            raise lib.NrpnError("ragged conv launches take no per-call options")
        wsb = query("conv3d_fwd_workspace_bytes", n, gx, gy, gz, cin, cout, ksize, _dt(x))
        ws = torch.empty(wsb, dtype=torch.uint8, device=x.device) if wsb else None
        dims = _seg_dims(segs)
        call("conv3d_fwd_ragged", _p(x), _p(wp), _p(bias), _p(y), len(segs), ctypes.addressof(dims), cin, cout, wrows, ksize, _dt(x), flags,
             _p(ws), _s())
        return y
    opts = lib.ConvOpts(tile=tile or CONV_TILE[0], scale=_p(scale), relu_mask=_p(mask), halo_pairing=halo_pairing or CONV_HALO_PAIRING[0])
    if stats is not None and segs is None and mask is None and out_dtype == x.dtype and wrows == cout:
        rows = _query_opts("conv3d_fwd_stats_rows_ex", opts, n, gx, gy, gz, cin, cout, ksize, _dt(x))
        if rows > 0:
            part = torch.empty((rows, 2, cout), dtype=torch.float32, device=x.device)
            opts.stats = part.data_ptr()
            call("conv3d_fwd_ex", _p(x), _p(wp), _p(bias), _p(y), n, gx, gy, gz, cin, cout, wrows, ksize, _dt(x), flags, 0, opts.ptr(), _s())
            stats["partials"] = part
            return y
    wsb = _query_opts("conv3d_fwd_workspace_bytes_ex", opts, n, gx, gy, gz, cin, cout, ksize, _dt(x))
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device) if wsb else None
    call("conv3d_fwd_ex", _p(x), _p(wp), _p(bias), _p(y), n, gx, gy, gz, cin, cout, wrows, ksize, _dt(x), flags, _p(ws), opts.ptr(), _s())
    return y


# Tile override of every forward / dgrad launch of this process ([0] = lib.TILE_*; 0 = the library's per-shape choice).  A per-call
# nrpn_conv_opts field underneath -- NOT a library global -- so it is safe next to other threads; bench.py / tools set it for A/B runs.
CONV_TILE = [int(_os.environ.get("NRPN_CONV_TILE", "0"))]
CONV_HALO_PAIRING = [int(_os.environ.get("NRPN_HALO_PAIRING", "0"))]      # A/B: 0 = library default, 1 = cross-chunk tap pairing, 2 = off


# Tools only (tools/launch_anatomy.py, nerf_rpn_amd/stamps.py): the forward launches on their stamped twins.  Nothing of the product path
# calls these two.
def conv3d_stamp_layout(n, gx, gy, gz, cin, cout, ksize, dtype=BF16, opts=None):
    """nrpn_conv3d_fwd_stamp_layout as a ``stamps.Layout``; raises lib.NrpnError (naming the plan code) for a plan without a stamped form."""
    from . import stamps
    lay = lib.StampLayout()
    call("conv3d_fwd_stamp_layout", n, gx, gy, gz, cin, cout, ksize, dtype, opts.ptr() if opts is not None else 0, lay.ptr())
    return stamps.Layout(words=lay.words, plan_code=lay.plan_code, conv_records=lay.conv_records, epilogue_records=lay.epilogue_records,
                         nbytes=lay.bytes, m_tiles=lay.m_tiles, n_tiles=lay.n_tiles, k_slices=lay.k_slices, k_steps=lay.k_steps,
                         slice_steps=tuple(lay.slice_steps[:lay.k_slices]))


def conv3d_fwd_stamped(x, wp, bias, cout, wrows, ksize, flags, out_dtype, opts=None):
    """The launches of the conv3d_fwd_ex call in ``_conv_fwd`` on the stamped instantiations: same plan, same bits -> (y, records) with
    records an int64 tensor [records, words] (conv launch first, then its split-K epilogue; decode with ``stamps.decode``).  ``opts``: a
    lib.ConvOpts (its scale / relu_mask pointers are the caller's to keep alive)."""
    _chk(x, wp, bias)
    n, gx, gy, gz, cin = x.shape
    y = torch.empty((n, gx, gy, gz, cout), dtype=out_dtype, device=x.device)
    if out_dtype == torch.float32 and x.dtype == torch.bfloat16:
        flags |= CONV_OUT_F32
    if bias is not None:
        flags |= CONV_BIAS
    if opts is None:
        opts = lib.ConvOpts(tile=CONV_TILE[0], halo_pairing=CONV_HALO_PAIRING[0])
    lay = conv3d_stamp_layout(n, gx, gy, gz, cin, cout, ksize, _dt(x), opts)
    wsb = _query_opts("conv3d_fwd_workspace_bytes_ex", opts, n, gx, gy, gz, cin, cout, ksize, _dt(x))
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device) if wsb else None
    from . import stamps
    rec = torch.full((lay.conv_records + lay.epilogue_records, lay.words), stamps.FILL_I64, dtype=torch.int64, device=x.device)
    call("conv3d_fwd_stamped", _p(x), _p(wp), _p(bias), _p(y), n, gx, gy, gz, cin, cout, wrows, ksize, _dt(x), flags, _p(ws), opts.ptr(), _s(),
         _p(rec), rec.numel() * 8)
    return y, rec


# wgrad workspace = [27-bit tap mask per voxel (k3) | per-slice bias partials]; the masks depend only on the grid, so one workspace per
# (grid shape, stream) is kept and the masks are built once (NRPN_WGRAD_MASK_READY afterwards); the bias partials are consumed by the
# same C call that writes them, or by the reduce_slices launch that follows it on the same stream.
_WGRAD_WS = {}


def _wgrad_workspace(device, key, nbytes):
    # keyed by the stream the wgrad is enqueued on as well: a layer with a frozen parameter keeps its wgrad on the main stream while
    # arena layers of the same grid shape run on the side stream -- their bias partials (and the one-time mask build) must not share
    # a buffer across streams
    key = (device.index, _s()) + key
    ent = _WGRAD_WS.get(key)
    if ent is None or ent[0].numel() < nbytes:
        ent = [torch.empty(nbytes, dtype=torch.uint8, device=device), False]
        _WGRAD_WS[key] = ent
    ready, ent[1] = ent[1], True
    return ent[0], ready


# Layer-chain hints for ConvFn (ConvMode.chain, set by modules that own a conv+ReLU -> conv chain, e.g. RPNHead):
#   CHAIN_MASK_INPUT_GRAD  this conv is the ONLY consumer of its input, and the input is the output of a fused conv+ReLU
#   CHAIN_GRAD_PREMASKED   this conv+ReLU's output goes only to a conv with CHAIN_MASK_INPUT_GRAD: the incoming gradient is
#                          already multiplied by the ReLU mask, so the separate relu_backward pass is skipped
CHAIN_MASK_INPUT_GRAD, CHAIN_GRAD_PREMASKED = 1, 2

# What a ConvFn launch does besides the GEMM.  chain: CHAIN_* above; stats: holder dict for BatchNorm statistics out of the epilogue and
# affine: (scale, shift) of a folded eval-mode BatchNorm (both: _conv_fwd); segs: x is a ragged voxel list [1, sum voxels, 1, 1, C] of grids
# with these (X, Y, Z) dims; differentiable: decided by the caller, where grad mode is visible (None: ctx.needs_input_grad, which mirrors
# requires_grad even under no_grad).  A plain bool in its place means ConvMode(relu).
ConvMode = namedtuple("ConvMode", "relu chain stats affine segs differentiable", defaults=(False, 0, None, None, None, None))
_RELU_ONLY = {False: ConvMode(False), True: ConvMode(True)}


IN_BACKWARD = [0]       # > 0 while ConvFn.backward is enqueuing (bench.py tells forward launches from dgrad launches of the same entry point)


class ConvFn(torch.autograd.Function):
    """Conv3d k in {1,3}, stride 1, 'same' padding, channels-last, optional fused bias + ReLU.
    ``weights``: one or more reference-layout parameters that share the GEMM (their rows are concatenated, then padded to
    ``rows_total``); the output has rows_total channels."""

    @staticmethod
    def forward(ctx, x, pack, rows_total, mode, out_f32, nw, *wb):
        relu, chain, stats, affine, segs, differentiable = mode if isinstance(mode, ConvMode) else _RELU_ONLY[bool(mode)]
        if differentiable is None:
            differentiable = any(ctx.needs_input_grad)
        weights, biases = wb[:nw], wb[nw:]
        _chk(x)
        ksize = weights[0].shape[2] if weights[0][0].numel() != x.shape[-1] else 1
        need_dgrad = x.requires_grad
        wp, wpd = pack.get(weights, x.dtype, rows_total, need_dgrad, x.shape[-1])
        bias = None
        if biases[0] is not None:
            single = nw == 1 and biases[0].numel() == rows_total
            bias = biases[0].detach().float().contiguous() if single else pack.fused_bias(biases, rows_total)
        out_dtype = torch.float32 if out_f32 else x.dtype
        x3 = _x3_ok(x, ksize, segs, rows_total, differentiable)
        xin = x
        if x3:      # bf16x3: split operands on the bf16 MFMA kernels, fp32 rows out; BatchNorm statistics then come from their own pass
            wp, wpd = _x3_weights(pack, weights, wp, wpd)
            xin, stats = split3(x, _ACT_I)[0], None
        if affine is not None:
            # eval-mode BatchNorm folded into this conv: y = acc * scale + shift (the conv's own bias is inside `shift`); forward only --
            # the HIP path has no eval-mode BatchNorm backward either (BatchNormFn.backward)
            scale, shift = affine
            y = _conv_fwd(xin, wp, shift, rows_total, rows_total, ksize, CONV_RELU if relu else 0, out_dtype, segs, None, None, scale)
            ctx.mark_non_differentiable(y)       # hip_nn._can_fold only folds when nothing upstream needs a gradient
            return y
        y = _conv_fwd(xin, wp, bias, rows_total, rows_total, ksize, CONV_RELU if relu else 0, out_dtype, segs, None, stats)
        ctx.save_for_backward(x, y if relu else None, wpd, *weights)
        ctx.x3 = x3
        ctx.meta = (rows_total, relu, nw, ksize, biases[0] is not None, segs, chain)
        ctx.sinks = ([_sink(w) for w in weights], [_sink(b) for b in biases])
        ctx.sinks_complete = _sinks_cover(wb, ctx.sinks[0] + ctx.sinks[1])
        return y

    @staticmethod
    def backward(ctx, dy):
        IN_BACKWARD[0] += 1
        try:
            return ConvFn._backward(ctx, dy)
        finally:
            IN_BACKWARD[0] -= 1

    @staticmethod
    def _backward(ctx, dy):
        x, y, wpd, *weights = ctx.saved_tensors
        rows_total, relu, nw, ksize, has_bias, segs, chain = ctx.meta
        n, gx, gy, gz, cin = x.shape
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = dy.to(x.dtype)
        if relu and not (chain & CHAIN_GRAD_PREMASKED):
            dyr = torch.empty_like(dy)
            yy = y if y.dtype == dy.dtype else y.to(dy.dtype)
            call("relu_backward", _p(yy), _p(dy), _p(dyr), dy.numel(), _dt(dy), _s())
            dy = dyr
        dx = None
        x3 = ctx.x3
        dyp = None
        if x3 and segs is not None:
            raise lib.NrpnError("bf16x3 backward of a ragged conv: the split dgrad / wgrad launches take no segments")
        if x3:
            # bf16x3: one pass over dy writes the interleaved operand of the dgrad launch and the planes of the wgrad launch
            dys, dyp = split3(dy, _ACT_I if ctx.needs_input_grad[0] else None, 3, _DY_P)
        if ctx.needs_input_grad[0]:
            _wait_dgrad_operands()
            # CHAIN_MASK_INPUT_GRAD: x is the ReLU output of the layer that receives dx and this conv is its only consumer, so that
            # layer's ReLU backward is applied in this dgrad's epilogue (dx = 0 where x <= 0) instead of a separate pass
            mask = x if (chain & CHAIN_MASK_INPUT_GRAD) and segs is None else None
            if x3:
                dx = _conv_fwd(dys, wpd, None, cin, cin, ksize, 0, torch.float32)
                if mask is not None:          # fp32 rows out of bf16 operands: the epilogue takes no mask, one elementwise pass instead
                    dxm = torch.empty_like(dx)
                    call("relu_backward", _p(x), _p(dx), _p(dxm), dx.numel(), _dt(dx), _s())
                    dx = dxm
            else:
                dx = _conv_fwd(dy, wpd, None, cin, cin, ksize, 0, x.dtype, segs, mask)
        return (dx, None, None, None, None, None,
                *_on_wgrad_stream(x.device, (x, dy, dyp), ctx.sinks_complete, lambda: ConvFn._wgrad(ctx, x, dy, dyp, weights)))

    @staticmethod
    def _wgrad(ctx, x, dy, dyp, weights):
        """Weight (+ bias) gradient of the layer.  With ``dyp`` (bf16x3): dW = dy_hi (x) x_hi + dy_hi (x) x_lo + dy_lo (x) x_hi as ONE bf16
        wgrad launch over three "scenes" (planes stacked on the batch axis, which the kernel sums over), and the bias gradient is the fp32
        column sum of dy."""
        rows_total, relu, nw, ksize, has_bias, segs, chain = ctx.meta
        n, gx, gy, gz, cin = x.shape
        x3, dt = dyp is not None, _dt(x)
        if x3:
            x, dy, dy2d, n, dt = split3(x, None, 3, _X_P)[1], dyp, dy.reshape(-1, rows_total), 3 * n, BF16
        dest = _WgradDest(weights, *ctx.sinks, has_bias and not x3, rows_total)
        shape = (n, gx, gy, gz, cin, rows_total, rows_total, ksize, dt)
        slices = query("conv3d_wgrad_slices", *shape)
        gwp = torch.empty((slices, ksize ** 3, rows_total, cin), dtype=torch.float32, device=x.device)     # per-slice partials, summed by deliver()
        ws, mask_ready = _wgrad_workspace(x.device, (n, gx, gy, gz, ksize, segs), query("conv3d_wgrad_workspace_bytes", *shape))
        wflags = dest.flags | (2 if mask_ready else 0)
        if segs is None or ksize == 1:
            call("conv3d_wgrad", _p(x), _p(dy), _p(gwp), _p(dest.gb), n, gx, gy, gz, cin, rows_total, rows_total, ksize, dt, wflags, _p(ws), _s())
        else:
            dims = _seg_dims(segs)
            call("conv3d_wgrad_ragged", _p(x), _p(dy), _p(gwp), _p(dest.gb), len(segs), ctypes.addressof(dims), cin, rows_total, rows_total, ksize,
                 dt, wflags, _p(ws), _s())
        bias_part = ws.data_ptr() + query("conv3d_wgrad_bias_offset", n, gx, gy, gz, ksize) if dest.defer_bias else 0
        res = dest.deliver(gwp, slices, bias_part)
        return (*res[:nw], *dest.summed_bias(dy2d)) if x3 and has_bias else res


class _WgradDest:
    """Where the weight / bias gradients of one conv GEMM go (one weight, or several sharing the GEMM's rows), decided once per wgrad launch:
    the table in DESIGN.md 3.10, "Where a parameter gradient goes".  ``has_bias``: the launch produces the bias gradient (False for a conv
    without bias and for the bf16x3 forms, which call ``summed_bias`` instead).  The launch gets ``gb`` as its bias pointer and ``flags``:
    1 = add the bias gradient into gb, the sink's slot; 4 = leave the per-slice bias partials in the workspace for ``deliver``."""

    def __init__(self, weights, wsinks, bsinks, has_bias, rows_total):
        self.weights, self.wsinks, self.bsinks, self.has_bias, self.rows_total = weights, wsinks, bsinks, has_bias, rows_total
        one = len(weights) == 1
        self.direct_bias = has_bias and one and bsinks[0] is not None
        # arena layout = the partials' own layout: weight-slice sum and bias-slice sum go out as ONE launch (reduce_slices)
        self.fused_reduce = one and wsinks[0] is not None and wsinks[0].flat is not None and rows_total == weights[0].shape[0]
        self.defer_bias = self.fused_reduce and self.direct_bias
        self.flags = int(self.direct_bias) | (4 if self.defer_bias else 0)
        self.gb = bsinks[0].slot if self.direct_bias else (torch.empty(rows_total, dtype=torch.float32, device=weights[0].device) if has_bias else None)

    def deliver(self, gwp, slices, bias_part):
        """Sum the per-slice partials ``gwp`` [slices, taps, rows_total, cin] into their destinations; ``bias_part``: address of the per-slice
        bias partials (read when defer_bias).  -> (*weight grads, *bias grads), None where a sink took the gradient."""
        taps, cin = gwp.shape[1], gwp.shape[3]
        gws, gbs, row = [], [], 0
        for w, sk, bsk in zip(self.weights, self.wsinks, self.bsinks):
            rows = w.shape[0]
            if self.fused_reduce:        # ordered sum of the slices, added in place
                call("reduce_slices", _p(gwp), slices, gwp[0].numel(), _p(sk.flat), 1, bias_part if self.defer_bias else 0, self.rows_total,
                     self.rows_total, _p(self.gb) if self.defer_bias else 0, 1, _s())
            elif sk is not None:
                if not sk.slot.is_contiguous():
                    raise lib.NrpnError("a GEMM-layout arena weight reached a fused multi-weight GEMM (mark the module _nrpn_fused_gemm)")
                call("unpack_conv_wgrad", _p(gwp), rows, cin, taps, self.rows_total, row, _p(sk.slot), 1, slices, _s())
            else:
                gw = torch.empty_like(w, dtype=torch.float32)
                call("unpack_conv_wgrad", _p(gwp), rows, cin, taps, self.rows_total, row, _p(gw), 0, slices, _s())
            if sk is not None:
                sk.notify()
            gws.append(None if sk is not None else gw)
            if self.direct_bias:
                bsk.notify()
            gbs.append(hand_in(bsk, self.gb[row:row + rows], copy=True) if self.has_bias and not self.direct_bias else None)
            row += rows
        return (*gws, *gbs)

    def summed_bias(self, dy2d):
        """Bias gradients from the fp32 column sums of dy [voxels, rows_total]."""
        gb, out, row = column_sum_f32(dy2d), [], 0
        for w, bsk in zip(self.weights, self.bsinks):
            out.append(hand_in(bsk, gb[row:row + w.shape[0]], copy=True))
            row += w.shape[0]
        return out

    def nothing(self):
        """No voxel contributed: zero gradients are handed back; sinks are only told that this use of the parameter is done."""
        def zero(sk, shape):
            if sk is None:
                return torch.zeros(tuple(shape), dtype=torch.float32, device=self.weights[0].device)
            sk.notify()
        gws = [zero(sk, w.shape) for w, sk in zip(self.weights, self.wsinks)]
        return (*gws, *[zero(sk, w.shape[:1]) if self.has_bias else None for w, sk in zip(self.weights, self.bsinks)])


def _on_wgrad_stream(device, tensors, sinks_complete, fn):
    """Run ``fn()`` (a weight-gradient launch sequence) on the weight-gradient side stream behind the current stream when all its results
    go into GradSinks, or inline when one has to be handed back to autograd / the side stream is off.  ``tensors``: what fn's kernels read."""
    side = _wgrad_side_stream(device) if sinks_complete else None
    if side is None:
        return fn()
    side.wait_stream(torch.cuda.current_stream(device))      # the operands are ready; also orders fn behind the arena's zero fill
    tensors = tuple(t for t in tensors if t is not None)
    for t in tensors:
        t.record_stream(side)
    _WGRAD_SIDE["keep"].append(tensors)
    with torch.cuda.stream(side):
        res = fn()
    if not _WGRAD_SIDE["dirty"]:        # first side-stream work of this backward pass: join when the pass ends
        _WGRAD_SIDE["dirty"] = True
        torch.autograd.Variable._execution_engine.queue_callback(wgrad_stream_join)
    return res


# ======================================================================================================================
# sampled-anchor cones of the RPN head (training)
# ======================================================================================================================
CONE_ENABLED = [_os.environ.get("NRPN_CONE", "1") != "0"]      # A/B switch: cone evaluation of the RPN head in training; default on


class ConePlan:
    """Sorted voxel lists S_0 c ... c S_depth of one training step (csrc/cone.hip) over the ragged (level-major, scene-major) voxel space
    of the pyramid: ``lists`` int32 [depth + 1, total, 2] on the device, ``counts`` on the host once the sampler's read-back has happened."""

    def __init__(self, grids, n_scenes, depth, device):
        self.grids = [tuple(int(v) for v in g) for g in grids]
        self.n, self.depth = int(n_scenes), int(depth)
        self.segs = [g for g in self.grids for _ in range(self.n)]
        self.nseg = len(self.segs)
        self.dims = _seg_dims(self.segs)
        self.dims_ptr = ctypes.addressof(self.dims)
        self.cells = [g[0] * g[1] * g[2] for g in self.grids]
        self.level_start = [0]
        for c in self.cells:
            self.level_start.append(self.level_start[-1] + c * self.n)
        self.total = self.level_start[-1]
        self.lists = torch.empty((self.depth + 1, self.total, 2), dtype=torch.int32, device=device)
        self.counts_dev = torch.empty(self.depth + 2, dtype=torch.int32, device=device)
        self.counts = None

    def finish(self, host):
        if host[self.depth + 1]:
            raise RuntimeError("cone_build: a sampled anchor index lies outside the anchor pyramid")
        self.counts = [int(v) for v in host[:self.depth + 1]]

    def rows(self, k):
        return self.lists[k].data_ptr(), self.counts[k]

    def tensors(self):
        return [self.lists, self.counts_dev]


# A/B switch: with the cone head and no box gradient needed, take the sampled loss and its gradient from the head rows of S_0 directly
# (no flattened logits / deltas, no dense gradient buffers); default on
CONE_ROWS_LOSS = [_os.environ.get("NRPN_CONE_ROWS_LOSS", "1") != "0"]


def _head_levels(plan):
    """(level_start, cells, levels) of ``plan`` as the host arrays nrpn_rpn_sampled_loss_rows_f32 / nrpn_head_grad_rows copy into their launch."""
    if getattr(plan, "_head_levels", None) is None:
        L = len(plan.cells)
        plan._head_levels = ((ctypes.c_int64 * L)(*plan.level_start[:L]), (ctypes.c_int64 * L)(*plan.cells))
    start, cells = plan._head_levels
    return ctypes.addressof(start), ctypes.addressof(cells), len(plan.cells)


def cone_from_indices(plan, pos, neg, table):
    """Build ``plan`` from flat batch indices (scene * T + anchor), e.g. a test's injected sample; synchronises (sizes of boolean selections)."""
    T, n = table.total, plan.n
    ps = [(pos[(pos >= i * T) & (pos < (i + 1) * T)] - i * T).long() for i in range(n)]
    ns = [(neg[(neg >= i * T) & (neg < (i + 1) * T)] - i * T).long() for i in range(n)]
    mp, mn = max(1, max(p.numel() for p in ps)), max(1, max(q.numel() for q in ns))
    dev = plan.lists.device
    out_pos = torch.zeros((n, mp), dtype=torch.int64, device=dev)
    out_neg = torch.zeros((n, mn), dtype=torch.int64, device=dev)
    cnt = []
    for i in range(n):
        out_pos[i, :ps[i].numel()] = ps[i]
        out_neg[i, :ns[i].numel()] = ns[i]
        cnt += [ps[i].numel(), ns[i].numel(), 0]
    counts = torch.tensor(cnt, dtype=torch.int32, device=dev)
    plan.finish(cone_build(plan, out_pos, out_neg, counts, table).cpu().tolist())
    return plan


def cone_build(plan, out_pos, out_neg, counts, table):
    """Enqueue the list build of ``plan`` on the current stream from the sampler's raw output (see sample_pos_neg); no synchronisation."""
    if table.A * sum(plan.cells) != table.total or len(table.counts) != len(plan.grids):
        raise lib.NrpnError("cone_build: the anchor table and the feature grids disagree")
    offs = (ctypes.c_int64 * (len(table.offsets)))(*[int(v) for v in table.offsets])
    ws = torch.empty(query("cone_workspace_bytes", plan.total), dtype=torch.uint8, device=out_pos.device)
    call("cone_build", _p(out_pos), _p(out_neg), _p(counts), plan.n, out_pos.shape[1], out_neg.shape[1], len(plan.grids), ctypes.addressof(offs),
         table.A, plan.dims_ptr, plan.depth, _p(plan.lists), plan.total, _p(plan.counts_dev), _p(ws), _s())
    return plan.counts_dev


def conv_rows_fwd(x, wp, bias, y, plan, k, cin, cout, wrows, ksize, flags, mask=None):
    """Forward / dgrad of a k1 / k3 conv on the rows of list S_k only: x [total, cin], y [total, cout] (rows outside the list untouched)."""
    rows, nrows = plan.rows(k)
    if nrows == 0:
        return y
    if y.dtype == torch.float32 and x.dtype == torch.bfloat16:
        flags |= CONV_OUT_F32
    if bias is not None:
        flags |= CONV_BIAS
    wsb = lib.query("conv3d_fwd_rows_workspace_bytes", nrows, cin, cout, ksize, _dt(x))      # (not memoised: the list length changes every step)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device) if wsb else None
    call("conv3d_fwd_rows", _p(x), _p(wp), _p(bias), _p(y), rows, nrows, plan.nseg, plan.dims_ptr, cin, cout, wrows, ksize, _dt(x), flags, _p(mask),
         _p(ws), _s())
    return y


def conv_rows_wgrad(x, dy, weights, biases, rows_total, ksize, plan, k, sinks=None):
    """Weight (+ bias) gradient of a conv from the rows of S_k only (dy is zero elsewhere); delivery as ConvFn._wgrad.
    ``sinks``: (weight sinks, bias sinks) looked up by the caller on the original Parameter objects; default: on ``weights`` / ``biases``."""
    rows, nrows = plan.rows(k)
    cin = x.shape[-1]
    wsinks, bsinks = sinks if sinks is not None else ([_sink(w) for w in weights], [_sink(b) for b in biases])
    dest = _WgradDest(weights, wsinks, bsinks, biases[0] is not None, rows_total)
    if nrows == 0:      # nothing sampled
        return dest.nothing()
    slices = lib.query("conv3d_wgrad_slices", 1, nrows, 1, 1, cin, rows_total, rows_total, ksize, _dt(x))      # (not memoised: nrows changes every step)
    gwp = torch.empty((slices, ksize ** 3, rows_total, cin), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(256, slices * rows_total * 4), dtype=torch.uint8, device=x.device)
    call("conv3d_wgrad_rows", _p(x), _p(dy), _p(gwp), _p(dest.gb), rows, nrows, plan.nseg, plan.dims_ptr, cin, rows_total, rows_total, ksize, _dt(x),
         dest.flags, _p(ws), _s())
    return dest.deliver(gwp, slices, ws.data_ptr())


def conv_rows_wgrad_x3(x, dy, weights, biases, rows_total, ksize, plan, k, sinks=None):
    """bf16x3 form of conv_rows_wgrad (one weight): the three split products dy_hi (x) x_hi, dy_hi (x) x_lo, dy_lo (x) x_hi as three bf16
    row-list launches whose slice partials are summed together by the usual delivery; bias gradient = fp32 column sum of dy (zero outside
    the list)."""
    rows, nrows = plan.rows(k)
    if nrows == 0 or len(weights) != 1:
        return conv_rows_wgrad(x, dy, weights, biases, rows_total, ksize, plan, k, sinks)
    cin = x.shape[-1]
    wsinks, bsinks = sinks if sinks is not None else ([_sink(w) for w in weights], [_sink(b) for b in biases])
    dest = _WgradDest(weights, wsinks, bsinks, False, rows_total)
    xpl = split3(x, None, 2, 0b10)[1]          # [hi ; lo]
    dpl = split3(dy, None, 2, 0b10)[1]
    slices = lib.query("conv3d_wgrad_slices", 1, nrows, 1, 1, cin, rows_total, rows_total, ksize, BF16)
    gwp = torch.empty((3 * slices, ksize ** 3, rows_total, cin), dtype=torch.float32, device=x.device)
    ws = torch.empty(max(256, slices * rows_total * 4), dtype=torch.uint8, device=x.device)
    for j, (di, xi) in enumerate(((0, 0), (0, 1), (1, 0))):
        call("conv3d_wgrad_rows", _p(xpl[xi]), _p(dpl[di]), gwp[j * slices].data_ptr(), 0, rows, nrows, plan.nseg, plan.dims_ptr, cin, rows_total,
             rows_total, ksize, BF16, 0, _p(ws), _s())
    gw = dest.deliver(gwp, 3 * slices, 0)[0]
    return (gw, *(dest.summed_bias(dy.reshape(-1, rows_total)) if biases[0] is not None else (None,)))


class ConeHeadFn(torch.autograd.Function):
    """The whole RPN head in training -- conv_depth x [Conv3d k3 + ReLU] + the fused cls / bbox GEMM over all pyramid levels + the
    reference's flatten (anchor.py:RPNHead, rpn.py:105-130) -- evaluated on the sampled-anchor cones of ``plan`` only: layer i (0-based,
    D layers) is computed on S_{D-1-i}, the output GEMM on S_0; backward visits the same sets (weight gradients from the listed rows, input
    gradients on the next larger set, the first layer's input gradient densely per level for the FPN).  One autograd node, ~25 launches,
    instead of ~150 for the dense head at four levels.  logits / deltas are exact on the sampled anchors' voxels and ZERO elsewhere: only
    the training loss, which reads the sampled rows, may consume them (RegionProposalNetwork.forward decides).
    With a loss pack ``(targets, pos, neg, beta, T)`` (CONE_ROWS_LOSS; no loss term differentiates through the decoded boxes) the node ends in
    the sampled loss itself, read in place from the head rows of S_0: it returns (loss_objectness, smooth-L1 box loss, deltas of the positives
    [npos, dw], non-differentiable), its backward takes the two scalar gradients, and nothing outside S_0 is filled, copied or scaled."""

    @staticmethod
    def forward(ctx, plan, head, A, dw, pack, *tensors):
        L = len(plan.grids)
        feats = tensors[:L]
        convs = [m for m in head.conv if isinstance(m, torch.nn.Conv3d)]
        D = len(convs)
        cw, cb = tensors[L:L + D], tensors[L + D:L + 2 * D]
        ow, ob = tensors[L + 2 * D:L + 2 * D + 2], tensors[L + 2 * D + 2:L + 2 * D + 4]
        if plan.depth != max(D - 1, 0):
            raise lib.NrpnError("ConeHeadFn: the plan must hold the lists S_0 .. S_{conv_depth - 1}")
        n, C = feats[0].shape[0], feats[0].shape[-1]
        dt = feats[0].dtype
        dev = feats[0].device
        V = plan.total
        for f in feats:
            _chk(f)
        x0 = torch.cat([f.reshape(-1, C) for f in feats], dim=0)
        if x0.shape[0] != V:
            raise lib.NrpnError("ConeHeadFn: feature maps and cone plan disagree on the voxel count")
        from .model.hip_nn import _pack_of
        hs, ops_w = [x0], []
        need_dgrad = any(f.requires_grad for f in feats)
        x3 = SPLIT3[0] and dt == torch.float32 and C % 32 == 0      # bf16x3: the 3x3x3 layers multiply split operands (the output GEMM stays fp32)
        for i, cv in enumerate(convs):
            wp, wpd = _pack_of(cv).get([cw[i]], dt, C, True, C)
            bias = cb[i].detach().float().contiguous() if cb[i] is not None else None
            y = torch.empty((V, C), dtype=dt, device=dev)
            if x3:
                wp, wpd = _x3_weights(_pack_of(cv), [cw[i]], wp, wpd)
                # (rows outside the cone hold whatever the allocator left: split like the rest, never read by a listed row's taps)
                conv_rows_fwd(split3(hs[-1], _ACT_I)[0], wp, bias, y, plan, D - 1 - i, 3 * C, C, C, 3, CONV_RELU)
            else:
                conv_rows_fwd(hs[-1], wp, bias, y, plan, D - 1 - i, C, C, C, 3, CONV_RELU)
            hs.append(y)
            ops_w.append(wpd)
        rows_total = head.head_rows
        wpo, wpdo = head._pack.get(list(ow), dt, rows_total, True, C)
        bias_o = head._pack.fused_bias(ob, rows_total) if ob[0] is not None else None
        # with a loss pack only the rows of S_0 are ever read (the loss kernel visits the sampled anchors' rows): no fill
        out = (torch.zeros if pack is None else torch.empty)((V, rows_total), dtype=torch.float32, device=dev)
        conv_rows_fwd(hs[-1], wpo, bias_o, out, plan, 0, C, rows_total, rows_total, 1, 0)
        T = sum(plan.cells) * A
        ctx.save_for_backward(*hs, *ops_w, wpdo, *cw, *[b for b in cb if b is not None], *ow, *[b for b in ob if b is not None])
        ctx.meta = (plan, head, A, dw, L, D, n, C, dt, rows_total, [b is not None for b in cb], [b is not None for b in ob], need_dgrad)
        ctx.x3 = x3
        # gradient sinks are attributes of the Parameter objects: looked up here, on the objects the caller passed (as ConvFn does)
        ctx.sinks = ([_sink(w) for w in cw], [_sink(b) for b in cb], [_sink(w) for w in ow], [_sink(b) for b in ob])
        ctx.rows_loss = None
        if pack is not None:
            # the sampled loss read in place from the head rows: no flattened logits / deltas, compact gradient factors for the backward
            targets, pos, neg, beta, pack_T = pack
            if pack_T != T or n != plan.n:
                raise lib.NrpnError("ConeHeadFn: the loss pack and the cone plan disagree on the anchor count")
            targets = targets.contiguous()
            _chk(targets, pos, neg)
            npos, nneg = pos.numel(), neg.numel()
            loss2 = torch.empty(2, dtype=torch.float32, device=dev)
            g_obj = torch.empty(npos + nneg, dtype=torch.float32, device=dev)
            g_reg = torch.empty((npos, dw), dtype=torch.float32, device=dev)
            deltas_pos = torch.empty((npos, dw), dtype=torch.float32, device=dev)
            call("rpn_sampled_loss_rows_f32", _p(out), rows_total, *_head_levels(plan), n, T, A, dw, _p(targets), _p(pos), npos, _p(neg), nneg,
                 float(beta), _p(loss2), _p(g_obj), _p(g_reg), _p(deltas_pos), _s())
            ctx.rows_loss = (pos, neg, g_obj, g_reg, T)
            ctx.mark_non_differentiable(deltas_pos)
            ctx.set_materialize_grads(False)      # no zero tensor (a fill launch) for the gradient slot of deltas_pos
            return loss2[0], loss2[1], deltas_pos
        logits = torch.empty((n, T), dtype=torch.float32, device=dev)
        deltas = torch.empty((n, T, dw), dtype=torch.float32, device=dev)
        off = 0
        for l, c in enumerate(plan.cells):
            for i in range(n):
                r0 = plan.level_start[l] + i * c
                call("head_flatten_f32", _p(out[r0:r0 + c]), c, rows_total, A, dw, _p(logits[i, off:]), _p(deltas[i, off:]), _s())
            off += c * A
        return logits, deltas

    @staticmethod
    def backward(ctx, g_logits, g_deltas, _g_deltas_pos=None):
        IN_BACKWARD[0] += 1
        try:
            return ConeHeadFn._backward(ctx, g_logits, g_deltas)
        finally:
            IN_BACKWARD[0] -= 1

    @staticmethod
    def _backward(ctx, g_logits, g_deltas):
        """``g_logits`` / ``g_deltas``: the dense gradients of the two outputs, or -- with a loss pack -- the scalar gradients of the two losses."""
        plan, head, A, dw, L, D, n, C, dt, rows_total, has_cb, has_ob, need_dgrad = ctx.meta
        saved = list(ctx.saved_tensors)
        hs, saved = saved[:D + 1], saved[D + 1:]
        wpds, saved = saved[:D], saved[D:]
        wpdo, saved = saved[0], saved[1:]
        cw, saved = saved[:D], saved[D:]
        cb = []
        for h in has_cb:
            cb.append(saved.pop(0) if h else None)
        ow, saved = saved[:2], saved[2:]
        ob = [saved.pop(0) if h else None for h in has_ob]
        dev = hs[0].device
        V = plan.total
        dout = torch.empty((V, rows_total), dtype=dt, device=dev)
        if ctx.rows_loss is not None:
            # only the rows of S_0 are written (sampled columns: factor x upstream scalar, read on the device; the rest of the row zero);
            # the weight gradient and the dgrad below read those rows only
            pos, neg, g_obj, g_reg, T = ctx.rows_loss
            # (gradients are not materialised on this path: a loss the caller left out of its total arrives as None)
            s_obj, s_reg = [torch.zeros((), dtype=torch.float32, device=dev) if g is None else g.float().contiguous() for g in (g_logits, g_deltas)]
            rows, nrows = plan.rows(0)
            call("head_grad_rows", _p(dout), _dt(dout), rows_total, rows, nrows, *_head_levels(plan), n, T, A, dw, _p(pos), pos.numel(), _p(neg),
                 neg.numel(), _p(g_obj), _p(g_reg), _p(s_obj), _p(s_reg), _s())
        else:
            g_logits, g_deltas = g_logits.contiguous(), g_deltas.contiguous()
            off = 0
            for l, c in enumerate(plan.cells):
                for i in range(n):
                    r0 = plan.level_start[l] + i * c
                    call("head_unflatten", _p(g_logits[i, off:]), _p(g_deltas[i, off:]), c, rows_total, A, dw, 0, _p(dout[r0:r0 + c]), _dt(dout), _s())
                off += c * A
        _wait_dgrad_operands()

        cws, cbs, ows, obs = ctx.sinks
        # output GEMM: weight / bias gradients from the rows of S_0; input gradient on S_0 with the last layer's ReLU mask
        g_ow = _on_wgrad_stream(dev, [hs[D], dout, plan.lists], _sinks_cover((*ow, *ob), (*ows, *obs)),
                                lambda: conv_rows_wgrad(hs[D], dout, list(ow), list(ob), rows_total, 1, plan, 0, (ows, obs)))
        dh = torch.zeros((V, C), dtype=dt, device=dev)
        conv_rows_fwd(dout, wpdo, None, dh, plan, 0, rows_total, C, C, 1, 0, mask=hs[D] if D > 0 else None)
        g_cw, g_cb = [None] * D, [None] * D
        g_feats = [None] * L
        if D == 0 and need_dgrad:       # no hidden layers: the output GEMM reads the FPN maps directly
            for l in range(L):
                g = plan.grids[l]
                g_feats[l] = dh[plan.level_start[l]:plan.level_start[l + 1]].view(n, g[0], g[1], g[2], C)
        x3 = ctx.x3
        rows_wgrad = conv_rows_wgrad_x3 if x3 else conv_rows_wgrad
        for i in range(D - 1, -1, -1):
            k = D - 1 - i
            x_i, dy_i = hs[i], dh
            res = _on_wgrad_stream(dev, [x_i, dy_i, plan.lists], _sinks_cover((cw[i], cb[i]), (cws[i], cbs[i])),
                                   lambda x_i=x_i, dy_i=dy_i, i=i, k=k: rows_wgrad(x_i, dy_i, [cw[i]], [cb[i]], C, 3, plan, k, ([cws[i]], [cbs[i]])))
            g_cw[i] = res[0]
            g_cb[i] = res[1] if len(res) > 1 else None
            dhs = split3(dh, _ACT_I)[0] if (x3 and (i > 0 or need_dgrad)) else None      # bf16x3: the dgrad launches read the split gradient
            if i > 0:
                dprev = torch.zeros((V, C), dtype=dt, device=dev)
                if x3:       # fp32 rows out of bf16 operands take no epilogue mask: the layer's ReLU backward is one elementwise pass
                    raw = torch.zeros((V, C), dtype=dt, device=dev)
                    conv_rows_fwd(dhs, wpds[i], None, raw, plan, k + 1, 3 * C, C, C, 3, 0)
                    call("relu_backward", _p(hs[i]), _p(raw), _p(dprev), raw.numel(), _dt(raw), _s())
                else:
                    conv_rows_fwd(dh, wpds[i], None, dprev, plan, k + 1, C, C, C, 3, 0, mask=hs[i])
                dh = dprev
            elif need_dgrad:
                # first layer: its input gradient goes to the FPN output convs of every level -- dense, per level (halo kernel on the
                # finest grid); dh is zero outside S_{D-1}
                for l, c in enumerate(plan.cells):
                    g = plan.grids[l]
                    if x3:
                        dyl = dhs[plan.level_start[l]:plan.level_start[l + 1]].view(n, g[0], g[1], g[2], 3 * C)
                        g_feats[l] = _conv_fwd(dyl, wpds[0], None, C, C, 3, 0, torch.float32)
                        continue
                    dyl = dh[plan.level_start[l]:plan.level_start[l + 1]].view(n, g[0], g[1], g[2], C)
                    g_feats[l] = _conv_fwd(dyl, wpds[0], None, C, C, 3, 0, dt)
        return (None, None, None, None, None, *g_feats, *g_cw, *g_cb, *g_ow)


STEM_HALO = [_os.environ.get("NRPN_STEM_HALO", "1") != "0"]      # A/B switch: halo-form stem forward (bf16, stride 2, even Z, Cout 64); default on


class StemFn(torch.autograd.Function):
    """Conv3d(4 -> C, k7, pad 3, stride s) on [N,X,Y,Z,4] (reference feature_extractor.py:336,341)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, cache, affine=None, relu=False):
        _chk(x)
        n, gx, gy, gz, _ = x.shape
        cout = weight.shape[0]
        halo = STEM_HALO[0] and bool(query("stem_halo_supported", gz, cout, stride, _dt(x)))
        key = (weight.data_ptr(), weight._version, x.dtype, _weight_epoch, halo)
        if cache.get("key") != key:
            PACK_COUNT["stem"] += 1
            wc = weight.detach().contiguous()
            if halo:      # bf16 [Cout][50 * 32]: (dx, dy) slot major, 8 z positions x 4 channels inside a slot
                wp = torch.empty((cout, query("stem_halo_kpad")), dtype=x.dtype, device=x.device)
                call("pack_stem_weight_halo", _p(wc), cout, _p(wp), _s())
            else:
                kpad = query("stem_kpad", _dt(x))
                wp = torch.empty((cout, kpad), dtype=x.dtype, device=x.device)
                call("pack_stem_weight", _p(wc), cout, _dt(x), _p(wp), _s())
            cache["key"], cache["wp"] = key, wp
        wp = cache["wp"]
        o = [(g - 1) // stride + 1 for g in (gx, gy, gz)]
        y = torch.empty((n, o[0], o[1], o[2], cout), dtype=x.dtype, device=x.device)
        if affine is not None:       # eval-mode BatchNorm (+ ReLU) folded into the stem: no-grad forward only
            scale, shift = affine
            if halo:
                call("conv3d_stem_fwd_halo", _p(x), _p(wp), _p(shift), _p(scale), _p(y), n, gx, gy, gz, cout, CONV_BIAS | (CONV_RELU if relu else 0), _s())
            else:
                opts = lib.ConvOpts(scale=_p(scale))
                call("conv3d_stem_fwd_ex", _p(x), _p(wp), _p(shift), _p(y), n, gx, gy, gz, cout, stride, _dt(x),
                     CONV_BIAS | (CONV_RELU if relu else 0), opts.ptr(), _s())
            ctx.mark_non_differentiable(y)
            return y
        b = bias.detach().float().contiguous() if bias is not None else None
        if halo:
            call("conv3d_stem_fwd_halo", _p(x), _p(wp), _p(b), 0, _p(y), n, gx, gy, gz, cout, CONV_BIAS if b is not None else 0, _s())
        else:
            call("conv3d_stem_fwd", _p(x), _p(wp), _p(b), _p(y), n, gx, gy, gz, cout, stride, _dt(x), CONV_BIAS if b is not None else 0, _s())
        ctx.save_for_backward(x, weight)
        ctx.meta = (stride, bias is not None)
        ctx.sinks = (_sink(weight), _sink(bias))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        stride, has_bias = ctx.meta
        dy = dy.contiguous()
        n, gx, gy, gz, _ = x.shape
        cout = weight.shape[0]
        kpad = query("stem_kpad", _dt(x))
        slices = query("stem_wgrad_slices", n, gx, gy, gz, cout, stride, _dt(x))
        per = query("stem_wgrad_slice_floats", n, gx, gy, gz, cout, stride, _dt(x))
        gwp = torch.empty((slices, per), dtype=torch.float32, device=x.device)
        wsink, bsink = ctx.sinks
        direct_bias = has_bias and bsink is not None
        gb = bsink.slot if direct_bias else (torch.empty(cout, dtype=torch.float32, device=x.device) if has_bias else None)
        ws = torch.empty(query("stem_wgrad_workspace_bytes", n, gx, gy, gz, cout, stride, _dt(x)), dtype=torch.uint8, device=x.device) if has_bias else None
        call("conv3d_stem_wgrad", _p(x), _p(dy), _p(gwp), _p(gb), n, gx, gy, gz, cout, stride, _dt(x), int(direct_bias), _p(ws), _s())
        if wsink is not None:
            call("unpack_stem_wgrad", _p(gwp), cout, _dt(x), _p(wsink.slot), 1, slices, per, _s())
            wsink.notify()
            gw = None
        else:
            gw = torch.empty_like(weight, dtype=torch.float32)
            call("unpack_stem_wgrad", _p(gwp), cout, _dt(x), _p(gw), 0, slices, per, _s())
        if direct_bias:
            bsink.notify()
            gb = None
        return None, gw, gb, None, None, None, None


BN_STATS_EPOCH = [0]      # bumped by every training-mode BatchNorm forward (running statistics rewritten behind torch's back)


class BatchNormFn(torch.autograd.Function):
    """BatchNorm3d (+ fused ReLU) on channels-last rows; training uses per-rank batch statistics (no SyncBN, as the reference)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rmean, rvar, training, momentum, eps, relu, partials=None):
        _chk(x)
        c = x.shape[-1]
        rows = x.numel() // c
        dev = x.device
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        if training:
            # the statistics kernels update running_mean / running_var through raw pointers (no tensor._version bump): folded eval-mode
            # (scale, shift) pairs cached on the buffer versions would go stale -- hip_nn.bn_fold keys on this epoch as well
            BN_STATS_EPOCH[0] += 1
            mean = torch.empty(c, dtype=torch.float32, device=dev)
            var = torch.empty(c, dtype=torch.float32, device=dev)
            if partials is not None:      # the producing conv left (sum, sum of squares) partials of x in its epilogue: only finish them
                call("bn_stats_finalize", _p(partials), partials.shape[0], rows, c, _p(mean), _p(var), _p(rmean), _p(rvar), float(momentum), _s())
            else:
                ws = torch.empty(query("bn_workspace_bytes", rows, c), dtype=torch.uint8, device=dev)
                call("bn_stats", _p(x), rows, c, _dt(x), _p(mean), _p(var), _p(rmean), _p(rvar), float(momentum), _p(ws), _s())
        else:
            mean, var = rmean.float().contiguous(), rvar.float().contiguous()
        y = torch.empty_like(x)
        call("bn_apply", _p(x), _p(y), rows, c, _dt(x), _p(mean), _p(var), _p(g32), _p(b32), float(eps), int(relu), _s())
        ctx.save_for_backward(x, mean, var, g32, b32)      # y is not kept: the backward recomputes the ReLU mask from x
        ctx.meta = (training, eps, relu)
        ctx.sinks = (_sink(gamma), _sink(beta))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, var, g32, b32 = ctx.saved_tensors
        training, eps, relu = ctx.meta
        if not training:
            raise lib.NrpnError("BatchNorm backward in eval mode is not supported by the HIP path")
        dy = dy.contiguous()
        c = x.shape[-1]
        rows = x.numel() // c
        dev = x.device
        dx = torch.empty_like(x)
        dgamma = torch.empty(c, dtype=torch.float32, device=dev)
        dbeta = torch.empty(c, dtype=torch.float32, device=dev)
        ws = torch.empty(query("bn_workspace_bytes", rows, c), dtype=torch.uint8, device=dev)
        gsink, bsink = ctx.sinks
        call("bn_backward", _p(x), 0, _p(dy), _p(dx), rows, c, _dt(x), _p(mean), _p(var), _p(g32), _p(b32), float(eps), int(relu), _p(dgamma),
             _p(dbeta), _p(gsink.slot) if gsink is not None else 0, _p(bsink.slot) if bsink is not None else 0, _p(ws), _s())
        if gsink is not None:
            gsink.notify()
            dgamma = None
        if bsink is not None:
            bsink.notify()
            dbeta = None
        return dx, dgamma, dbeta, None, None, None, None, None, None, None


class MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p, ceil_mode):
        _chk(x)
        n, gx, gy, gz, c = x.shape
        o = [query("pool_out_size", g, k, s, p, int(ceil_mode)) for g in (gx, gy, gz)]
        y = torch.empty((n, o[0], o[1], o[2], c), dtype=x.dtype, device=x.device)
        arg = torch.empty(y.shape, dtype=torch.int8, device=x.device) if x.requires_grad else None
        call("maxpool3d_fwd", _p(x), _p(y), _p(arg), n, gx, gy, gz, c, k, s, p, int(ceil_mode), _dt(x), _s())
        ctx.save_for_backward(arg)
        ctx.meta = (x.shape, k, s, p, ceil_mode)
        return y

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        shape, k, s, p, ceil_mode = ctx.meta
        dy = dy.contiguous()
        n, gx, gy, gz, c = shape
        dx = torch.empty(shape, dtype=dy.dtype, device=dy.device)
        call("maxpool3d_bwd", _p(dy), _p(arg), _p(dx), n, gx, gy, gz, c, k, s, p, int(ceil_mode), _dt(dy), _s())
        return dx, None, None, None, None


class UpsampleAddFn(torch.autograd.Function):
    """fine += nearest_upsample(coarse), in place on ``fine`` (FPN top-down, reference fpn.py:150-155)."""

    @staticmethod
    def forward(ctx, fine, coarse):
        _chk(fine, coarse)
        n, fx, fy, fz, c = fine.shape
        _, cx, cy, cz, _ = coarse.shape
        call("upsample_add_fwd", _p(fine), _p(coarse), n, fx, fy, fz, cx, cy, cz, c, _dt(fine), _s())
        ctx.mark_dirty(fine)
        ctx.meta = (fine.shape, coarse.shape)
        return fine

    @staticmethod
    def backward(ctx, d):
        fshape, cshape = ctx.meta
        d = d.contiguous()
        n, fx, fy, fz, c = fshape
        _, cx, cy, cz, _ = cshape
        dc = torch.empty(cshape, dtype=d.dtype, device=d.device)
        call("upsample_add_bwd", _p(d), _p(dc), n, fx, fy, fz, cx, cy, cz, c, _dt(d), 0, _s())
        return d, dc


class SubsampleFn(torch.autograd.Function):
    """Every s-th voxel per axis (the spatial part of a stride-s 1x1x1 convolution)."""

    @staticmethod
    def forward(ctx, x, s):
        _chk(x)
        n, gx, gy, gz, c = x.shape
        o = [(g - 1) // s + 1 for g in (gx, gy, gz)]
        y = torch.empty((n, o[0], o[1], o[2], c), dtype=x.dtype, device=x.device)
        call("subsample3d", _p(x), _p(y), n, gx, gy, gz, c, s, 0, _dt(x), _s())
        ctx.meta = (x.shape, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        shape, s = ctx.meta
        dy = dy.contiguous()
        n, gx, gy, gz, c = shape
        dx = torch.empty(shape, dtype=dy.dtype, device=dy.device)
        call("subsample3d", _p(dy), _p(dx), n, gx, gy, gz, c, s, 1, _dt(dy), _s())
        return dx, None


class AddReluFn(torch.autograd.Function):
    """y = relu(a + b): the residual join of a bottleneck (reference feature_extractor.py:63-66)."""

    @staticmethod
    def forward(ctx, a, b, relu):
        a, b = a.contiguous(), b.contiguous()
        _chk(a, b)
        y = torch.empty_like(a)
        call("add_relu", _p(a), _p(b), _p(y), a.numel(), int(relu), _dt(a), _s())
        ctx.relu = relu
        ctx.save_for_backward(y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.relu:
            g = torch.empty_like(dy)
            call("relu_backward", _p(y), _p(dy), _p(g), dy.numel(), _dt(dy), _s())
        else:
            g = dy
        return g, g, None


# ======================================================================================================================
# Swin-3D pieces (csrc/swin.hip)
# ======================================================================================================================
def patchify(x, patch):
    """[N,X,Y,Z,4] -> [N,X/p,Y/p,Z/p,4p^3] (the network input carries no gradient, so this is not an autograd node)."""
    x = x.contiguous()
    _chk(x)
    n, gx, gy, gz, c = x.shape
    if c != 4:
        raise lib.NrpnError("patchify expects the 4-channel rgb-sigma grid")
    y = torch.empty((n, gx // patch, gy // patch, gz // patch, 4 * patch ** 3), dtype=x.dtype, device=x.device)
    call("patchify", _p(x), _p(y), n, gx, gy, gz, patch, _dt(x), _s())
    return y


def _slots_direct(gs, bs, c):
    """Both parameter gradients of a normalisation layer go to fp32 arena slots of c contiguous elements: the kernels may add in place."""
    return (gs is not None and bs is not None and gs.slot.dtype == torch.float32 and bs.slot.dtype == torch.float32
            and gs.slot.numel() == c and bs.slot.numel() == c and gs.slot.is_contiguous() and bs.slot.is_contiguous())


class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm(C) on the last dimension of a channels-last token tensor."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = x.contiguous()
        _chk(x)
        c = x.shape[-1]
        rows = x.numel() // c
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        call("layernorm_fwd", _p(x), _p(y), _p(g32), _p(b32), _p(mean), _p(rstd), rows, c, float(eps), _dt(x), _s())
        ctx.save_for_backward(x, g32, mean, rstd)
        ctx.sinks = (_sink(gamma), _sink(beta))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g32, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        c = x.shape[-1]
        dx = torch.empty_like(x)
        ws = torch.empty(query("layernorm_workspace_bytes", x.numel() // c, c), dtype=torch.uint8, device=x.device)
        gs, bs = ctx.sinks
        if _slots_direct(gs, bs, c):
            # arena training: the parameter-gradient finish adds straight into the two slots (round 6: ~100 torch adds per Swin-S step gone)
            call("layernorm_bwd", _p(x), _p(dy), _p(dx), _p(g32), _p(mean), _p(rstd), _p(gs.slot), _p(bs.slot), x.numel() // c, c, _dt(x), 1, _p(ws), _s())
            gs.notify()
            bs.notify()
            return dx, None, None, None
        dg = torch.empty(c, dtype=torch.float32, device=x.device)
        db = torch.empty(c, dtype=torch.float32, device=x.device)
        call("layernorm_bwd", _p(x), _p(dy), _p(dx), _p(g32), _p(mean), _p(rstd), _p(dg), _p(db), x.numel() // c, c, _dt(x), 0, _p(ws), _s())
        return dx, hand_in(gs, dg), hand_in(bs, db), None


class GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _chk(x)
        y = torch.empty_like(x)
        call("gelu", _p(x), None, _p(y), x.numel(), 0, _dt(x), _s())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        call("gelu", _p(x), _p(dy), _p(dx), x.numel(), 1, _dt(x), _s())
        return dx


class ScaleAddFn(torch.autograd.Function):
    """y = a + scale[n] * b -- residual join with the StochasticDepth('row') factor (scale None: plain add)."""

    @staticmethod
    def forward(ctx, a, b, scale):
        a, b = a.contiguous(), b.contiguous()
        _chk(a, b)
        y = torch.empty_like(a)
        call("scale_add", _p(a), _p(b), _p(scale), _p(y), a.shape[0], a[0].numel(), _dt(a), _s())
        ctx.save_for_backward(scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        (scale,) = ctx.saved_tensors
        dy = dy.contiguous()
        if scale is None:
            return dy, dy, None
        db = torch.empty_like(dy)
        call("scale_add", None, _p(dy), _p(scale), _p(db), dy.shape[0], dy[0].numel(), _dt(dy), _s())
        return dy, db, None


class PatchMergeFn(torch.autograd.Function):
    """[N,X,Y,Z,C] -> [N,ceil(X/2),ceil(Y/2),ceil(Z/2),8C], reference PatchMerging gather order (feature_extractor.py:403-419)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _chk(x)
        n, gx, gy, gz, c = x.shape
        y = torch.empty((n, (gx + 1) // 2, (gy + 1) // 2, (gz + 1) // 2, 8 * c), dtype=x.dtype, device=x.device)
        call("patch_merge", _p(x), _p(y), n, gx, gy, gz, c, 0, _dt(x), _s())
        ctx.shape = tuple(x.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        n, gx, gy, gz, c = ctx.shape
        dx = torch.empty(ctx.shape, dtype=dy.dtype, device=dy.device)
        call("patch_merge", _p(dy), _p(dx), n, gx, gy, gz, c, 1, _dt(dy), _s())
        return dx


class WindowAttnFn(torch.autograd.Function):
    """Shifted-window attention core between the qkv and proj Linears (reference feature_extractor.py:424-530), window
    4x4x4, head_dim 32.  ``qkv_bias`` is what zero-padded tokens turn into after the qkv Linear."""

    @staticmethod
    def forward(ctx, qkv, qkv_bias, table, rel_index, heads, shift):
        qkv = qkv.contiguous()
        _chk(qkv, table, rel_index)
        n, gx, gy, gz, c3 = qkv.shape
        c = c3 // 3
        qb = qkv_bias.detach().float().contiguous() if qkv_bias is not None else None
        t32 = table.detach().float().contiguous()
        out = torch.empty((n, gx, gy, gz, c), dtype=qkv.dtype, device=qkv.device)
        call("window_attn_fwd", _p(qkv), _p(qb), _p(t32), _p(rel_index), _p(out), n, gx, gy, gz, c, heads, int(shift), _dt(qkv), _s())
        ctx.save_for_backward(qkv, qb, t32, rel_index)
        ctx.meta = (heads, int(shift), any(g % 4 for g in (gx, gy, gz)))
        ctx.sinks = (_sink(qkv_bias), _sink(table))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, qb, t32, rel_index = ctx.saved_tensors
        heads, shift, padded = ctx.meta
        dout = dout.contiguous()
        n, gx, gy, gz, c3 = qkv.shape
        c = c3 // 3
        dqkv = torch.empty_like(qkv)
        dpad = torch.empty(c3, dtype=torch.float32, device=qkv.device) if (padded and qb is not None) else None
        ws = torch.empty(query("window_attn_bwd_workspace_bytes", n, gx, gy, gz, heads), dtype=torch.uint8, device=qkv.device)
        bsink, tsink = ctx.sinks
        if (tsink is not None and dpad is None and tsink.slot.dtype == torch.float32 and tsink.slot.is_contiguous()
                and tsink.slot.numel() == t32.numel()):
            # no padded tokens: the relative-position table is this block's only parameter gradient and nothing else writes its slot -- the
            # table reduction adds into the arena itself (main stream, behind the optimiser's gradient clear), no torch add, no side-stream hop
            call("window_attn_bwd", _p(qkv), _p(qb), _p(t32), _p(rel_index), _p(dout), _p(dqkv), _p(tsink.slot), 0, n, gx, gy, gz, c, heads,
                 shift, _dt(qkv), 1, _p(ws), _s())
            tsink.notify()
            return dqkv, None, None, None, None, None
        dtable = torch.empty_like(t32)
        call("window_attn_bwd", _p(qkv), _p(qb), _p(t32), _p(rel_index), _p(dout), _p(dqkv), _p(dtable), _p(dpad), n, gx, gy, gz, c, heads,
             shift, _dt(qkv), 0, _p(ws), _s())
        if _sinks_cover((dtable, dpad), (tsink, bsink)):
            # arena training: both parameter gradients are added to their slots here instead of travelling through autograd's AccumulateGrad
            # (which runs on the stream it was created on and would fall out of a captured backward, graphs.py).  The qkv bias also receives
            # the bias gradient of the qkv Linear on the weight-gradient stream: same stream, enqueue order = a fixed summation order.
            def deliver():
                hand_in(tsink, dtable.view_as(tsink.slot))
                if dpad is not None:
                    hand_in(bsink, dpad.view_as(bsink.slot))
            _on_wgrad_stream(qkv.device, (dtable, dpad), True, deliver)
            return dqkv, None, None, None, None, None
        return dqkv, dpad, dtable, None, None, None


# ======================================================================================================================
# FCOS pieces (csrc/fcos.hip)
# ======================================================================================================================
class GroupNormFn(torch.autograd.Function):
    """nn.GroupNorm(groups, C) (+ fused ReLU) on a channels-last [N,X,Y,Z,C] tensor."""

    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, relu):
        x = x.contiguous()
        _chk(x)
        n, c = x.shape[0], x.shape[-1]
        rows = x[0].numel() // c
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        mean = torch.empty(n * groups, dtype=torch.float32, device=x.device)
        rstd = torch.empty(n * groups, dtype=torch.float32, device=x.device)
        ws = torch.empty(query("groupnorm_workspace_bytes", n, c, groups), dtype=torch.uint8, device=x.device)
        y = torch.empty_like(x)
        call("groupnorm_fwd", _p(x), _p(y), _p(g32), _p(b32), _p(mean), _p(rstd), n, rows, c, groups, float(eps), int(relu), _dt(x), _p(ws), _s())
        ctx.save_for_backward(x, y if relu else None, g32, mean, rstd)
        ctx.meta = (groups, relu)
        ctx.sinks = (_sink(gamma), _sink(beta))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, g32, mean, rstd = ctx.saved_tensors
        groups, relu = ctx.meta
        dy = dy.contiguous()
        n, c = x.shape[0], x.shape[-1]
        dx = torch.empty_like(x)
        ws = torch.empty(query("groupnorm_workspace_bytes", n, c, groups), dtype=torch.uint8, device=x.device)
        gs, bs = ctx.sinks
        if _slots_direct(gs, bs, c):
            call("groupnorm_bwd", _p(x), _p(y), _p(dy), _p(dx), _p(g32), _p(mean), _p(rstd), _p(gs.slot), _p(bs.slot), n, x[0].numel() // c, c, groups,
                 int(relu), _dt(x), 1, _p(ws), _s())
            gs.notify()
            bs.notify()
            return dx, None, None, None, None, None
        dg = torch.empty(c, dtype=torch.float32, device=x.device)
        db = torch.empty(c, dtype=torch.float32, device=x.device)
        call("groupnorm_bwd", _p(x), _p(y), _p(dy), _p(dx), _p(g32), _p(mean), _p(rstd), _p(dg), _p(db), n, x[0].numel() // c, c, groups,
             int(relu), _dt(x), 0, _p(ws), _s())
        return dx, hand_in(gs, dg), hand_in(bs, db), None, None, None


class FcosHeadOutFn(torch.autograd.Function):
    """Head epilogue of one pyramid level: fused-GEMM outputs [rows, wrows] f32 -> (logits [rows], reg [rows, D], ctr [rows])
    with Scale / ReLU / stride (reference fcos.py:104-128)."""

    @staticmethod
    def forward(ctx, cls_out, box_out, scale, stride_mul, norm_reg, reg_dim, ctr_on_reg):
        _chk(cls_out, box_out)
        wrows = cls_out.shape[-1]
        rows = cls_out.numel() // wrows
        sc = scale.detach().float().contiguous()
        dev = cls_out.device
        logits = torch.empty(rows, dtype=torch.float32, device=dev)
        reg = torch.empty((rows, reg_dim), dtype=torch.float32, device=dev)
        ctr = torch.empty(rows, dtype=torch.float32, device=dev)
        call("fcos_head_out_f32", _p(cls_out), _p(box_out), wrows, _p(sc), float(stride_mul), int(norm_reg), reg_dim, int(ctr_on_reg), rows,
             _p(logits), _p(reg), _p(ctr), _s())
        ctx.save_for_backward(box_out, sc)
        ctx.meta = (wrows, rows, float(stride_mul), int(norm_reg), reg_dim, int(ctr_on_reg), cls_out.shape)
        ctx.sink = _sink(scale)
        return logits, reg, ctr

    @staticmethod
    def backward(ctx, d_logits, d_reg, d_ctr):
        box_out, sc = ctx.saved_tensors
        wrows, rows, stride_mul, norm_reg, reg_dim, ctr_on_reg, shape = ctx.meta
        d_cls = torch.empty(shape, dtype=torch.float32, device=box_out.device)
        d_box = torch.empty(shape, dtype=torch.float32, device=box_out.device)
        d_scale = torch.zeros(query("fcos_reduce_floats"), dtype=torch.float32, device=box_out.device)     # [0] result, [1] ticket, partials
        dl = d_logits.contiguous() if d_logits is not None else None
        dr = d_reg.contiguous() if d_reg is not None else None
        dc = d_ctr.contiguous() if d_ctr is not None else None
        call("fcos_head_out_bwd_f32", _p(box_out), wrows, _p(sc), stride_mul, norm_reg, reg_dim, ctr_on_reg, rows, _p(dl), _p(dr), _p(dc),
             _p(d_cls), _p(d_box), _p(d_scale), _s())
        if ctx.sink is not None:        # straight into the trainer's arena: a gradient handed back to autograd would be accumulated outside a
            ctx.sink.slot.add_(d_scale[:1].view_as(ctx.sink.slot))      # captured backward (graphs.py) and replays would miss it
            ctx.sink.notify()
            return d_cls, d_box, None, None, None, None, None
        return d_cls, d_box, d_scale[:1], None, None, None, None


class FcosGeometry:
    """Host description of the flattened FCOS location list (level-major, then scene, then voxel)."""

    def __init__(self, n, dims, strides):
        self.n, self.levels = int(n), len(dims)
        self.dims = [tuple(int(v) for v in d) for d in dims]
        self.strides = [int(s) for s in strides]
        self.counts = [d[0] * d[1] * d[2] for d in self.dims]            # locations per scene per level
        self.total = self.n * sum(self.counts)
        self._dims = (ctypes.c_int32 * (3 * self.levels))(*[v for d in self.dims for v in d])
        self._strides = (ctypes.c_int32 * self.levels)(*self.strides)
        self.segment_offsets = [0]
        for c in self.counts:
            for _ in range(self.n):
                self.segment_offsets.append(self.segment_offsets[-1] + c)

    def args(self):
        return self.n, self.levels, ctypes.addressof(self._dims), ctypes.addressof(self._strides)

    @staticmethod
    def sizes(ori_sizes):
        if ori_sizes is None:
            return None, 0
        buf = (ctypes.c_float * (3 * len(ori_sizes)))(*[float(v) for s in ori_sizes for v in s])
        return buf, ctypes.addressof(buf)


def fcos_gt_summary(gt):
    gt = _f32(gt).contiguous()
    _chk(gt)
    out = torch.empty((gt.shape[0], 8), dtype=torch.float32, device=gt.device)
    if gt.shape[0]:
        call("fcos_gt_summary_f32", _p(gt), gt.shape[0], gt.shape[1], _p(out), _s())
    return out


def fcos_targets(geom, targets, ori_sizes, radius, norm_reg, reg_dim, device):
    """labels int8 [total] in {1,0,-1}, reg_targets f32 [total, reg_dim], num_pos int32 [1] (reference loss.py:270-437)."""
    summ = [fcos_gt_summary(t) for t in targets]
    offs = [0]
    for t in targets:
        offs.append(offs[-1] + t.shape[0])
    summary = torch.cat(summ) if offs[-1] else None
    host = (ctypes.c_int32 * len(offs))(*offs)
    labels = torch.empty(geom.total, dtype=torch.int8, device=device)
    reg_t = torch.empty((geom.total, reg_dim), dtype=torch.float32, device=device)
    npos = torch.empty(1, dtype=torch.int32, device=device)
    keep, sizes = FcosGeometry.sizes(ori_sizes)
    n, levels, dims, strides = geom.args()
    call("fcos_targets_f32", _p(summary), ctypes.addressof(host), n, levels, dims, strides, sizes, float(radius), int(norm_reg), reg_dim,
         _p(labels), _p(reg_t), _p(npos), _s())
    return labels, reg_t, npos


class FocalLossFn(torch.autograd.Function):
    """sum of sigmoid focal loss (alpha, gamma 2) over the locations with label >= 0; the gradient is produced in the same pass."""

    @staticmethod
    def forward(ctx, logits, labels, alpha):
        logits = logits.contiguous()
        _chk(logits, labels)
        out = torch.empty(query("fcos_reduce_floats"), dtype=torch.float32, device=logits.device)      # [0] result, [1] ticket, partials
        grad = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        call("fcos_focal_f32", _p(logits), _p(labels), logits.numel(), float(alpha), _p(out), _p(grad), _s())
        ctx.save_for_backward(grad)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None


def fcos_scores(geom, logits, ctr, ori_sizes, thresh):
    _chk(logits, ctr)
    scores = torch.empty(geom.total, dtype=torch.float32, device=logits.device)
    keep, sizes = FcosGeometry.sizes(ori_sizes)
    n, levels, dims, strides = geom.args()
    call("fcos_scores_f32", _p(logits), _p(ctr), n, levels, dims, strides, sizes, float(thresh), _p(scores), _s())
    return scores


def fcos_decode(geom, idx, score, reg, ori_sizes, reg_dim, min_size):
    """idx / score: [levels*n, k] from segmented_topk -> boxes [levels*n*k, 6|7], sqrt scores (-1 = dropped), levels (f32)."""
    _chk(idx, score, reg)
    count, k = idx.numel(), idx.shape[1]
    w = 7 if reg_dim == 8 else 6
    dev = reg.device
    boxes = torch.empty((count, w), dtype=torch.float32, device=dev)
    out_s = torch.empty(count, dtype=torch.float32, device=dev)
    out_l = torch.empty(count, dtype=torch.float32, device=dev)
    keep, sizes = FcosGeometry.sizes(ori_sizes)
    n, levels, dims, strides = geom.args()
    call("fcos_decode_f32", _p(idx), _p(score), count, k, _p(reg), n, levels, dims, strides, sizes, reg_dim, float(min_size), _p(boxes),
         _p(out_s), _p(out_l), _s())
    return boxes, out_s, out_l


class _ToChannelsLast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        x = x.float().contiguous()
        _chk(x)
        n, c = x.shape[:2]
        out = torch.empty((n, *x.shape[2:], c), dtype=dtype, device=x.device)
        call("ncdhw_to_ndhwc", _p(x), _p(out), n, c, x[0, 0].numel(), _dt(out), _s())
        return out

    @staticmethod
    def backward(ctx, g):
        return to_channels_first(g.contiguous()), None


def to_channels_last(x, dtype):
    """[N,C,X,Y,Z] fp32 -> [N,X,Y,Z,C] dtype (differentiable).  A tensor that is already channels-last in memory (e.g. the output
    of ``ingest_rgbsigma``) passes through as a view."""
    cl = x.permute(0, 2, 3, 4, 1)
    if cl.is_contiguous() and cl.dtype == dtype and not x.requires_grad:
        return cl
    return _ToChannelsLast.apply(x, dtype)


def ingest_rgbsigma(raw, alpha_mode=0, dtype=torch.float32):
    """On-disk layout (W,L,H,4) f32|uint8 on the device -> the reference's logical [4,W,L,H] scene tensor, backed by
    channels-last memory in the compute dtype (reference datasets.py:39-63; alpha_mode 1 = density_to_alpha, 2 = ScanNet's)."""
    raw = raw.contiguous()
    _chk(raw)
    if raw.dim() != 4 or raw.shape[-1] != 4 or raw.dtype not in (torch.float32, torch.uint8):
        raise lib.NrpnError("ingest_rgbsigma expects a (W,L,H,4) float32 or uint8 tensor")
    out = torch.empty(raw.shape, dtype=dtype, device=raw.device)
    call("ingest_rgbsigma", _p(raw), int(raw.dtype == torch.uint8), _p(out), raw.numel() // 4, int(alpha_mode), _dt(out), _s())
    return out.permute(3, 0, 1, 2)


def as_channels_last(x):
    """Logical [N,C,X,Y,Z] (fp32 / bf16) -> channels-last tensor [N,X,Y,Z,C]: a free view when the memory already is channels-last
    (what the HIP backbones return), one conversion kernel otherwise."""
    cl = x.permute(0, 2, 3, 4, 1)
    if cl.is_contiguous():
        return cl
    if x.dtype == torch.float32 or x.dtype == torch.bfloat16:
        return to_channels_last(x.float(), x.dtype)
    raise lib.NrpnError(f"unsupported dtype {x.dtype}")


def roi_align_rotated_3d_fwd(feat_cl, rois, spatial_scale, output_size, sampling_ratio):
    """feat_cl [N,X,Y,Z,C], rois f32 [R,8] -> [R,pw,pl,ph,C] in feat's dtype (reference ROIAlignRotated3D_cuda.cu:78-170)."""
    feat_cl, rois = feat_cl.contiguous(), _f32(rois).contiguous()
    _chk(feat_cl, rois)
    n, x, y, z, c = feat_cl.shape
    pw, pl, ph = output_size
    out = torch.empty((rois.shape[0], pw, pl, ph, c), dtype=feat_cl.dtype, device=feat_cl.device)
    call("roi_align_rotated_3d_fwd", _p(feat_cl), _p(rois), rois.shape[0], n, x, y, z, c, float(spatial_scale), pw, pl, ph, int(sampling_ratio),
         _p(out), _dt(feat_cl), _s())
    return out


def roi_align_rotated_3d_bwd(grad_cl, rois, feat_shape, spatial_scale, output_size, sampling_ratio):
    """grad_cl [R,pw,pl,ph,C] -> gradient of the feature map [N,X,Y,Z,C] (deterministic fixed-point accumulation)."""
    grad_cl, rois = grad_cl.contiguous(), _f32(rois).contiguous()
    _chk(grad_cl, rois)
    n, x, y, z, c = feat_shape
    pw, pl, ph = output_size
    gi = torch.empty(feat_shape, dtype=grad_cl.dtype, device=grad_cl.device)
    ws = torch.empty(query("roi_align_rotated_3d_bwd_workspace_bytes", n, x, y, z, c), dtype=torch.uint8, device=grad_cl.device)
    call("roi_align_rotated_3d_bwd", _p(grad_cl), _p(rois), rois.shape[0], n, x, y, z, c, float(spatial_scale), pw, pl, ph, int(sampling_ratio),
         _p(gi), _p(ws), _dt(grad_cl), _s())
    return gi


def ingest_augment(raw, alpha_mode, dtype, plan):
    """``ingest_rgbsigma`` + the training augmentation of ``plan`` (datasets.AugPlan) in one pass on the device: 90-degree rotation and
    flips as index remaps, rotate_and_scale_scene as a trilinear resample (reference datasets.py:109-163, 291-329)."""
    raw = raw.contiguous()
    _chk(raw)
    if raw.dim() != 4 or raw.shape[-1] != 4 or raw.dtype not in (torch.float32, torch.uint8):
        raise lib.NrpnError("ingest_augment expects a (W,L,H,4) float32 or uint8 tensor")
    w, l, h = (int(v) for v in raw.shape[:3])
    ow, ol, oh = ((l, w, h) if plan.z_up else (h, l, w)) if plan.rot90 else (w, l, h)
    out = torch.empty((ow, ol, oh, 4), dtype=dtype, device=raw.device)
    xf = plan.xform()
    host, hp = None, 0
    if xf is not None:
        host = (ctypes.c_float * 9)(*[float(v) for v in xf.reshape(-1)])
        hp = ctypes.addressof(host)
    call("ingest_augment", _p(raw), int(raw.dtype == torch.uint8), _p(out), w, l, h, int(alpha_mode), _dt(out), int(plan.rot90), int(plan.z_up),
         int(plan.flips[0]), int(plan.flips[1]), hp, _s())
    return out.permute(3, 0, 1, 2)


def stack_scenes(meshes):
    """torch.stack for scene tensors [4,W,L,H]: keeps channels-last memory when every scene has it (no layout round trip)."""
    if len(meshes) == 1:           # a view: torch.stack would copy the whole scene (65 MB at 160^3)
        return meshes[0].unsqueeze(0)
    if all(m.permute(1, 2, 3, 0).is_contiguous() for m in meshes):
        return torch.stack([m.permute(1, 2, 3, 0) for m in meshes], dim=0).permute(0, 4, 1, 2, 3)
    return torch.stack(meshes, dim=0)


def to_channels_first(x):
    """[N,X,Y,Z,C] -> [N,C,X,Y,Z] fp32 (a real copy; use ``x.permute(0,4,1,2,3)`` for a free view)."""
    _chk(x)
    n, c = x.shape[0], x.shape[-1]
    out = torch.empty((n, c, *x.shape[1:4]), dtype=torch.float32, device=x.device)
    call("ndhwc_to_ncdhw", _p(x), _p(out), n, c, x[0, ..., 0].numel(), _dt(x), _s())
    return out


# ======================================================================================================================
# flat-arena optimiser
# ======================================================================================================================
def grad_sumsq(grad_flat, out, grad_scale=1.0):
    call("grad_sumsq", _p(grad_flat), grad_flat.numel(), float(grad_scale), _p(out), _s())


def adamw_step(p, g, m, v, sumsq, max_norm, lr, betas, eps, wd, step, grad_scale=1.0, shadow=None, zero_grad=False):
    """``zero_grad``: the kernel clears the gradient it has just consumed (no separate fill of the arena)."""
    call("adamw_step_zero_grad" if zero_grad else "adamw_step", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(sumsq), float(grad_scale), float(max_norm),
         float(lr), float(betas[0]), float(betas[1]), float(eps), float(wd), int(step), _p(shadow), _s())


# ======================================================================================================================
# ROIPool without the RoIAlign op (the reference CLI's default second-stage pooling, detector.py:264-438) -- csrc/roipool.hip
# ======================================================================================================================
class RoiPoolFn(torch.autograd.Function):
    """Per-RoI pyramid features of ONE scene: ``levels`` = the scene's maps, logical [C, X, Y, Z] (channels-last memory is consumed as is);
    ``meta`` = i32 [R, 6] crops (kind 'aabb') or f32 [R, 7] enlarged boxes ('pooling' / 'interpolation'); ``level_of`` i32 [R];
    ``scales`` = input voxels per level voxel.  -> f32 [R, C, o0, o1, o2] (a channels-last-backed view).  One launch per level, forward and
    backward; no host synchronisation."""

    @staticmethod
    def forward(ctx, kind, meta, level_of, scales, output_size, *levels):
        o0, o1, o2 = (int(v) for v in output_size)
        R = int(meta.shape[0])
        bad = [f for f in levels if not f.is_cuda or f.dtype not in (torch.float32, torch.bfloat16)]
        if bad:       # say what is supported instead of a generic "not a CUDA tensor" from deeper down
            raise lib.NrpnError(f"ROIPool runs on the HIP kernels only (csrc/roipool.hip): feature maps must be CUDA tensors in float32 or "
                                f"bfloat16, got {bad[0].device} / {bad[0].dtype}; the torch restatement of the reference's pooling "
                                "(oracle/roipool.py) is test infrastructure, not a fallback")
        cls = [as_channels_last(f[None])[0] for f in levels]          # [X, Y, Z, C]
        C = int(cls[0].shape[-1])
        dev = cls[0].device
        out = torch.zeros((R, o0, o1, o2, C), dtype=torch.float32, device=dev)
        arg = torch.full((R, o0, o1, o2, C), -1, dtype=torch.int32, device=dev) if kind != "interpolation" else None
        meta, level_of = meta.contiguous(), level_of.contiguous()
        _chk(meta, level_of, *cls)
        for l, f in enumerate(cls):
            X, Y, Z = (int(v) for v in f.shape[:3])
            if kind == "aabb":
                call("roipool_aabb_fwd", _p(f), X, Y, Z, C, _p(meta), _p(level_of), l, R, o0, o1, o2, _p(out), _p(arg), _dt(f), _s())
            else:
                call("roipool_obb_fwd", _p(f), X, Y, Z, C, _p(meta), _p(level_of), l, R, float(scales[l]), 1 if kind == "interpolation" else 0,
                     o0, o1, o2, _p(out), _p(arg), _dt(f), _s())
        ctx.save_for_backward(meta, level_of, *([arg] if arg is not None else []))
        ctx.info = (kind, [float(v) for v in scales], (o0, o1, o2), [(tuple(f.shape), f.dtype) for f in cls])
        return out.permute(0, 4, 1, 2, 3)

    @staticmethod
    def backward(ctx, g):
        kind, scales, (o0, o1, o2), shapes = ctx.info
        meta, level_of, *rest = ctx.saved_tensors
        arg = rest[0] if rest else None
        R = int(meta.shape[0])
        g = g.permute(0, 2, 3, 4, 1).contiguous().float()
        grads = []
        for l, ((X, Y, Z, C), dt) in enumerate(shapes):
            if not ctx.needs_input_grad[5 + l]:
                grads.append(None)
                continue
            df = torch.empty((X, Y, Z, C), dtype=dt, device=g.device)
            ws = torch.empty(query("roipool_bwd_workspace_bytes", X, Y, Z, C), dtype=torch.uint8, device=g.device)
            code = F32 if dt == torch.float32 else BF16
            if kind == "aabb":
                call("roipool_aabb_bwd", _p(g), _p(arg), _p(meta), _p(level_of), l, R, X, Y, Z, C, o0, o1, o2, _p(df), _p(ws), code, _s())
            else:
                call("roipool_obb_bwd", _p(g), _p(arg), _p(meta), _p(level_of), l, R, scales[l], 1 if kind == "interpolation" else 0, X, Y, Z, C,
                     o0, o1, o2, _p(df), _p(ws), code, _s())
            grads.append(df.permute(3, 0, 1, 2))
        return (None, None, None, None, None, *grads)


# ======================================================================================================================
# proposal heatmap (scripts/render_heatmap.py)  [f4]
# ======================================================================================================================
HEATMAP_KERNELS = {"gaussian": 0, "box": 1}      # enum nrpn_heatmap_kernel

# matplotlib's piecewise-linear 'jet' segment data (x, y0, y1), written out so the product does not import matplotlib
_JET_SEGMENTS = (((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
                 ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
                 ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)))


def jet_table(n=256):
    """float64 [n,3]: the 'jet' colormap's lookup table, built as a LinearSegmentedColormap builds it (linear interpolation of the
    segment data at linspace(0, 1, n), clipped to [0, 1])."""
    import numpy as np
    cols = []
    for seg in _JET_SEGMENTS:
        a = np.array(seg, dtype=np.float64)
        x, y0, y1 = a[:, 0], a[:, 1], a[:, 2]
        xi = np.linspace(0, 1, n)
        ind = np.searchsorted(x, xi)[1:-1]
        dist = (xi[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        cols.append(np.clip(np.concatenate([[y1[0]], dist * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]]), 0, 1))
    return np.stack(cols, axis=1)


def gkern_factors(w):
    """1-D factor of the reference's gkern_3d (render_heatmap.py:21-33) for a box extent w, float64 [w], computed with numpy exactly as
    the reference computes it (the 3-D kernel is their outer product)."""
    import numpy as np
    a = np.linspace(-(w - 1) / 2., (w - 1) / 2., w)
    return np.exp(-0.5 * np.square(a) / np.square(w / 5))


def heatmap_factor_tables(aabbs):
    """aabbs int [K,6] -> (factors float64 [sum of extents], offsets int32 [K]): gx | gy | gz of every box, box k's gx at offsets[k]."""
    import numpy as np
    parts, offs, at = [], [], 0
    for b in np.asarray(aabbs).reshape(-1, 6):
        offs.append(at)
        for e in (b[3] - b[0], b[4] - b[1], b[5] - b[2]):
            f = gkern_factors(e) if e > 0 else np.zeros(0)
            parts.append(f)
            at += f.size
    return (np.concatenate(parts) if parts else np.zeros(0)).astype(np.float64), np.array(offs, dtype=np.int32)


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage's gaussian_filter1d kernel (order 0): (radius, float64 [2 radius + 1])."""
    import numpy as np
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return radius, phi / phi.sum()


def heatmap_splat(aabbs, shape, kernel_type="gaussian", device="cuda"):
    """generate_heatmap's box loop: aabbs int [K,6] (half-open, clipped) -> float32 [X,Y,Z] on `device` (bit-identical to numpy)."""
    import numpy as np
    if kernel_type not in HEATMAP_KERNELS:
        raise lib.NrpnError(f"heatmap_splat: unknown kernel_type {kernel_type!r}")
    a = np.ascontiguousarray(np.asarray(aabbs).reshape(-1, 6), dtype=np.int32)
    X, Y, Z = (int(v) for v in shape)
    out = torch.empty((X, Y, Z), dtype=torch.float32, device=device)
    boxes = torch.from_numpy(a).to(device)
    fac = offs = None
    if kernel_type == "gaussian" and a.shape[0]:
        f, o = heatmap_factor_tables(a)
        fac, offs = torch.from_numpy(f if f.size else np.zeros(1)).to(device), torch.from_numpy(o).to(device)
    _chk(out, boxes, fac, offs)
    call("heatmap_splat", _p(boxes), a.shape[0], _p(fac), _p(offs), HEATMAP_KERNELS[kernel_type], X, Y, Z, _p(out), _s())
    return out


def gaussian_filter3d(vol, sigma):
    """scipy.ndimage.gaussian_filter(vol, sigma) of a float32 [X,Y,Z] volume (mode 'reflect', truncate 4), bit-identical."""
    vol = vol.contiguous()
    _chk(vol)
    if vol.dim() != 3 or vol.dtype != torch.float32:
        raise lib.NrpnError("gaussian_filter3d expects a float32 [X,Y,Z] tensor")
    sigma = float(sigma)
    radius, w = gaussian_weights(sigma) if sigma == sigma and sigma >= 0 else (0, None)
    wt = torch.from_numpy(w).to(vol.device) if w is not None else torch.ones(1, dtype=torch.float64, device=vol.device)
    out, work = torch.empty_like(vol), torch.empty_like(vol)
    call("gaussian_filter3d", _p(vol), *vol.shape, sigma, radius, _p(wt), _p(work), _p(out), _s())
    return out


def standardize(vol):
    """(vol - mean) / std (ddof 0) of a float32 tensor -> (out, mean_std float32 [2] on the device)."""
    vol = vol.contiguous()
    _chk(vol)
    if vol.dtype != torch.float32:
        raise lib.NrpnError("standardize expects a float32 tensor")
    out = torch.empty_like(vol)
    ms = torch.empty(2, dtype=torch.float32, device=vol.device)
    work = torch.empty(query("heatmap_work_doubles"), dtype=torch.float64, device=vol.device)
    call("heatmap_standardize", _p(vol), vol.numel(), _p(work), _p(out), _p(ms), _s())
    return out, ms


def render_mip(heatmap, cams, downsample=2, value_scale=20.0, width=640, height=480, jet=None, with_mip=False):
    """Maximum-intensity render of heatmap[::d, ::d, ::d] * value_scale (semantics: include/nerfrpn.h, nrpn_render_mip).
    cams float [F,6] = (position, focal point) in units of the downsampled grid -> uint8 [F,height,width,3] (+ float32 [F,height,width]
    ray maxima if with_mip)."""
    heatmap = heatmap.contiguous()
    _chk(heatmap)
    if heatmap.dim() != 3 or heatmap.dtype != torch.float32:
        raise lib.NrpnError("render_mip expects a float32 [X,Y,Z] tensor")
    dev = heatmap.device
    cams = torch.as_tensor(cams, dtype=torch.float64).reshape(-1, 6).contiguous().to(dev)
    jet = torch.as_tensor(jet_table() if jet is None else jet, dtype=torch.float64).contiguous().to(dev)
    F = int(cams.shape[0])
    rgb = torch.empty((F, int(height), int(width), 3), dtype=torch.uint8, device=dev)
    mip = torch.empty((F, int(height), int(width)), dtype=torch.float32, device=dev) if with_mip else None
    work = torch.empty(query("heatmap_work_doubles"), dtype=torch.float64, device=dev)
    call("render_mip", _p(heatmap), *heatmap.shape, int(downsample), float(value_scale), _p(cams), F, _p(jet), int(width), int(height),
         _p(work), _p(rgb), _p(mip), _s())
    return (rgb, mip) if with_mip else rgb


# ======================================================================================================================
# PLY export of scenes, boxes and objectness (scripts/visualize_rpn_input.py)  [f4]
# ======================================================================================================================
SPLINE_POLE = -0.267949192431122706472553658494127633     # scipy's cubic B-spline pole (the decimal literal, not sqrt(3) - 2)

# matplotlib's 'turbo' colour list (256 rgb triples), written out so the product does not import matplotlib
_TURBO = """
    0.18995 0.07176 0.23217  0.19483 0.08339 0.26149  0.19956 0.09498 0.29024  0.20415 0.10652 0.31844  0.2086 0.11802 0.34607  0.21291 0.12947 0.37314
    0.21708 0.14087 0.39964  0.22111 0.15223 0.42558  0.225 0.16354 0.45096  0.22875 0.17481 0.47578  0.23236 0.18603 0.50004  0.23582 0.1972 0.52373
    0.23915 0.20833 0.54686  0.24234 0.21941 0.56942  0.24539 0.23044 0.59142  0.2483 0.24143 0.61286  0.25107 0.25237 0.63374  0.25369 0.26327 0.65406
    0.25618 0.27412 0.67381  0.25853 0.28492 0.693  0.26074 0.29568 0.71162  0.2628 0.30639 0.72968  0.26473 0.31706 0.74718  0.26652 0.32768 0.76412
    0.26816 0.33825 0.7805  0.26967 0.34878 0.79631  0.27103 0.35926 0.81156  0.27226 0.3697 0.82624  0.27334 0.38008 0.84037  0.27429 0.39043 0.85393
    0.27509 0.40072 0.86692  0.27576 0.41097 0.87936  0.27628 0.42118 0.89123  0.27667 0.43134 0.90254  0.27691 0.44145 0.91328  0.27701 0.45152 0.92347
    0.27698 0.46153 0.93309  0.2768 0.47151 0.94214  0.27648 0.48144 0.95064  0.27603 0.49132 0.95857  0.27543 0.50115 0.96594  0.27469 0.51094 0.97275
    0.27381 0.52069 0.97899  0.27273 0.5304 0.98461  0.27106 0.54015 0.9893  0.26878 0.54995 0.99303  0.26592 0.55979 0.99583  0.26252 0.56967 0.99773
    0.25862 0.57958 0.99876  0.25425 0.5895 0.99896  0.24946 0.59943 0.99835  0.24427 0.60937 0.99697  0.23874 0.61931 0.99485  0.23288 0.62923 0.99202
    0.22676 0.63913 0.98851  0.22039 0.64901 0.98436  0.21382 0.65886 0.97959  0.20708 0.66866 0.97423  0.20021 0.67842 0.96833  0.19326 0.68812 0.9619
    0.18625 0.69775 0.95498  0.17923 0.70732 0.94761  0.17223 0.7168 0.93981  0.16529 0.7262 0.93161  0.15844 0.73551 0.92305  0.15173 0.74472 0.91416
    0.14519 0.75381 0.90496  0.13886 0.76279 0.8955  0.13278 0.77165 0.8858  0.12698 0.78037 0.8759  0.12151 0.78896 0.86581  0.11639 0.7974 0.85559
    0.11167 0.80569 0.84525  0.10738 0.81381 0.83484  0.10357 0.82177 0.82437  0.10026 0.82955 0.81389  0.0975 0.83714 0.80342  0.09532 0.84455 0.79299
    0.09377 0.85175 0.78264  0.09287 0.85875 0.7724  0.09267 0.86554 0.7623  0.0932 0.87211 0.75237  0.09451 0.87844 0.74265  0.09662 0.88454 0.73316
    0.09958 0.8904 0.72393  0.10342 0.896 0.715  0.10815 0.90142 0.70599  0.11374 0.90673 0.69651  0.12014 0.91193 0.6866  0.12733 0.91701 0.67627
    0.13526 0.92197 0.66556  0.14391 0.9268 0.65448  0.15323 0.93151 0.64308  0.16319 0.93609 0.63137  0.17377 0.94053 0.61938  0.18491 0.94484 0.60713
    0.19659 0.94901 0.59466  0.20877 0.95304 0.58199  0.22142 0.95692 0.56914  0.23449 0.96065 0.55614  0.24797 0.96423 0.54303  0.2618 0.96765 0.52981
    0.27597 0.97092 0.51653  0.29042 0.97403 0.50321  0.30513 0.97697 0.48987  0.32006 0.97974 0.47654  0.33517 0.98234 0.46325  0.35043 0.98477 0.45002
    0.36581 0.98702 0.43688  0.38127 0.98909 0.42386  0.39678 0.99098 0.41098  0.41229 0.99268 0.39826  0.42778 0.99419 0.38575  0.44321 0.99551 0.37345
    0.45854 0.99663 0.3614  0.47375 0.99755 0.34963  0.48879 0.99828 0.33816  0.50362 0.99879 0.32701  0.51822 0.9991 0.31622  0.53255 0.99919 0.30581
    0.54658 0.99907 0.29581  0.56026 0.99873 0.28623  0.57357 0.99817 0.27712  0.58646 0.99739 0.26849  0.59891 0.99638 0.26038  0.61088 0.99514 0.2528
    0.62233 0.99366 0.24579  0.63323 0.99195 0.23937  0.64362 0.98999 0.23356  0.65394 0.98775 0.22835  0.66428 0.98524 0.2237  0.67462 0.98246 0.2196
    0.68494 0.97941 0.21602  0.69525 0.9761 0.21294  0.70553 0.97255 0.21032  0.71577 0.96875 0.20815  0.72596 0.9647 0.2064  0.7361 0.96043 0.20504
    0.74617 0.95593 0.20406  0.75617 0.95121 0.20343  0.76608 0.94627 0.20311  0.77591 0.94113 0.2031  0.78563 0.93579 0.20336  0.79524 0.93025 0.20386
    0.80473 0.92452 0.20459  0.8141 0.91861 0.20552  0.82333 0.91253 0.20663  0.83241 0.90627 0.20788  0.84133 0.89986 0.20926  0.8501 0.89328 0.21074
    0.85868 0.88655 0.2123  0.86709 0.87968 0.21391  0.8753 0.87267 0.21555  0.88331 0.86553 0.21719  0.89112 0.85826 0.2188  0.8987 0.85087 0.22038
    0.90605 0.84337 0.22188  0.91317 0.83576 0.22328  0.92004 0.82806 0.22456  0.92666 0.82025 0.2257  0.93301 0.81236 0.22667  0.93909 0.80439 0.22744
    0.94489 0.79634 0.228  0.95039 0.78823 0.22831  0.9556 0.78005 0.22836  0.96049 0.77181 0.22811  0.96507 0.76352 0.22754  0.96931 0.75519 0.22663
    0.97323 0.74682 0.22536  0.97679 0.73842 0.22369  0.98 0.73 0.22161  0.98289 0.7214 0.21918  0.98549 0.7125 0.2165  0.98781 0.7033 0.21358
    0.98986 0.69382 0.21043  0.99163 0.68408 0.20706  0.99314 0.67408 0.20348  0.99438 0.66386 0.19971  0.99535 0.65341 0.19577  0.99607 0.64277 0.19165
    0.99654 0.63193 0.18738  0.99675 0.62093 0.18297  0.99672 0.60977 0.17842  0.99644 0.59846 0.17376  0.99593 0.58703 0.16899  0.99517 0.57549 0.16412
    0.99419 0.56386 0.15918  0.99297 0.55214 0.15417  0.99153 0.54036 0.1491  0.98987 0.52854 0.14398  0.98799 0.51667 0.13883  0.9859 0.50479 0.13367
    0.9836 0.49291 0.12849  0.98108 0.48104 0.12332  0.97837 0.4692 0.11817  0.97545 0.4574 0.11305  0.97234 0.44565 0.10797  0.96904 0.43399 0.10294
    0.96555 0.42241 0.09798  0.96187 0.41093 0.0931  0.95801 0.39958 0.08831  0.95398 0.38836 0.08362  0.94977 0.37729 0.07905  0.94538 0.36638 0.07461
    0.94084 0.35566 0.07031  0.93612 0.34513 0.06616  0.93125 0.33482 0.06218  0.92623 0.32473 0.05837  0.92105 0.31489 0.05475  0.91572 0.3053 0.05134
    0.91024 0.29599 0.04814  0.90463 0.28696 0.04516  0.89888 0.27824 0.04243  0.89298 0.26981 0.03993  0.88691 0.26152 0.03753  0.88066 0.25334 0.03521
    0.87422 0.24526 0.03297  0.8676 0.2373 0.03082  0.86079 0.22945 0.02875  0.8538 0.2217 0.02677  0.84662 0.21407 0.02487  0.83926 0.20654 0.02305
    0.83172 0.19912 0.02131  0.82399 0.19182 0.01966  0.81608 0.18462 0.01809  0.80799 0.17753 0.0166  0.79971 0.17055 0.0152  0.79125 0.16368 0.01387
    0.7826 0.15693 0.01264  0.77377 0.15028 0.01148  0.76476 0.14374 0.01041  0.75556 0.13731 0.00942  0.74617 0.13098 0.00851  0.73661 0.12477 0.00769
    0.72686 0.11867 0.00695  0.71692 0.11268 0.00629  0.7068 0.1068 0.00571  0.6965 0.10102 0.00522  0.68602 0.09536 0.00481  0.67535 0.0898 0.00449
    0.66449 0.08436 0.00424  0.65345 0.07902 0.00408  0.64223 0.0738 0.00401  0.63082 0.06868 0.00401  0.61923 0.06367 0.0041  0.60746 0.05878 0.00427
    0.5955 0.05399 0.00453  0.58336 0.04931 0.00486  0.57103 0.04474 0.00529  0.55852 0.04028 0.00579  0.54583 0.03593 0.00638  0.53295 0.03169 0.00705
    0.51989 0.02756 0.0078  0.50664 0.02354 0.00863  0.49321 0.01963 0.00955  0.4796 0.01583 0.01055
"""


def turbo_table():
    """uint8 [256,3]: (turbo(i / 255) * 255).astype(uint8) -- the colours write_objectness_heatmap_to_ply uses (the under colour is
    entry 0 and the over colour entry 255, matplotlib's defaults)."""
    import numpy as np
    return (np.array(_TURBO.split(), dtype=np.float64).reshape(256, 3) * 255).astype(np.uint8)


def zoom_output_shape(in_shape, out_shape):
    """scipy.ndimage.zoom's output shape for the factors out_shape / in_shape: int(round(n * (r / n))) per axis."""
    import numpy as np
    f = np.asarray(out_shape) / np.asarray(in_shape)
    return tuple(int(round(a * b)) for a, b in zip(in_shape, f))


def _zpow(shape):
    """pow(pole, n - 1) per axis with the host's libm pow, as scipy's prefilter computes it."""
    return [math.pow(SPLINE_POLE, int(n) - 1) for n in shape]


def zoom_cubic3d(x, out_shape):
    """scipy.ndimage.zoom(x, factors, order=3) of a float32 [X,Y,Z] tensor onto out_shape (mode 'constant', prefilter), bit-identical."""
    import numpy as np
    x = x.contiguous()
    _chk(x)
    if x.dim() != 3 or x.dtype != torch.float32:
        raise lib.NrpnError("zoom_cubic3d expects a float32 [X,Y,Z] tensor")
    o = tuple(int(v) for v in out_shape)
    out = torch.empty(o, dtype=torch.float32, device=x.device)
    coef = torch.empty(x.numel(), dtype=torch.float64, device=x.device)
    zp = np.array(_zpow(x.shape), dtype=np.float64)
    call("zoom_cubic3d", _p(x), *x.shape, zp.ctypes.data, *o, _p(coef), _p(out), _s())
    return out


def objectness_grid(levels, res):
    """get_objectness_grid: levels = float32 [w,l,h] device tensors in level order -> float64 [prod(res)] in point order (z, then y,
    then x): the sum of their cubic zooms onto res, divided by its maximum."""
    import numpy as np
    res = tuple(int(v) for v in res)
    if not 1 <= len(levels) <= 8:
        raise lib.NrpnError(f"objectness_grid: {len(levels)} levels (1 .. 8)")
    for t in levels:
        _chk(t)
        if t.dim() != 3 or t.dtype != torch.float32:
            raise lib.NrpnError("objectness_grid expects float32 [w,l,h] level grids")
        if zoom_output_shape(t.shape, res) != res:
            raise lib.NrpnError(f"objectness_grid: a zoom of {tuple(t.shape)} does not give {res}")
    dev = levels[0].device
    packed = torch.cat([t.reshape(-1) for t in levels])
    dims = np.array([list(t.shape) for t in levels], dtype=np.int32)
    zp = np.array([_zpow(t.shape) for t in levels], dtype=np.float64)
    coef = torch.empty(packed.numel(), dtype=torch.float64, device=dev)
    work = torch.empty(query("objectness_work_doubles"), dtype=torch.float64, device=dev)
    score = torch.empty(res[0] * res[1] * res[2], dtype=torch.float64, device=dev)
    call("objectness_grid", _p(packed), dims.ctypes.data, zp.ctypes.data, len(levels), *res, _p(coef), _p(work), _p(score), _s())
    return score


def ply_points(rgbsigma, res, alpha_threshold, score=None, turbo=None):
    """The grid rows of write_rgb_to_ply (score None) or write_objectness_heatmap_to_ply: rgbsigma float32 [sx,sy,sz,4] on the device,
    res = the scene's resolution (rx, ry, rz) -> (kept points, uint8 device tensor of the rows' bytes)."""
    rgbsigma = rgbsigma.contiguous()
    _chk(rgbsigma, score)
    if rgbsigma.dim() != 4 or rgbsigma.shape[3] != 4 or rgbsigma.dtype != torch.float32:
        raise lib.NrpnError("ply_points expects a float32 [sx,sy,sz,4] rgbsigma tensor")
    dev = rgbsigma.device
    sx, sy, sz = (int(v) for v in rgbsigma.shape[:3])
    rx, ry, rz = (int(v) for v in res)
    if score is not None:
        if score.dtype != torch.float64 or score.numel() != rx * ry * rz:
            raise lib.NrpnError("ply_points: score must be float64 with one value per grid point")
        turbo = torch.as_tensor(turbo_table() if turbo is None else turbo, dtype=torch.uint8).contiguous().to(dev)
    work = torch.empty(query("ply_points_work_int64", sx * sy * sz), dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    args = (_p(rgbsigma), sx, sy, sz, rx, ry, rz, float(alpha_threshold), _p(score), _p(turbo))
    call("ply_points_count", *args, _p(work), _p(totals), _s())
    count, nbytes = (int(v) for v in totals.tolist())
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if nbytes:
        call("ply_points_write", *args, _p(work), _p(out), _s())
    return count, out


# ======================================================================================================================
# ScanNet ground-truth boxes (scripts/scannet_generate_bbox.py)  [f4]
# ======================================================================================================================
def segment_csr(instance_segments):
    """The instances' segment lists (one iterable of segment ids per instance; set semantics, a segment may appear in several
    instances) -> (seg_ids ascending unique, seg_offsets [S + 1], seg_insts [P]) int32 numpy arrays: the instances of seg_ids[k] are
    seg_insts[seg_offsets[k]:seg_offsets[k + 1]], ascending."""
    import numpy as np
    pairs = sorted({(int(s), g) for g, segs in enumerate(instance_segments) for s in segs})
    if any(not -2 ** 31 <= s < 2 ** 31 for s, _ in pairs):
        raise lib.NrpnError("segment ids must fit int32")
    seg = np.array([s for s, _ in pairs], dtype=np.int32)
    insts = np.array([g for _, g in pairs], dtype=np.int32)
    ids, first = np.unique(seg, return_index=True)
    offs = np.concatenate([first, [len(pairs)]]).astype(np.int32)
    return ids.astype(np.int32), offs, insts


def scannet_instance_boxes(vertices, seg_of_vertex, instance_segments):
    """Boxes of the G instances of a ScanNet-style scan: vertices float32 [V,3] and seg_of_vertex int32 [V] on the device,
    instance_segments = G iterables of segment ids -> (min_pt float32 [G,3], max_pt float32 [G,3], obb float64 [G,7], status int32 [G],
    num_vertices int64 [G]) on the device.

    obb = (cx, cy, cz, length_parallel, length_orthogonal, dz, angle) as the reference's find_minimum_bounding_box returns it: the
    minimum-area rectangle over the hull edges of the xy projection, in float64 of the float32 coordinates -- what the reference computes
    under its pinned numpy 1.x, where float32 / float widens; under numpy 2 the same reference code stays in float32 and lands 1e-7 to
    1e-6 relative away -- and cz, dz in the reference's float32 arithmetic.  Hull edges are taken counter-clockwise from the
    lexicographically smallest (x, y) hull vertex and the first edge of minimum area wins, so the result depends only on the set of
    vertices (the reference starts where Qhull does and may pick another edge of exactly equal area).
    status: 0 ok, 1 fewer than three vertices, 2 all collinear or coincident (the reference raises); obb is NaN there."""
    import numpy as np
    _chk(vertices, seg_of_vertex)
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32:
        raise lib.NrpnError("scannet_instance_boxes expects float32 [V,3] vertices")
    V, G = int(vertices.shape[0]), len(instance_segments)
    if seg_of_vertex.dtype != torch.int32 or tuple(seg_of_vertex.shape) != (V,):
        raise lib.NrpnError("scannet_instance_boxes expects int32 [V] seg_of_vertex")
    if G < 1:
        raise lib.NrpnError("scannet_instance_boxes: no instances")
    dev = vertices.device
    ids, offs, insts = (torch.from_numpy(a).to(dev) for a in segment_csr(instance_segments))
    S, P = int(ids.numel()), int(insts.numel())
    seg_args = (_p(seg_of_vertex), V, _p(ids), _p(offs), _p(insts), S, P, G)
    counts = torch.empty(G, dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    call("scanbox_count", *seg_args, _p(counts), _p(total), _s())
    M = int(total.item())
    nbytes = lib.query("scanbox_work_bytes", V, G, M)
    if nbytes < 0:
        raise lib.NrpnError("scanbox_work_bytes: bad sizes")
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    min_pt = torch.empty((G, 3), dtype=torch.float32, device=dev)
    max_pt = torch.empty((G, 3), dtype=torch.float32, device=dev)
    obb = torch.empty((G, 7), dtype=torch.float64, device=dev)
    status = torch.empty(G, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    call("scanbox_reduce", _p(vertices), *seg_args, _p(counts), M, _p(work), nbytes, _p(min_pt), _p(max_pt), _p(obb), _p(status),
         _p(info), _s())
    max_surv, num_large, err, _ = (int(v) for v in info.tolist())
    if err:
        raise lib.NrpnError("scanbox_reduce: the membership counts changed between the two passes")
    call("scanbox_hull", G, M, max_surv, num_large, _p(work), nbytes, _p(obb), _p(status), _s())
    return min_pt, max_pt, obb, status, counts


# ======================================================================================================================
# rgb-sigma grid of a trained NeRF MLP (scripts/nerf_extract.py)  [f5]
# ======================================================================================================================
NERF_GRID_DEFAULT_CHUNK = 1 << 20      # points per trunk / head launch pair: 512 MiB of scratch (128 floats per point)
_NERF_LAYOUTS = {"flat": 0, "wlh": 1}
NERF_DTYPES = ("fp32", "bf16x3")       # arithmetic of the trunk's matrix products; tensors are float32 either way


def nerf_check_dtype(dtype):
    """``dtype`` if it names an arithmetic of the NeRF trunk; ValueError otherwise."""
    if dtype not in NERF_DTYPES:
        raise ValueError(f"dtype {dtype!r}: expected 'fp32' or 'bf16x3'")
    return dtype


def nerf_check_backward_dtype(dtype, backward_dtype):
    """``backward_dtype`` if it names an arithmetic of the query's backward products that goes with the forward's ``dtype``: "fp32"
    with either, "bf16x3" with "bf16x3" only; ValueError otherwise."""
    if backward_dtype not in NERF_DTYPES:
        raise ValueError(f"backward_dtype {backward_dtype!r}: expected 'fp32' or 'bf16x3'")
    if backward_dtype == "bf16x3" and dtype != "bf16x3":
        raise ValueError(f"backward_dtype 'bf16x3' goes with dtype 'bf16x3' only, not with dtype {dtype!r}")
    return backward_dtype


def nerf_grid_config(cfg):
    """The options of the training run's args.json (a dict or a namespace) that decide the network -> dict(multires, multires_views,
    input_ch_cam).  Supported is what run_nerf.py's config_parser defaults to (run_nerf.py:924-1008): netdepth 8, netwidth 256, multires
    9, use_viewdirs, N_importance 0, i_embed 0, with any multires_views >= 0 and input_ch_cam >= 0; skips is [4] in create_nerf."""
    get = cfg.get if isinstance(cfg, dict) else lambda k, d=None: getattr(cfg, k, d)
    fixed = (("netdepth", 8), ("netwidth", 256), ("multires", 9), ("use_viewdirs", True), ("N_importance", 0), ("i_embed", 0))
    for name, want in fixed:
        have = get(name, want)
        if have != want:
            raise NotImplementedError(f"{name}={have!r}: the HIP NeRF grid kernels are specialised for {name}={want!r}")
    out = {"multires": 9}
    for name, default in (("multires_views", 0), ("input_ch_cam", 4)):
        v = get(name, default)
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise NotImplementedError(f"{name}={v!r}: expected an integer >= 0")
        out[name] = v
    return out


class NerfGridWeights:
    """The device-side weights of one NeRF MLP for nerf_grid_query: the packed trunk and rgb_linear (nrpn_nerfgrid_pack), the view
    columns W_d and the bias of views_linears.0 for the c_p table, and the options they were built for."""
    def __init__(self, packed, w_dirs, b_views, config, w_view=None, raw=None, dtype="fp32", split=None):
        self.packed, self.w_dirs, self.b_views, self.config = packed, w_dirs, b_views, config
        self.w_view = w_view        # the view and camera columns together, [128][views_ch + input_ch_cam]: nerf_render's head
        self.raw = raw              # what nrpn_nerfgrid_pack read: nerf_query's backward packs the transposes from it
        self.dtype = dtype          # "fp32", or "bf16x3" with split: the hi and lo bf16 planes of the trunk's matrices
        self.split = split

    def entry(self, name, *before_split):
        """(C entry, arguments up to and including the weights) of ``name`` in this object's arithmetic: the bf16x3 twins take the
        planes right after ``packed``, which ends ``before_split``."""
        if self.dtype == "fp32":
            return name, before_split
        return name + "_bf16x3", (*before_split, _p(self.split))


def _nerf_raw(t):
    """The float32 device tensors of a network, keyed without ``module.`` -> the one array nrpn_nerfgrid_pack reads."""
    return torch.cat([t[f"pts_linears.{i}.weight"].reshape(-1) for i in range(8)]
                     + [t["feature_linear.weight"].reshape(-1), t["views_linears.0.weight"][:, :256].reshape(-1)]
                     + [t[f"pts_linears.{i}.bias"] for i in range(8)]
                     + [t["feature_linear.bias"], t["alpha_linear.weight"].reshape(-1), t["alpha_linear.bias"],
                        t["rgb_linear.weight"].reshape(-1), t["rgb_linear.bias"]]).contiguous()


def nerf_grid_pack(state_dict, cfg, dtype="fp32"):
    """Upload and pack a checkpoint's network_fn_state_dict once (keys with or without DataParallel's ``module.``) -> NerfGridWeights,
    which nerf_grid_query accepts in place of the state dict.  dtype "bf16x3": the weights also hold the split planes of the trunk's
    matrices, and every consumer of them runs the trunk in that arithmetic."""
    nerf_check_dtype(dtype)
    c = nerf_grid_config(cfg)
    if not torch.cuda.is_available():
        raise lib.NrpnError("nerf_grid_query needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
    W, input_ch, views_ch = 256, 3 + 6 * c["multires"], 3 + 6 * c["multires_views"]
    want = {f"pts_linears.{i}.weight": (W, input_ch if i == 0 else W + input_ch if i == 5 else W) for i in range(8)}
    want.update({f"pts_linears.{i}.bias": (W,) for i in range(8)})
    want.update({"feature_linear.weight": (W, W), "feature_linear.bias": (W,), "alpha_linear.weight": (1, W), "alpha_linear.bias": (1,),
                 "views_linears.0.weight": (W // 2, views_ch + c["input_ch_cam"] + W), "views_linears.0.bias": (W // 2,),
                 "rgb_linear.weight": (3, W // 2), "rgb_linear.bias": (3,)})
    for k, shape in want.items():
        if k not in sd:
            raise lib.NrpnError(f"nerf_grid_query: the state dict has no {k}")
        if tuple(sd[k].shape) != shape:
            raise lib.NrpnError(f"nerf_grid_query: {k} has shape {tuple(sd[k].shape)}, the configuration implies {shape}")
    t = {k: sd[k].detach().to(device=dev, dtype=torch.float32) for k in want}
    wv = t["views_linears.0.weight"]
    raw = _nerf_raw(t)
    packed = torch.empty(lib.query("nerfgrid_work_bytes", 0, 0) // 4, dtype=torch.float32, device=dev)
    call("nerfgrid_pack", _p(raw), input_ch, _p(packed), _s())
    split = None
    if dtype == "bf16x3":
        split = torch.empty(lib.query("nerfgrid_work_bytes", 2, 0) // 2, dtype=torch.bfloat16, device=dev)
        call("nerfgrid_pack_bf16x3", _p(raw), input_ch, _p(split), _s())
    return NerfGridWeights(packed, wv[:, W:W + views_ch].contiguous(), t["views_linears.0.bias"], c, wv[:, W:].contiguous(), raw, dtype,
                           split)


def _nerf_weights(who, weights_or_state, cfg, dtype=None):
    """The NerfGridWeights given, or those of a given network_fn_state_dict (packed for ``dtype``, default fp32); either way they
    must fit cfg, and given weights carry their own arithmetic: a ``dtype`` that contradicts it is an error -> NerfGridWeights."""
    if dtype is not None:
        nerf_check_dtype(dtype)
    if isinstance(weights_or_state, NerfGridWeights):
        weights = weights_or_state
        if dtype is not None and dtype != weights.dtype:
            raise ValueError(f"{who}: dtype {dtype!r} given with weights packed for {weights.dtype!r}")
    else:
        weights = nerf_grid_pack(weights_or_state, cfg, dtype or "fp32")
    if weights.config != nerf_grid_config(cfg):
        raise lib.NrpnError(f"{who}: the weights were packed for other options")
    return weights


def _nerf_bounds(bb_center, bb_scale):
    """The scene normalisation as the kernels take it: the float32 values of bb_center [3] and bb_scale -> (cx, cy, cz, scale)."""
    center, scale = (torch.as_tensor(x, dtype=torch.float32) for x in (bb_center, bb_scale))
    return (*center.reshape(3).tolist(), scale.reshape(()).item())


def nerf_grid_query(state_dict, cfg, xs, ys, zs, bb_center, bb_scale, poses, layout="flat", chunk=None, dtype=None):
    """extract_nerf of the reference's run_nerf.py (:1157-1194) for the NeRF MLP of DESIGN.md 3.16.

    state_dict: the checkpoint's network_fn_state_dict (keys with or without DataParallel's ``module.``), or the NerfGridWeights
    nerf_grid_pack made of it (several queries of one network then pack once); cfg: the run's args.json;
    xs / ys / zs: the float32 torch.linspace values of the grid axes; bb_center [3], bb_scale: the scene normalisation of run_network;
    poses [P, >=3, >=3]: the training camera-to-world matrices.  Returns a float32 device tensor: layout "flat" (N, 4) with row
    (iz * res_y + iy) * res_x + ix -- the reference's array -- or "wlh" (res_x, res_y, res_z, 4), the grid datasets.py reads.
    Channels: mean over the poses of sigmoid(rgb), summed in pose order, and the raw density.  The trunk of the MLP runs once per point
    on the exact-fp32 MFMA; the poses loop over views_linears.0 / rgb_linear only.  ``chunk`` (points, default 2^20) bounds the scratch
    and never changes the result.  The arithmetic of the trunk is the weights' (nerf_grid_pack's dtype); with a state dict, ``dtype`` selects it."""
    if layout not in _NERF_LAYOUTS:
        raise ValueError(f"layout {layout!r}: expected 'flat' or 'wlh'")
    weights = _nerf_weights("nerf_grid_query", state_dict, cfg, dtype)
    c, packed, dev = weights.config, weights.packed, weights.packed.device
    # c_p = W_d embed_dirs(d_p) + b: the camera embedding is zero at extraction (run_nerf.py:1177), its columns drop out
    poses = torch.as_tensor(poses, dtype=torch.float32).to(dev)
    if poses.dim() != 3 or poses.shape[0] < 1 or poses.shape[1] < 3 or poses.shape[2] < 3:
        raise lib.NrpnError(f"nerf_grid_query expects poses [P, >=3, >=3], got {tuple(poses.shape)}")
    d = poses[:, :3, :3] @ torch.tensor([0.0, 0.0, -1.0], device=dev)
    emb = [d]
    for freq in 2. ** torch.linspace(0., c["multires_views"] - 1, steps=c["multires_views"]):
        emb += [torch.sin(d * freq.item()), torch.cos(d * freq.item())]
    ctab = (torch.cat(emb, -1) @ weights.w_dirs.T + weights.b_views).contiguous()

    axes = [torch.as_tensor(a, dtype=torch.float32).reshape(-1).to(dev).contiguous() for a in (xs, ys, zs)]
    rx, ry, rz = (int(a.numel()) for a in axes)
    if min(rx, ry, rz) < 1:
        raise lib.NrpnError(f"nerf_grid_query: empty axis in resolution {rx} x {ry} x {rz}")
    n = rx * ry * rz
    chunk = NERF_GRID_DEFAULT_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise lib.NrpnError(f"nerf_grid_query: chunk {chunk}")
    nbytes = lib.query("nerfgrid_work_bytes", 1, min(chunk, n))
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((n, 4) if layout == "flat" else (rx, ry, rz, 4), dtype=torch.float32, device=dev)
    name, head = weights.entry("nerfgrid_query", _p(axes[0]), _p(axes[1]), _p(axes[2]), rx, ry, rz, *_nerf_bounds(bb_center, bb_scale),
                               c["multires"], _p(packed))
    call(name, *head, _p(ctab), int(ctab.shape[0]), _NERF_LAYOUTS[layout], chunk, _p(work), nbytes, _p(out), _s())
    return out


# ======================================================================================================================
# views of a trained NeRF MLP (scripts/nerf_render.py)  [f6]
# ======================================================================================================================
NERF_RENDER_DEFAULT_CHUNK = 4096       # rays per launch group: 256 MiB of g scratch at 128 samples per pass


def _nerf_render_inputs(who, weights_or_state, cfg, H, W, intrinsic, c2w, rays, near, far, bb_center, bb_scale, z_samples, n_samples,
                        lindisp, embedded_cam, z2, chunk, dtype=None):
    """The arguments nerf_render and nerf_camopt_prepare share, checked and on the device -> namespace."""
    weights = _nerf_weights(who, weights_or_state, cfg, dtype)
    c, packed, dev = weights.config, weights.packed, weights.packed.device

    def f32(x, shape=None):
        x = torch.as_tensor(x, dtype=torch.float32).to(dev)
        return (x if shape is None else x.reshape(shape)).contiguous()
    cam_ch = c["input_ch_cam"]
    cam = torch.zeros(cam_ch, dtype=torch.float32, device=dev) if embedded_cam is None else f32(embedded_cam, -1)
    if cam.numel() != cam_ch:
        raise lib.NrpnError(f"{who}: embedded_cam has {cam.numel()} values, input_ch_cam is {cam_ch}")
    if (near is None or far is None) and (z_samples is None or z2 is None):
        raise lib.NrpnError(f"{who}: near and far are needed to place the samples")
    near, far = (0. if near is None else float(near)), (0. if far is None else float(far))
    if z_samples is not None:
        z1 = f32(z_samples, -1)
        s1 = int(z1.numel())
        mode, s2 = (1, s1) if z2 is None else (2, int(torch.as_tensor(z2).shape[-1]))
        if mode == 1 and s1 < 3:
            raise lib.NrpnError(f"{who}: {s1} precomputed samples, the depth-guided pass needs at least 3")
    else:
        if z2 is not None:
            raise lib.NrpnError(f"{who}: z2 goes with z_samples")
        if n_samples is None or int(n_samples) < 1:
            raise lib.NrpnError(f"{who}: n_samples {n_samples!r}")
        # render_rays :571, :602-606 on [1, 1] bounds: the float32 values the reference gives every ray
        t_vals = torch.linspace(0., 1., steps=int(n_samples))
        n_t, f_t = torch.full((1, 1), near), torch.full((1, 1), far)
        z1 = n_t * (1. - t_vals) + f_t * t_vals if not lindisp else 1. / (1. / n_t * (1. - t_vals) + 1. / f_t * t_vals)
        z1 = f32(z1, -1)
        s1, mode, s2 = int(z1.numel()), 0, 0
    frame = [x is not None for x in (H, W, intrinsic, c2w)]
    if rays is not None and any(frame):
        raise lib.NrpnError(f"{who}: give H, W, intrinsic and c2w, or rays, not both")
    if rays is not None:
        rays_t = f32(rays)
        if rays_t.dim() != 2 or rays_t.shape[1] != 6 or rays_t.shape[0] < 1:
            raise lib.NrpnError(f"{who} expects rays [R, 6], got {tuple(rays_t.shape)}")
        lead = (int(rays_t.shape[0]),)
    else:
        if not all(frame) or int(H) < 1 or int(W) < 1:
            raise lib.NrpnError(f"{who}: give H, W, intrinsic and c2w, or rays")
        pose = torch.as_tensor(c2w, dtype=torch.float32)
        if pose.dim() != 2 or pose.shape[0] < 3 or pose.shape[1] != 4:
            raise lib.NrpnError(f"{who} expects c2w [>=3, 4], got {tuple(pose.shape)}")
        camera = f32(torch.cat([torch.as_tensor(intrinsic, dtype=torch.float32).reshape(4), pose[:3].reshape(12)]))
        lead = (int(H), int(W))
    n = lead[0] if len(lead) == 1 else lead[0] * lead[1]
    z2_t = None
    if mode == 2:
        z2_t = f32(z2)
        if tuple(z2_t.shape) != (n, s2) or s2 < 1:
            raise lib.NrpnError(f"{who} expects z2 [{n}, S2], got {tuple(z2_t.shape)}")
    chunk = NERF_RENDER_DEFAULT_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise lib.NrpnError(f"{who}: chunk {chunk}")
    *center, scale = _nerf_bounds(bb_center, bb_scale)
    return SimpleNamespace(weights=weights, c=c, packed=packed, dev=dev, cam_ch=cam_ch, cam=cam, near=near, far=far, z1=z1, s1=s1, mode=mode,
                           s2=s2, rays_t=rays_t if rays is not None else None, camera=camera if rays is None else None, lead=lead, n=n,
                           z2_t=z2_t, center=center, scale=scale, chunk=chunk, f32=f32)


def nerf_render(weights_or_state, cfg, H=None, W=None, intrinsic=None, c2w=None, rays=None, near=None, far=None, bb_center=(0., 0., 0.),
                bb_scale=1., z_samples=None, n_samples=None, lindisp=False, embedded_cam=None, chunk=None, return_samples=False,
                z2=None, return_stages=False, dtype=None):
    """render (run_nerf.py:82-157) with render_rays (:514-614) at test time for the NeRF MLP of DESIGN.md 3.16, on the GPU.

    weights_or_state: the NerfGridWeights of nerf_grid_pack, or a network_fn_state_dict; cfg: the run's args.json.  The rays are those
    of every pixel of an H x W frame with intrinsic = (fx, fy, cx, cy) and the camera-to-world matrix c2w [>=3, 4] (the assumed
    get_rays: d = R [(u - cx) / fx, -(v - cy) / fy, -1], o = t), or ``rays`` [R, 6] = (o, d); giving both is an error.  near, far: the
    ray bounds, which the plain path's samples span and the drawn samples are clamped to -- required there; with z2 given nothing
    reads them.  bb_center [3], bb_scale: the scene normalisation of run_network.  z_samples [N / 2] float32 (precomputed_z_samples) selects the two-pass
    path: those samples on every ray, then as many around the depth they predict (compute_samples_around_depth), both composited.
    z_samples None selects the plain path: n_samples between near and far, linear in depth or, with lindisp, in inverse depth.
    embedded_cam [input_ch_cam]: the camera embedding (default zeros, as video and test use).  chunk: rays per launch group (default
    4096); it never changes the result.

    Returns a dict of float32 device tensors keyed as render_rays returns them -- rgb_map [.., 3], depth_map, acc_map, disp_map [..]
    -- plus depth_std = sqrt(clamp(sum((z - depth)^2 w), 0, 1)) (render_video :184-185), with leading shape (H, W) or (R,);
    return_samples adds z_vals and weights [.., S].  z2 [R, S2]: run the second pass on these samples instead of drawing them;
    return_stages adds raw1 [R, S1, 4] (the first pass's rgb before the sigmoid and sigma) and z2 (the drawn samples).  The trunk of
    both passes runs in the weights' arithmetic (nerf_grid_pack's dtype); with a state dict, ``dtype`` selects it."""
    a = _nerf_render_inputs("nerf_render", weights_or_state, cfg, H, W, intrinsic, c2w, rays, near, far, bb_center, bb_scale, z_samples,
                            n_samples, lindisp, embedded_cam, z2, chunk, dtype)
    c, n, s1, s2 = a.c, a.n, a.s1, a.s2
    nbytes = lib.query("nerfrender_work_bytes", min(a.chunk, n), s1, s2)
    if nbytes < 0:
        raise lib.NrpnError(f"nerf_render: chunk {a.chunk} with {s1} + {s2} samples is outside the supported range")
    work = torch.empty(nbytes, dtype=torch.uint8, device=a.dev)

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=a.dev)
    out = {"rgb_map": new(n, 3), "depth_map": new(n), "acc_map": new(n), "disp_map": new(n), "depth_std": new(n)}
    if return_samples:
        out["z_vals"], out["weights"] = new(n, s1 + s2), new(n, s1 + s2)
    if return_stages:
        out["raw1"] = new(n, s1, 4)
        if a.mode == 1:
            out["z2"] = new(n, s2)

    def opt(k):
        return _p(out[k]) if k in out else None
    to_packed = (a.near, a.far, *a.center, a.scale, c["multires"], c["multires_views"], a.cam_ch, _p(a.packed))
    common = (_p(a.weights.w_view), _p(a.weights.b_views), _p(a.cam) if a.cam_ch else None, _p(a.z1), s1, a.mode, _p(a.z2_t) if a.z2_t is not None else None,
              s2, a.chunk, _p(work), nbytes, _p(out["rgb_map"]), _p(out["depth_map"]), _p(out["acc_map"]), _p(out["disp_map"]),
              _p(out["depth_std"]), opt("z_vals"), opt("weights"), opt("raw1"), opt("z2"), _s())
    if a.rays_t is not None:
        name, head = a.weights.entry("nerfrender_rays", _p(a.rays_t), n, *to_packed)
    else:
        name, head = a.weights.entry("nerfrender_frame", a.lead[0], a.lead[1], _p(a.camera), *to_packed)
    call(name, *head, *common)
    return {k: (v if k in ("raw1", "z2") else v.reshape(*a.lead, *v.shape[1:])) for k, v in out.items()}


NERF_BOX_MODES = ("keep", "remove")
NERF_MAX_BOXES = 1024


def nerf_box_table(boxes):
    """boxes [K, 7] = (cx, cy, cz, w, l, h, theta), rotated about z by theta (the ``obb`` of scannet_generate_bbox's instance json,
    proposals2ngp.obb_to_ngp_boxes' convention), or [K, 6] = (min, max) with theta = 0, in the NeRF's world coordinates -> float64
    numpy [K, 8]: centre, half extents, cos(theta), sin(theta) -- what the kernels and the checker read.  K = 0 is allowed.
    ValueError for another shape, a value that is not finite, an extent <= 0 or K > 1024."""
    b = np.asarray(boxes.detach().cpu().numpy() if isinstance(boxes, torch.Tensor) else boxes, dtype=np.float64)
    if b.ndim == 1 and b.size == 0:
        b = b.reshape(0, 7)
    if b.ndim != 2 or b.shape[1] not in (6, 7):
        raise ValueError(f"boxes of shape {tuple(b.shape)}: expected [K, 7] = (cx, cy, cz, w, l, h, theta) or [K, 6] = (min, max)")
    if b.shape[0] > NERF_MAX_BOXES:
        raise ValueError(f"{b.shape[0]} boxes: at most {NERF_MAX_BOXES} are supported")
    bad = np.argwhere(~np.isfinite(b))
    if len(bad):
        k, j = bad[0]
        raise ValueError(f"box {int(k)} has the value {float(b[k, j])!r} in column {int(j)}")
    if b.shape[1] == 6:
        centre, half, theta = (b[:, :3] + b[:, 3:]) * 0.5, (b[:, 3:] - b[:, :3]) * 0.5, np.zeros(len(b))
    else:
        centre, half, theta = b[:, :3], b[:, 3:6] * 0.5, b[:, 6]
    small = np.argwhere(~(half > 0))
    if len(small):
        k, j = small[0]
        raise ValueError(f"box {int(k)} has the extent {float(2 * half[k, j])!r} on axis {int(j)}: extents must be > 0")
    return np.ascontiguousarray(np.concatenate([centre, half, np.cos(theta)[:, None], np.sin(theta)[:, None]], 1))


def nerf_check_box_mode(mode):
    if mode not in NERF_BOX_MODES:
        raise ValueError(f"mode {mode!r}: expected 'keep' or 'remove'")
    return NERF_BOX_MODES.index(mode)


def nerf_boxes_to_world(boxes_grid, features):
    """Proposals in grid coordinates -> boxes in the world coordinates of the NeRF the grid was extracted from.  boxes_grid [K, 7] =
    (x, y, z, w, l, h, theta) or [K, 6] = (min, max) as run_rpn / run_fcos write them; features: the feature file of nerf_extract (a
    mapping with resolution, bbox_min, bbox_max, scale, offset, from_ddp_nerf).  Per axis p / resolution * (bbox_max - bbox_min) +
    bbox_min for centres and corners and the same scale for extents, as proposals2ngp does; theta is kept.  Scenes of instant-ngp
    (from_ddp_nerf false, or a scale / offset other than 1 / 0) are refused: they keep going through proposals2ngp.  Host numpy."""
    keys = features.keys() if hasattr(features, "keys") else ()
    ddp = bool(np.asarray(features["from_ddp_nerf"]).item()) if "from_ddp_nerf" in keys else False
    if not ddp:
        raise ValueError("nerf_boxes_to_world: the feature file is not from_ddp_nerf; instant-ngp scenes go through proposals2ngp")
    scale, offset = np.asarray(features["scale"], dtype=np.float64), np.asarray(features["offset"], dtype=np.float64)
    if not (np.all(scale == 1.0) and np.all(offset == 0.0)):
        raise ValueError(f"nerf_boxes_to_world: scale {scale.tolist()!r} / offset {offset.tolist()!r}: expected 1 and 0")
    b = np.asarray(boxes_grid, dtype=np.float64)
    if b.ndim == 1 and b.size == 0:
        b = b.reshape(0, 7)
    if b.ndim != 2 or b.shape[1] not in (6, 7):
        raise ValueError(f"nerf_boxes_to_world: boxes of shape {tuple(b.shape)}: expected [K, 7] or [K, 6]")
    res = np.asarray(features["resolution"], dtype=np.float64).reshape(3)
    lo, hi = (np.asarray(features[k], dtype=np.float64).reshape(3) for k in ("bbox_min", "bbox_max"))
    diag = hi - lo
    if b.shape[1] == 6:
        return np.concatenate([b[:, :3] / res * diag + lo, b[:, 3:] / res * diag + lo], 1)
    return np.concatenate([b[:, :3] / res * diag + lo, b[:, 3:6] / res * diag, b[:, 6:]], 1)


def nerf_render_boxes(weights_or_state, cfg, boxes, mode="keep", *, skip=True, H=None, W=None, intrinsic=None, c2w=None, rays=None,
                      near=None, far=None, bb_center=(0., 0., 0.), bb_scale=1., z_samples=None, n_samples=None, lindisp=False,
                      embedded_cam=None, chunk=None, return_samples=False, z2=None, return_stages=False, dtype=None):
    """nerf_render restricted to 3D boxes: the scene inside the boxes only (mode "keep": a proposed object, cut out) or with them
    removed (mode "remove").  boxes: nerf_box_table's input, in the NeRF's world coordinates (before bb_center / bb_scale); every
    other argument is nerf_render's.  A sample counts if its float32 world point o + d z lies in at least one box (keep) or in none
    (remove), tested in float64 with closed faces; the raw values of every other sample are +0 after the head of each pass, so the
    second list is drawn from the masked first pass and the composite gives those samples weight 0.  A ray without a counted sample
    has rgb, depth and acc 0 and a NaN disp_map (the reference's 0 / 0).  skip: leave out the trunk and head of every 64-point tile
    without a counted point; False runs every tile and gives the same bits.

    Returns nerf_render's dict (return_samples / return_stages included; raw1 is the masked raw) plus tiles_total and tiles_run:
    int64 device tensors [2], the 64-point tiles of each pass over all chunks and those whose trunk ran."""
    table = nerf_box_table(boxes)
    mode_i = nerf_check_box_mode(mode)
    a = _nerf_render_inputs("nerf_render_boxes", weights_or_state, cfg, H, W, intrinsic, c2w, rays, near, far, bb_center, bb_scale,
                            z_samples, n_samples, lindisp, embedded_cam, z2, chunk, dtype)
    c, n, s1, s2 = a.c, a.n, a.s1, a.s2
    per = min(a.chunk, n)
    nbytes = lib.query("nerfrender_boxes_work_bytes", per, s1, s2)
    if nbytes < 0:
        raise lib.NrpnError(f"nerf_render_boxes: chunk {a.chunk} with {s1} + {s2} samples is outside the supported range")
    work = torch.empty(nbytes, dtype=torch.uint8, device=a.dev)
    k = int(table.shape[0])
    boxes_t = torch.from_numpy(table if k else np.zeros((1, 8))).to(a.dev)      # never null; with K = 0 nothing of it is read

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=a.dev)
    out = {"rgb_map": new(n, 3), "depth_map": new(n), "acc_map": new(n), "disp_map": new(n), "depth_std": new(n)}
    if return_samples:
        out["z_vals"], out["weights"] = new(n, s1 + s2), new(n, s1 + s2)
    if return_stages:
        out["raw1"] = new(n, s1, 4)
        if a.mode == 1:
            out["z2"] = new(n, s2)
    sizes = [per] * (n // per) + ([n % per] if n % per else [])
    tiles_total = torch.tensor([sum(-(-r * s // 64) for r in sizes) for s in (s1, s2)], dtype=torch.int64).to(a.dev)
    tiles_run = torch.empty(2, dtype=torch.int64, device=a.dev)

    def opt(key):
        return _p(out[key]) if key in out else None
    args = (a.near, a.far, *a.center, a.scale, c["multires"], c["multires_views"], a.cam_ch, _p(a.packed),
            _p(a.weights.split) if a.weights.dtype == "bf16x3" else None, _p(a.weights.w_view), _p(a.weights.b_views),
            _p(a.cam) if a.cam_ch else None, _p(a.z1), s1, a.mode, _p(a.z2_t) if a.z2_t is not None else None, s2, a.chunk, _p(work),
            nbytes, _p(out["rgb_map"]), _p(out["depth_map"]), _p(out["acc_map"]), _p(out["disp_map"]), _p(out["depth_std"]),
            opt("z_vals"), opt("weights"), opt("raw1"), opt("z2"), _p(boxes_t), k, mode_i, 1 if skip else 0, _p(tiles_run), _s())
    if a.rays_t is not None:
        call("nerfrender_rays_boxes", _p(a.rays_t), n, *args)
    else:
        call("nerfrender_frame_boxes", a.lead[0], a.lead[1], _p(a.camera), *args)
    res = {key: (v if key in ("raw1", "z2") else v.reshape(*a.lead, *v.shape[1:])) for key, v in out.items()}
    res["tiles_total"], res["tiles_run"] = tiles_total, tiles_run
    return res


def nerf_render_samples(raw, rays, z_samples, near, far):
    """compute_samples_around_depth (run_nerf.py:497-502) on its own: raw [R, S, 4] and rays [R, 6] on the first-pass samples
    z_samples [S] -> z2 [R, S] float32, the depth-guided samples nerf_render draws between its two passes."""
    if not torch.cuda.is_available():
        raise lib.NrpnError("nerf_render_samples needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    raw = torch.as_tensor(raw, dtype=torch.float32).to(dev).contiguous()
    rays = torch.as_tensor(rays, dtype=torch.float32).to(dev).contiguous()
    z = torch.as_tensor(z_samples, dtype=torch.float32).to(dev).reshape(-1).contiguous()
    n, s = int(rays.shape[0]), int(z.numel())
    if tuple(raw.shape) != (n, s, 4) or rays.dim() != 2 or rays.shape[1] != 6:
        raise lib.NrpnError(f"nerf_render_samples expects raw [R, {s}, 4] and rays [R, 6], got {tuple(raw.shape)} and {tuple(rays.shape)}")
    z2 = torch.empty((n, s), dtype=torch.float32, device=dev)
    call("nerfrender_samples", _p(raw), _p(rays), _p(z), s, float(near), float(far), n, _p(z2), _s())
    return z2


# ======================================================================================================================
# test-time optimisation of the camera embedding (scripts/nerf_test_opt.py)  [f8]
# ======================================================================================================================
class NerfCamoptState:
    """What nerf_camopt_prepare keeps of one image for nerf_camopt_eval: the rays, the second-pass samples, every sample's float64
    compositing weight, the trunk's g of the chunks that fit the cache, the target and the ray weights."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def nerf_camopt_prepare(weights_or_state, cfg, target, H=None, W=None, intrinsic=None, c2w=None, rays=None, near=None, far=None,
                        bb_center=(0., 0., 0.), bb_scale=1., z_samples=None, n_samples=None, lindisp=False, chunk=None, z2=None,
                        ray_weight=None, cache_bytes=None):
    """Everything of optimize_camera_embedding's objective (run_nerf.py:193-229) that does not depend on the embedding, once per image.

    The arguments of nerf_render select the model, the rays and the samples; ``target`` [R, 3] or [H, W, 3] float32 is the image;
    ``ray_weight`` [R] float64 the weight rw of each ray's squared error (default 1 / (3 R), the image's mean squared error; the
    reference's batches: camopt.ray_weights).  The embedding enters the network at views_linears.0 only, so sigma, both sample lists
    and every compositing weight are computed here; ``cache_bytes`` (default: what all chunks need, capped at half of the free
    device memory, torch's unused reserve included) decides how many chunks also keep the trunk's output g, 512 bytes per sample -- the others re-run the trunk at
    every evaluation, to the same bits.  ``chunk`` fixes the chunks (default 4096 rays).  -> NerfCamoptState"""
    a = _nerf_render_inputs("nerf_camopt_prepare", weights_or_state, cfg, H, W, intrinsic, c2w, rays, near, far, bb_center, bb_scale,
                            z_samples, n_samples, lindisp, None, z2, chunk)
    if a.weights.dtype != "fp32":
        raise NotImplementedError(f"nerf_camopt_prepare: the weights were packed for {a.weights.dtype!r}; the camera-embedding objective "
                                  "runs in fp32 only")
    if a.cam_ch < 1:
        raise lib.NrpnError("nerf_camopt_prepare: the model has no camera embedding (input_ch_cam is 0)")
    dev, n, s1, s2, chunk = a.dev, a.n, a.s1, a.s2, a.chunk
    target = a.f32(target, (-1, 3))
    if target.shape[0] != n:
        raise lib.NrpnError(f"nerf_camopt_prepare: target has {target.shape[0]} pixels, there are {n} rays")
    if ray_weight is None:
        rw = torch.full((n,), 1. / (3. * n), dtype=torch.float64, device=dev)
    else:
        rw = torch.as_tensor(ray_weight, dtype=torch.float64).to(dev).reshape(-1).contiguous()
        if rw.numel() != n:
            raise lib.NrpnError(f"nerf_camopt_prepare: ray_weight has {rw.numel()} values, there are {n} rays")
    sizes = [lib.query("nerfcamopt_work_bytes", what, n, chunk, s1, s2) for what in range(3)]
    if min(sizes) < 0:
        raise lib.NrpnError(f"nerf_camopt_prepare: chunk {chunk} with {s1} + {s2} samples is outside the supported range")
    chunks = -(-n // min(chunk, n))
    if cache_bytes is None:       # free on the device, plus what torch's allocator holds but has not handed out
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        cache_bytes = min(chunks * sizes[2], free // 2)
    cached = max(0, min(chunks, int(cache_bytes) // sizes[2]))
    st = NerfCamoptState(inputs=a, n=n, lead=a.lead, chunk=chunk, chunks=chunks, cached_chunks=cached, g_bytes=cached * sizes[2],
                         eval_bytes=sizes[1], target=target, rw=rw, work=None)
    st.rays = a.rays_t if a.rays_t is not None else torch.empty((n, 6), dtype=torch.float32, device=dev)
    st.z2 = a.z2_t if a.mode == 2 else torch.empty((n, s2), dtype=torch.float32, device=dev) if a.mode == 1 else None
    st.w1 = torch.empty((n, s1), dtype=torch.float64, device=dev)
    st.w2 = torch.empty((n, s2), dtype=torch.float64, device=dev) if s2 else None
    st.g = torch.empty(cached * sizes[2] // 4, dtype=torch.float32, device=dev) if cached else None
    work = torch.empty(sizes[0], dtype=torch.uint8, device=dev)
    frame = a.camera is not None
    call("nerfcamopt_prepare", None if frame else _p(st.rays), a.lead[0] if frame else 0, a.lead[1] if frame else 0,
         _p(a.camera) if frame else None, n, a.near, a.far, *a.center, a.scale, a.c["multires"], _p(a.packed), _p(a.z1), s1, a.mode,
         _p(a.z2_t) if a.mode == 2 else None, s2, chunk, _p(work), sizes[0], _p(st.rays) if frame else None,
         _p(st.z2) if a.mode == 1 else None, _p(st.w1), _p(st.w2) if s2 else None, _p(st.g) if cached else None, cached, _s())
    return st


def nerf_camopt_eval(state, cam, return_rgb=False):
    """The objective of optimize_camera_embedding at the embedding ``cam`` [input_ch_cam] for a prepared image: -> (loss, grad) or
    (loss, grad, rgb_map).  loss (a Python float) = sum_r rw[r] sum_ch (rgb_map - target)^2 and grad (float64 [input_ch_cam], on the
    device) its derivative; rgb_map (float32, shaped like nerf_render's) is bit-equal to nerf_render's at this embedding.  float64
    after the head's raw rgb, fixed-order sums: repeated calls are bit-equal, and so are different cache budgets."""
    st, a = state, state.inputs
    dev = a.dev
    cam = a.f32(cam, -1)
    if cam.numel() != a.cam_ch:
        raise lib.NrpnError(f"nerf_camopt_eval: cam has {cam.numel()} values, input_ch_cam is {a.cam_ch}")
    if st.work is None:
        st.work = torch.empty(st.eval_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(1 + a.cam_ch, dtype=torch.float64, device=dev)
    rgb = torch.empty((st.n, 3), dtype=torch.float32, device=dev) if return_rgb else None
    call("nerfcamopt_eval", _p(st.rays), st.n, *a.center, a.scale, a.c["multires"], a.c["multires_views"], a.cam_ch, _p(a.packed),
         _p(a.weights.w_view), _p(a.weights.b_views), _p(cam), _p(a.z1), a.s1, _p(st.z2) if a.s2 else None, a.s2, _p(st.w1),
         _p(st.w2) if a.s2 else None, _p(st.target), _p(st.rw), st.chunk, _p(st.g) if st.cached_chunks else None, st.cached_chunks,
         _p(st.work), st.eval_bytes, _p(out), _p(rgb) if return_rgb else None, _s())
    loss = float(out[0].item())
    return (loss, out[1:], rgb.reshape(*st.lead, 3)) if return_rgb else (loss, out[1:])


# ======================================================================================================================
# metrics of a rendered view against its ground truth (scripts/nerf_test.py)  [f7]
# ======================================================================================================================
NERF_SSIM_WINDOW = 7


def nerf_view_metrics(rgb, target_rgb, depth=None, target_depth=None, valid_depth=None, far=None, return_images=False):
    """What render_images_with_metrics (run_nerf.py:231-311) computes for one rendered frame, on the GPU (csrc/nerfmetrics.hip).

    rgb [H, W, 3] float32: the raw rgb_map; target_rgb [H, W, 3] float32.  depth, target_depth [H, W] float32 and valid_depth [H, W]
    bool / uint8 go together (all three or none).  Returns a dict of Python numbers:
      img_loss    mean of (rgb - target)^2 over H W 3, on the unclamped rgb (:283);  psnr = -10 log10(img_loss) (:284)
      ssim        skimage's structural_similarity(clamp(rgb, 0, 1), target, data_range=1., channel_axis=-1) with its defaults (:286-287)
      depth_rmse  sqrt of the mean of (depth - target_depth)^2 over the selected pixels (:277), None if none is selected (:278) or
                  no depth is given; an unselected target is never read, so it may hold NaN or inf
      n_valid     the number of selected pixels
    All sums run in float64 on the widened float32 values, without atomics: repeated calls are bit-equal.  return_images adds the
    device tensors rgb8 [H, W, 3] uint8 = to8b(clamp(rgb)) (:291, :325) and, given depth and ``far``, depth16 [H, W] uint16 =
    to16b(depth / far) (:293, :327).  Shape or dtype mismatches raise lib.NrpnError; a frame below 7 x 7 raises ValueError, as
    skimage does."""
    if not torch.cuda.is_available():
        raise lib.NrpnError("nerf_view_metrics needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())

    def dev_tensor(name, x, dtypes, shape=None):
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(x)
        if x.dtype not in dtypes:
            raise lib.NrpnError(f"nerf_view_metrics: {name} is {x.dtype}, expected {' / '.join(str(d) for d in dtypes)}")
        if shape is not None and tuple(x.shape) != shape:
            raise lib.NrpnError(f"nerf_view_metrics: {name} has shape {tuple(x.shape)}, expected {shape}")
        return x.to(dev).contiguous()
    rgb = dev_tensor("rgb", rgb, (torch.float32,))
    if rgb.dim() != 3 or rgb.shape[2] != 3:
        raise lib.NrpnError(f"nerf_view_metrics expects rgb [H, W, 3], got {tuple(rgb.shape)}")
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    target = dev_tensor("target_rgb", target_rgb, (torch.float32,), (H, W, 3))
    given = [x is not None for x in (depth, target_depth, valid_depth)]
    if any(given) and not all(given):
        raise lib.NrpnError("nerf_view_metrics: depth, target_depth and valid_depth go together")
    if all(given):
        depth = dev_tensor("depth", depth, (torch.float32,), (H, W))
        target_depth = dev_tensor("target_depth", target_depth, (torch.float32,), (H, W))
        valid = dev_tensor("valid_depth", valid_depth, (torch.bool, torch.uint8), (H, W))
        valid = valid.view(torch.uint8) if valid.dtype == torch.bool else valid
    else:
        depth = target_depth = valid = None
    if return_images and depth is not None and far is None:
        raise lib.NrpnError("nerf_view_metrics: far is needed for depth16 = to16b(depth / far)")
    if H < NERF_SSIM_WINDOW or W < NERF_SSIM_WINDOW:
        raise ValueError(f"nerf_view_metrics: a {H} x {W} frame is smaller than the 7 x 7 SSIM window")
    nbytes = lib.query("nerfmetrics_work_bytes", H, W)
    if nbytes < 0:
        raise lib.NrpnError(f"nerf_view_metrics: a {H} x {W} frame is outside the supported range")
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    call("nerfmetrics_frame", _p(rgb), _p(target), H, W, _p(depth) or None, _p(target_depth) or None, _p(valid) or None, _p(work),
         nbytes, _p(sums), _s())
    out = {}
    if return_images:
        out["rgb8"] = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        if depth is not None:
            out["depth16"] = torch.empty((H, W), dtype=torch.uint16, device=dev)
        call("nerfmetrics_quantise", _p(rgb), H * W * 3, _p(out["rgb8"]), _p(depth) or None, float(far) if depth is not None else 1.0,
             H * W if depth is not None else 0, _p(out.get("depth16")) or None, _s())
    s = sums.cpu().tolist()          # the frame's only float traffic to the host: eight doubles
    windows = (H - NERF_SSIM_WINDOW + 1) * (W - NERF_SSIM_WINDOW + 1)
    img_loss = s[0] / (H * W * 3)
    n_valid = int(s[5])
    out.update(img_loss=img_loss, psnr=-10. * math.log10(img_loss) if img_loss > 0. else (math.inf if img_loss == 0. else math.nan),
               ssim=(s[1] / windows + s[2] / windows + s[3] / windows) / 3.,
               depth_rmse=math.sqrt(s[4] / n_valid) if n_valid > 0 else None, n_valid=n_valid)
    return out


# ======================================================================================================================
# the NeRF MLP query as a differentiable operation  [f9]
# ======================================================================================================================
NERF_QUERY_DEFAULT_CHUNK = 1 << 16     # points per launch group: 720 MiB of backward scratch (11520 bytes per point)
NERF_QUERY_PARAMS = tuple([f"pts_linears.{i}.weight" for i in range(8)]
                          + ["feature_linear.weight", "alpha_linear.weight", "views_linears.0.weight", "rgb_linear.weight"]
                          + [f"pts_linears.{i}.bias" for i in range(8)]
                          + ["feature_linear.bias", "alpha_linear.bias", "views_linears.0.bias", "rgb_linear.bias"])


class NerfQueryFn(torch.autograd.Function):
    """run_network (run_nerf.py:50-65) and its backward on the GPU (csrc/nerfquery.hip).  forward(pts [R, S, 3], viewdirs [R, 3], cam
    [input_ch_cam], cfg, bounds, chunk, dtype, backward_dtype, *params): params are the 24 tensors in NERF_QUERY_PARAMS order -> raw
    [R, S, 4].  Nothing but the inputs is kept for the backward: it runs the forward again, chunk by chunk, into the scratch, in the
    arithmetic ``dtype`` of the forward; its own products run in ``backward_dtype``."""

    @staticmethod
    def forward(ctx, pts, viewdirs, cam, cfg, bounds, chunk, dtype, backward_dtype, *params):
        c = nerf_grid_config(cfg)
        weights = nerf_grid_pack(dict(zip(NERF_QUERY_PARAMS, params)), cfg, dtype)
        R, S = int(pts.shape[0]), int(pts.shape[1])
        size = (R, S, chunk, c["multires"], c["multires_views"], c["input_ch_cam"])
        nbytes = lib.query("nerfquery_work_bytes", 0, *size)
        if nbytes < 0:
            raise lib.NrpnError(f"nerf_query: {R} rays of {S} points in chunks of {chunk} are outside the supported range")
        work = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
        raw = torch.empty((R, S, 4), dtype=torch.float32, device=pts.device)
        name, head = weights.entry("nerfquery_forward", _p(pts), _p(viewdirs), R, S, *bounds, c["multires"], c["multires_views"],
                                   c["input_ch_cam"], _p(weights.packed))
        call(name, *head, _p(weights.w_view), _p(weights.b_views), _p(cam) if c["input_ch_cam"] else None, chunk, _p(work), nbytes,
             _p(raw), _s())
        ctx.save_for_backward(pts, viewdirs, cam)
        ctx.weights, ctx.size, ctx.bounds, ctx.shapes = weights, size, bounds, [tuple(p.shape) for p in params]
        ctx.backward_dtype = backward_dtype
        return raw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, draw):
        pts, viewdirs, cam = ctx.saved_tensors
        weights, size = ctx.weights, ctx.size
        R, S, chunk, multires, multires_views, cam_ch = size
        dev = pts.device
        if ctx.backward_dtype == "bf16x3":      # the planes of the transposes take packed_t's place
            packed_t = torch.empty(lib.query("nerfquery_work_bytes", 5, *size) // 2, dtype=torch.bfloat16, device=dev)
            call("nerfquery_pack_t_bf16x3", _p(weights.raw), 3 + 6 * multires, _p(packed_t), _s())
        else:
            packed_t = torch.empty(lib.query("nerfquery_work_bytes", 2, *size) // 4, dtype=torch.float32, device=dev)
            call("nerfquery_pack_t", _p(weights.raw), 3 + 6 * multires, _p(packed_t), _s())
        nbytes = lib.query("nerfquery_work_bytes", 1, *size)
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        grads = torch.empty(lib.query("nerfquery_work_bytes", 3, *size), dtype=torch.float32, device=dev)
        draw = draw.to(torch.float32).contiguous()
        name, head = weights.entry("nerfquery_backward", _p(pts), _p(viewdirs), R, S, *ctx.bounds, multires, multires_views, cam_ch,
                                   _p(weights.packed))
        if ctx.backward_dtype == "bf16x3":
            name += "_split"
        call(name, *head, _p(packed_t), _p(weights.w_view), _p(weights.b_views), _p(cam) if cam_ch else None, _p(draw), chunk, _p(work), nbytes,
             _p(grads), _s())
        out, at = [], 0
        for shape in ctx.shapes:
            n = math.prod(shape)
            out.append(grads[at:at + n].view(shape))
            at += n
        dcam = grads[at:at + cam_ch]
        return (None, None, dcam, None, None, None, None, None, *out)


def nerf_query(params, cfg, pts, viewdirs, embedded_cam=None, bb_center=(0., 0., 0.), bb_scale=1., chunk=None, dtype="fp32",
               backward_dtype="fp32"):
    """network_query_fn(pts, viewdirs, embedded_cam, network_fn) of the reference (run_network, run_nerf.py:50-65) for the NeRF MLP of
    DESIGN.md 3.16, differentiable with respect to the network's 24 parameter tensors and to embedded_cam.

    params: a mapping from the checkpoint's key names (with or without ``module.``) to float32 device tensors; cfg: the run's
    args.json, through nerf_grid_config.  pts [R, S, 3] float32 world points; viewdirs [R, 3] float32, used as given (render has
    normalised them; nothing is normalised here); embedded_cam [input_ch_cam] (default zeros); bb_center [3], bb_scale: the scene
    normalisation.  Returns raw [R, S, 4] float32 on the device: rgb before the sigmoid, sigma before the relu.  pts or viewdirs that
    require grad raise NotImplementedError (no entry point of the reference differentiates them).

    The view branch and the rgb head are nerf_render's own code (csrc/nerf_mlp.cuh), so raw is nerf_render's first-pass raw bit for
    bit when pts and viewdirs are formed in float32 as it forms them from a ray (o, d) and a sample z: pts = o + d * z with the
    product and the sum rounded one after the other, and viewdirs = d / n with n = sqrt((d0 * d0 + d1 * d1) + d2 * d2), every
    operation rounded on its own (unit_dir) -- the products summed left to right, then one square root and three divisions.

    chunk (points, default 2^16, rounded up to tiles of 64) bounds the scratch: the forward keeps 512 bytes per point of a chunk and
    nothing for the backward, which re-runs the forward chunk by chunk and keeps 11264 + 4 * ceil64(views_ch + input_ch_cam) bytes
    per point (11520 for the default options), plus 512 + 4 * ceil64(views_ch + input_ch_cam) bytes per ray, 16 MiB of slice partials
    and the float64 gradient (lib.query("nerfquery_work_bytes", ...) has the figures).  raw does not depend on chunk, bit for bit.
    The gradients are sums over points: for a given chunk and given inputs they are bit-equal from call to call (no atomics,
    fixed-order sums); for different chunks they differ in rounding only.

    dtype "bf16x3": the trunk's matrix products, in the forward and in the backward's re-run of it, use the split arithmetic of
    DESIGN.md 3.23; the backward's own products stay exact fp32 on the activations that forward produced -- unless backward_dtype is
    "bf16x3" too (accepted with dtype "bf16x3" only; ValueError otherwise): then the dgrads and the weight gradients of the trunk's ten
    matrices use the same split arithmetic.  raw, the gradients of rgb_linear, alpha_linear and views_linears.0.bias
    and embedded_cam's do not depend on backward_dtype, bit for bit."""
    nerf_check_dtype(dtype)
    nerf_check_backward_dtype(dtype, backward_dtype)
    c = nerf_grid_config(cfg)
    if not torch.cuda.is_available():
        raise lib.NrpnError("nerf_query needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, x in (("pts", pts), ("viewdirs", viewdirs)):
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise NotImplementedError(f"nerf_query: {name} requires grad; the query is differentiable in the parameters and embedded_cam only")
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in params.items()}
    for k in NERF_QUERY_PARAMS:
        if k not in sd:
            raise lib.NrpnError(f"nerf_query: the parameters have no {k}")
        if not isinstance(sd[k], torch.Tensor) or sd[k].dtype != torch.float32 or not sd[k].is_cuda:
            raise lib.NrpnError(f"nerf_query: {k} must be a float32 device tensor")
    pts = torch.as_tensor(pts, dtype=torch.float32).to(dev).contiguous()
    viewdirs = torch.as_tensor(viewdirs, dtype=torch.float32).to(dev).contiguous()
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.shape[0] < 1 or pts.shape[1] < 1:
        raise lib.NrpnError(f"nerf_query expects pts [R, S, 3], got {tuple(pts.shape)}")
    if tuple(viewdirs.shape) != (pts.shape[0], 3):
        raise lib.NrpnError(f"nerf_query expects viewdirs [{pts.shape[0]}, 3], got {tuple(viewdirs.shape)}")
    cam_ch = c["input_ch_cam"]
    if embedded_cam is None:
        cam = torch.zeros(cam_ch, dtype=torch.float32, device=dev)
    else:
        cam = embedded_cam if isinstance(embedded_cam, torch.Tensor) else torch.as_tensor(embedded_cam, dtype=torch.float32)
        cam = cam.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if cam.numel() != cam_ch:
        raise lib.NrpnError(f"nerf_query: embedded_cam has {cam.numel()} values, input_ch_cam is {cam_ch}")
    chunk = NERF_QUERY_DEFAULT_CHUNK if chunk is None else int(chunk)
    if chunk < 1:
        raise lib.NrpnError(f"nerf_query: chunk {chunk}")
    return NerfQueryFn.apply(pts, viewdirs, cam, cfg, _nerf_bounds(bb_center, bb_scale), chunk, dtype, backward_dtype,
                             *(sd[k] for k in NERF_QUERY_PARAMS))


# ======================================================================================================================
# the ray stage of NeRF training as differentiable operations  [f10]
# ======================================================================================================================
class NerfCompositeFn(torch.autograd.Function):
    """forward_with_additonal_samples' merge (run_nerf.py:504-512) and raw2outputs (:437-469) with their backward on the GPU
    (csrc/nerfcomposite.hip).  Nothing but the inputs is kept for the backward: it walks every ray again."""

    @staticmethod
    def forward(ctx, raw1, raw2, z1, z2, rays_d, noise1, noise2):
        R, S1 = int(raw1.shape[0]), int(raw1.shape[1])
        S2 = 0 if raw2 is None else int(raw2.shape[1])
        dev = raw1.device

        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)
        rgb, depth, acc, disp, weights, z_vals = new(R, 3), new(R), new(R), new(R), new(R, S1 + S2), new(R, S1 + S2)
        ctx.lists = (_p(raw1), _p(z1), 0 if z1.dim() == 1 else S1, S1, _p(raw2) if S2 else None, _p(z2) if S2 else None, S2,
                     None if noise1 is None else _p(noise1), None if noise2 is None or not S2 else _p(noise2), _p(rays_d), R)
        call("nerfcomposite_forward", *ctx.lists, _p(rgb), _p(depth), _p(acc), _p(disp), _p(weights), _p(z_vals), _s())
        ctx.keep = (raw1, raw2, z1, z2, rays_d, noise1, noise2)       # the pointers of ctx.lists stay valid with them
        ctx.set_materialize_grads(False)      # an output nobody differentiates sends None: a null cotangent
        ctx.mark_non_differentiable(disp, z_vals)
        return rgb, disp, acc, weights, depth, z_vals

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth, g_z):
        raw1, raw2 = ctx.keep[:2]
        cot = [None if g is None else g.to(torch.float32).contiguous() for g in (g_rgb, g_depth, g_acc, g_w)]
        draw1 = torch.empty_like(raw1)
        draw2 = None if raw2 is None else torch.empty_like(raw2)
        call("nerfcomposite_backward", *ctx.lists, *(None if g is None else _p(g) for g in cot), _p(draw1),
             None if draw2 is None else _p(draw2), _s())
        return draw1, draw2, None, None, None, None, None


def _f32_device(who, name, x, dev, shape):
    """x as a contiguous float32 tensor on dev (a tensor that requires grad stays in the graph); shape: its expected shape."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=torch.float32)
    t = t.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise lib.NrpnError(f"{who} expects {name} {list(shape)}, got {list(t.shape)}")
    return t


def nerf_composite(raw1, z1, rays_d, raw2=None, z2=None, noise=None, check=False):
    """raw2outputs (run_nerf.py:437-469) on the merged samples of forward_with_additonal_samples (:504-512), differentiable with
    respect to raw1 and raw2.

    raw1 [R, S1, 4] float32 at z1 [S1] (every ray's) or [R, S1]; raw2 [R, S2, 4] at z2 [R, S2], both or neither; rays_d [R, 3].  Each
    list is non-decreasing along a ray; the lists are merged, list 1 first on a tie (where the lists share no value this is the
    reference's sort of the concatenation).  check=True verifies the order and raises NrpnError on an unsorted list; it
    synchronises, so it is off by default.  noise [R, S1 + S2]: added to sigma before the relu (raw_noise_std's, :426), columns
    [:S1] for list 1 and [S1:] for list 2 in each list's own order.

    Returns (rgb_map [R, 3], disp_map [R], acc_map [R], weights [R, S1 + S2], depth_map [R], z_vals [R, S1 + S2]): raw2outputs'
    tuple with the merged z_vals appended, float32 on the device.  disp_map and z_vals are not differentiable, and z1, z2, rays_d
    or noise that require grad raise NotImplementedError (no entry point of the reference differentiates them).  Without noise the
    outputs are nerf_render's for the same raw, bit for bit.  Two calls are bit-equal, forward and backward."""
    who = "nerf_composite"
    if not torch.cuda.is_available():
        raise lib.NrpnError(f"{who} needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, x in (("z1", z1), ("z2", z2), ("rays_d", rays_d), ("noise", noise)):
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise NotImplementedError(f"{who}: {name} requires grad; the composite is differentiable in raw1 and raw2 only")
    if (raw2 is None) != (z2 is None):
        raise lib.NrpnError(f"{who}: raw2 and z2 go together")
    if not isinstance(raw1, torch.Tensor) or raw1.dim() != 3 or raw1.shape[2] != 4 or raw1.shape[0] < 1 or raw1.shape[1] < 1:
        raise lib.NrpnError(f"{who} expects raw1 [R, S1, 4], got {tuple(getattr(raw1, 'shape', ()))}")
    R, S1 = int(raw1.shape[0]), int(raw1.shape[1])
    raw1 = _f32_device(who, "raw1", raw1, dev, (R, S1, 4))
    z1 = torch.as_tensor(z1, dtype=torch.float32)
    z1 = _f32_device(who, "z1", z1, dev, (S1,) if z1.dim() == 1 else (R, S1))
    rays_d = _f32_device(who, "rays_d", rays_d, dev, (R, 3))
    S2 = 0
    if raw2 is not None:
        if not isinstance(raw2, torch.Tensor) or raw2.dim() != 3 or raw2.shape[1] < 1:
            raise lib.NrpnError(f"{who} expects raw2 [R, S2, 4], got {tuple(getattr(raw2, 'shape', ()))}")
        S2 = int(raw2.shape[1])
        raw2 = _f32_device(who, "raw2", raw2, dev, (R, S2, 4))
        z2 = _f32_device(who, "z2", z2, dev, (R, S2))
    if lib.query("nerfcomposite_work_bytes", R, S1, S2) < 0:
        raise lib.NrpnError(f"{who}: {R} rays with {S1} + {S2} samples are outside the supported range")
    noise1 = noise2 = None
    if noise is not None:
        noise = _f32_device(who, "noise", noise, dev, (R, S1 + S2))
        noise1, noise2 = noise[:, :S1].contiguous(), noise[:, S1:].contiguous()
    if check:
        for name, z in (("z1", z1), ("z2", z2)):
            if z is not None and z.shape[-1] > 1 and not bool((z[..., 1:] >= z[..., :-1]).all()):
                raise lib.NrpnError(f"{who}: {name} is not non-decreasing along every ray")
    return NerfCompositeFn.apply(raw1, raw2, z1, z2, rays_d, noise1, noise2)


class NerfRayLossesFn(torch.autograd.Function):
    """img2mse (run_nerf.py:837) and compute_depth_loss (:841) with their backward on the GPU (csrc/nerfcomposite.hip)."""

    @staticmethod
    def forward(ctx, rgb_map, depth_map, weights, target_s, z_vals, target_d, target_vd):
        R = int(rgb_map.shape[0])
        S = 1 if target_d is None else int(weights.shape[1])
        dev = rgb_map.device
        nbytes = lib.query("nerfcomposite_work_bytes", R, S - S // 2, S // 2)      # S = S1 + S2 of a composite: two lists of up to 65536
        if nbytes < 0:
            raise lib.NrpnError(f"nerf_ray_losses: {R} rays with {S} samples are outside the supported range")
        work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        if target_d is None:
            ctx.args = (_p(rgb_map), _p(target_s), None, None, None, None, None, R, S)
        else:
            ctx.args = (_p(rgb_map), _p(target_s), _p(depth_map), _p(z_vals), _p(weights), _p(target_d), _p(target_vd), R, S)
        call("nerfraylosses_forward", *ctx.args, _p(work), nbytes, _p(losses), _s())
        ctx.keep = (rgb_map, target_s, depth_map, z_vals, weights, target_d, target_vd)      # the pointers of ctx.args stay valid with them
        ctx.set_materialize_grads(False)
        return losses[0], losses[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_img, g_depth_loss):
        rgb_map, _, depth_map, _, weights, target_d, _ = ctx.keep
        zero = torch.zeros((), dtype=torch.float32, device=rgb_map.device)
        g = torch.stack([zero if x is None else x.to(torch.float32).reshape(()) for x in (g_img, g_depth_loss)])
        g_rgb = torch.empty_like(rgb_map)
        if target_d is None:
            call("nerfraylosses_backward", *ctx.args, _p(g), _p(g_rgb), None, None, _s())
            return g_rgb, None, None, None, None, None, None
        g_depth, g_w = torch.empty_like(depth_map), torch.empty_like(weights)
        call("nerfraylosses_backward", *ctx.args, _p(g), _p(g_rgb), _p(g_depth), _p(g_w), _s())
        return g_rgb, g_depth, g_w, None, None, None, None


def nerf_ray_losses(rgb_map, target_s, depth_map=None, z_vals=None, weights=None, target_d=None, target_vd=None):
    """The losses of a training step (run_nerf.py:837-842) on the GPU, differentiable with respect to rgb_map, depth_map and weights
     -> (img_loss, depth_loss), float32 scalars on the device.

    img_loss = mean((rgb_map - target_s)^2) over the 3 R values (img2mse).  depth_loss = compute_depth_loss(depth_map, z_vals,
    weights, target_d, target_vd): target_d [R, 2] holds the target depth and its standard deviation, target_vd [R] (bool) the rays
    that have one; over those rays with |m - t| - s > 0 or s^2 < v, where m = depth_map and v = sum (z - m)^2 w + 1e-5, the Gaussian
    negative log-likelihood (log v_c + (m - t)^2 / v_c) / 2 with v_c = max(v, 1e-3), summed and divided by R.  With no valid or no
    applied ray it is exactly 0 and so is every gradient.  target_d=None gives img_loss alone (depth_loss 0, detached from the depth
    inputs).  The caller applies depth_loss_weight (:842).  z_vals, the targets and target_vd are not differentiated."""
    who = "nerf_ray_losses"
    if not torch.cuda.is_available():
        raise lib.NrpnError(f"{who} needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    for name, x in (("target_s", target_s), ("z_vals", z_vals), ("target_d", target_d)):
        if isinstance(x, torch.Tensor) and x.requires_grad:
            raise NotImplementedError(f"{who}: {name} requires grad; the losses are differentiable in rgb_map, depth_map and weights only")
    if not isinstance(rgb_map, torch.Tensor) or rgb_map.dim() != 2 or rgb_map.shape[1] != 3 or rgb_map.shape[0] < 1:
        raise lib.NrpnError(f"{who} expects rgb_map [R, 3], got {tuple(getattr(rgb_map, 'shape', ()))}")
    R = int(rgb_map.shape[0])
    rgb_map = _f32_device(who, "rgb_map", rgb_map, dev, (R, 3))
    target_s = _f32_device(who, "target_s", target_s, dev, (R, 3))
    if target_d is None:
        return NerfRayLossesFn.apply(rgb_map, None, None, target_s, None, None, None)
    if depth_map is None or z_vals is None or weights is None or target_vd is None:
        raise lib.NrpnError(f"{who}: target_d goes with depth_map, z_vals, weights and target_vd")
    if not isinstance(weights, torch.Tensor) or weights.dim() != 2 or weights.shape[0] != R or weights.shape[1] < 1:
        raise lib.NrpnError(f"{who} expects weights [{R}, S], got {tuple(getattr(weights, 'shape', ()))}")
    S = int(weights.shape[1])
    weights = _f32_device(who, "weights", weights, dev, (R, S))
    depth_map = _f32_device(who, "depth_map", depth_map, dev, (R,))
    z_vals = _f32_device(who, "z_vals", z_vals, dev, (R, S))
    target_d = _f32_device(who, "target_d", target_d, dev, (R, 2))
    target_vd = torch.as_tensor(target_vd).to(dev)
    if tuple(target_vd.shape) != (R,):
        raise lib.NrpnError(f"{who} expects target_vd [{R}], got {list(target_vd.shape)}")
    target_vd = (target_vd != 0).to(torch.uint8).contiguous()
    return NerfRayLossesFn.apply(rgb_map, depth_map, weights, target_s, z_vals, target_d, target_vd)


# ======================================================================================================================
# the front end of a NeRF training step (nerf_train.py)  [f11]
# ======================================================================================================================
def nerf_train_batch(intrinsic, c2w, H, W, pix, image, depth=None, valid=None, z=None, t_rand=None, check=False):
    """get_ray_batch_from_one_image (run_nerf.py:650-670) after the pixel draw, in one launch.

    intrinsic = (fx, fy, cx, cy) and c2w [>=3, 4] as nerf_render takes them; pix [R] integer row-major pixel indices v * W + u, in any
    order, repeats allowed; image [H, W, 3]; depth [H, W, 2] (depth, std) with valid [H, W], both or neither; z [S], the base sample
    list, with t_rand [R, S] in [0, 1), both or neither.  check=True verifies 0 <= pix < H W and raises NrpnError; it synchronises, so
    it is off by default and an index outside the image is clamped into it.

    Returns a dict of device tensors: rays [R, 6] (o, d; nerf_render's rays of those pixels, bit for bit), viewdirs [R, 3], target_s
    [R, 3]; with depth: target_d [R, 2], target_vd [R] (bool), depth_range [R, 3] (precompute_depth_sampling :159-162); with t_rand:
    z1 [R, S] (perturb_z_vals :480-495 of z, bit-equal to it for the same t_rand)."""
    who = "nerf_train_batch"
    if not torch.cuda.is_available():
        raise lib.NrpnError(f"{who} needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise lib.NrpnError(f"{who}: image {H} x {W}")
    pose = torch.as_tensor(c2w, dtype=torch.float32)
    if pose.dim() != 2 or pose.shape[0] < 3 or pose.shape[1] != 4:
        raise lib.NrpnError(f"{who} expects c2w [>=3, 4], got {tuple(pose.shape)}")
    intr = torch.as_tensor(intrinsic, dtype=torch.float32)
    if intr.numel() != 4:
        raise lib.NrpnError(f"{who} expects intrinsic (fx, fy, cx, cy), got {tuple(intr.shape)}")
    camera = torch.cat([intr.reshape(4).to(dev), pose[:3].reshape(12).to(dev)]).contiguous()
    pix = torch.as_tensor(pix)
    if pix.dim() != 1 or pix.shape[0] < 1 or pix.dtype.is_floating_point or pix.dtype == torch.bool:
        raise lib.NrpnError(f"{who} expects pix [R] of integers, got {tuple(pix.shape)} {pix.dtype}")
    pix = pix.to(device=dev, dtype=torch.int32).contiguous()
    R = int(pix.shape[0])
    if check and not bool(((pix >= 0) & (pix < H * W)).all()):
        raise lib.NrpnError(f"{who}: pix outside [0, {H * W})")
    image = _f32_device(who, "image", image, dev, (H, W, 3))
    if (depth is None) != (valid is None):
        raise lib.NrpnError(f"{who}: depth and valid go together")
    if (z is None) != (t_rand is None):
        raise lib.NrpnError(f"{who}: z and t_rand go together")
    S = 0
    if z is not None:
        z = torch.as_tensor(z, dtype=torch.float32)
        if z.dim() != 1 or z.shape[0] < 1:
            raise lib.NrpnError(f"{who} expects z [S], got {tuple(z.shape)}")
        S = int(z.shape[0])
        z = _f32_device(who, "z", z, dev, (S,))
        t_rand = _f32_device(who, "t_rand", t_rand, dev, (R, S))

    def new(*shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=dev)
    out = {"rays": new(R, 6), "viewdirs": new(R, 3), "target_s": new(R, 3)}
    vd = None
    if depth is not None:
        depth = _f32_device(who, "depth", depth, dev, (H, W, 2))
        valid = torch.as_tensor(valid).to(dev)
        if tuple(valid.shape) != (H, W):
            raise lib.NrpnError(f"{who} expects valid [{H}, {W}], got {list(valid.shape)}")
        valid = (valid != 0).to(torch.uint8).contiguous()
        out["target_d"], out["depth_range"], vd = new(R, 2), new(R, 3), new(R, dtype=torch.uint8)
    if S:
        out["z1"] = new(R, S)

    def opt(t):
        return None if t is None else _p(t)
    call("nerftrain_batch", _p(camera), H, W, _p(pix), R, _p(image), opt(depth), opt(valid), opt(z), opt(t_rand), S, _p(out["rays"]),
         _p(out["viewdirs"]), _p(out["target_s"]), opt(out.get("target_d")), opt(vd), opt(out.get("depth_range")), opt(out.get("z1")),
         _s())
    if vd is not None:
        out["target_vd"] = vd.view(torch.bool)
    return out


def nerf_train_samples(raw1, z1, rays, near, far, lower_bound, depth_range=None, u=None):
    """The second sample list of render_rays at train time (run_nerf.py:588-592) in one launch, with no host decision (DESIGN.md
    3.22).

    raw1 [R, S, 4] (detached: nothing here is differentiated) on the first list z1 [S] (every ray's) or [R, S]; rays [R, 6].  A ray
    with depth_range[r, 0] >= near (depth_range [R, 3] of nerf_train_batch, or None) is sampled within depth_range[r, 1:]
    (sample_3sigma :471-478); every other ray around the depth its first list predicts, with the std clamped below at lower_bound
    (compute_samples_around_depth :497-502).  u [R, S]: the uniforms of sample_pdf, in any order; None selects the deterministic
    u = linspace(0, 1, S) and then, with depth_range None and a shared z1, the result is nerf_render_samples', bit for bit.

    Returns z2 [R, S] float32 in u's order -- not sorted: the inverse cdf is monotone in exact arithmetic only."""
    who = "nerf_train_samples"
    if not torch.cuda.is_available():
        raise lib.NrpnError(f"{who} needs a gfx950 device (the product path has no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(raw1, torch.Tensor) or raw1.dim() != 3 or raw1.shape[2] != 4 or raw1.shape[0] < 1:
        raise lib.NrpnError(f"{who} expects raw1 [R, S, 4], got {tuple(getattr(raw1, 'shape', ()))}")
    if raw1.requires_grad:
        raise NotImplementedError(f"{who}: raw1 requires grad; the reference samples on raw.detach() (:590)")
    R, S = int(raw1.shape[0]), int(raw1.shape[1])
    nbytes = lib.query("nerftrain_work_bytes", R, S)
    if nbytes < 0:
        raise lib.NrpnError(f"{who}: {R} rays with {S} samples are outside the supported range (S >= 2)")
    raw1 = _f32_device(who, "raw1", raw1, dev, (R, S, 4))
    z1 = torch.as_tensor(z1, dtype=torch.float32)
    z1 = _f32_device(who, "z1", z1, dev, (S,) if z1.dim() == 1 else (R, S))
    rays = _f32_device(who, "rays", rays, dev, (R, 6))
    if depth_range is not None:
        depth_range = _f32_device(who, "depth_range", depth_range, dev, (R, 3))
    if u is not None:
        u = _f32_device(who, "u", u, dev, (R, S))
    near, far, lower_bound = float(near), float(far), float(lower_bound)
    if not near <= far:
        raise lib.NrpnError(f"{who}: near {near} above far {far}")
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    z2 = torch.empty((R, S), dtype=torch.float32, device=dev)
    call("nerftrain_samples", _p(raw1), _p(z1), 0 if z1.dim() == 1 else S, _p(rays), None if depth_range is None else _p(depth_range),
         None if u is None else _p(u), S, lower_bound, near, far, R, _p(work), nbytes, _p(z2), _s())
    return z2
