"""float64 reference of the shifted-window attention *core* (what ops.WindowAttnFn computes between the qkv and proj Linears), padding
included, with the magnitudes its per-element error bounds are made of; a CPU emulation of the bf16 MFMA kernels' rounding points; the
input families and the checker shared by tests/test_attention_bounds_host.py (no GPU) and tests/test_gpu_attention.py.

Bounds (u = 2^-8, bf16 round to nearest; s = 32^-0.5; P = softmax probabilities, dP = dO V^T, dS = P (dP - rowsum(P dP)),
S^ = P (|dP| + rowsum(P |dP|)) >= |dS| before cancellation).  The fp32 arithmetic gets a per-query-row factor
    phi_i = 2^-24 (64 + 8 Lambda_i),   Lambda_i = max_j (s sum_d |q_id k_jd| + |bias_ij|):
an absolute error of a logit is a relative error of its probability, a 32-term fp32 dot product of magnitude Lambda carries up to
32 * 2^-24 * Lambda of it (8: a quarter of the worst case), and 64 stands for the two 64-term sums (denominator, P V).

    output      fp32 term T32 (every kernel)          bf16 VALU adds   bf16 MFMA adds (P / dS rounded as MFMA operands, bf16 store)
    out[i]      phi_i P|V|                            u |ref|          u (|ref| + P|V|)
    dq[i]       phi_i s S^|K|                         u |ref|          u (|ref| + s |dS||K|)
    dk[j]       s (phi S^)^T |Q|                      u |ref|          u (|ref| + s |dS|^T |Q|)
    dv[j]       (phi P)^T |dO|                        u |ref|          u (|ref| + P^T |dO|)
    dtable[k]   sum of phi_i S^ on the entry          -                -   (summed from fp32 dS)
    dbias_pad   the dk / dv terms of padded keys      -                u * (the |dS|^T|Q|, P^T|dO| terms of padded keys)

The assertion is |err| <= k * T32 + (the u terms), k = max(1, min(2, 4 r)), r = max |err| / T32 of a torch fp32 CPU evaluation of the same
case: the kernels sum in another order than torch, so torch's own distance to T32 sets the allowance, capped at 2 so that it cannot hide
a real error.  The u terms are worst-case rounding bounds and carry no margin.  T32 also holds an absolute underflow floor of the order of
2^-126 (see attn_core_ref): probabilities behind the -100 mask are below the smallest normal fp32 number, and outputs made of nothing else
(a table entry whose only pairs are masked, next to zero padded tokens) have no relative accuracy in fp32 - torch's own fp32 evaluation
misses the purely relative bound there by 1e5."""
import types

import torch
import torch.nn.functional as F

WS, WT, HD = 4, 64, 32
U = 2.0 ** -8
SCALE = 32 ** -0.5
ETA, FLUSHES = 2.0 ** -126, 4
KERNELS = ("f32", "bf16_valu", "bf16_mfma")


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def relative_position_index(ws=WS):
    """The reference's define_relative_position_index for a cubic window (oracle.nets.WindowAttention builds the same)."""
    a = torch.arange(ws)
    c = torch.stack(torch.meshgrid(a, a, a, indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (ws - 1)
    return (rel[..., 0] * (2 * ws - 1) ** 2 + rel[..., 1] * (2 * ws - 1) + rel[..., 2]).flatten()


class Frame:
    """Pad-to-window / cyclic shift / window partition of a [B, H, W, D, c] token tensor and their inverses (oracle.nets.window_attention)."""

    def __init__(self, shape, shift):
        self.B, self.H, self.W, self.D = shape
        self.pad = [(-s) % WS for s in shape[1:]]
        self.P = [s + p for s, p in zip(shape[1:], self.pad)]
        self.sh = [0 if WS >= p else int(shift) for p in self.P]          # an axis one window long is not shifted
        self.nW = (self.P[0] // WS) * (self.P[1] // WS) * (self.P[2] // WS)
        self.windows = self.B * self.nW

    def _partition(self, t):
        b, c = t.shape[0], t.shape[-1]
        p = self.P
        t = t.reshape(b, p[0] // WS, WS, p[1] // WS, WS, p[2] // WS, WS, c).permute(0, 1, 3, 5, 2, 4, 6, 7)
        return t.reshape(-1, WT, c)

    def pad_mask(self, dtype):
        m = torch.ones(1, *self.P, 1, dtype=dtype)
        m[:, :self.H, :self.W, :self.D] = 0
        return m

    def to_windows(self, t, fill=None):
        """[B, H, W, D, c] -> [B * nW, 64, c]; padded tokens hold ``fill`` ([c], zeros where None)."""
        pd = self.pad
        t = F.pad(t, (0, 0, 0, pd[2], 0, pd[1], 0, pd[0]))
        if fill is not None and sum(pd):
            t = t + self.pad_mask(t.dtype) * fill
        if sum(self.sh):
            t = torch.roll(t, shifts=(-self.sh[0], -self.sh[1], -self.sh[2]), dims=(1, 2, 3))
        return self._partition(t)

    def from_windows(self, y):
        """[B * nW, 64, c] -> [B, H, W, D, c] (padded tokens dropped)."""
        c, p = y.shape[-1], self.P
        y = y.reshape(self.B, p[0] // WS, p[1] // WS, p[2] // WS, WS, WS, WS, c).permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(self.B, *p, c)
        if sum(self.sh):
            y = torch.roll(y, shifts=tuple(self.sh), dims=(1, 2, 3))
        return y[:, :self.H, :self.W, :self.D]

    def region_mask(self, dtype):
        """[B * nW, 1, 64, 64] of 0 / -100 (None when nothing is shifted)."""
        if not sum(self.sh):
            return None
        sh = self.sh
        region = torch.zeros(self.P, dtype=dtype)
        cnt = 0
        for h in ((0, -WS), (-WS, -sh[0]), (-sh[0], None)):
            for w in ((0, -WS), (-WS, -sh[1]), (-sh[1], None)):
                for d in ((0, -WS), (-WS, -sh[2]), (-sh[2], None)):
                    region[h[0]:h[1], w[0]:w[1], d[0]:d[1]] = cnt
                    cnt += 1
        rr = self._partition(region[None, ..., None])[..., 0]
        mask = rr.unsqueeze(1) - rr.unsqueeze(2)
        mask = torch.where(mask != 0, torch.full_like(mask, -100.0), torch.zeros_like(mask))
        return mask.repeat(self.B, 1, 1)[:, None]


def _heads(t, heads):          # [nWB, 64, heads * 32] -> [nWB, heads, 64, 32]
    return t.reshape(t.shape[0], WT, heads, HD).permute(0, 2, 1, 3)


def _unheads(t):               # [nWB, heads, 64, 32] -> [nWB, 64, heads * 32]
    return t.permute(0, 2, 1, 3).reshape(t.shape[0], WT, -1)


def _split(fr, qkv, qkv_bias, heads):
    c = qkv.shape[-1] // 3
    xw = fr.to_windows(qkv, qkv_bias)
    return [_heads(xw[..., i * c:(i + 1) * c], heads) for i in range(3)]


def _bias(table, index, heads):
    return table[index].view(WT, WT, heads).permute(2, 0, 1).unsqueeze(0)


def _pad_sum(fr, t):
    """Sum of a per-key window tensor [nWB, heads, 64, 32] over the padded keys -> [heads * 32]."""
    pw = fr.to_windows(torch.zeros(fr.B, fr.H, fr.W, fr.D, 1, dtype=t.dtype), torch.ones(1, dtype=t.dtype))      # 1 on padded tokens
    return (t * pw[:, None]).sum(dim=(0, 2)).reshape(-1)


def _scatter_table(index, t):
    """Per-window score-shaped tensor [nWB, heads, 64, 64] summed over the windows and scattered onto the table entries -> [343, heads]."""
    heads = t.shape[1]
    return torch.zeros((2 * WS - 1) ** 3, heads, dtype=t.dtype).index_add_(0, index, t.sum(0).permute(1, 2, 0).reshape(-1, heads))


def attn_core_explicit(qkv, qkv_bias, table, index, heads, shift, dout, mfma_rounding=False, transpose_bias=False):
    """The same operation with the backward written out, in the dtype of ``qkv`` (float32: the torch fp32 CPU evaluation the allowance k
    is measured on).  ``mfma_rounding`` rounds to bf16 where the MFMA kernels do (P and dS as matrix operands, the stored out / dq / dk /
    dv; the table gradient is summed from the unrounded dS, the padded-token bias gradient from the unrounded accumulators);
    ``transpose_bias`` reads the relative-position bias of (j, i) for the pair (i, j): the bug the bounds have to catch.
    -> out, dqkv, dtable, dbias_pad (None without a bias)."""
    rnd = bf16_round if mfma_rounding else (lambda t: t)
    with torch.no_grad():
        fr = Frame(qkv.shape[:4], shift)
        q, k, v = _split(fr, qkv, qkv_bias, heads)
        do = _heads(fr.to_windows(dout), heads)
        b = _bias(table, index, heads)
        s = (q * SCALE) @ k.transpose(-2, -1) + (b.transpose(-2, -1) if transpose_bias else b)
        mask = fr.region_mask(qkv.dtype)
        if mask is not None:
            s = s + mask
        p = F.softmax(s, dim=-1)
        o = rnd(rnd(p) @ v)
        dp = do @ v.transpose(-2, -1)
        ds = p * (dp - (p * dp).sum(-1, keepdim=True))
        dk_acc = (rnd(ds).transpose(-2, -1) @ q) * SCALE
        dv_acc = rnd(p).transpose(-2, -1) @ do
        dq = rnd((rnd(ds) @ k) * SCALE)
        out = fr.from_windows(_unheads(o))
        dqkv = torch.cat([fr.from_windows(_unheads(t)) for t in (dq, rnd(dk_acc), rnd(dv_acc))], -1)
        dtable = _scatter_table(index, ds)
        dpad = None
        if qkv_bias is not None:
            dpad = torch.cat([torch.zeros(heads * HD, dtype=qkv.dtype), _pad_sum(fr, dk_acc), _pad_sum(fr, dv_acc)])
        return out.contiguous(), dqkv.contiguous(), dtable, dpad


def attn_core_ref(qkv, qkv_bias, table, index, heads, shift, dout=None):
    """float64 attention core on [B, X, Y, Z, 3C] with autograd: pad each axis to a multiple of 4 filling with ``qkv_bias`` (what a zero
    token becomes behind the qkv Linear; zeros where None), roll / partition / q 32^-0.5 k^T + table[index] / -100 region mask / softmax /
    @ v / inverse, crop.  Returns a namespace: ``out``; ``s`` (the score tensor after the bias add, a retained autograd node); ``frame``;
    and with ``dout`` the gradients ``dqkv``, ``dtable``, ``dbias_pad`` (autograd through the fill; None without a bias) plus
    ``t32`` / ``mfma`` / ``terms``: per output name the fp32 term of the bound, the magnitude the MFMA kernels' operand rounding acts on, and
    sum |dS| per table entry (all float64, from the same tensors)."""
    assert qkv.dtype == torch.float64 and table.dtype == torch.float64
    fr = Frame(qkv.shape[:4], shift)
    x = qkv.detach().clone().requires_grad_()
    tb = table.detach().clone().requires_grad_()
    qb = qkv_bias.detach().clone().requires_grad_() if qkv_bias is not None else None
    with torch.enable_grad():
        q, k, v = _split(fr, x, qb, heads)
        s = (q * SCALE) @ k.transpose(-2, -1) + _bias(tb, index, heads)
        s.retain_grad()
        mask = fr.region_mask(x.dtype)
        a = s if mask is None else s + mask
        o = F.softmax(a, dim=-1) @ v
        out = fr.from_windows(_unheads(o)).contiguous()
    r = types.SimpleNamespace(out=out.detach(), s=s, frame=fr)
    if dout is None:
        return r
    out.backward(dout)
    r.dqkv, r.dtable = x.grad, tb.grad
    r.dbias_pad = None if qb is None else (qb.grad if qb.grad is not None else torch.zeros_like(qb))
    with torch.no_grad():
        q, k, v, a = q.detach(), k.detach(), v.detach(), a.detach()
        do = _heads(fr.to_windows(dout), heads)
        p = F.softmax(a, dim=-1)
        lam = (SCALE * (q.abs() @ k.abs().transpose(-2, -1)) + _bias(tb.detach(), index, heads).abs()).amax(-1, keepdim=True)
        phi = 2.0 ** -24 * (64.0 + 8.0 * lam)                                   # [nWB, heads, 64, 1], per query row
        dp = do @ v.transpose(-2, -1)
        ds = p * (dp - (p * dp).sum(-1, keepdim=True))
        sh = p * (dp.abs() + (p * dp.abs()).sum(-1, keepdim=True))              # S^
        a_o = p @ v.abs()
        t_dq = phi * SCALE * (sh @ k.abs())
        t_dk = SCALE * ((phi * sh).transpose(-2, -1) @ q.abs())
        t_dv = (phi * p).transpose(-2, -1) @ do.abs()
        m_dq = SCALE * (ds.abs() @ k.abs())
        m_dk = SCALE * (ds.abs().transpose(-2, -1) @ q.abs())
        m_dv = p.transpose(-2, -1) @ do.abs()
        # underflow floor: a probability behind the -100 mask is ~ e^-100 = 4e-44, below the smallest normal fp32 / bf16 number ETA = 2^-126,
        # where a flush to zero (or a denormal's few bits) is an ABSOLUTE error of up to ETA that no relative factor covers.  Up to FLUSHES
        # such points lie on a path (expf, P = e / den, the bf16 operand, the dS product), each entering the sums like an error ETA of P
        # or dS: s1 is S^ with those errors in place of P.  ~1e-36 in the units of the data: it cannot hide anything.
        s1 = ETA * (1.0 + dp.abs() + (p * dp.abs()).sum(-1, keepdim=True) + p * dp.abs().sum(-1, keepdim=True))
        f_o = FLUSHES * ETA * (1.0 + v.abs().sum(-2, keepdim=True)).expand_as(a_o)
        f_dq = FLUSHES * (ETA + SCALE * (s1 @ k.abs()))
        f_dk = FLUSHES * (ETA + SCALE * (s1.transpose(-2, -1) @ q.abs()))
        f_dv = FLUSHES * ETA * (1.0 + do.abs().sum(-2, keepdim=True)).expand_as(t_dv)
        tok = lambda t: fr.from_windows(_unheads(t)).contiguous()               # noqa: E731
        zero = torch.zeros(heads * HD, dtype=torch.float64)
        r.t32 = {"out": tok(phi * a_o + f_o), "dqkv": torch.cat([tok(t_dq + f_dq), tok(t_dk + f_dk), tok(t_dv + f_dv)], -1),
                 "dtable": _scatter_table(index, phi * sh + FLUSHES * s1),
                 "dbias_pad": torch.cat([zero, _pad_sum(fr, t_dk + f_dk), _pad_sum(fr, t_dv + f_dv)])}
        r.mfma = {"out": tok(a_o), "dqkv": torch.cat([tok(m_dq), tok(m_dk), tok(m_dv)], -1), "dtable": None,
                  "dbias_pad": torch.cat([zero, _pad_sum(fr, m_dk), _pad_sum(fr, m_dv)])}
        r.terms = {"dtable": _scatter_table(index, ds.abs())}
        r.ds, r.lam_max = ds, lam.max().item()
    return r


# ======================================================================================================================
# bounds and the checker
# ======================================================================================================================
NAMES = ("out", "dqkv", "dtable", "dbias_pad")


def _ratio(err, tol):
    return torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))


def torch32_ratios(ref, got32):
    """max |err| / T32 per output of a torch fp32 CPU evaluation ``got32`` = (out, dqkv, dtable, dbias_pad)."""
    r = {}
    for name, got in zip(NAMES, got32):
        want = getattr(ref, name)
        if got is None or want is None:
            continue
        r[name] = _ratio((got.double() - want).abs(), ref.t32[name]).max().item()
    return r


def allowance(r_torch):
    return max(1.0, min(2.0, 4.0 * r_torch))


def tolerance(ref, name, kernel, k):
    """Per-element bound of output ``name`` for ``kernel`` in KERNELS (module docstring)."""
    want = getattr(ref, name)
    tol = k * ref.t32[name]
    if kernel == "bf16_valu" and name in ("out", "dqkv"):
        tol = tol + U * want.abs()
    if kernel == "bf16_mfma":
        if name in ("out", "dqkv"):
            tol = tol + U * (want.abs() + ref.mfma[name])
        elif name == "dbias_pad":
            tol = tol + U * ref.mfma[name]
    return tol


def ratio_map(ref, name, kernel, got, k):
    """|err| / bound per element (inf where the bound is zero and the error is not)."""
    want = getattr(ref, name)
    got = got.detach().double().cpu().reshape(want.shape)
    return _ratio((got - want).abs(), tolerance(ref, name, kernel, k))


def check(ref, name, kernel, got, k, what=""):
    """Every element of ``got`` within its bound; the message says where the worst one is."""
    m = ratio_map(ref, name, kernel, got, k)
    worst = m.max().item()
    print(f"{what} {kernel} {name}: max err/bound = {worst:.3f} (k = {k:.2f})")
    if not worst <= 1.0:
        flat = int(m.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), m.shape))
        raise AssertionError((what, kernel, name, "bad elements", int((m > 1).sum()), "of", m.numel(), "worst ratio", worst, "at", idx,
                              "k", k))
    return worst


# ======================================================================================================================
# input families
# ======================================================================================================================
FAMILIES = ("normal", "peaked", "offset_v", "selector", "uniform")


def make_case(family, shape, heads, seed, with_bias=True, bf16=False):
    """Seeded float32 inputs (qkv, qkv_bias or None, table, dout) of one family on grid ``shape`` = (B, X, Y, Z); with ``bf16`` qkv, dout
    and the bias hold bf16-representable values (the MFMA kernels stage padded tokens as bf16, the VALU kernels keep the fp32 bias: on a
    representable bias both read the same numbers)."""
    g = torch.Generator().manual_seed(seed)
    c = heads * HD
    qkv = torch.randn(*shape, 3 * c, generator=g)
    dout = torch.randn(*shape, c, generator=g)
    table = torch.randn((2 * WS - 1) ** 3, heads, generator=g) * 0.5
    bias = torch.randn(3 * c, generator=g) * 0.5 if with_bias else None
    if family == "peaked":                      # logits ~ 50: max subtraction, near-one-hot rows, dP - rowdot cancellation
        qkv[..., :2 * c] *= 4
        if bias is not None:
            bias[:2 * c] *= 4
    elif family == "offset_v":                  # |V| ~ 50, as after a LayerNorm with a large beta
        qkv[..., 2 * c:] += 50
        if bias is not None:
            bias[2 * c:] += 50
    elif family == "selector":                  # the row attends to one relative offset: fixes the sign convention of the index
        qkv[..., :2 * c] *= 0.05
        if bias is not None:
            bias[:2 * c] *= 0.05
        table = torch.zeros_like(table)
        for h in range(heads):
            for e in torch.randint(0, table.shape[0], (4,), generator=g).tolist():
                table[e, h] = 60.0
    elif family == "uniform":                   # q = 0, table = 0: every row is uniform over its window-and-region set
        qkv[..., :c] = 0
        table = torch.zeros_like(table)
        if bias is not None:
            bias[:c] = 0
        b, x, y, z = shape
        coords = torch.stack(torch.meshgrid(torch.arange(x), torch.arange(y), torch.arange(z), indexing="ij"), -1).float()
        for h in range(heads):
            o = 2 * c + h * HD
            qkv[..., o:o + 3] = coords
            qkv[..., o + 3] = 1.0
            qkv[..., o + 4] = torch.arange(b).float().view(b, 1, 1, 1)
    elif family != "normal":
        raise ValueError(family)
    if bf16:
        qkv, dout = bf16_round(qkv), bf16_round(dout)
        bias = bf16_round(bias) if bias is not None else None
    return qkv, bias, table, dout


def uniform_closed_form(shape, shift):
    """Family 5 without the reference: [B, X, Y, Z, 5] = mean of (x, y, z, 1, b) over the tokens that share the output token's window and
    region in the rolled, zero-padded frame (padded tokens count as zeros: use with qkv_bias None).  Plain index arithmetic, float64."""
    b_, x_, y_, z_ = shape
    p = [(s + WS - 1) // WS * WS for s in (x_, y_, z_)]
    sh = [0 if WS >= q else shift for q in p]
    sums, out = {}, torch.zeros(b_, x_, y_, z_, 5, dtype=torch.float64)

    def key(b, x, y, z):
        r = [(c - s) % q for c, s, q in zip((x, y, z), sh, p)]                      # position in the rolled frame
        reg = tuple(2 if s == 0 else (0 if c < q - WS else (1 if c < q - s else 2)) for c, s, q in zip(r, sh, p))
        return (b, r[0] // WS, r[1] // WS, r[2] // WS) + reg

    for b in range(b_):
        for x in range(p[0]):
            for y in range(p[1]):
                for z in range(p[2]):
                    acc = sums.setdefault(key(b, x, y, z), [torch.zeros(5, dtype=torch.float64), 0])
                    acc[1] += 1
                    if x < x_ and y < y_ and z < z_:
                        acc[0] += torch.tensor([x, y, z, 1.0, b], dtype=torch.float64)
    for b in range(b_):
        for x in range(x_):
            for y in range(y_):
                for z in range(z_):
                    acc = sums[key(b, x, y, z)]
                    out[b, x, y, z] = acc[0] / acc[1]
    return out
