"""GPU tests of the four weight packs of the NeRF MLP (nrpn_nerfgrid_pack, nrpn_nerfgrid_pack_bf16x3, nrpn_nerfquery_pack_t,
nrpn_nerfquery_pack_t_bf16x3; include/nerfrpn.h) against their layouts written out on the host, element for element.

raw holds the tensors in torch's [out][in] layout back to back; every element is its flat index plus one, so a misplaced element
shows.  A matrix B [K][n_out] (k the summed index) is packed as fragments: fp32, the four floats of (k-group kg, column o, half h) at
((kg * n_out + o) * 2 + h) * 4 hold B[8 kg + 4 h + j][o]; bf16x3, the eight bf16 of (k-step ks, o, h) at ((ks * n_out + o) * 2 + h) * 8
of the hi plane hold bfloat16(B[16 ks + 8 h + j][o]), and the lo plane holds bfloat16 of what that rounding left.  The forward's
matrices are B = W^T with the encoding columns zero-padded to 64; the backward's are B = W[:, h columns]."""
import pytest
import torch

from nerf_rpn_amd import lib
from nerf_rpn_amd.ops import _p, _s, call

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, HALF, ENC = 256, 128, 64


def raw_tensors(input_ch):
    """-> raw [n] float32 (flat index + 1), the ten matrices as views of it in raw's order, and the small tensors' slice."""
    shapes = [(W, input_ch)] + [(W, W)] * 4 + [(W, input_ch + W)] + [(W, W)] * 2 + [(W, W), (HALF, W)]
    small = 9 * W + W + 1 + 3 * HALF + 3
    raw = torch.arange(1, sum(a * b for a, b in shapes) + small + 1, dtype=torch.float32)
    mats, at = [], 0
    for a, b in shapes:
        mats.append(raw[at:at + a * b].view(a, b))
        at += a * b
    return raw, mats, raw[at:]


def fragments(b, frag):
    """B [K][n_out] -> its fragments of ``frag`` elements, flat: index (kg, o, h, j) holds B[2 frag kg + frag h + j][o]."""
    k, n_out = b.shape
    return b.reshape(k // (2 * frag), 2, frag, n_out).permute(0, 3, 1, 2).reshape(-1)


def forward_matrices(mats, input_ch):
    """The ten B = W^T of the trunk with the encoding columns of pts_linears.0 and .5 zero-padded to 64 rows."""
    out = []
    for i, w in enumerate(mats):
        if i in (0, 5):
            w = torch.cat([w[:, :input_ch], torch.zeros(w.shape[0], ENC - input_ch), w[:, input_ch:]], 1)
        out.append(w.t().contiguous())
    return out


def transposed_matrices(mats, input_ch):
    """The nine B = W[:, h columns] of the backward's dgrads: pts_linears.1 .. 7, feature_linear, W_f."""
    return [(w[:, input_ch:] if i == 5 else w).contiguous() for i, w in enumerate(mats) if i > 0]


def split_planes(bs):
    """-> (hi, lo) int16 bit patterns of the bf16x3 planes of the matrices bs, back to back."""
    v = torch.cat([fragments(b, 8) for b in bs])
    hi = v.to(torch.bfloat16)
    lo = (v - hi.to(torch.float32)).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


@pytest.fixture(scope="module", params=[3, 57, 64])
def packs(request):
    """input_ch -> (input_ch, matrices, small tensors, the four packed buffers on the host); every buffer is filled beforehand with a
    pattern no pack writes, so an element the pack leaves alone shows."""
    input_ch = request.param
    raw, mats, small = raw_tensors(input_ch)
    d = raw.to(DEV)
    packed = torch.full((lib.query("nerfgrid_work_bytes", 0, 0) // 4,), -7.0, dtype=torch.float32, device=DEV)
    planes = torch.full((lib.query("nerfgrid_work_bytes", 2, 0) // 2,), -1, dtype=torch.int16, device=DEV)
    packed_t = torch.full((lib.query("nerfquery_work_bytes", 2, 1, 1, 1, 0, 0, 0) // 4,), -7.0, dtype=torch.float32, device=DEV)
    planes_t = torch.full((lib.query("nerfquery_work_bytes", 5, 1, 1, 1, 0, 0, 0) // 2,), -1, dtype=torch.int16, device=DEV)
    call("nerfgrid_pack", _p(d), input_ch, _p(packed), _s())
    call("nerfgrid_pack_bf16x3", _p(d), input_ch, _p(planes), _s())
    call("nerfquery_pack_t", _p(d), input_ch, _p(packed_t), _s())
    call("nerfquery_pack_t_bf16x3", _p(d), input_ch, _p(planes_t), _s())
    return input_ch, mats, small, packed.cpu(), planes.cpu(), packed_t.cpu(), planes_t.cpu()


def test_packed_fp32(packs):
    """The ten matrices as fp32 fragments with their zero padding, then the small tensors: nine biases, alpha_linear.weight,
    alpha_linear.bias and three zeros, rgb_linear.weight, rgb_linear.bias and one zero."""
    input_ch, mats, small, packed, _, _, _ = packs
    z = torch.zeros
    s = small
    want = torch.cat([fragments(b, 4) for b in forward_matrices(mats, input_ch)]
                     + [s[:10 * W], s[10 * W:10 * W + 1], z(3), s[10 * W + 1:10 * W + 1 + 3 * HALF], s[10 * W + 1 + 3 * HALF:], z(1)])
    assert packed.shape == want.shape
    assert torch.equal(packed, want)


def test_planes_bf16x3(packs):
    input_ch, mats, _, _, planes, _, _ = packs
    hi, lo = split_planes(forward_matrices(mats, input_ch))
    assert planes.numel() == 2 * hi.numel()
    assert torch.equal(planes[:hi.numel()], hi)
    assert torch.equal(planes[hi.numel():], lo)


def test_packed_transposes_fp32(packs):
    input_ch, mats, _, _, _, packed_t, _ = packs
    want = torch.cat([fragments(b, 4) for b in transposed_matrices(mats, input_ch)])
    assert packed_t.shape == want.shape
    assert torch.equal(packed_t, want)


def test_planes_of_transposes_bf16x3(packs):
    input_ch, mats, _, _, _, _, planes_t = packs
    hi, lo = split_planes(transposed_matrices(mats, input_ch))
    assert planes_t.numel() == 2 * hi.numel()
    assert torch.equal(planes_t[:hi.numel()], hi)
    assert torch.equal(planes_t[hi.numel():], lo)
