"""GPU (-m gpu): the FP8 Q.K path (csrc/qattn.hip).  jenga_quant_fp8_blocks bit for bit against its recipe in torch on the CPU;
jenga_bsattn_fp8_fwd against the semantics of include/jenga_amd.h evaluated in float64 on the dequantised q and k; the front end
(qk_dtype="fp8") against the same steps composed by hand.  H = 2, D = 128, seeded randn.

Worst max |o - ref| measured on an MI355X: see DESIGN.md section 3.9."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

H = 2
BOUND = {torch.bfloat16: 1e-2, torch.float16: 2e-3}     # tests/test_gpu_dense_varlen.py: the same roundings (P and o)
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])


def _quant_cpu(x, offset=None):
    """The recipe of jenga_quant_fp8_blocks: x [B,S,H,128] on the CPU -> (bytes uint8 [B,S,H,128], scale fp32 [B,H,S/128])."""
    B, S, Hh, D = x.shape
    xf = x.float() if offset is None else x.float() - offset[:, None]
    xb = xf.view(B, S // 128, 128, Hh, D)
    s = xb.abs().amax(dim=(2, 4)).clamp(min=1e-30) / 448.0
    x8 = (xb / s[:, :, None, :, None]).to(torch.float8_e4m3fn).view(torch.uint8).view(B, S, Hh, D)
    return x8, s.permute(0, 2, 1).contiguous()


@DTYPES
@pytest.mark.parametrize("with_offset", [False, True], ids=["plain", "offset"])
@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("zero_block", [False, True], ids=["randn", "zeroblock"])
def test_quantiser_is_bit_exact(dtype, with_offset, strided, zero_block):
    from jenga_amd import _capi
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    buf = torch.randn(1, 384, 3, H, 128, generator=gen).to(dtype)
    if zero_block:
        buf[0, 128:256, 0, 1] = 0
    offset = torch.randn(1, H, 128, generator=gen) if with_offset else None
    xd = buf.to(dev)[:, :, 0] if strided else buf[:, :, 0].contiguous().to(dev)
    assert xd.is_contiguous() != strided
    x8, scale = _capi.quant_fp8_blocks(xd, None if offset is None else offset.to(dev))
    ref8, ref_scale = _quant_cpu(buf[:, :, 0], offset)
    assert torch.equal(scale.cpu(), ref_scale)
    assert torch.equal(x8.cpu(), ref8)


def _ref_attention(qd, kd, v, kept, seqlen, text_block_start, text_amp):
    """qd, kd float64 [S,H,128] (dequantised), v [S,H,128]; kept = the kept kv blocks of every image query block."""
    S = qd.shape[0]
    cols = torch.arange(S)
    o = torch.zeros(S, H, 128, dtype=torch.float64)
    for m in range(S // 128):
        rows = slice(128 * m, 128 * m + 128)
        s = torch.einsum("qhd,khd->hqk", qd[rows], kd) * (128 ** -0.5 * math.log2(math.e))     # base-2 logits
        if m < len(kept):
            keep = torch.zeros(S, dtype=torch.bool)
            for j in kept[m]:
                keep[128 * j:128 * j + 128] = True
            s = s + text_amp * (cols >= 128 * text_block_start)
            s = s.masked_fill(~(keep & (cols < seqlen)), -math.inf)
        p = torch.exp2(s - s.amax(-1, keepdim=True))
        o[rows] = torch.einsum("hqk,khd->qhd", p / p.sum(-1, keepdim=True), v.double())
        if m < len(kept):
            o[rows][cols[rows] >= seqlen] = 0
    return o


KEPT = [[0], [0, 1, 3]]     # the shortest list (two tiles); a gap and an odd count


@DTYPES
@pytest.mark.parametrize("seqlen", [512, 256 + 70, 128 + 70])   # all valid | kept block 3 wholly masked | + a cut inside kept block 1
@pytest.mark.parametrize("text_amp", [0.0, 0.5])
@pytest.mark.parametrize("xcd_remap", [True, False], ids=["xcd", "plain"])
def test_attention_against_float64(dtype, seqlen, text_amp, xcd_remap):
    from jenga_amd import _capi
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(11)
    q, k, v = [torch.randn(1, 512, H, 128, generator=gen).to(dtype) for _ in range(3)]
    q8, qs = _quant_cpu(q)
    k8, ks = _quant_cpu(k, k.float().mean(1))
    idx = torch.zeros(1, H, 2, 4, dtype=torch.int32)
    for m, js in enumerate(KEPT):
        idx[:, :, m, :len(js)] = torch.tensor(js, dtype=torch.int32)
    cnt = torch.tensor([len(js) for js in KEPT], dtype=torch.int32).expand(1, H, 2).contiguous()
    vt = _capi.pack_v(v.to(dev), 4)
    o = _capi.bsattn_fp8_fwd(q8.to(dev), qs.to(dev), k8.to(dev), ks.to(dev), vt, torch.tensor([seqlen], dtype=torch.int32),
                             idx.to(dev), cnt.to(dev), 2, 128 ** -0.5, text_amp, 2, xcd_remap=xcd_remap).cpu()
    deq = lambda x8, s: (x8.view(torch.float8_e4m3fn).float().double()
                         * s.double().permute(0, 2, 1).repeat_interleave(128, 1)[..., None])[0]
    ref = _ref_attention(deq(q8, qs), deq(k8, ks), v[0], KEPT, seqlen, 2, text_amp)
    assert o.dtype == dtype and torch.isfinite(o.float()).all()
    err = (o[0].double() - ref).abs().max().item()
    print(f"{dtype} seqlen {seqlen} amp {text_amp}: max |o - ref| = {err:.3e}")
    assert err <= BOUND[dtype]
    assert torch.equal(o[0, seqlen:256], torch.zeros_like(o[0, seqlen:256]))     # image rows behind the valid length


@pytest.mark.parametrize("flavour", ["hunyuan", "wan"])
def test_front_end_routes_through_the_fp8_kernels(flavour):
    from jenga_amd import _capi
    from jenga_amd.modules import attention_block_sparse as A
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    S, tb = (640, 2) if flavour == "hunyuan" else (300, 0)
    q, k, v = [torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16).to(dev) for _ in range(3)]
    if flavour == "hunyuan":
        cu = torch.tensor([0, 384 + 70, 640], dtype=torch.int32, device=dev)
        call = lambda **kw: A.block_sparse_attention(q, k, v, 2, cu_seqlens_q=cu, cu_seqlens_kv=cu, text_blocks=2,
                                                     p_remain_rates=0.5, return_mask=True, **kw)
        valid, p = 384 + 70, 0.5
    else:
        call = lambda **kw: A.block_sparse_attention_wan(q, k, v, 2, return_mask=True, **kw)
        valid, p = S, 0.9
    (o, mask), (o16, mask16) = call(qk_dtype="fp8"), call()
    assert torch.equal(mask, mask16) and o.shape == o16.shape == (1, S, H * 128)
    with pytest.raises(ValueError):
        call(qk_dtype="int4")
    # the same steps by hand
    qp, kp, vp = (A._pad_seq(t, -S % 128) for t in (q, k, v))
    nb = qp.shape[1] // 128
    kpool = _capi.block_pool(kp, nb)
    _, idx, cnt = _capi.block_select(_capi.block_pool(qp, nb - tb), kpool, None, nb - tb, tb, 2, p)
    q8, qs = _capi.quant_fp8_blocks(qp)
    k8, ks = _capi.quant_fp8_blocks(kp, kpool.float().mean(2))
    seqlens = torch.tensor([valid], dtype=torch.int32, device=dev)
    hand = _capi.bsattn_fp8_fwd(q8, qs, k8, ks, _capi.pack_v(vp, nb), seqlens, idx, cnt, nb - tb, 128 ** -0.5, 0.0, nb - tb)
    assert torch.equal(o, hand[:, :S].reshape(1, S, H * 128))
    assert o.float().abs().max() > 0.01
