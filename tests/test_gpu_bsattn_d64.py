"""GPU (-m gpu): the native 64-channel path (csrc/bsattn64.hip: jenga_block_pool_d64, jenga_bsattn_d64_fwd) -- pooling bit for
bit against the 128-channel pooling of the zero-padded rows, attention against the header's semantics in float64 on the 16-bit
inputs, and block_sparse_attention*(narrow_heads="native") against the three steps composed by hand and against "pad".
Seeded randn, H = 2 (1 for the long list).  Worst max |o - ref| measured on an MI355X: float64 cases 2.00e-3 (bf16) / 2.61e-4 (fp16), long list 2.72e-3, native vs pad 7.8e-3."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = {torch.bfloat16: 1e-2, torch.float16: 2e-3}   # the project's bounds for the two roundings of P and o
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
DEV = torch.device("cuda:0")


@DTYPES
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "fused_view"])
def test_pooling_is_bit_identical_to_the_padded_pooling(dtype, strided):
    from jenga_amd import _capi
    buf = torch.randn(1, 384, 2, 192, generator=torch.Generator().manual_seed(3)).to(dtype).to(DEV)
    x = buf[..., 64:128] if strided else buf[..., 64:128].contiguous()
    pooled = _capi.block_pool_d64(x, 3)
    assert pooled.shape == (1, 2, 3, 128) and pooled[..., :64].abs().max() > 0
    assert torch.equal(pooled, _capi.block_pool(torch.nn.functional.pad(x, [0, 64]), 3))


def _ref(q, k, v, lists, seqlen, text_block_start, amp):
    """include/jenga_amd.h, jenga_bsattn_d64_fwd, in float64; q, k, v [S,H,64]; lists[m]: kept kv blocks of image block m."""
    S, H, _ = q.shape
    c = torch.tensor(64 ** -0.5 * 1.44269504, dtype=torch.float32)
    kd, vd = k.double(), v.double()
    o = torch.zeros(S, H, 64, dtype=torch.float64)
    for m in range(S // 128):
        rows = slice(m * 128, (m + 1) * 128)
        if m < len(lists):    # image rows: pre-scaled, rounded q; base-2 logits; amp on text kv blocks; length mask
            cols = torch.cat([torch.arange(j * 128, (j + 1) * 128) for j in lists[m]])
            cols = cols[cols < seqlen]
            qt = (q[rows].float() * c).to(q.dtype).double()
            s = (torch.einsum("qhd,khd->hqk", qt, kd[cols]) + amp * (cols >= text_block_start * 128)) * math.log(2)
        else:                 # text rows: every key, unrounded q
            cols = torch.arange(S)
            s = torch.einsum("qhd,khd->hqk", q[rows].double(), kd) * 64 ** -0.5
        o[rows] = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), vd[cols])
    o[seqlen:len(lists) * 128] = 0
    return o


def _run(q, k, v, lists, seqlen, text_block_start, amp, xcd_remap=True):
    from jenga_amd import _capi
    S, H, _ = q.shape
    idx = torch.zeros(1, H, len(lists), S // 128, dtype=torch.int32)
    for m, kept in enumerate(lists):
        idx[:, :, m, :len(kept)] = torch.tensor(kept, dtype=torch.int32)
    cnt = torch.tensor([len(kept) for kept in lists], dtype=torch.int32).expand(1, H, -1).contiguous()
    o = _capi.bsattn_d64_fwd(q[None].to(DEV), k[None].to(DEV), v[None].to(DEV), torch.tensor([seqlen], dtype=torch.int32),
                             idx.to(DEV), cnt.to(DEV), len(lists), 64 ** -0.5, amp, text_block_start, xcd_remap=xcd_remap)
    return o[0].cpu()


LISTS = [[0], [0, 1, 3]]   # one block (two tiles, the ring never wraps); a gap, an odd count and a ring wrap


@functools.lru_cache(maxsize=None)
def _case(S, H, dtype):
    gen = torch.Generator().manual_seed(11)
    return [torch.randn(S, H, 64, generator=gen).to(dtype) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def _ref_small(seqlen, amp, dtype):
    return _ref(*_case(512, 2, dtype), LISTS, seqlen, 2, amp)


@DTYPES
@pytest.mark.parametrize("xcd_remap", [True, False], ids=["xcd", "plain"])
@pytest.mark.parametrize("amp", [0.0, 0.5])
@pytest.mark.parametrize("seqlen", [512, 326, 198])   # all valid / kept block 3 wholly masked / + a cut inside kept block 1
def test_attention_against_float64(seqlen, amp, xcd_remap, dtype):
    o = _run(*_case(512, 2, dtype), LISTS, seqlen, 2, amp, xcd_remap)
    err = (o.double() - _ref_small(seqlen, amp, dtype)).abs().max().item()
    print(f"seqlen {seqlen} amp {amp} xcd {xcd_remap} {dtype}: max |o - ref| = {err:.3e}")
    assert torch.isfinite(o.float()).all()
    assert err <= BOUND[dtype]
    assert not o[seqlen:256].any()           # image rows behind the valid length: exact zeros


def test_list_longer_than_one_fetch():
    """66 blocks: query block 0 keeps all of them (more than one 64-entry fetch of the list), block m keeps [m]."""
    nb, seqlen = 66, 66 * 128 - 50
    lists = [list(range(nb))] + [[m] for m in range(1, nb)]
    q, k, v = _case(nb * 128, 1, torch.bfloat16)
    o = _run(q, k, v, lists, seqlen, nb, 0.0)
    err = (o.double() - _ref(q, k, v, lists, seqlen, nb, 0.0)).abs().max().item()
    print(f"long list: max |o - ref| = {err:.3e}")
    assert torch.isfinite(o.float()).all() and err <= BOUND[torch.bfloat16]
    assert not o[seqlen:].any()


def _front_end_inputs():
    """The inputs of the narrow-head case of test_gpu_parity.py at D = 64: 10 blocks, clustered block means."""
    import inputs  # tests/golden/inputs.py
    from oracle import gilbert as og
    gen = torch.Generator().manual_seed(50 + 64)
    q, k = inputs.peaky_qk(gen, 1, 2, 10, 10, 64, 0.8)
    q, k = (t.transpose(1, 2).to(torch.bfloat16).contiguous().to(DEV) for t in (q, k))
    v = torch.randn(1, 1280, 2, 64, generator=gen).to(torch.bfloat16).to(DEV)
    nbm = torch.from_numpy(og.gilbert_block_neighbor_mapping(2, 8, 64, 128))
    return q, k, v, nbm, torch.tensor([0, 8 * 128 + 60, 1280], dtype=torch.int32, device=DEV)


def test_front_end_native_is_the_three_steps_and_selects_like_pad():
    from jenga_amd import _capi
    from jenga_amd.modules import attention_block_sparse as op
    q, k, v, nbm, cu = _front_end_inputs()
    kw = dict(cu_seqlens_q=cu, cu_seqlens_kv=cu, text_blocks=2, text_amp=0.2, block_neighbor_list=nbm, p_remain_rates=0.3,
              return_mask=True)
    o, mask = op.block_sparse_attention(q, k, v, 3, narrow_heads="native", **kw)
    o_pad, mask_pad = op.block_sparse_attention(q, k, v, 3, **kw)
    _, idx, cnt = _capi.block_select(_capi.block_pool_d64(q, 8), _capi.block_pool_d64(k, 10), nbm, 8, 2, 3, 0.3, head_dim=64)
    hand = _capi.bsattn_d64_fwd(q, k, v, cu[1:2], idx, cnt, 8, 64 ** -0.5, 0.2, 8)
    assert o.shape == (1, 1280, 2 * 64) and torch.equal(o, hand.reshape(1, 1280, 128))
    assert torch.equal(mask, mask_pad)
    diff = (o.float() - o_pad.float()).abs().max().item()
    print(f"native vs pad: max |diff| = {diff:.3e}")
    assert diff <= 2 * BOUND[torch.bfloat16]


def test_front_end_i2v_pads_the_sequence_only():
    from jenga_amd.modules import attention_block_sparse as op
    q, k, v, _, _ = _front_end_inputs()
    S = 1280 - 37
    q, k, v = q[:, :S], k[:, :S], v[:, :S]
    cu = torch.tensor([0, 8 * 128 + 60, S], dtype=torch.int32, device=DEV)
    kw = dict(cu_seqlens_q=cu, cu_seqlens_kv=cu, text_blocks=2, text_amp=0.2, p_remain_rates=0.3)
    o = op.block_sparse_attention_i2v(q, k, v, 3, narrow_heads="native", **kw)
    o_pad = op.block_sparse_attention_i2v(q, k, v, 3, **kw)
    assert o.shape == (1, S, 2 * 64)
    assert (o.float() - o_pad.float()).abs().max().item() <= 2 * BOUND[torch.bfloat16]
