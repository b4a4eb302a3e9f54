"""AttenCarve operator: drop-in for the reference's `block_sparse_attention`.

Mirrors (same names, argument order, defaults, return layout):
  hyvideo/modules/attention_block_triton_diffres.py:399-424      -> block_sparse_attention         (HunyuanVideo)
  hyvideo_i2v/modules/attention_block_triton_diffres.py:398-423  -> block_sparse_attention_i2v     (pads, text_blocks=4)
  wan/modules/attention_block_triton_diffres.py:535-562          -> block_sparse_attention_wan     (pads, bf16, first frame)

Everything numeric runs in libjenga_amd.so (HIP, gfx950) through jenga_amd._capi:
  jenga_block_pool + jenga_block_select  (reference :198-295)   selection -> ascending kept-block lists
  jenga_pack_v + jenga_bsattn_fwd        (reference :38-196, :371-380)   image rows + text rows in one launch
  qk_dtype="fp8" (opt-in, jenga_amd extension): jenga_quant_fp8_blocks on q and k + jenga_bsattn_fp8_fwd in its place
  narrow_heads="native" (opt-in, head_dim 64): jenga_block_pool_d64 + jenga_bsattn_d64_fwd on the 64-channel rows as given
torch is used for allocation, views and zero-padding only.  No CPU fallback.
"""

import torch

from .. import _capi

BLOCK = 128


def _seqlens_from_cu(cu_seqlens_q, device):
    # reference :327-329: seqlens = cu_seqlens_q[1:2] (only batch element 0's valid length is ever used)
    s = cu_seqlens_q[1:2]
    return s.to(device=device, dtype=torch.int32)


def build_block_index(query, key, top_k, text_blocks, prob_threshold, block_neighbor_list=None,
                      first_frame_blocks=0, want_mask=False, pooled=None, head_dim=128):
    """query/key [B,S,H,128] (S multiple of 128).  -> (mask|None, idx, cnt) for the image query blocks.
    Replaces _build_block_index_with_importance_optimized (:198-295).  pooled = (qpool [B,H,nimg,128],
    kpool [B,H,nb,128]) when the caller's norm+RoPE kernel already produced the block means.  head_dim < 128: the
    tensors are zero-padded to 128 channels, the scores scaled by head_dim ** -0.5 (:232)."""
    B, S, H, D = query.shape
    nb = S // BLOCK
    nimg = nb - text_blocks
    if pooled is not None:
        qpool, kpool = pooled
    else:
        qpool = _capi.block_pool(query, nimg)
        kpool = _capi.block_pool(key, nb)
    return _capi.block_select(qpool, kpool, block_neighbor_list, nimg, text_blocks, top_k, prob_threshold,
                              first_frame_blocks=first_frame_blocks, want_mask=want_mask, head_dim=head_dim)


def _check_qk_dtype(qk_dtype, head_dim):
    if qk_dtype not in (None, "fp8"):
        raise ValueError(f"jenga_amd: qk_dtype must be None or 'fp8' (got {qk_dtype!r})")
    if qk_dtype == "fp8" and head_dim != 128:
        raise ValueError(f"jenga_amd: qk_dtype='fp8' needs head_dim 128 (got {head_dim})")


def _check_narrow_heads(narrow_heads, head_dim, qk_dtype):
    if narrow_heads not in ("pad", "native"):
        raise ValueError(f"jenga_amd: narrow_heads must be 'pad' or 'native' (got {narrow_heads!r})")
    if narrow_heads == "native" and head_dim != 64:
        raise ValueError(f"jenga_amd: narrow_heads='native' needs head_dim 64 (got {head_dim})")
    if narrow_heads == "native" and qk_dtype == "fp8":
        raise ValueError("jenga_amd: narrow_heads='native' cannot be combined with qk_dtype='fp8'")


def _pooled_for(qk_dtype, q, k, nimg, nb, pooled=None):
    """The (qpool, kpool) the selection runs on.  FP8 needs the block means of k whether the caller has them or not (they
    give K's smoothing offset): pooled here, once, they serve the selection too.  Otherwise the caller's, or None."""
    if qk_dtype == "fp8" and pooled is None:
        pooled = (_capi.block_pool(q, nimg) if nimg > 0 else None, _capi.block_pool(k, nb))
    return pooled


def _attend_fp8(q, k, vt, kpool, seqlens, idx, cnt, nimg, text_amp, out=None):
    """The FP8 Q.K path behind the (unchanged) selection: q and k quantised per 128-token block, K after subtracting its
    mean over the sequence -- the mean of the block means the selection already has, so no further pass over K."""
    q8, q_scale = _capi.quant_fp8_blocks(q)
    k8, k_scale = _capi.quant_fp8_blocks(k, kpool.float().mean(2))
    return _capi.bsattn_fp8_fwd(q8, q_scale, k8, k_scale, vt, seqlens, idx, cnt, nimg, 128 ** -0.5, text_amp, nimg, out=out)


def attencarve_packed(q, k, vt, top_k, seqlens, text_blocks, text_amp, prob_threshold, block_neighbor_list,
                      first_frame_blocks=0, out=None, return_lists=False, pooled=None, qk_dtype=None):
    """Core used by the DiT blocks: q/k [B,S,H,128] already normed+roped (any strides), vt = packed V workspace
    (jenga_pack_v), seqlens int32 [B] on the device.  Selection + one attention launch; returns o [B,S,H,128]
    (written into `out` if given, which may be a strided view, e.g. the left part of the single-stream blocks'
    concat buffer)."""
    B, S, H, D = q.shape
    _check_qk_dtype(qk_dtype, D)
    nb = S // BLOCK
    nimg = nb - text_blocks
    pooled = _pooled_for(qk_dtype, q, k, nimg, nb, pooled)
    idx = cnt = None
    if nimg > 0:
        _, idx, cnt = build_block_index(q, k, top_k, text_blocks, prob_threshold, block_neighbor_list,
                                        first_frame_blocks, pooled=pooled)
    if qk_dtype == "fp8":
        o = _attend_fp8(q, k, vt, pooled[1], seqlens, idx, cnt, nimg, text_amp, out=out)
    else:
        o = _capi.bsattn_fwd(q, k, vt, seqlens, idx, cnt, nimg, D ** -0.5, text_amp, nimg, out=out)
    return (o, idx, cnt) if return_lists else o


def _combined(query, key, value, top_k, seqlens, text_blocks, text_amp, prob_threshold, block_neighbor_list,
              shape_xfuse, first_frame_blocks=0, context_size=None, return_mask=False, qk_dtype=None, narrow_heads="pad"):
    B, S, H, D = query.shape
    if D not in (16, 32, 64, 128):         # the Triton kernel's own assert (:155)
        raise ValueError(f"jenga_amd: head_dim must be 16, 32, 64 or 128 (got {D})")
    _check_qk_dtype(qk_dtype, D)
    _check_narrow_heads(narrow_heads, D, qk_dtype)
    head_dim = D
    if D != 128 and narrow_heads == "pad":
        # Narrow heads run on the 128-channel kernels with zero channels appended: the extra products are exact zeros in
        # every dot product (pooled scores, QK^T), the extra output channels are dropped, and the two scales keep the true
        # head_dim ** -0.5.  No entry script of the reference reaches this (all three models have 128-channel heads), so
        # it is kept simple rather than fast: 128 / D times the FLOPs.
        query, key, value = (torch.nn.functional.pad(t, [0, 128 - D]) for t in (query, key, value))
        D = 128
    if S % BLOCK:
        raise ValueError(f"jenga_amd: sequence length {S} is not a multiple of {BLOCK}")
    nb = S // BLOCK
    nimg = nb - text_blocks
    if nimg < 0:
        raise ValueError("text_blocks exceeds the number of blocks")
    mask = idx = cnt = None
    if narrow_heads == "native":
        # 64-channel rows as they lie in memory: no channel padding, no pack_v workspace, no output slice (csrc/bsattn64.hip)
        if nimg > 0:
            mask, idx, cnt = _capi.block_select(_capi.block_pool_d64(query, nimg), _capi.block_pool_d64(key, nb),
                                                block_neighbor_list, nimg, text_blocks, top_k, prob_threshold,
                                                first_frame_blocks=first_frame_blocks, want_mask=return_mask, head_dim=64)
        out = _capi.bsattn_d64_fwd(query, key, value, seqlens, idx, cnt, nimg, 64 ** -0.5, text_amp, nimg)
    else:
        pooled = _pooled_for(qk_dtype, query, key, nimg, nb)
        if nimg > 0:
            mask, idx, cnt = build_block_index(query, key, top_k, text_blocks, prob_threshold, block_neighbor_list,
                                               first_frame_blocks, want_mask=return_mask, pooled=pooled, head_dim=head_dim)
        vt = _capi.pack_v(value, nb)
        if qk_dtype == "fp8":
            out = _attend_fp8(query, key, vt, pooled[1], seqlens, idx, cnt, nimg, text_amp)
        else:
            out = _capi.bsattn_fwd(query, key, vt, seqlens, idx, cnt, nimg, head_dim ** -0.5, text_amp, nimg)
    if context_size is not None and context_size != S:
        out = out[:, :context_size]
    if D != head_dim:           # the padded channels
        out = out[..., :head_dim].contiguous()
    if not shape_xfuse:
        out = out.reshape(B, out.shape[1], H * head_dim)
    return (out, mask) if return_mask else out


def _check_inputs(query, key, value):
    if query.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"jenga_amd: dtype must be bfloat16 or float16, got {query.dtype}")
    if key.dtype != query.dtype or value.dtype != query.dtype:
        raise ValueError("jenga_amd: query/key/value dtypes differ")
    if query.dim() != 4 or key.shape != value.shape or query.shape != key.shape:
        raise ValueError("jenga_amd: expected query/key/value of identical shape [B,S,H,D]")


def _unit_inner(t):
    return t if t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:-1]) else t.contiguous()


def block_sparse_attention(
    query: torch.Tensor,
    key: torch.Tensor,
    value: torch.Tensor,
    top_k: int,
    block_size_M: int = 128,
    block_size_N: int = 128,
    cu_seqlens_q: torch.Tensor = None,
    cu_seqlens_kv: torch.Tensor = None,
    max_seqlen_q: int = None,
    max_seqlen_kv: int = None,
    text_blocks: int = 2,
    text_amp: float = 0.0,
    block_neighbor_list: torch.Tensor = None,
    shape_xfuse: bool = False,
    p_remain_rates: float = 0.5,
    return_mask: bool = False,
    qk_dtype: str = None,
    narrow_heads: str = "pad",
):
    """HunyuanVideo flavour.  q/k/v [B,S,H,128], S % 128 == 0 (the reference's padding branch is dead code, :331-336),
    cu_seqlens_q from get_cu_seqlens (only element [1] is used).  Returns [B,S,H*D], or [B,S,H,D] if shape_xfuse.
    qk_dtype (jenga_amd extension, also on the I2V and Wan flavours): None = 16-bit Q.K (the default); "fp8" = the same kept
    lists, then Q and K quantised per 128-token block to e4m3fn and QK^T on the FP8 MFMA (csrc/qattn.hip), head_dim 128 only.
    narrow_heads (jenga_amd extension, also on the I2V and Wan flavours): how heads narrower than 128 channels run.  "pad" (the
    default): zero-padded to 128 channels on the 128-channel kernels.  "native": head_dim 64 only -- block_pool_d64,
    block_select(head_dim=64) and bsattn_d64_fwd on the tensors as given (csrc/bsattn64.hip); same kept blocks as "pad"."""
    _check_inputs(query, key, value)
    if block_size_M != BLOCK or block_size_N != BLOCK:
        raise ValueError("jenga_amd: block sizes must be 128")
    if cu_seqlens_q is None or cu_seqlens_kv is None:
        raise ValueError("jenga_amd (HunyuanVideo flavour): cu_seqlens_q / cu_seqlens_kv are required")
    if query.shape[0] != 1:
        raise ValueError("jenga_amd (HunyuanVideo flavour): batch must be 1 (the reference reads cu_seqlens_q[1:2] only)")
    query, key, value = _unit_inner(query), _unit_inner(key), _unit_inner(value)
    seqlens = _seqlens_from_cu(cu_seqlens_q, query.device)
    return _combined(query, key, value, top_k, seqlens, text_blocks, text_amp, p_remain_rates, block_neighbor_list,
                     shape_xfuse, return_mask=return_mask, qk_dtype=qk_dtype, narrow_heads=narrow_heads)


def _pad_seq(t, pad):
    return torch.nn.functional.pad(t, [0, 0, 0, 0, 0, pad]) if pad else t


def block_sparse_attention_i2v(query, key, value, top_k, block_size_M=128, block_size_N=128, cu_seqlens_q=None,
                               cu_seqlens_kv=None, max_seqlen_q=None, max_seqlen_kv=None, text_blocks=4,
                               text_amp=0.0, block_neighbor_list=None, shape_xfuse=False, p_remain_rates=0.5,
                               return_mask=False, qk_dtype=None, narrow_heads="pad"):
    """HunyuanVideo-I2V flavour: pads S to a multiple of 128, text_blocks defaults to 4, output sliced back."""
    _check_inputs(query, key, value)
    if cu_seqlens_q is None:
        raise ValueError("jenga_amd (I2V flavour): cu_seqlens_q is required")
    B, S, H, D = query.shape
    pad = (BLOCK - S % BLOCK) % BLOCK
    q, k, v = (_pad_seq(_unit_inner(t), pad) for t in (query, key, value))
    seqlens = _seqlens_from_cu(cu_seqlens_q, query.device)
    return _combined(q, k, v, top_k, seqlens, text_blocks, text_amp, p_remain_rates, block_neighbor_list,
                     shape_xfuse, context_size=S, return_mask=return_mask, qk_dtype=qk_dtype, narrow_heads=narrow_heads)


def block_sparse_attention_wan(query, key, value, top_k, block_size_M=128, block_size_N=128, cu_seqlens_q=None,
                               cu_seqlens_kv=None, max_seqlen_q=None, max_seqlen_kv=None, text_blocks=0,
                               text_amp=0.0, block_neighbor_list=None, shape_xfuse=False, p_remain_rates=0.9,
                               first_frame_blocks=0, return_mask=False, kv_lens=None, qk_dtype=None,
                               narrow_heads="pad"):
    """Wan flavour: always pads, computes in bf16 whatever the input dtype, seqlen = unpadded S, dense first-frame
    rule, returns the input dtype.  kv_lens (int32 [B] tensor, jenga_amd extension): keys at or beyond it are masked
    -- what WanSelfAttention's dense branch gets from flash_attention(k_lens=seq_lens) (wan/modules/model_mul.py:153-159)
    when teacache_forward padded the tokens beyond the real sequence; the reference's sparse branch has no such mask."""
    out_dtype = query.dtype
    B, S, H, D = query.shape
    pad = (BLOCK - S % BLOCK) % BLOCK
    q, k, v = (_pad_seq(_unit_inner(t.to(torch.bfloat16)), pad) for t in (query, key, value))
    if kv_lens is not None:
        seqlens = torch.clamp(torch.as_tensor(kv_lens).to(device=query.device, dtype=torch.int32).reshape(-1), max=S)
        if seqlens.numel() != B:
            raise ValueError("kv_lens must have one entry per batch element")
    else:
        seqlens = torch.full((B,), S, dtype=torch.int32, device=query.device)
    res = _combined(q, k, v, top_k, seqlens, text_blocks, text_amp, p_remain_rates, block_neighbor_list,
                    shape_xfuse, first_frame_blocks=first_frame_blocks, context_size=S, return_mask=return_mask,
                    qk_dtype=qk_dtype, narrow_heads=narrow_heads)
    if return_mask:
        return res[0].to(out_dtype), res[1]
    return res.to(out_dtype)
