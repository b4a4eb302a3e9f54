"""Attention front-end helpers, counterpart of hyvideo/modules/attenion.py."""
import torch

from .. import _capi


def get_cu_seqlens(text_mask, img_len):
    """cu_seqlens for (valid | padding) segments per sample -- same values as attenion.py:34-57, but built on
    text_mask's device without a Python loop over device scalars (the reference hard-codes device="cuda" and syncs
    per batch element)."""
    batch_size = text_mask.shape[0]
    text_len = text_mask.sum(dim=1).to(torch.int32)
    max_len = text_mask.shape[1] + img_len
    base = torch.arange(batch_size, device=text_mask.device, dtype=torch.int32) * max_len
    cu = torch.zeros(2 * batch_size + 1, dtype=torch.int32, device=text_mask.device)
    cu[1::2] = base + text_len + img_len
    cu[2::2] = base + max_len
    return cu


def my_parallel_attention(hybrid_seq_parallel_attn, q, k, v, img_q_len, img_kv_len, cu_seqlens_q, cu_seqlens_kv,
                          top_k: int = 10e7, text_amp: float = 0.0, block_neighbor_list=None,
                          p_remain_rates: float = 0.0):
    """Adapter with the argument convention of attenion.py:159-195."""
    attn = hybrid_seq_parallel_attn(
        None, q[:, :img_q_len], k[:, :img_kv_len], v[:, :img_kv_len], dropout_p=0.0, causal=False,
        joint_tensor_query=q[:, img_q_len:], joint_tensor_key=k[:, img_kv_len:], joint_tensor_value=v[:, img_kv_len:],
        joint_strategy="rear", top_k=top_k, cu_seqlens_q=cu_seqlens_q, cu_seqlens_kv=cu_seqlens_kv,
        text_amp=text_amp, block_neighbor_list=block_neighbor_list, p_remain_rates=p_remain_rates)
    b, s, a, d = attn.shape
    return attn.reshape(b, s, -1)


def parallel_attention(hybrid_seq_parallel_attn, q, k, v, img_q_len, img_kv_len, cu_seqlens_q, cu_seqlens_kv):
    """attenion.py:198-251: the DENSE sequence-parallel attention (no AttenCarve: yunchang's LongContextAttention over
    image + valid text, then a separate flash call among the text-padding tokens).  Callers in the reference: the non-Jenga
    blocks (hyvideo/modules/models.py:216, 381) and -- in their sequence-parallel branch only -- the Jenga I2V blocks
    (hyvideo_i2v/modules/models_mul.py:265, 484): the reference has no Jenga-aware sequence parallelism for I2V (SURVEY.md
    section 2 #22).  Here: the exchange of my_parallel_attention around the DENSE kernel call of `attention` (every block
    kept for every query block, image AND text rows masked at the valid length), i.e. the rank's heads attend over all
    image tokens and the valid text tokens -- what LongContextAttention computes.  Requirements of that path: hybrid_seq_parallel_attn is a
    jenga_amd.modules.ulysses.UlyssesAttenCarve, the image tokens of all ranks together are whole 128-token blocks, the text
    length is a multiple of 128.  The text-PADDING rows (beyond cu_seqlens_q[1]) attend among themselves like the reference's
    second flash call (:222-247): padding_segment on the rank's heads.  I2V sequence parallelism WITH AttenCarve is jenga_amd.dit's own path
    (JengaHYVideoDiT, i2v_condition_type = "token_replace"; tests/test_gpu_sp_dit.py)."""
    from . import ulysses
    if not isinstance(hybrid_seq_parallel_attn, ulysses.UlyssesAttenCarve):
        raise TypeError("parallel_attention: hybrid_seq_parallel_attn must be a jenga_amd.modules.ulysses.UlyssesAttenCarve "
                        f"(got {type(hybrid_seq_parallel_attn).__name__}); yunchang's LongContextAttention is not available here")
    if img_q_len != img_kv_len:
        raise ValueError("parallel_attention: img_q_len and img_kv_len must agree (self-attention)")
    n = hybrid_seq_parallel_attn.exchange().size()
    if (img_q_len * n) % 128:
        raise ValueError(f"parallel_attention: {n} ranks x {img_q_len} image tokens are not whole 128-token blocks")
    attn = hybrid_seq_parallel_attn(
        None, q[:, :img_q_len], k[:, :img_kv_len], v[:, :img_kv_len], dropout_p=0.0, causal=False,
        joint_tensor_query=q[:, img_q_len:], joint_tensor_key=k[:, img_kv_len:], joint_tensor_value=v[:, img_kv_len:],
        joint_strategy="rear", cu_seqlens_q=cu_seqlens_q, cu_seqlens_kv=cu_seqlens_kv, dense=True)
    b, s, a, d = attn.shape
    return attn.reshape(b, s, -1)


def padding_segment(q, k, v, seqlens, out):
    """The SECOND segment of the reference's dense varlen call (attenion.py:34-57 builds cu_seqlens = [0, n_valid, S] per
    sample; flash_attn_varlen_func :108-121, and parallel_attention's second flash call :222-247): the text-PADDING rows
    [n_valid, S) attend among themselves -- keys of that segment only, softmax scale head_dim ** -0.5.  No valid token ever
    reads them; they are computed so that the dense path returns what the reference returns, row for row (until round 5 they
    came back as zeros).  q / k / v [1, S, H, 128], seqlens int32 [1] on the device, out [1, S, H, 128] (rows >= n_valid are
    overwritten).  Reads n_valid on the host (one synchronisation per call: the dense path is the non-Jenga path)."""
    S, H, D = q.shape[1], q.shape[2], q.shape[3]
    n_valid = int(seqlens.reshape(-1)[0].item())
    L = S - n_valid
    if L <= 0:
        return out
    Lp = -(-L // 128) * 128
    buf = torch.zeros((3, 1, Lp, H, D), dtype=q.dtype, device=q.device)
    for i, t in enumerate((q, k, v)):
        buf[i, :, :L] = t[:, n_valid:]
    o = _capi.cross_attn_fwd(buf[0], buf[1], buf[2], sm_scale=D ** -0.5, kv_len=L)
    out[:, n_valid:] = o[:, :L]
    return out


_DENSE_LISTS = {}


def _dense_lists(device, B, H, nb):
    """"every block kept" lists for the dense path, built once per (device, B, H, nb): 78 MB at the 720p shape."""
    key = (str(device), B, H, nb)
    if key not in _DENSE_LISTS:
        if len(_DENSE_LISTS) > 8:
            _DENSE_LISTS.clear()
        idx = torch.arange(nb, device=device, dtype=torch.int32).expand(B, H, nb, nb).contiguous()
        cnt = torch.full((B, H, nb), nb, dtype=torch.int32, device=device)
        _DENSE_LISTS[key] = (idx, cnt)
    return _DENSE_LISTS[key]


class UnsupportedAttentionArgument(NotImplementedError, ValueError):
    """attention(): a mode / argument of the reference's front-end that this implementation does not compute.  (Both a
    ValueError -- the boundary's error type for rejected arguments -- and the NotImplementedError the reference raises for an
    unknown mode, attenion.py:150.)"""


def attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_kv=None, sm_scale=None, out=None):
    """flash_attn_varlen_func (attenion.py:108-121) in one launch of the dense varlen kernel (_capi.dense_varlen_fwd): query rows
    of segment i attend to the keys of segment i, softmax scale head_dim ** -0.5 unless given.  q / k / v: packed [T,H,128], or
    [B,S,H,128] flattened over B * S the way the reference's cu_seqlens count tokens (get_cu_seqlens: sample b starts at
    b * S); q and k / v may differ in length.  cu_seqlens_*: int32 [n+1] on the device with any boundaries; they are never read
    on the host, so the call neither synchronises nor breaks a graph capture.  Rows behind the last boundary and rows of a
    segment without keys are zeros.  Returns a tensor shaped like q."""
    if q.dim() == 3:
        return _capi.dense_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_kv, sm_scale, out)
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("attention_varlen: q / k / v must be [T,H,128] or [B,S,H,128]")
    flat = lambda t: t.reshape(t.shape[0] * t.shape[1], t.shape[2], t.shape[3])   # a view wherever the strides allow one
    o = _capi.dense_varlen_fwd(flat(q), flat(k), flat(v), cu_seqlens_q, cu_seqlens_kv, sm_scale,
                               None if out is None else out.view(-1, out.shape[2], out.shape[3]))
    return o.view(q.shape)


def attention(q, k, v, mode="flash", drop_rate=0, attn_mask=None, causal=False, cu_seqlens_q=None,
              cu_seqlens_kv=None, max_seqlen_q=None, max_seqlen_kv=None, batch_size=1, kernel="lists"):
    """Dense path taken when sa_drop_rate == 0 (attenion.py:60-157, mode "flash" = flash_attn_varlen_func over the
    (valid | padding) segments).  Runs the same HIP kernel with every kv block kept and the kv-length mask on, for all
    query blocks of the valid segment; the padding segment (text padding attending among itself) is one small dense call
    (padding_segment): both segments as the reference computes them.

    Only what the Jenga entry scripts call is computed: mode "flash" without mask, causality or dropout.  The reference's
    "torch" / "vanilla" modes (attenion.py:102-150: SDPA / explicit softmax with attn_mask, causal, dropout) have other
    semantics (a mask instead of cu_seqlens, [B,H,S,D] layout); they raise instead of silently running the flash semantics
    (VERDICT r5 missing 4).  In "flash" mode the reference itself drops attn_mask / causal / drop_rate on the floor
    (flash_attn_varlen_func is called without them, :108-116); a caller that passes them expects something this call does
    not do, so they raise too.

    kernel: "lists" (default) is the path described above: batch 1, S a multiple of 128, the (valid | padding) pair.  "varlen"
    hands the whole call to the dense varlen kernel (attention_varlen) in one launch over the cu_seqlens as given: any batch,
    any S, any segments, no host read of cu_seqlens (graph-capturable).  Same semantics, not bit-equal with "lists"."""
    if kernel not in ("lists", "varlen"):
        raise ValueError(f"jenga_amd attention: kernel {kernel!r} is not one of \"lists\", \"varlen\"")
    if mode != "flash":
        raise UnsupportedAttentionArgument(f"jenga_amd attention: mode {mode!r} is not implemented (only \"flash\")")
    if attn_mask is not None:
        raise UnsupportedAttentionArgument("jenga_amd attention: attn_mask is not supported (varlen via cu_seqlens only)")
    if causal:
        raise UnsupportedAttentionArgument("jenga_amd attention: causal=True is not supported")
    if drop_rate:
        raise UnsupportedAttentionArgument("jenga_amd attention: drop_rate != 0 is not supported (inference only)")
    if cu_seqlens_q is None:
        raise ValueError("jenga_amd attention: cu_seqlens_q is required (get_cu_seqlens)")
    if kernel == "varlen":
        o = attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_kv)
        return o.reshape(q.shape[0], q.shape[1], -1)
    if q.shape[0] != 1:
        raise ValueError("jenga_amd dense attention: batch must be 1")
    B, S, H, D = q.shape
    if S % 128:
        raise ValueError("jenga_amd dense attention: S must be a multiple of 128")
    nb = S // 128
    seqlens = cu_seqlens_q[1:2].to(device=q.device, dtype=torch.int32)
    idx, cnt = _dense_lists(q.device, B, H, nb)
    vt = _capi.pack_v(v if v.stride(-1) == 1 else v.contiguous(), nb)
    o = _capi.bsattn_fwd(q, k, vt, seqlens, idx, cnt, nb, D ** -0.5, 0.0, nb)
    padding_segment(q, k, v, seqlens, o)
    return o.reshape(B, S, H * D)
