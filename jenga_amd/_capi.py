"""ctypes binding of libjenga_amd.so (include/jenga_amd.h).  No compute happens in Python: every function
enqueues HIP kernels on torch's current stream and raises if the library is missing or a call fails.
There is NO CPU fallback on purpose: the product path must fail loudly when the HIP extension is absent."""
import collections
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JENGA_LIB", os.path.join(_HERE, "libjenga_amd.so"))

JENGA_BF16, JENGA_FP16 = 0, 1
# jenga_bsattn_fwd flags.  XCD_REMAP, BALANCE and LP are the header's (include/jenga_amd.h); SORTED and PAIR are resolved here.
ATTN_XCD_REMAP = 1   # contiguous ranges of query blocks per XCD (L2 locality); without it: plain head-major order
ATTN_BALANCE = 4     # query blocks (pairs) DRAWN from per-XCD queues on an oversubscribed grid: evens out the speed differences
#                      between the XCDs of a chip; bit-identical to the static mapping
ATTN_LEGACY = 0      # (readability alias) no kernel bit: the plain kernel, one query block per 4-wave workgroup (csrc/bsattn.hip)
ATTN_LP = 8          # the same decomposition with an in-wave software pipeline (csrc/bsattn3.hip)
ATTN_SORTED = 16     # (Python-side) kept-count-aware launch order: jenga_order_by_count feeds jenga_bsattn_fwd's `order`
ATTN_PAIR = 64       # (Python-side) route to jenga_pair_merge + jenga_bsattn_pair_fwd: the pair kernel
#                      (csrc/bsattn5.hip: two Hilbert-adjacent query blocks per workgroup, 64 query rows per wave)
# LP default: LP kernel, XCD remap, kept-count-aware order inside every XCD's range (+3.3 % sustained on lists whose counts
# vary: profiles/r03_attn_order_ab.json), cross-XCD balancing (-1.7 % loop time: profiles/r04_attn_balance_ab.json).
ATTN_LP_FLAGS = ATTN_XCD_REMAP | ATTN_BALANCE | ATTN_LP | ATTN_SORTED
ATTN_PAIR_FLAGS = ATTN_XCD_REMAP | ATTN_BALANCE | ATTN_SORTED | ATTN_PAIR
ATTN_DEFAULT_FLAGS = int(os.environ.get("JENGA_ATTN_FLAGS", str(ATTN_LP_FLAGS)))


SELECT_DEVICE_SCAN = 1   # jenga_block_select flags: torch's DEVICE cumsum semantics for the kept-count rule
SELECT_DEFAULT_FLAGS = int(os.environ.get("JENGA_SELECT_FLAGS", "0"))

_vp, _i64, _i32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float

# name -> (restype, argtypes): every symbol the header declares
SIGNATURES = {
    "jenga_abi_version": (_i32, []),
    "jenga_last_error": (ctypes.c_char_p, []),
    "jenga_gilbert_map": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "jenga_gilbert_neighbors": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "jenga_gather_rows": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64]),
    "jenga_rmsnorm_rope": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp] + [_i64] * 10 + [_f32, _i32]),
    "jenga_rmsnorm_rows": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _i32, _i32]),
    "jenga_rope_complex": (_i32, [_vp, _vp, _vp, _vp, _vp] + [_i64] * 10 + [_i32, _i32]),
    "jenga_wan_norm_rope": (_i32, [_vp] * 6 + [_i64] * 5 + [_f32, _i32]),
    "jenga_ln_modulate": (_i32, [_vp] * 8 + [_i64] * 4 + [_f32, _i32]),
    "jenga_gate_residual": (_i32, [_vp] * 7 + [_i64] * 5 + [_i32]),
    "jenga_gelu_tanh": (_i32, [_vp, _vp, _vp] + [_i64] * 4 + [_i32]),
    "jenga_wan_ln_modulate": (_i32, [_vp] * 7 + [_i64] * 4 + [_f32, _i32, _i32]),
    "jenga_wan_gate_residual": (_i32, [_vp] * 5 + [_i64] * 5 + [_i32]),
    "jenga_qk_norm_rope_pool": (_i32, [_vp] * 11 + [_i64] * 13 + [_f32, _i32]),
    "jenga_sp_qkv_prologue": (_i32, [_vp] * 11 + [_i64] * 14 + [_f32, _i32]),
    "jenga_linear": (_i32, [_vp] * 7 + [_i64] * 7 + [_i32, _vp, _i64, _i32]),
    "jenga_block_pool": (_i32, [_vp, _vp, _vp] + [_i64] * 6 + [_i32]),
    "jenga_block_select": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp] + [_i64] * 6 + [_f32, _i64, _i32, _i32]),
    "jenga_order_by_count": (_i32, [_vp, _vp, _i64, _i64, _i64, _vp]),
    "jenga_pack_v_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "jenga_pack_v": (_i32, [_vp, _vp, _vp] + [_i64] * 8 + [_i32]),
    "jenga_bsattn_fwd": (_i32, [_vp] * 9 + [_i64] * 13 + [_f32, _f32, _i64, _i32, _i32]),
    "jenga_ulysses_pack_heads": (_i32, [_vp, _vp, _vp] + [_i64] * 7),
    "jenga_ulysses_unpack_heads": (_i32, [_vp, _vp, _vp] + [_i64] * 7),
    "jenga_stream_delay": (_i32, [_vp, ctypes.c_double]),
    "jenga_cross_attn_fwd": (_i32, [_vp] * 5 + [_i64] * 14 + [_f32, _i32]),
    "jenga_dense_varlen_fwd": (_i32, [_vp] * 7 + [_i64] * 12 + [_f32, _i32]),
    "jenga_quant_fp8_blocks": (_i32, [_vp] * 5 + [_i64] * 6 + [_i32]),
    "jenga_bsattn_fp8_fwd": (_i32, [_vp] * 10 + [_i64] * 13 + [_f32, _f32, _i64, _i32, _i32]),
    "jenga_quant_fp8_rows": (_i32, [_vp] * 4 + [_i64] * 4 + [_i32]),
    "jenga_linear_fp8": (_i32, [_vp] * 9 + [_i64] * 7 + [_i32, _i32]),
    "jenga_block_pool_d64": (_i32, [_vp, _vp, _vp] + [_i64] * 6 + [_i32]),
    "jenga_bsattn_d64_fwd": (_i32, [_vp] * 8 + [_i64] * 16 + [_f32, _f32, _i64, _i32, _i32]),
    "jenga_linear_export_choices": (_i64, [_vp, _i64]),
    "jenga_linear_import_choices": (_i32, [_vp, _i64]),
    "jenga_linear_import_mismatches": (_i64, []),
    "jenga_pair_merge": (_i32, [_vp, _vp, _vp] + [_i64] * 4 + [_vp, _vp]),
    "jenga_bsattn_pair_fwd": (_i32, [_vp] * 9 + [_i64] * 13 + [_f32, _f32, _i64, _i32, _i32]),
}

_lib = None
_bound = {}     # name -> the library's function, filled by lib(): the launch helpers look a name up once, here


class AttnProfile:
    """Optional per-launch timing of jenga_bsattn_fwd with HIP events recorded on the launch stream (bench.py's
    roofline leg).  Enable with `_capi.ATTN_PROFILE = AttnProfile()`; read with .summary() after a synchronize."""

    def __init__(self):
        self.events = []        # (start, stop)
        self.pairs = None       # device int64 scalar: kept (q-block, kv-block) pairs over all recorded launches
        self.launches = 0
        self.last_lists = None  # (idx, cnt) of the most recent launch with image query blocks
        self.tag = None         # set by the caller (bench.py: the step's sa-drop rate); recorded per launch
        self.per_launch = []    # (tag, device scalar: pairs of the launch), aligned with `events`

    def summary(self):
        ms = sum(a.elapsed_time(b) for a, b in self.events)
        out = dict(launches=self.launches, total_ms=ms, pairs=int(self.pairs.item()) if self.pairs is not None else 0)
        by_tag = {}
        for (tag, pr), (a, b) in zip(self.per_launch, self.events):
            t = by_tag.setdefault(tag, dict(launches=0, total_ms=0.0, pairs=0))
            t["launches"] += 1
            t["total_ms"] += a.elapsed_time(b)
            t["pairs"] += int(pr.item()) if torch.is_tensor(pr) else int(pr)
        out["by_tag"] = by_tag
        if self.last_lists is not None:
            # share of a query block's kept image kv blocks that the NEXT query block of the same head keeps too
            # (how coherent the lists are: ~0.35 for random lists at 30 % density, ~0.9 for a trained model's)
            idx, cnt = self.last_lists
            B, H, nq, nb = idx.shape
            valid = torch.arange(nb, device=idx.device)[None, None, None, :] < cnt[..., None]
            hit = torch.zeros((B, H, nq, nb), dtype=torch.int8, device=idx.device)
            hit.scatter_add_(-1, torch.where(valid, idx, torch.zeros_like(idx)).long(), valid.to(torch.int8))
            img = hit[..., :nq].bool()
            both = (img[:, :, :-1] & img[:, :, 1:]).sum(-1).float()
            out["adjacent_shared_frac"] = float((both / img[:, :, :-1].sum(-1).clamp(min=1).float()).mean().item())
        return out


ATTN_PROFILE = None


def _profile_start():
    """-> the start event of one attention launch, recorded on the current stream (inside the launch's device guard)"""
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _profile_stop(prof, e0, B, H, n_blocks, nq_img, idx, cnt):
    """the stop event of that launch, and its kept (q-block, kv-block) pairs: the lists' counts + every pair of the text rows"""
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    prof.events.append((e0, e1))
    prof.launches += 1
    tot = (cnt.sum(dtype=torch.int64) if cnt is not None else 0) + B * H * (n_blocks - nq_img) * n_blocks
    prof.pairs = tot if prof.pairs is None else prof.pairs + tot
    prof.per_launch.append((prof.tag, tot))
    if idx is not None and nq_img > 1:
        prof.last_lists = (idx, cnt)


class JengaError(RuntimeError):
    pass


def lib():
    """Load the shared library (once).  Raises JengaError with build instructions if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise JengaError(
                f"{LIB_PATH} is missing: build it with `python -m jenga_amd.build` (hipcc --offload-arch=gfx950). "
                "jenga_amd has no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        bound = {}
        for name, (res, args) in SIGNATURES.items():
            fn = bound[name] = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        if L.jenga_abi_version() != 4:
            raise JengaError("libjenga_amd.so ABI version mismatch; rebuild")
        _lib = L
        _bound.update(bound)
    return _lib


def _check(rc, what):
    if rc != 0:
        raise JengaError(f"{what} failed (code {rc}): {lib().jenga_last_error().decode()}")


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _Here:
    """No-op context: the tensor's device is already the current one (the common case: one process per GPU)."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_HERE_CTX = _Here()
_ALWAYS_GUARD = os.environ.get("JENGA_DEVICE_GUARD", "") == "always"     # (A/B switch: torch's device guard around every launch)


def _on(device):
    """`with torch.cuda.device(device)` only when it would change anything: the guard's two set_device calls cost more
    host time than the ctypes call they surround (60 layers x ~30 launches per step; the per-rank steps of the
    low-resolution stages of an 8-rank job are host-bound)."""
    if not _ALWAYS_GUARD and (device.index is None or device.index == torch.cuda.current_device()):
        return _HERE_CTX
    return torch.cuda.device(device)


def _need_gpu(t, what):
    if not t.is_cuda:
        raise JengaError(f"{what}: tensors must live on the GPU (got {t.device}); jenga_amd has no CPU path")


def dtype_code(dt):
    if dt == torch.bfloat16:
        return JENGA_BF16
    if dt == torch.float16:
        return JENGA_FP16
    raise ValueError(f"jenga_amd supports bfloat16 and float16 only, got {dt}")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _bshd_strides(t):
    """[B,S,H,D] tensor with unit innermost stride -> (sb, ss, sh) in elements."""
    if t.dim() != 4 or t.stride(3) != 1:
        raise ValueError("expected a [B,S,H,D] tensor with contiguous head_dim")
    return t.stride(0), t.stride(1), t.stride(2)


def _enqueue(name, device, *args):
    """The library's `name` on torch's current stream of `device`, which the caller has made current (_on)."""
    rc = (_bound.get(name) or getattr(lib(), name))(_stream(device), *args)
    if rc:
        _check(rc, name)


def _launch(name, device, *args):
    """_enqueue under the device guard.  Written out, not a call of it: this is the host path of every launch, and a Python
    frame is a measurable share of it (tools/host_overhead.py)."""
    fn = _bound.get(name) or getattr(lib(), name)
    with _on(device):
        rc = fn(_stream(device), *args)
    if rc:
        _check(rc, name)


# ------------------------------------------------------------------------------------------------ shared argument checks
def _flat(t, dtype):
    """A per-channel vector ([C], [1,C], ...) or None -> contiguous [C] in `dtype`."""
    return None if t is None else t.reshape(-1).to(dtype=dtype).contiguous()


def _norm_weight(w, like):
    """RMSNorm weight or None -> contiguous, on the device and in the dtype of the tensor it scales."""
    return None if w is None else w.to(device=like.device, dtype=like.dtype).contiguous()


def _rope_tables(cos, sin, s_rope, S):
    """cos / sin fp32 [>= s_rope, 128] -> (cos, sin, s_rope) with contiguous tables; s_rope defaults to the tables' length and
    may exceed neither them nor the sequence.  No tables: s_rope = 0."""
    if cos is None:
        return cos, sin, 0
    if cos.dtype != torch.float32 or sin.dtype != torch.float32 or cos.shape[-1] != 128:
        raise ValueError("cos/sin must be float32 [S,128]")
    if s_rope is None:
        s_rope = cos.shape[0]
    if s_rope > cos.shape[0] or s_rope > S:
        raise ValueError("s_rope exceeds the table / sequence length")
    return cos.contiguous(), sin.contiguous(), s_rope


def _pool_blocks(pool, name, B, H, dtype):
    """A block-mean output [B,H,n,128] of qk_norm_rope_pool -> n (0: no such output)."""
    if pool is None:
        return 0
    if pool.dim() != 4 or pool.shape[0] != B or pool.shape[1] != H or pool.shape[3] != 128 or not pool.is_contiguous() \
            or pool.dtype != dtype:
        raise ValueError(f"{name} must be a contiguous [B,H,n,128] tensor of the input dtype")
    return pool.shape[2]


def _attn_lists(what, device, B, H, n_blocks, nq_img, seqlens, idx, cnt):
    """The list arguments of the block-sparse attention entries -> seqlens as int32 on `device`.  seqlens: at least B entries;
    0 <= nq_img <= n_blocks; with image query blocks, idx / cnt contiguous int32 [B,H,nq_img,n_blocks] / [B,H,nq_img] there."""
    if seqlens is not None and (seqlens.dtype != torch.int32 or seqlens.device != device):
        seqlens = seqlens.to(device=device, dtype=torch.int32)
    if seqlens is not None and seqlens.numel() < B:
        # the reference passes cu_seqlens_q[1:2] whatever the batch (attention_block_triton_diffres.py:327-329) and its
        # kernel then reads past it for B > 1; here that is an error instead of an out-of-bounds read
        raise ValueError(f"{what}: seqlens has {seqlens.numel()} entries for batch {B}")
    if not 0 <= nq_img <= n_blocks:
        raise ValueError(f"{what}: nq_img must lie in [0, n_blocks]")
    if nq_img > 0 and (idx is None or cnt is None or tuple(idx.shape) != (B, H, nq_img, n_blocks)
                       or tuple(cnt.shape) != (B, H, nq_img) or idx.dtype != torch.int32 or cnt.dtype != torch.int32
                       or not idx.is_contiguous() or not cnt.is_contiguous() or idx.device != device
                       or cnt.device != device):
        raise ValueError(f"{what}: idx / cnt must be contiguous int32 [B,H,nq_img,n_blocks] / [B,H,nq_img] on the device")
    return seqlens


def _out_f32(res, out):
    """a float32 residual (or out) selects the fp32 C / D form of the GEMMs (the Wan blocks' residual stream)"""
    return (res is not None and res.dtype == torch.float32) or (out is not None and out.dtype == torch.float32)


def _gemm_epilogue(what, x, M, N, dtype, bias, act, gate, res, out, stride_multiple=1):
    """The epilogue operands linear and linear_fp8 share -> (bias, gate32, res2d, res_row_stride, out, out2d, out_row_stride,
    act).  A float32 res or out selects the fp32 C / D form (OUT_F32 in `act`; res and out then both float32), otherwise both
    are `dtype`; out is allocated beside x if not given; a float32 bias stays float32 (BIAS_F32 in `act`), any other is cast to
    `dtype`; gate becomes fp32 [N].  stride_multiple: what the row strides of res and out must be a multiple of (the FP8
    kernel's vector stores: 8).  Which activations go with which operands is the caller's rule."""
    out32 = _out_f32(res, out)
    odt = torch.float32 if out32 else dtype
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=odt, device=x.device)
    o2, Mo, No, ors = _rows2d(out)
    if Mo != M or No != N or out.dtype != odt or ors % stride_multiple:
        raise ValueError(f"{what}: out must be [..., N] with as many rows as the input, float32 when the residual is float32"
                         + (f", row stride a multiple of {stride_multiple}" if stride_multiple > 1 else ""))
    r2, rrs = None, 0
    if res is not None:
        r2, Mr, Nr, rrs = _rows2d(res)
        if Mr != M or Nr != N or res.dtype != odt or rrs % stride_multiple:
            raise ValueError(f"{what}: res must match out")
    act = int(act) | (OUT_F32 if out32 else 0)
    if bias is not None:
        bias32 = bias.dtype == torch.float32     # (the gated bias of proj / fc2 / linear2: kept unrounded)
        act |= BIAS_F32 if bias32 else 0
        bias = bias.reshape(-1).contiguous() if bias32 else bias.reshape(-1).to(dtype=dtype).contiguous()
        if bias.numel() != N:
            raise ValueError(f"{what}: bias must have N entries")
    g32 = None
    if gate is not None:
        g32 = gate.reshape(-1).to(dtype=torch.float32).contiguous()
        if g32.numel() != N:
            raise ValueError(f"{what}: gate must have N entries")
    return bias, g32, r2, rrs, out, o2, ors, act


# ------------------------------------------------------------------------------------------------ geometry
def gilbert_map(t, h, w, sliced, device):
    n = t * h * w
    l2h = torch.empty(n, dtype=torch.int64, device=device)
    h2l = torch.empty(n, dtype=torch.int64, device=device)
    _need_gpu(l2h, "gilbert_map")
    _launch("jenga_gilbert_map", l2h.device, t, h, w, int(bool(sliced)), _p(l2h), _p(h2l))
    return l2h, h2l


def gilbert_neighbors(t, h, w, block, l2h):
    _need_gpu(l2h, "gilbert_neighbors")
    n = t * h * w
    nb = (n + block - 1) // block
    out = torch.zeros((nb, nb), dtype=torch.uint8, device=l2h.device)
    _launch("jenga_gilbert_neighbors", l2h.device, t, h, w, block, _p(l2h), _p(out))
    return out.view(torch.bool)


# ------------------------------------------------------------------------------------------------ row ops
def gather_rows(src, index, out=None):
    """src [B, N, C] contiguous rows; index int64 [M] on the same device -> out [B, M, C] = src[:, index]."""
    _need_gpu(src, "gather_rows")
    if src.dim() != 3 or not src.is_contiguous():
        raise ValueError("gather_rows expects a contiguous [B, N, C] tensor")
    if index.dtype != torch.int64 or index.device != src.device:
        raise ValueError("index must be an int64 tensor on the same device")
    B, N, C = src.shape
    M = index.numel()
    if out is None:
        out = torch.empty((B, M, C), dtype=src.dtype, device=src.device)
    rb = C * src.element_size()
    _launch("jenga_gather_rows", src.device, _p(src), _p(out), _p(index), B, M, rb, N * rb, M * rb)
    return out


def rmsnorm_rope(x, weight, cos, sin, s_rope=None, eps=1e-6, out=None):
    """x [B,S,H,128] (any B/S/H strides); weight [128] or None; cos/sin fp32 [>=s_rope,128] or None."""
    _need_gpu(x, "rmsnorm_rope")
    if x.shape[-1] != 128:
        raise ValueError("head_dim must be 128")
    B, S, H, _ = x.shape
    if out is None:
        out = torch.empty((B, S, H, 128), dtype=x.dtype, device=x.device)
    xs, os_ = _bshd_strides(x), _bshd_strides(out)
    weight = _norm_weight(weight, x)
    cos, sin, s_rope = _rope_tables(cos, sin, s_rope, S)
    _launch("jenga_rmsnorm_rope", x.device, _p(x), _p(out), _p(weight), _p(cos), _p(sin), B, S, H, *xs, *os_, s_rope,
            float(eps), dtype_code(x.dtype))
    return out


def qk_norm_rope_pool(xq, xk, wq, wk, cos, sin, out_q, out_k, s_rope=None, qpool=None, kpool=None, pool_block0=0,
                      eps=1e-6):
    """Fused per-head RMSNorm + RoPE of Q and K (+ 128-token block means of the results).
    xq, xk [B,S,H,128] with the SAME strides (the q / k slices of one QKV GEMM output), S a multiple of 128;
    out_q, out_k [B,S,H,128] with the same strides as each other; qpool [B,H,nq,128] / kpool [B,H,nk,128] receive the
    means of blocks pool_block0 .. pool_block0 + S/128 - 1 (where inside the pooled tensor)."""
    _need_gpu(xq, "qk_norm_rope_pool")
    B, S, H, D = xq.shape
    if D != 128 or S % 128 or xk.shape != xq.shape or out_q.shape != xq.shape or out_k.shape != xq.shape:
        raise ValueError("qk_norm_rope_pool: q / k / outputs must be [B, n*128, H, 128] of one shape")
    if _bshd_strides(xq) != _bshd_strides(xk) or _bshd_strides(out_q) != _bshd_strides(out_k):
        raise ValueError("qk_norm_rope_pool: q and k (and their outputs) must share their strides")
    if H > 64:
        raise ValueError("qk_norm_rope_pool: at most 64 heads")
    wq, wk = _norm_weight(wq, xq), _norm_weight(wk, xq)
    cos, sin, s_rope = _rope_tables(cos, sin, s_rope, S)
    nq = _pool_blocks(qpool, "qpool", B, H, xq.dtype)
    nk = _pool_blocks(kpool, "kpool", B, H, xq.dtype)
    _launch("jenga_qk_norm_rope_pool", xq.device, _p(xq), _p(xk), _p(out_q), _p(out_k), _p(wq), _p(wk), _p(cos), _p(sin),
            _p(qpool), _p(kpool), B, S // 128, H, *_bshd_strides(xq), *_bshd_strides(out_q), int(s_rope), int(pool_block0),
            nq, nk, float(eps), dtype_code(xq.dtype))
    return out_q, out_k


def sp_qkv_prologue(xq, xk, xv, wq, wk, cos, sin, out_q, out_k, out_v, heads_per_peer, head0=0, n_heads=None,
                    s_rope=None, eps=1e-6):
    """Sequence-parallel prologue: per-head RMSNorm + RoPE of Q and K and the Ulysses head scatter of Q, K, V in one
    launch.  xq, xk, xv [B,S,H,128] with the SAME strides (any S).  Outputs, all of one shape and stride set:
      peer-major send buffers [N,B,S,H/N,128] (head0 = 0, all heads; contiguous or any 16-byte-aligned strides), or
      [B,S,n_heads,128] views (any strides) receiving the head window [head0, head0 + n_heads) -- a rank's own slice
      of the replicated text rows, written in place behind the gathered image rows.
    Either (xq, xk, out_q, out_k) or (xv, out_v) may be None: the blocks run the Q|K and the V GEMM separately and post
    the Q, K exchange before the V GEMM (exchange / compute overlap)."""
    has_qk, has_v = xq is not None, xv is not None
    if not (has_qk or has_v) or (has_qk and (xk is None or out_q is None or out_k is None)) \
            or (not has_qk and xk is not None) or (has_v and out_v is None):
        raise ValueError("sp_qkv_prologue: pass (xq, xk, out_q, out_k) and / or (xv, out_v)")
    xs = [t for t in (xq, xk, xv) if t is not None]
    outs = ([out_q, out_k] if has_qk else []) + ([out_v] if has_v else [])
    x0, o0 = xs[0], outs[0]
    _need_gpu(x0, "sp_qkv_prologue")
    B, S, H, D = x0.shape
    if D != 128 or any(t.shape != x0.shape for t in xs):
        raise ValueError("sp_qkv_prologue: q / k / v must be [B, S, H, 128] of one shape")
    if any(_bshd_strides(t) != _bshd_strides(x0) for t in xs):
        raise ValueError("sp_qkv_prologue: q, k and v must share their strides")
    if n_heads is None:
        n_heads = H - head0
    Hn = int(heads_per_peer)
    if o0.dim() == 5:
        N = o0.shape[0]
        if head0 != 0 or n_heads != H or tuple(o0.shape) != (N, B, S, Hn, 128) or N * Hn != H \
                or o0.stride(4) != 1 or any(st % 8 for st in o0.stride()[:4]):
            raise ValueError("sp_qkv_prologue: peer-major outputs must be [N, B, S, H/N, 128] (unit inner stride; the "
                             "other strides multiples of 8 elements: contiguous, or the head-group-major view of the "
                             "pipelined sequence-parallel call)")
        o_sp, o_sb, o_ss, o_sh = o0.stride(0), o0.stride(1), o0.stride(2), o0.stride(3)
    else:
        if tuple(o0.shape) != (B, S, n_heads, 128) or n_heads > Hn or head0 % Hn + n_heads > Hn:
            raise ValueError("sp_qkv_prologue: head-window outputs must be [B, S, n_heads, 128] inside one peer's heads")
        o_sp = 0
        o_sb, o_ss, o_sh = _bshd_strides(o0)
        if head0 % Hn:      # the kernel writes head h at local index h % Hn: shift the base so that head0 lands on 0
            raise ValueError("sp_qkv_prologue: head0 must be a multiple of heads_per_peer")
    for t in outs:
        if t.shape != o0.shape or t.stride() != o0.stride() or t.dtype != x0.dtype:
            raise ValueError("sp_qkv_prologue: the outputs must share shape, strides and dtype")
    wq, wk = _norm_weight(wq, x0), _norm_weight(wk, x0)
    cos, sin, s_rope = _rope_tables(cos, sin, s_rope, S)
    _launch("jenga_sp_qkv_prologue", x0.device, _p(xq), _p(xk), _p(xv), _p(out_q), _p(out_k), _p(out_v), _p(wq), _p(wk),
            _p(cos), _p(sin), B, S, H, int(head0), int(n_heads), Hn, *_bshd_strides(x0), int(o_sp), int(o_sb), int(o_ss),
            int(o_sh), int(s_rope), float(eps), dtype_code(x0.dtype))
    return out_q, out_k, out_v


def stream_delay(microseconds, stream=None, device=None):
    """Measurement aid (bench.py --simulate-ranks): keep `stream` (default: the current one) busy for that long."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with _on(dev):
        _check(lib().jenga_stream_delay(ctypes.c_void_p(st.cuda_stream), float(microseconds)), "jenga_stream_delay")


def rmsnorm_rows(x, weight, eps):
    """WanRMSNorm: x [..., C] (bf16/fp16, last dim contiguous), weight [C] fp32 or x.dtype -> x.dtype*weight.dtype."""
    _need_gpu(x, "rmsnorm_rows")
    C = x.shape[-1]
    x2 = x.reshape(-1, C)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    w32 = weight.dtype == torch.float32
    w = weight.to(device=x.device).contiguous() if w32 else weight.to(device=x.device, dtype=x.dtype).contiguous()
    out = torch.empty(x2.shape, dtype=torch.float32 if w32 else x.dtype, device=x.device)
    _launch("jenga_rmsnorm_rows", x.device, _p(x2), _p(out), _p(w), x2.shape[0], C, x2.stride(0), out.stride(0), float(eps),
            dtype_code(x.dtype), int(w32))
    return out.reshape(x.shape)


def rope_complex(x, cos64, sin64, s_rope, out_dtype=torch.float32):
    """x [B,S,H,128] (bf16/fp16/fp32); cos64/sin64 float64 [>=s_rope, 64] -> fp32 (rope_apply's result) or bf16."""
    _need_gpu(x, "rope_complex")
    B, S, H, D = x.shape
    if D != 128 or cos64.dtype != torch.float64 or cos64.shape[-1] != 64 or cos64.shape[0] < s_rope:
        raise ValueError("rope_complex: head_dim 128 and float64 [S,64] tables required")
    codes = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
    if x.dtype not in codes or out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("rope_complex: unsupported dtype")
    if x.stride(-1) != 1:
        x = x.contiguous()
    out = torch.empty((B, S, H, D), dtype=out_dtype, device=x.device)
    _launch("jenga_rope_complex", x.device, _p(x), _p(out), _p(cos64.contiguous()), _p(sin64.contiguous()), B, S, H,
            *_bshd_strides(x), *_bshd_strides(out), int(s_rope), codes[x.dtype], codes[out_dtype])
    return out


def wan_norm_rope(x, weight, cos64, sin64, s_rope, eps, out=None):
    """Wan q / k prologue in one pass: x [..., C] (bf16/fp16, uniform row stride) -> bf16 [..., C] = bf16( rope64(
    round(x * rsqrt(mean x^2 + eps)) * weight_fp32 ) ); cos64/sin64 float64 [>= s_rope, 64] or None (norm + cast only).
    `out` may be the first rows of a larger (block-padded) buffer."""
    _need_gpu(x, "wan_norm_rope")
    C = x.shape[-1]
    if cos64 is not None and x.dim() > 2 and x.shape[:-2].numel() != 1:
        # the kernel takes the flattened ROW index as the RoPE position: with a batch > 1 only the first s_rope rows would
        # be rotated, each at the wrong position (the WanSelfAttention call site runs batch 1)
        raise ValueError("wan_norm_rope: with RoPE tables the input must be one sequence ([S, C] or [1, S, C])")
    x2 = x.reshape(-1, C)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    rows = x2.shape[0]
    w = weight.to(device=x.device, dtype=torch.float32).contiguous()
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (C,), dtype=torch.bfloat16, device=x.device)
    o2 = out.reshape(-1, C) if out.is_contiguous() else out
    if o2.dim() != 2 or o2.shape[0] < rows or o2.stride(1) != 1 or out.dtype != torch.bfloat16:
        raise ValueError("wan_norm_rope: out must be bf16 [>= rows, C] with contiguous channels")
    if cos64 is not None:
        if cos64.dtype != torch.float64 or sin64.dtype != torch.float64 or cos64.shape[-1] != 64 or cos64.shape[0] < s_rope:
            raise ValueError("wan_norm_rope: float64 [S,64] tables required")
        cos64, sin64 = cos64.contiguous(), sin64.contiguous()
    else:
        s_rope = 0
    _launch("jenga_wan_norm_rope", x.device, _p(x2), _p(o2), _p(w), _p(cos64), _p(sin64), rows, C, x2.stride(0), o2.stride(0),
            int(s_rope), float(eps), dtype_code(x.dtype))
    return out


def _rows2d(t):
    """[..., C] with unit inner stride and a single uniform row stride -> (rows, C, row_stride)."""
    C = t.shape[-1]
    t2 = t.reshape(-1, C) if t.is_contiguous() else t
    if t2.dim() == 3 and t2.shape[0] == 1:
        t2 = t2[0]
    if t2.dim() != 2 or t2.stride(1) != 1:
        raise ValueError("expected a [rows, C] (or [1, rows, C]) tensor with contiguous channels")
    return t2, t2.shape[0], C, t2.stride(0)


def ln_modulate(x, shift, scale, eps=1e-6, shift2=None, scale2=None, mask=None, out=None):
    """x [1,S,C]; shift/scale [1,C] or [C] -> LayerNorm(x)*(1+scale)+shift; rows with mask use (shift2, scale2)."""
    _need_gpu(x, "ln_modulate")
    x2, rows, C, xrs = _rows2d(x)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    o2, _, _, ors = _rows2d(out)
    dt = x.dtype
    sh, sc, sh2, sc2 = _flat(shift, dt), _flat(scale, dt), _flat(shift2, dt), _flat(scale2, dt)
    m = None if mask is None else mask.to(torch.uint8).contiguous()
    _launch("jenga_ln_modulate", x.device, _p(x2), _p(o2), _p(sh), _p(sc), _p(sh2), _p(sc2), _p(m), rows, C, xrs, ors,
            float(eps), dtype_code(x.dtype))
    return out


def gate_residual(res, y, gate, gate2=None, mask=None, out=None):
    """res + y * gate (per-channel gate [1,C]); rows with mask use gate2."""
    _need_gpu(res, "gate_residual")
    r2, rows, C, rrs = _rows2d(res)
    y2, _, _, yrs = _rows2d(y)
    if out is None:
        out = torch.empty(res.shape, dtype=res.dtype, device=res.device)
    o2, _, _, ors = _rows2d(out)
    g = gate.reshape(-1).to(dtype=res.dtype).contiguous()
    g2 = _flat(gate2, res.dtype)
    m = None if mask is None else mask.to(torch.uint8).contiguous()
    _launch("jenga_gate_residual", res.device, _p(r2), _p(y2), _p(g), _p(g2), _p(m), _p(o2), rows, C, rrs, yrs, ors,
            dtype_code(res.dtype))
    return out


def gelu_tanh(x, out=None):
    """tanh-GELU; x / out may be strided views (uniform row stride, contiguous channels)."""
    _need_gpu(x, "gelu_tanh")
    x2, rows, C, xrs = _rows2d(x)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    o2, _, _, ors = _rows2d(out)
    _launch("jenga_gelu_tanh", x.device, _p(x2), _p(o2), rows, C, xrs, ors, dtype_code(x.dtype))
    return out


ACT_NONE, ACT_GELU_TANH = 0, 1
BIAS_F32 = 256     # OR-ed into jenga_linear's `act`: the bias vector is float32
OUT_F32 = 512      # OR-ed into jenga_linear's `act`: res and out are float32
_GEMM_WORKSPACE = collections.OrderedDict()
_GEMM_WORKSPACE_MAX = 8         # scratch buffers kept per process (64 MiB each), least recently used evicted


def _gemm_workspace(device):
    """One 64 MiB scratch buffer per (device, stream): two jenga_linear calls in flight on different streams (the
    sequence-parallel blocks issue GEMMs beside the exchange stream) must not share split-K scratch.  Bounded: at most
    _GEMM_WORKSPACE_MAX buffers are kept (threads simulating ranks, short-lived side streams); an evicted buffer goes back
    to torch's caching allocator, which hands it out again in stream order of the stream it was allocated on -- the stream
    that used it -- so a GEMM still in flight on it is not disturbed."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    buf = _GEMM_WORKSPACE.get(key)
    if buf is None:
        buf = _GEMM_WORKSPACE[key] = torch.empty(64 << 20, dtype=torch.uint8, device=device)
        while len(_GEMM_WORKSPACE) > _GEMM_WORKSPACE_MAX:
            _GEMM_WORKSPACE.popitem(last=False)
    else:
        _GEMM_WORKSPACE.move_to_end(key)
    return buf


def linear_export_choices():
    """The current device's jenga_linear algorithm choices as an int64 tensor [n, 12] (CPU)."""
    n = int(lib().jenga_linear_export_choices(None, 0))
    rec = torch.zeros((max(n, 1), 12), dtype=torch.int64)
    n2 = int(lib().jenga_linear_export_choices(ctypes.c_void_p(rec.data_ptr()), n))
    return rec[: min(n, n2)]


def linear_import_choices(records):
    """records int64 [n, 12] (linear_export_choices of the rank whose choices everybody adopts)."""
    rec = records.to(device="cpu", dtype=torch.int64).contiguous()
    if rec.dim() != 2 or rec.shape[1] != 12:
        raise ValueError("linear_import_choices: records must be int64 [n, 12]")
    _check(lib().jenga_linear_import_choices(ctypes.c_void_p(rec.data_ptr()), rec.shape[0]), "jenga_linear_import_choices")


def linear_import_mismatches():
    """Plans rebuilt from imported choices so far whose hipBLASLt solution index is not the exported one (0 = this rank runs
    the exporting rank's algorithms)."""
    return int(lib().jenga_linear_import_mismatches())


def linear(x, weight, bias=None, act=ACT_NONE, gate=None, res=None, out=None):
    """out = act(gate * (x @ weight.T) + bias + res) in ONE hipBLASLt call (jenga_linear): x [..., K] with a uniform
    row stride, weight [N, K] (nn.Linear layout), bias [N] (added as given; a float32 bias is passed on as float32), gate [N] or [1, N] (per-channel; the
    caller folds it into the bias), res / out [..., N] (may be strided views: the MLP half of the single-stream blocks'
    concat buffer).  fp32 accumulation, one rounding."""
    _need_gpu(x, "linear")
    x2, M, K, xrs = _rows2d(x)
    N = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != K or weight.stride(1) != 1 or weight.dtype != x.dtype:
        raise ValueError("linear: weight must be [N, K] in the input dtype with contiguous rows")
    if int(act) & 0xff and _out_f32(res, out):      # (with a 16-bit gate / res the C entry decides)
        raise ValueError("linear: the float32 residual form has no activation epilogue")
    bias, g32, r2, rrs, out, o2, ors, act = _gemm_epilogue("linear", x, M, N, x.dtype, bias, act, gate, res, out)
    ws = _gemm_workspace(x.device)
    _launch("jenga_linear", x.device, _p(x2), _p(weight), _p(bias), _p(r2), _p(g32), _p(o2), M, N, K, xrs, weight.stride(0),
            rrs, ors, act, _p(ws), ws.numel(), dtype_code(x.dtype))
    return out


def quant_fp8_rows(x, out=None):
    """x [..., K] (bf16 / fp16, uniform row stride, K a multiple of 16) -> (x8 uint8 [..., K] of e4m3fn bytes, scale fp32
    [rows]): per row s = max(amax |x|, 1e-30) / 448, x8 = e4m3fn(x / s) (csrc/gemm8.hip).  out: a uint8 [..., K] destination
    (may be a row-strided view).  Serves activations (a scale per token) and weights [N, K] (a scale per output channel)."""
    x2, rows, K, xrs = _rows2d(x)
    if rows < 1 or K % 16 or xrs % 8:
        raise ValueError("quant_fp8_rows: x must have at least one row, K a multiple of 16 and a row stride multiple of 8")
    _need_gpu(x, "quant_fp8_rows")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    o2, ro, Ko, ors = _rows2d(out)
    if out.dtype != torch.uint8 or ro != rows or Ko != K or ors % 16 or out.device != x.device:
        raise ValueError("quant_fp8_rows: out must be uint8 [..., K] on x's device with a row stride multiple of 16")
    scale = torch.empty(rows, dtype=torch.float32, device=x.device)
    _launch("jenga_quant_fp8_rows", x.device, _p(x2), _p(o2), _p(scale), rows, K, xrs, ors, dtype_code(x.dtype))
    return out, scale


def linear_fp8(x8, x_scale, w8, w_scale, bias=None, act=ACT_NONE, gate=None, res=None, out=None, dtype=torch.bfloat16):
    """linear() on e4m3fn operands (jenga_linear_fp8, csrc/gemm8.hip): out = act(gate * (x_scale[m] * w_scale[n] * (x8 @ w8.T))
    + bias + res).  x8 uint8 [..., K] and x_scale fp32 [rows], w8 uint8 [N, K] and w_scale fp32 [N] from quant_fp8_rows; K a
    multiple of 128, N of 8.  bias / gate / res / out as for linear(): a float32 bias is passed on as float32, a float32 res or
    out selects the fp32 form, res / out may be strided views.  dtype: the 16-bit type of bias, res and out."""
    x2, M, K, xrs = _rows2d(x8)
    if x8.dtype != torch.uint8 or w8.dtype != torch.uint8 or w8.dim() != 2 or w8.shape[1] != K or w8.stride(1) != 1:
        raise ValueError("linear_fp8: x8 must be uint8 [..., K] and w8 uint8 [N, K] with contiguous rows")
    N = w8.shape[0]
    if M < 1 or K % 128 or N % 8 or xrs % 16 or w8.stride(0) % 16:
        raise ValueError("linear_fp8: M >= 1, K a multiple of 128, N a multiple of 8, row strides of x8 / w8 multiples of 16")
    for s_, n_, what in ((x_scale, M, "x_scale"), (w_scale, N, "w_scale")):
        if s_.dtype != torch.float32 or s_.dim() != 1 or s_.numel() != n_ or not s_.is_contiguous() or s_.device != x8.device:
            raise ValueError(f"linear_fp8: {what} must be a contiguous float32 vector with one entry per row")
    code = dtype_code(dtype)
    if int(act) & 0xff and (gate is not None or res is not None or _out_f32(res, out)):
        raise ValueError("linear_fp8: the activation epilogue cannot be combined with gate / residual / float32 output")
    _need_gpu(x8, "linear_fp8")
    _need_gpu(w8, "linear_fp8")
    bias, g32, r2, rrs, out, o2, ors, act = _gemm_epilogue("linear_fp8", x8, M, N, dtype, bias, act, gate, res, out,
                                                           stride_multiple=8)
    _launch("jenga_linear_fp8", x8.device, _p(x2), _p(x_scale), _p(w8), _p(w_scale), _p(bias), _p(r2), _p(g32), _p(o2), M, N,
            K, xrs, w8.stride(0), rrs, ors, act, code)
    return out


def wan_ln_modulate(x, weight=None, bias=None, shift=None, scale=None, eps=1e-6, out_dtype=torch.bfloat16,
                    round_ln=False):
    """Wan block glue: x fp32 [1,S,C] -> out_dtype( LN(x) [*weight+bias] [*(1+scale)+shift] ), vectors fp32 [C]."""
    _need_gpu(x, "wan_ln_modulate")
    if x.dtype != torch.float32:
        raise ValueError("wan_ln_modulate: the Wan residual stream is float32")
    x2, rows, C, xrs = _rows2d(x)
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    o2, _, _, ors = _rows2d(out)
    f32 = torch.float32
    w, b, sh, sc = _flat(weight, f32), _flat(bias, f32), _flat(shift, f32), _flat(scale, f32)
    _launch("jenga_wan_ln_modulate", x.device, _p(x2), _p(o2), _p(w), _p(b), _p(sh), _p(sc), rows, C, xrs, ors, float(eps),
            dtype_code(out_dtype), int(bool(round_ln)))
    return out


def wan_gate_residual(x, y, gate=None, out=None):
    """x fp32 + float(y) [* gate] -> fp32; out=x updates the residual stream in place."""
    _need_gpu(x, "wan_gate_residual")
    if x.dtype != torch.float32:
        raise ValueError("wan_gate_residual: the Wan residual stream is float32")
    x2, rows, C, xrs = _rows2d(x)
    y2, _, _, yrs = _rows2d(y)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    o2, _, _, ors = _rows2d(out)
    g = _flat(gate, torch.float32)
    _launch("jenga_wan_gate_residual", x.device, _p(x2), _p(y2), _p(g), _p(o2), rows, C, xrs, yrs, ors, dtype_code(y.dtype))
    return out


def block_pool(x, n_blocks):
    """x [B,S,H,128] -> [B,H,n_blocks,128] means over 128-token blocks."""
    _need_gpu(x, "block_pool")
    B, S, H, D = x.shape
    if D != 128 or n_blocks * 128 > S:
        raise ValueError("block_pool: head_dim must be 128 and n_blocks*128 <= S")
    out = torch.empty((B, H, n_blocks, 128), dtype=x.dtype, device=x.device)
    _launch("jenga_block_pool", x.device, _p(x), _p(out), B, H, n_blocks, *_bshd_strides(x), dtype_code(x.dtype))
    return out


def block_select(qpool, kpool, neighbors, nk_img, text_blocks, top_k, p, first_frame_blocks=0, want_mask=False,
                 want_lists=True, flags=None, head_dim=128):
    """-> (mask uint8 [B,H,nq,nk_all] | None, idx int32 [B,H,nq,nk_all] | None, cnt int32 [B,H,nq] | None).
    flags: SELECT_DEVICE_SCAN = the kept-count rule with torch's DEVICE cumsum semantics (default: CPU semantics, or
    the JENGA_SELECT_FLAGS environment variable).  head_dim in (16, 32, 64): the pooled rows are zero-padded to 128
    channels and the scores are scaled by head_dim ** -0.5 (JENGA_SELECT_HEAD_DIM)."""
    _need_gpu(qpool, "block_select")
    if head_dim not in (16, 32, 64, 128):
        raise ValueError(f"block_select: head_dim must be 16, 32, 64 or 128 (got {head_dim})")
    B, H, nq, _ = qpool.shape
    nk_all = nk_img + text_blocks
    if kpool.shape != (B, H, nk_all, 128):
        raise ValueError(f"kpool shape {tuple(kpool.shape)} != {(B, H, nk_all, 128)}")
    dev = qpool.device
    mask = torch.empty((B, H, nq, nk_all), dtype=torch.uint8, device=dev) if want_mask else None
    idx = torch.empty((B, H, nq, nk_all), dtype=torch.int32, device=dev) if want_lists else None
    cnt = torch.empty((B, H, nq), dtype=torch.int32, device=dev) if want_lists else None
    nbr, nbc = 0, 0
    if neighbors is not None:
        if neighbors.dtype == torch.bool:
            neighbors = neighbors.view(torch.uint8)
        neighbors = neighbors.to(dev).contiguous()
        nbr, nbc = neighbors.shape
    _launch("jenga_block_select", dev, _p(qpool.contiguous()), _p(kpool.contiguous()), _p(neighbors), nbr, nbc, _p(mask),
            _p(idx), _p(cnt), B, H, nq, nk_img, text_blocks, int(top_k), float(p), int(first_frame_blocks),
            dtype_code(qpool.dtype),
            int(SELECT_DEFAULT_FLAGS if flags is None else flags) | (0 if head_dim == 128 else (head_dim << 8)))
    return mask, idx, cnt


def pack_v(v, n_blocks=None, out=None, dst_block0=0, dst_blocks_total=None):
    """v [B,S,H,128] -> opaque re-tiled workspace [B,H,2*blocks_total,128,64] for bsattn_fwd.
    With out/dst_block0/dst_blocks_total a part (e.g. image or text V) fills its slice of a shared workspace."""
    _need_gpu(v, "pack_v")
    B, S, H, D = v.shape
    if n_blocks is None:
        n_blocks = S // 128
    if D != 128 or n_blocks * 128 != S:
        raise ValueError("pack_v: S must equal n_blocks*128 and head_dim 128")
    if dst_blocks_total is None:
        dst_blocks_total = n_blocks if out is None else out.shape[2] // 2
    if out is None:
        out = torch.empty((B, H, dst_blocks_total * 2, 128, 64), dtype=v.dtype, device=v.device)
    _launch("jenga_pack_v", v.device, _p(v), _p(out), B, H, n_blocks, *_bshd_strides(v), dst_block0, dst_blocks_total,
            dtype_code(v.dtype))
    return out


def bsattn_fwd(q, k, vt, seqlens, idx, cnt, nq_img, sm_scale, text_amp, text_block_start, out=None, xcd_remap=True,
               flags=None, order=None):
    """q,k [B,S,H,128]; vt from pack_v; seqlens int32 [B] device; idx/cnt from block_select -> o [B,S,H,128].
    order: optional launch-order hint (order_by_count); flags & ATTN_SORTED builds it from cnt."""
    _need_gpu(q, "bsattn_fwd")
    B, S, H, D = q.shape
    if D != 128 or S % 128:
        raise ValueError("bsattn_fwd: head_dim must be 128 and S a multiple of 128")
    n_blocks = S // 128
    if out is None:
        out = torch.empty((B, S, H, 128), dtype=q.dtype, device=q.device)
    if idx is not None and idx.shape[-1] != n_blocks:       # (also without image query blocks, where nothing reads idx)
        raise ValueError("idx row length must equal the number of kv blocks")
    seqlens = _attn_lists("bsattn_fwd", q.device, B, H, n_blocks, nq_img, seqlens, idx, cnt)
    if k.shape != q.shape or out.shape != q.shape:
        raise ValueError("bsattn_fwd: q, k and out must have the same [B,S,H,128] shape")
    if tuple(vt.shape) != (B, H, 2 * n_blocks, 128, 64) or not vt.is_contiguous() or vt.dtype != q.dtype:
        raise ValueError(f"bsattn_fwd: vt must be the contiguous pack_v workspace {(B, H, 2 * n_blocks, 128, 64)}")
    fl = ATTN_DEFAULT_FLAGS if flags is None else flags
    if not xcd_remap:
        fl &= ~ATTN_XCD_REMAP
    pair = bool(fl & ATTN_PAIR)
    if pair and order is not None:
        # `order` ranks query BLOCKS; the pair kernel launches block PAIRS in an order of its own (ATTN_SORTED) -- dropping a
        # caller's hint silently would misreport what ran
        raise ValueError("bsattn_fwd: a launch-order hint (order=) cannot be combined with the pair kernel (ATTN_PAIR)")
    prof = ATTN_PROFILE
    with _on(q.device):
        pidx = pcnt = order_t = None
        porder = None
        if pair and nq_img > 0:
            pidx, pcnt = pair_merge(idx, cnt, n_blocks)
            npair = pidx.shape[2]
            if (fl & ATTN_SORTED) and npair > 1:
                # work-aware launch order of the pairs inside every XCD's range: a shared block costs two 32-row items per
                # wave and tile, an unshared one one
                seg = (npair + 7) // 8 if ((fl & ATTN_XCD_REMAP) and npair >= 64) else npair
                if seg <= 2048:
                    work = (2 * pcnt[..., 0] + pcnt[..., 1] + pcnt[..., 2]).contiguous()
                    porder = order_by_count(work, seg)
        if order is not None:
            order_t = order
        elif (fl & ATTN_SORTED) and nq_img > 0 and (fl & ATTN_LP) and not pair:
            seg = (nq_img + 7) // 8 if ((fl & ATTN_XCD_REMAP) and nq_img >= 64) else nq_img
            if seg <= 2048:      # (jenga_order_by_count ranks one segment per workgroup; beyond that: plain order)
                order_t = order_by_count(cnt, seg)
        if order_t is not None and (tuple(order_t.shape) != (B, H, nq_img) or order_t.dtype != torch.int32
                                    or not order_t.is_contiguous() or order_t.device != q.device):
            raise ValueError("bsattn_fwd: order must be a contiguous int32 [B,H,nq_img] tensor on the device")
        e0 = _profile_start() if prof is not None else None
        common = (B, H, n_blocks, nq_img, *_bshd_strides(q), *_bshd_strides(k), *_bshd_strides(out), float(sm_scale),
                  float(text_amp), int(text_block_start), dtype_code(q.dtype))
        cflags = fl & (ATTN_XCD_REMAP | ATTN_BALANCE | ATTN_LP)
        if not pair:
            _enqueue("jenga_bsattn_fwd", q.device, _p(q), _p(k), _p(vt), _p(out), _p(seqlens), _p(idx), _p(cnt), _p(order_t),
                     *common, cflags)
        else:
            _enqueue("jenga_bsattn_pair_fwd", q.device, _p(q), _p(k), _p(vt), _p(out), _p(seqlens), _p(pidx), _p(pcnt),
                     _p(porder), *common, cflags & ~ATTN_LP)
        if prof is not None:
            _profile_stop(prof, e0, B, H, n_blocks, nq_img, idx, cnt)
    return out


def quant_fp8_blocks(x, offset=None):
    """x [B,S,H,128] (bf16 / fp16, unit head_dim stride, S a multiple of 128) -> (x8 uint8 [B,S,H,128] of e4m3fn bytes, scale
    fp32 [B,H,S/128]): per (b, h, 128-token block) s = max(amax |x - offset|, 1e-30) / 448, x8 = e4m3fn((x - offset) / s)
    (csrc/qattn.hip).  offset: fp32 [B,H,128] or None (the K smoothing of block_sparse_attention(qk_dtype="fp8"))."""
    _need_gpu(x, "quant_fp8_blocks")
    if x.dim() != 4 or x.shape[3] != 128 or x.shape[1] % 128 or x.shape[1] == 0:
        raise ValueError("quant_fp8_blocks: x must be [B, n*128, H, 128]")
    B, S, H, _ = x.shape
    if offset is not None and (tuple(offset.shape) != (B, H, 128) or offset.dtype != torch.float32
                               or not offset.is_contiguous() or offset.device != x.device):
        raise ValueError("quant_fp8_blocks: offset must be a contiguous float32 [B,H,128] tensor on x's device")
    x8 = torch.empty((B, S, H, 128), dtype=torch.uint8, device=x.device)
    scale = torch.empty((B, H, S // 128), dtype=torch.float32, device=x.device)
    _launch("jenga_quant_fp8_blocks", x.device, _p(x), _p(x8), _p(scale), _p(offset), B, H, S // 128, *_bshd_strides(x),
            dtype_code(x.dtype))
    return x8, scale


def bsattn_fp8_fwd(q8, q_scale, k8, k_scale, vt, seqlens, idx, cnt, nq_img, sm_scale, text_amp, text_block_start, out=None,
                   xcd_remap=True):
    """bsattn_fwd with e4m3fn q and k: q8, k8 uint8 [B,S,H,128] and q_scale, k_scale fp32 [B,H,S/128] from quant_fp8_blocks; vt
    from pack_v (its dtype is the output's); seqlens / idx / cnt as for bsattn_fwd -> o [B,S,H,128] (csrc/qattn.hip)."""
    _need_gpu(q8, "bsattn_fp8_fwd")
    if q8.dim() != 4 or q8.shape[3] != 128 or q8.shape[1] % 128 or q8.dtype != torch.uint8 or k8.dtype != torch.uint8 \
            or k8.shape != q8.shape:
        raise ValueError("bsattn_fp8_fwd: q8 and k8 must be uint8 [B, n*128, H, 128] of one shape")
    B, S, H, _ = q8.shape
    n_blocks = S // 128
    for name, t in (("q_scale", q_scale), ("k_scale", k_scale)):
        if tuple(t.shape) != (B, H, n_blocks) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != q8.device:
            raise ValueError(f"bsattn_fp8_fwd: {name} must be a contiguous float32 [B,H,n_blocks] tensor on q8's device")
    if tuple(vt.shape) != (B, H, 2 * n_blocks, 128, 64) or not vt.is_contiguous() or vt.device != q8.device:
        raise ValueError(f"bsattn_fp8_fwd: vt must be the contiguous pack_v workspace {(B, H, 2 * n_blocks, 128, 64)}")
    dt = dtype_code(vt.dtype)
    if out is None:
        out = torch.empty((B, S, H, 128), dtype=vt.dtype, device=q8.device)
    elif out.shape != q8.shape or out.dtype != vt.dtype or out.device != q8.device:
        raise ValueError("bsattn_fp8_fwd: out must be [B,S,H,128] in vt's dtype")
    seqlens = _attn_lists("bsattn_fp8_fwd", q8.device, B, H, n_blocks, nq_img, seqlens, idx, cnt)
    prof = ATTN_PROFILE
    with _on(q8.device):
        e0 = _profile_start() if prof is not None else None
        _enqueue("jenga_bsattn_fp8_fwd", q8.device, _p(q8), _p(q_scale), _p(k8), _p(k_scale), _p(vt), _p(out), _p(seqlens),
                 _p(idx), _p(cnt), B, H, n_blocks, nq_img, *_bshd_strides(q8), *_bshd_strides(k8), *_bshd_strides(out),
                 float(sm_scale), float(text_amp), int(text_block_start), dt, ATTN_XCD_REMAP if xcd_remap else 0)
        if prof is not None:
            _profile_stop(prof, e0, B, H, n_blocks, nq_img, idx, cnt)
    return out


def block_pool_d64(x, n_blocks):
    """x [B,S,H,64] -> [B,H,n_blocks,128]: means over 128-token blocks in channels 0..63, zeros in 64..127 -- what block_pool
    gives for the zero-padded rows, bit for bit (csrc/bsattn64.hip); block_select(head_dim=64) takes it as it is."""
    _need_gpu(x, "block_pool_d64")
    if x.dim() != 4 or x.shape[3] != 64 or n_blocks * 128 > x.shape[1]:
        raise ValueError("block_pool_d64: x must be [B,S,H,64] with n_blocks*128 <= S")
    B, S, H, _ = x.shape
    out = torch.empty((B, H, n_blocks, 128), dtype=x.dtype, device=x.device)
    _launch("jenga_block_pool_d64", x.device, _p(x), _p(out), B, H, n_blocks, *_bshd_strides(x), dtype_code(x.dtype))
    return out


def bsattn_d64_fwd(q, k, v, seqlens, idx, cnt, nq_img, sm_scale, text_amp, text_block_start, out=None, xcd_remap=True):
    """bsattn_fwd for 64-channel heads: q, k, v [B,S,H,64] as they lie in memory (unit channel stride, no pack_v workspace),
    seqlens / idx / cnt as for bsattn_fwd -> o [B,S,H,64] (csrc/bsattn64.hip)."""
    _need_gpu(q, "bsattn_d64_fwd")
    if q.dim() != 4 or q.shape[3] != 64 or q.shape[1] % 128 or q.shape[1] == 0:
        raise ValueError("bsattn_d64_fwd: q must be [B, n*128, H, 64]")
    B, S, H, _ = q.shape
    n_blocks = S // 128
    if out is None:
        out = torch.empty((B, S, H, 64), dtype=q.dtype, device=q.device)
    for name, t in (("k", k), ("v", v), ("out", out)):
        if t.shape != q.shape or t.dtype != q.dtype or t.device != q.device:
            raise ValueError(f"bsattn_d64_fwd: {name} must have q's shape, dtype and device")
    seqlens = _attn_lists("bsattn_d64_fwd", q.device, B, H, n_blocks, nq_img, seqlens, idx, cnt)
    # (does not record into ATTN_PROFILE)
    _launch("jenga_bsattn_d64_fwd", q.device, _p(q), _p(k), _p(v), _p(out), _p(seqlens), _p(idx), _p(cnt), B, H, n_blocks,
            nq_img, *_bshd_strides(q), *_bshd_strides(k), *_bshd_strides(v), *_bshd_strides(out), float(sm_scale),
            float(text_amp), int(text_block_start), dtype_code(q.dtype), ATTN_XCD_REMAP if xcd_remap else 0)
    return out


def cross_attn_fwd(q, k, v, sm_scale=None, out=None, kv_len=None):
    """Dense cross-attention (WanT2VCrossAttention): q [B,Sq,H,128], k / v [B,Skv,H,128], Sq and Skv multiples of 128
    (pad the buffers; query rows are independent, keys >= kv_len are masked) -> o [B,Sq,H,128]."""
    _need_gpu(q, "cross_attn_fwd")
    B, Sq, H, D = q.shape
    Skv = k.shape[1]
    if D != 128 or Sq % 128 or Skv % 128 or Sq == 0 or Skv == 0 or tuple(k.shape) != (B, Skv, H, 128) \
            or v.shape != k.shape or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError("cross_attn_fwd: q [B,Sq,H,128], k / v [B,Skv,H,128] of one dtype, Sq and Skv multiples of 128")
    kv_len = Skv if kv_len is None else int(kv_len)
    if not (Skv - 128 < kv_len <= Skv):
        raise ValueError("cross_attn_fwd: kv_len must lie inside the last 128-key block of k / v")
    if out is None:
        out = torch.empty((B, Sq, H, 128), dtype=q.dtype, device=q.device)
    vt = pack_v(v, Skv // 128)
    _launch("jenga_cross_attn_fwd", q.device, _p(q), _p(k), _p(vt), _p(out), B, H, Sq // 128, Skv // 128, kv_len,
            *_bshd_strides(q), *_bshd_strides(k), *_bshd_strides(out), float(D ** -0.5 if sm_scale is None else sm_scale),
            dtype_code(q.dtype))
    return out


def dense_varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_kv=None, sm_scale=None, out=None):
    """Dense variable-length attention in one launch (csrc/dattn.hip; flash_attn_varlen_func, attenion.py:108-121): q [Tq,H,128],
    k / v [Tk,H,128] packed tokens (unit head_dim stride), cu_seqlens_* int32 [n+1] on q's device (kv defaults to q's).  Query rows
    of segment i attend to the keys of segment i; rows >= cu_seqlens_q[-1] and rows of a segment without keys come back as
    zeros.  Nothing is read back from the device: the call can be captured in a graph."""
    _need_gpu(q, "dense_varlen_fwd")
    if cu_seqlens_kv is None:
        cu_seqlens_kv = cu_seqlens_q
    if q.dim() != 3 or q.shape[2] != 128 or k.dim() != 3 or tuple(k.shape[1:]) != tuple(q.shape[1:]) or v.shape != k.shape \
            or k.dtype != q.dtype or v.dtype != q.dtype or q.shape[0] == 0:
        raise ValueError("dense_varlen_fwd: q [Tq,H,128], k / v [Tk,H,128] of one dtype, Tq >= 1")
    for name, c in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_kv", cu_seqlens_kv)):
        if c.dtype != torch.int32 or c.dim() != 1 or c.device != q.device or not c.is_contiguous():
            raise ValueError(f"dense_varlen_fwd: {name} must be a contiguous int32 vector on q's device (it is never read on "
                             "the host)")
    if cu_seqlens_kv.numel() != cu_seqlens_q.numel() or cu_seqlens_q.numel() < 2:
        raise ValueError("dense_varlen_fwd: cu_seqlens_q and cu_seqlens_kv must have the same length n + 1 >= 2")
    q, k, v = (t if t.stride(2) == 1 else t.contiguous() for t in (q, k, v))
    if out is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
    elif out.shape != q.shape or out.dtype != q.dtype or out.stride(2) != 1 or out.device != q.device:
        raise ValueError("dense_varlen_fwd: out must match q (unit head_dim stride)")
    Tq, H, D = q.shape
    _launch("jenga_dense_varlen_fwd", q.device, _p(q), _p(k), _p(v), _p(out), _p(cu_seqlens_q), _p(cu_seqlens_kv),
            cu_seqlens_q.numel() - 1, Tq, k.shape[0], H, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0),
            v.stride(1), out.stride(0), out.stride(1), float(D ** -0.5 if sm_scale is None else sm_scale),
            dtype_code(q.dtype))
    return out


def order_by_count(cnt, segment):
    """cnt int32 [B,H,nq] -> order int32 [B,H,nq]: inside every run of `segment` consecutive query blocks, the blocks by
    descending kept count (the launch-order hint of jenga_bsattn_fwd)."""
    _need_gpu(cnt, "order_by_count")
    if cnt.dim() != 3 or cnt.dtype != torch.int32 or not cnt.is_contiguous():
        raise ValueError("order_by_count: cnt must be a contiguous int32 [B,H,nq] tensor")
    B, H, nq = cnt.shape
    order = torch.empty_like(cnt)
    _launch("jenga_order_by_count", cnt.device, _p(cnt), B * H, nq, int(segment), _p(order))
    return order


def pair_merge(idx, cnt, n_blocks):
    """idx int32 [B,H,nq,n_blocks], cnt int32 [B,H,nq] (jenga_block_select) -> (pidx
    [B,H,ceil(nq/2),n_blocks], pcnt [B,H,ceil(nq/2),4]): per query-block pair the kv blocks both keep | only the even
    row | only the odd row."""
    _need_gpu(idx, "pair_merge")
    B, H, nq, nb = idx.shape
    if nb != n_blocks or tuple(cnt.shape) != (B, H, nq) or idx.dtype != torch.int32 or cnt.dtype != torch.int32:
        raise ValueError("pair_merge: idx / cnt must be int32 [B,H,nq,n_blocks] / [B,H,nq]")
    npair = (nq + 1) // 2
    pidx = torch.empty((B, H, npair, nb), dtype=torch.int32, device=idx.device)
    pcnt = torch.empty((B, H, npair, 4), dtype=torch.int32, device=idx.device)
    _launch("jenga_pair_merge", idx.device, _p(idx.contiguous()), _p(cnt.contiguous()), B, H, nq, nb, _p(pidx), _p(pcnt))
    return pidx, pcnt


def ulysses_pack_heads(x, n_ranks, out=None):
    """x [B,S_loc,H,128] -> [N,B,S_loc,H/N,128] (peer-major send buffer)."""
    _need_gpu(x, "ulysses_pack_heads")
    B, S, H, D = x.shape
    if out is None:
        out = torch.empty((n_ranks, B, S, H // n_ranks, D), dtype=x.dtype, device=x.device)
    _launch("jenga_ulysses_pack_heads", x.device, _p(x), _p(out), B, S, H, n_ranks, *_bshd_strides(x))
    return out


def ulysses_unpack_heads(recv, n_ranks, out=None):
    """recv [N,B,S_loc,H/N,128] -> [B,S_loc,H,128]."""
    _need_gpu(recv, "ulysses_unpack_heads")
    N, B, S, Hn, D = recv.shape
    if out is None:
        out = torch.empty((B, S, Hn * N, D), dtype=recv.dtype, device=recv.device)
    _launch("jenga_ulysses_unpack_heads", recv.device, _p(recv.contiguous()), _p(out), B, S, Hn * N, N, *_bshd_strides(out))
    return out
