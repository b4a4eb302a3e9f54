#!/usr/bin/env python3
"""Every jenga_amd._capi wrapper once on small seeded inputs -> one JSON of sha256 digests of every output tensor (GPU box).
A/B aid for changes to the binding layer: run it from two checkouts that load the same library and compare the files -- all
digests must be equal.  A few seconds.
  python tools/capi_ab.py OUT.json            python tools/capi_ab.py --compare A.json B.json"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jenga_amd import _capi  # noqa: E402

H = 2
F32, F64, I32 = torch.float32, torch.float64, torch.int32


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


class Run:
    def __init__(self, dev, seed):
        self.dev, self.out, self.g = dev, {}, torch.Generator().manual_seed(seed)

    def rnd(self, *shape, dtype=F32, scale=1.0):
        return (torch.randn(*shape, generator=self.g, dtype=F64) * scale).to(dtype).to(self.dev)

    def put(self, name, *tensors):
        assert name not in self.out, name
        for i, t in enumerate(tensors):
            if t is not None:
                self.out[name if len(tensors) == 1 else f"{name}.{i}"] = sha(t) if torch.is_tensor(t) else t


def rows(r, dt, tag):
    """the row kernels: one sequence of 128 rows x 256 channels, contiguous and as a strided view"""
    x, y = r.rnd(1, 128, 256, dtype=dt), r.rnd(1, 128, 256, dtype=dt)
    wide = r.rnd(1, 128, 512, dtype=dt)
    v = [r.rnd(1, 256, dtype=dt) for _ in range(4)]
    mask = (torch.arange(128, device=r.dev) % 3 == 0)
    r.put(f"ln_modulate/{tag}", _capi.ln_modulate(x, v[0], v[1]))
    r.put(f"ln_modulate_mask/{tag}", _capi.ln_modulate(x, v[0], v[1], shift2=v[2], scale2=v[3], mask=mask))
    r.put(f"gate_residual/{tag}", _capi.gate_residual(x, y, v[0]))
    r.put(f"gate_residual_mask/{tag}", _capi.gate_residual(x, y, v[0], gate2=v[1], mask=mask))
    r.put(f"gelu_tanh/{tag}", _capi.gelu_tanh(x))
    buf = torch.zeros(1, 128, 512, dtype=dt, device=r.dev)
    _capi.gelu_tanh(wide[..., :256], out=buf[..., 256:])
    r.put(f"gelu_tanh_strided/{tag}", buf)
    r.put(f"rmsnorm_rows_w32/{tag}", _capi.rmsnorm_rows(x, r.rnd(256), 1e-6))
    r.put(f"rmsnorm_rows_w16/{tag}", _capi.rmsnorm_rows(wide[..., :256], r.rnd(256, dtype=dt), 1e-6))
    perm = torch.randperm(128, generator=r.g).to(r.dev)
    r.put(f"gather_rows/{tag}", _capi.gather_rows(x, perm))
    x32 = r.rnd(1, 128, 256)
    f = [r.rnd(256) for _ in range(4)]
    r.put(f"wan_ln_modulate/{tag}", _capi.wan_ln_modulate(x32, shift=f[0], scale=f[1], out_dtype=dt))
    r.put(f"wan_ln_modulate_affine/{tag}", _capi.wan_ln_modulate(x32, weight=f[2], bias=f[3], out_dtype=dt, round_ln=True))
    r.put(f"wan_gate_residual/{tag}", _capi.wan_gate_residual(x32, y, f[0]))
    acc = x32.clone()
    _capi.wan_gate_residual(acc, y, None, out=acc)
    r.put(f"wan_gate_residual_inplace/{tag}", acc)
    ang = r.rnd(128, 64, dtype=F64)
    cos64, sin64 = ang.cos(), ang.sin()
    r.put(f"wan_norm_rope/{tag}", _capi.wan_norm_rope(x, f[0], cos64, sin64, 100, 1e-6))
    pad = torch.full((160, 256), 5.0, dtype=torch.bfloat16, device=r.dev)
    _capi.wan_norm_rope(wide[..., :256], f[0], None, None, 0, 1e-6, out=pad)
    r.put(f"wan_norm_rope_plain/{tag}", pad)
    x4 = x.view(1, 128, H, 128)
    r.put(f"rope_complex_f32/{tag}", _capi.rope_complex(x4, cos64, sin64, 100))
    r.put(f"rope_complex_bf16/{tag}", _capi.rope_complex(x32.view(1, 128, H, 128), cos64, sin64, 128, out_dtype=torch.bfloat16))


def attention(r, dt, S, nimg, tag):
    """norm + RoPE + pooling, selection and every attention entry at [1, S, 2, 128]: nimg image blocks, the rest text"""
    dev = r.dev
    nb = S // 128
    S_img = nimg * 128
    qkv = r.rnd(1, S, 3, H, 128, dtype=dt, scale=1.3)
    xq, xk, xv = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]                    # strided, as the QKV GEMM leaves them
    wq, wk = (1 + 0.1 * r.rnd(128)).to(dt), (1 + 0.1 * r.rnd(128)).to(dt)
    cos, sin = r.rnd(S_img, 128), r.rnd(S_img, 128)
    r.put(f"rmsnorm_rope/{tag}", _capi.rmsnorm_rope(xq, wq, cos, sin))
    r.put(f"rmsnorm_rope_plain/{tag}", _capi.rmsnorm_rope(xq, None, None, None))
    q, k = torch.empty(1, S, H, 128, dtype=dt, device=dev), torch.empty(1, S, H, 128, dtype=dt, device=dev)
    qp, kp = torch.zeros(1, H, nimg, 128, dtype=dt, device=dev), torch.zeros(1, H, nb, 128, dtype=dt, device=dev)
    _capi.qk_norm_rope_pool(xq, xk, wq, wk, cos, sin, q, k, s_rope=S_img, qpool=qp, kpool=kp)
    r.put(f"qk_norm_rope_pool/{tag}", q, k, qp, kp)
    q2, k2, kp2 = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(kp)
    _capi.qk_norm_rope_pool(xq[:, S_img:], xk[:, S_img:], None, None, None, None, q2[:, S_img:], k2[:, S_img:],
                            kpool=kp2, pool_block0=nimg)
    r.put(f"qk_norm_rope_pool_text/{tag}", q2, k2, kp2)
    r.put(f"block_pool/{tag}", _capi.block_pool(q, nimg), _capi.block_pool(k, nb))
    v = xv.contiguous()
    vt = _capi.pack_v(v, nb)
    r.put(f"pack_v/{tag}", vt)
    mask, idx, cnt = _capi.block_select(qp, kp, None, nimg, nb - nimg, 1, 0.5, want_mask=True)
    r.put(f"block_select/{tag}", mask, idx, cnt)
    seqlens = torch.tensor([S - 40], dtype=I32, device=dev)
    args = (seqlens, idx, cnt, nimg, 128 ** -0.5, 0.3, nimg)
    for name, fl in (("lp", _capi.ATTN_LP_FLAGS), ("pair", _capi.ATTN_PAIR_FLAGS), ("plain", _capi.ATTN_XCD_REMAP),
                     ("lp_static", _capi.ATTN_LP | _capi.ATTN_SORTED)):
        r.put(f"bsattn_fwd_{name}/{tag}", _capi.bsattn_fwd(q, k, vt, *args, flags=fl))
    order = _capi.order_by_count(cnt, nimg)
    r.put(f"order_by_count/{tag}", order)
    r.put(f"pair_merge/{tag}", *_capi.pair_merge(idx, cnt, nb))
    buf = torch.zeros(1, S, 2 * H, 128, dtype=dt, device=dev)
    _capi.bsattn_fwd(q, k, vt, *args, out=buf[:, :, H:], flags=_capi.ATTN_LP, order=order)
    r.put(f"bsattn_fwd_order_strided/{tag}", buf)
    r.put(f"bsattn_fwd_text_only/{tag}", _capi.bsattn_fwd(q, k, vt, None, None, None, 0, 128 ** -0.5, 0.0, nb))
    q8, qs = _capi.quant_fp8_blocks(q)
    k8, ks = _capi.quant_fp8_blocks(k, kp.float().mean(2))
    r.put(f"quant_fp8_blocks/{tag}", q8, qs, k8, ks)
    r.put(f"bsattn_fp8_fwd/{tag}", _capi.bsattn_fp8_fwd(q8, qs, k8, ks, vt, *args))
    _capi.ATTN_PROFILE = prof = _capi.AttnProfile()
    try:
        prof.tag = "ab"
        _capi.bsattn_fwd(q, k, vt, *args)
        _capi.bsattn_fp8_fwd(q8, qs, k8, ks, vt, *args)
        torch.cuda.synchronize()
        s = prof.summary()
    finally:
        _capi.ATTN_PROFILE = None
    r.put(f"attn_profile/{tag}", s["launches"], s["pairs"], s["by_tag"]["ab"]["pairs"], len(prof.events),
          s.get("adjacent_shared_frac", -1.0))
    q64, k64, v64 = (r.rnd(1, S, H, 64, dtype=dt) for _ in range(3))
    qp64, kp64 = _capi.block_pool_d64(q64, nimg), _capi.block_pool_d64(k64, nb)
    _, idx64, cnt64 = _capi.block_select(qp64, kp64, None, nimg, nb - nimg, 1, 0.5, head_dim=64)
    r.put(f"block_pool_d64/{tag}", qp64, kp64)
    r.put(f"bsattn_d64_fwd/{tag}", _capi.bsattn_d64_fwd(q64, k64, v64, seqlens, idx64, cnt64, nimg, 64 ** -0.5, 0.3, nimg))
    r.put(f"cross_attn_fwd/{tag}", _capi.cross_attn_fwd(q, k[:, :256], v[:, :256], kv_len=200))
    cu = torch.tensor([0, 100, S - 28], dtype=I32, device=dev)
    r.put(f"dense_varlen_fwd/{tag}", _capi.dense_varlen_fwd(q[0], k[0], v[0], cu))
    packed = _capi.ulysses_pack_heads(q, 2)
    r.put(f"ulysses/{tag}", packed, _capi.ulysses_unpack_heads(packed, 2))
    # sp_qkv_prologue: the peer-major layout (all three, then Q|K and V apart) and the head-window layout
    sends = [torch.zeros(2, 1, S_img, 1, 128, dtype=dt, device=dev) for _ in range(6)]
    img = [t[:, :S_img] for t in (xq, xk, xv)]
    _capi.sp_qkv_prologue(*img, wq, wk, cos, sin, *sends[:3], 1, s_rope=S_img)
    _capi.sp_qkv_prologue(img[0], img[1], None, wq, wk, cos, sin, sends[3], sends[4], None, 1)
    _capi.sp_qkv_prologue(None, None, img[2], None, None, None, None, None, None, sends[5], 1)
    r.put(f"sp_qkv_prologue_peer_major/{tag}", *sends)
    fulls = [torch.zeros(1, S, 1, 128, dtype=dt, device=dev) for _ in range(3)]
    _capi.sp_qkv_prologue(xq[:, S_img:], xk[:, S_img:], xv[:, S_img:], wq, wk, None, None, *(f[:, S_img:] for f in fulls), 1,
                          head0=1, n_heads=1)
    r.put(f"sp_qkv_prologue_head_window/{tag}", *fulls)


def linears(r, dt, tag):
    M, N, K = 128, 256, 256
    dev = r.dev
    x, w = r.rnd(M, K, dtype=dt), r.rnd(N, K, dtype=dt, scale=0.05)
    b, b32, gate = r.rnd(N, dtype=dt), r.rnd(N), r.rnd(1, N, dtype=dt)
    res, res32 = r.rnd(M, N, dtype=dt), r.rnd(M, N)
    wide = torch.zeros(M, 2 * N, dtype=dt, device=dev)
    _capi.linear(x, w, b, out=wide[:, N:])
    forms = {
        "plain": _capi.linear(x, w), "bias": _capi.linear(x, w, b), "bias32": _capi.linear(x, w, b32),
        "gelu": _capi.linear(x, w, b, act=_capi.ACT_GELU_TANH), "gate_res": _capi.linear(x, w, b32, gate=gate, res=res),
        "strided_out": wide, "res32": _capi.linear(x, w, b32, gate=gate, res=res32),
    }
    for name, t in forms.items():
        r.put(f"linear_{name}/{tag}", t)
    rec = _capi.linear_export_choices()
    _capi.linear_import_choices(rec)
    r.put(f"linear_choices/{tag}", rec, _capi.linear(x, w, b), _capi.linear_import_mismatches())
    K8 = 128
    x8, xs = _capi.quant_fp8_rows(r.rnd(M, K8, dtype=dt))
    w8, ws = _capi.quant_fp8_rows(r.rnd(N, K8, dtype=dt, scale=0.05))
    q8buf = torch.zeros(M, 2 * K8, dtype=torch.uint8, device=dev)
    _capi.quant_fp8_rows(r.rnd(M, K8, dtype=dt), out=q8buf[:, K8:])
    r.put(f"quant_fp8_rows/{tag}", x8, xs, w8, ws, q8buf)
    wide8 = torch.zeros(M, 2 * N, dtype=dt, device=dev)
    _capi.linear_fp8(x8, xs, w8, ws, b, out=wide8[:, N:], dtype=dt)
    forms8 = {
        "plain": _capi.linear_fp8(x8, xs, w8, ws, dtype=dt), "bias": _capi.linear_fp8(x8, xs, w8, ws, b, dtype=dt),
        "bias32": _capi.linear_fp8(x8, xs, w8, ws, b32, dtype=dt),
        "gelu": _capi.linear_fp8(x8, xs, w8, ws, b, act=_capi.ACT_GELU_TANH, dtype=dt),
        "gate_res": _capi.linear_fp8(x8, xs, w8, ws, b32, gate=gate, res=res, dtype=dt), "strided_out": wide8,
        "res32": _capi.linear_fp8(x8, xs, w8, ws, b32, gate=gate, res=res32, dtype=dt),
    }
    for name, t in forms8.items():
        r.put(f"linear_fp8_{name}/{tag}", t)


def main(path):
    dev = torch.device("cuda:0")
    r = Run(dev, 20240)
    l2h, h2l = _capi.gilbert_map(2, 8, 32, False, dev)
    r.put("gilbert_map", l2h, h2l)
    r.put("gilbert_map_sliced", *_capi.gilbert_map(2, 8, 32, True, dev))
    r.put("gilbert_neighbors", _capi.gilbert_neighbors(2, 8, 32, 128, l2h))
    _capi.stream_delay(50.0)
    for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
        rows(r, dt, tag)
        attention(r, dt, 256, 1, f"S256/{tag}")
        attention(r, dt, 384, 2, f"S384/{tag}")
        linears(r, dt, tag)
    attention(r, torch.bfloat16, 768, 4, "S768/bf16")       # two pairs: the pair kernel's own launch order
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump(r.out, f, indent=1, sort_keys=True)
    print(json.dumps({"outputs": len(r.out), "all": hashlib.sha256(json.dumps(r.out, sort_keys=True).encode()).hexdigest()}))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    diff = sorted(k for k in set(A) | set(B) if A.get(k) != B.get(k))
    print(json.dumps({"outputs": len(A), "equal": not diff, "differing": diff}))
    return 1 if diff else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--compare"]:
        sys.exit(compare(*sys.argv[2:4]))
    main(sys.argv[1] if len(sys.argv) > 1 else "capi_ab.json")
