#!/usr/bin/env python3
"""Kernel-level micro-benchmark of the AttenCarve op at the HunyuanVideo 720p x 125f shape
(S_img = 115200 = 900 blocks, S_txt = 256, H = 24, D = 128, bf16).  Prints one JSON line per stage.
  python tools/bench_attn.py [--heads 24] [--drop 0.75] [--p 0.3] [--peaky 0] [--iters 5] [--no-xcd]"""
import argparse
import json
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jenga_amd import _capi, gilbert as G  # noqa: E402


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, out


DENSE_SHAPES = {   # name -> (image tokens, text tokens, valid text, heads)
    "hunyuan_720p": (115200, 256, 64, 24),
    "wan14b_720p": (75600, 48, 0, 40),     # 21 x 45 x 80 tokens, padded to 591 blocks by the Wan attention op
}
PEAK_BF16_TFLOPS, PEAK_HBM_TBPS = 2500.0, 8.0


def dense_ab(a):
    """--dense: the dense call of the product, old path against new path, same tensors, same process, alternating.
    old: attention() as shipped -- jenga_pack_v + jenga_bsattn_fwd over the cached all-kept lists + padding_segment (the
         one-time list build happens in the warm-up and is not timed; everything per call is);
    new: attention(kernel="varlen") -- one jenga_dense_varlen_fwd launch.
    Device events around `--iters` calls (choose it so that a window is >= 1 s), `--repeats` windows per path."""
    from jenga_amd.modules.attention import attention
    dev = torch.device("cuda:0")
    record = {"peak_bf16_TFLOPs": PEAK_BF16_TFLOPS, "peak_HBM_TBps": PEAK_HBM_TBPS, "iters_per_window": a.iters,
              "repeats": a.repeats, "shapes": {}}
    for name, (s_img, s_txt, valid, H) in DENSE_SHAPES.items():
        if a.dense_shapes and name not in a.dense_shapes:
            continue
        S = s_img + s_txt
        torch.manual_seed(0)
        q, k, v = [torch.randn(1, S, H, 128, device=dev, dtype=torch.bfloat16) for _ in range(3)]
        cu = torch.tensor([0, s_img + valid, S], dtype=torch.int32, device=dev)
        paths = {"old_lists": lambda: attention(q, k, v, cu_seqlens_q=cu, cu_seqlens_kv=cu),
                 "new_varlen": lambda: attention(q, k, v, cu_seqlens_q=cu, cu_seqlens_kv=cu, kernel="varlen")}
        outs = {n: f() for n, f in paths.items()}          # warm both (code objects, the cached lists)
        torch.cuda.synchronize()
        diff = (outs["old_lists"].float() - outs["new_varlen"].float()).abs().max().item()
        del outs
        ms = {n: [] for n in paths}
        for _ in range(a.repeats):
            for n, f in paths.items():                     # alternate the two inside every repeat
                ms[n].append(timed(f, a.iters, warmup=0)[0])
        n_valid, n_pad = s_img + valid, S - s_img - valid
        flops = 4 * (n_valid ** 2 + n_pad ** 2) * 128 * H
        t_flops = flops / (PEAK_BF16_TFLOPS * 1e12)
        t_bytes = 4 * S * H * 128 * 2 / (PEAK_HBM_TBPS * 1e12)   # q, k, v read and o written once
        row = {"S": S, "H": H, "segments": [n_valid, n_pad], "flop": flops, "max_abs_old_vs_new": diff,
               "tolerance_bf16": 1e-2, "bound": "compute" if t_flops >= t_bytes else "memory"}
        for n, xs in ms.items():
            med = sorted(xs)[len(xs) // 2]
            row[n] = {"ms_per_call": xs, "median_ms": med, "spread_ms": max(xs) - min(xs),
                      "TFLOPs": flops / (med * 1e-3) / 1e12,
                      "share_of_peak": max(t_flops, t_bytes) / (med * 1e-3)}
        row["speedup_new_over_old"] = row["old_lists"]["median_ms"] / row["new_varlen"]["median_ms"]
        record["shapes"][name] = row
        print(json.dumps({name: row}), flush=True)
        del q, k, v
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)


def fp8_ab(a, q, k, vt, seqlens, idx, cnt, nimg, kpool, flops, res):
    """--fp8: the shipped 16-bit default against the FP8 Q.K kernel on the SAME tensors and kept lists, one process, alternating
    windows of `--iters` calls (choose it so that a window is >= 1 s), `--repeats` windows each:
      default    bsattn_fwd with ATTN_DEFAULT_FLAGS;
      fp8_attn   bsattn_fp8_fwd alone (q8 / k8 quantised once, outside the windows);
      fp8_total  the two quantiser launches (K with the mean-of-block-means offset) + bsattn_fp8_fwd."""
    off = kpool.float().mean(2)
    q8, qs = _capi.quant_fp8_blocks(q)
    k8, ks = _capi.quant_fp8_blocks(k, off)
    sm = 128 ** -0.5
    attn8 = lambda a8, b8: _capi.bsattn_fp8_fwd(a8[0], a8[1], b8[0], b8[1], vt, seqlens, idx, cnt, nimg, sm, 0.0, nimg)
    paths = {"default": lambda: _capi.bsattn_fwd(q, k, vt, seqlens, idx, cnt, nimg, sm, 0.0, nimg),
             "fp8_attn": lambda: attn8((q8, qs), (k8, ks)),
             "fp8_total": lambda: attn8(_capi.quant_fp8_blocks(q), _capi.quant_fp8_blocks(k, off))}
    o16, o8 = paths["default"]().float(), paths["fp8_total"]().float()          # warm-up; the error figures
    torch.cuda.synchronize()
    d = o8 - o16
    rec = {"shape": res["shape"], "pairs": res["pairs"], "flop": flops, "default_flags": _capi.ATTN_DEFAULT_FLAGS,
           "iters_per_window": a.iters, "repeats": a.repeats, "finite": bool(torch.isfinite(o8).all().item()),
           "fp8_vs_16bit_kernel": {"max_abs": float(d.abs().max().item()),
                                   "rms_rel": float((d.pow(2).mean().sqrt() / o16.pow(2).mean().sqrt()).item())}}
    del o16, o8, d
    ms = {n: [] for n in paths}
    for _ in range(a.repeats):
        for n, f in paths.items():                     # alternate inside every repeat
            ms[n].append(timed(f, a.iters, warmup=0)[0])
    for n, xs in ms.items():
        med = sorted(xs)[len(xs) // 2]
        rec[n] = {"ms_per_call": xs, "median_ms": med, "spread_ms": max(xs) - min(xs),
                  "TFLOPs": flops / (med * 1e-3) / 1e12}
    rec["speedup_fp8_attn_over_default"] = rec["default"]["median_ms"] / rec["fp8_attn"]["median_ms"]
    rec["speedup_fp8_total_over_default"] = rec["default"]["median_ms"] / rec["fp8_total"]["median_ms"]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.fp8_out)), exist_ok=True)
    with open(a.fp8_out, "w") as f:
        json.dump(rec, f, indent=1)


def d64_ab(a):
    """--d64: 64-channel heads, the padded path against the native one on the SAME q, k, v and kept lists (the selection runs
    once, outside the windows: it is the same work on both sides), one process, alternating windows of `--iters` calls
    (choose it so that a window is >= 1 s), `--repeats` windows each:
      pad_total     F.pad of q, k, v to 128 channels + pack_v + bsattn_fwd (default flags) + the slice back to 64 channels;
      pad_attn      that bsattn_fwd alone on the padded tensors;
      native_total = native_attn: bsattn_d64_fwd on the tensors as given (there is nothing else on that side)."""
    import torch.nn.functional as F
    dev = torch.device("cuda:0")
    t, h, w = a.grid
    S_img, tb, H = t * h * w, 2, a.heads
    nimg, nb = S_img // 128, S_img // 128 + tb
    S = nb * 128
    torch.manual_seed(0)
    q, k, v = [torch.randn(1, S, H, 64, device=dev, dtype=torch.bfloat16) for _ in range(3)]
    nbm = G.gilbert_block_neighbor_mapping(t, h, w, as_tensor=True)
    top_k = int((1 - a.drop) * nimg)
    seqlens = torch.tensor([S_img + a.valid_text], dtype=torch.int32, device=dev)
    _, idx, cnt = _capi.block_select(_capi.block_pool_d64(q, nimg), _capi.block_pool_d64(k, nb), nbm, nimg, tb, top_k, a.p,
                                     head_dim=64)
    sm = 64 ** -0.5
    pad = lambda x: F.pad(x, [0, 64])
    qp, kp, vtp = pad(q), pad(k), _capi.pack_v(pad(v), nb)
    paths = {"pad_total": lambda: _capi.bsattn_fwd(pad(q), pad(k), _capi.pack_v(pad(v), nb), seqlens, idx, cnt, nimg, sm, 0.0,
                                                   nimg)[..., :64].contiguous(),
             "pad_attn": lambda: _capi.bsattn_fwd(qp, kp, vtp, seqlens, idx, cnt, nimg, sm, 0.0, nimg),
             "native_attn": lambda: _capi.bsattn_d64_fwd(q, k, v, seqlens, idx, cnt, nimg, sm, 0.0, nimg)}
    o_pad, o_nat = paths["pad_total"]().float(), paths["native_attn"]().float()      # warm-up; the difference at the timed size
    paths["pad_attn"]()
    torch.cuda.synchronize()
    d = o_nat - o_pad
    pairs = int(cnt.sum().item()) + H * tb * nb
    flops = 4 * 128 * 128 * 64 * pairs
    rec = {"shape": dict(S=S, H=H, D=64, nb=nb, top_k=top_k, p=a.p, drop=a.drop), "pairs": pairs, "flop": flops,
           "default_flags": _capi.ATTN_DEFAULT_FLAGS, "iters_per_window": a.iters, "repeats": a.repeats,
           "finite": bool(torch.isfinite(o_nat).all().item()),
           "native_vs_pad": {"max_abs": float(d.abs().max().item()), "rms": float(d.pow(2).mean().sqrt().item()),
                             "rms_of_output": float(o_pad.pow(2).mean().sqrt().item())}}
    del o_pad, o_nat, d
    ms = {n: [] for n in paths}
    for _ in range(a.repeats):
        for n, f in paths.items():                     # alternate inside every repeat
            ms[n].append(timed(f, a.iters, warmup=0)[0])
    for n, xs in ms.items():
        med = sorted(xs)[len(xs) // 2]
        rec[n] = {"ms_per_call": xs, "median_ms": med, "spread_ms": max(xs) - min(xs), "TFLOPs": flops / (med * 1e-3) / 1e12}
    rec["speedup_native_over_pad_total"] = rec["pad_total"]["median_ms"] / rec["native_attn"]["median_ms"]
    rec["speedup_native_over_pad_attn"] = rec["pad_attn"]["median_ms"] / rec["native_attn"]["median_ms"]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.d64_out)), exist_ok=True)
    with open(a.d64_out, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d64", action="store_true", help="A/B at 64-channel heads: zero-padded 128-channel path vs bsattn_d64_fwd")
    ap.add_argument("--d64-out", default="profiles/bsattn_d64_ab.json", help="--d64: where the record goes")
    ap.add_argument("--fp8", action="store_true", help="A/B of the attention launch: 16-bit default vs the FP8 Q.K kernel")
    ap.add_argument("--fp8-out", default="profiles/bsattn_fp8_ab.json", help="--fp8: where the record goes")
    ap.add_argument("--dense", action="store_true", help="A/B of the dense call: lists path vs the dense varlen kernel")
    ap.add_argument("--dense-shapes", nargs="*", default=[], help="--dense: subset of " + ", ".join(DENSE_SHAPES))
    ap.add_argument("--repeats", type=int, default=3, help="--dense / --fp8 / --d64: timed windows per path")
    ap.add_argument("--out", default="profiles/dense_varlen_ab.json", help="--dense: where the record goes")
    ap.add_argument("--heads", type=int, default=24)
    ap.add_argument("--grid", type=int, nargs=3, default=[32, 45, 80])
    ap.add_argument("--drop", type=float, default=0.75)
    ap.add_argument("--p", type=float, default=0.3)
    ap.add_argument("--peaky", type=float, default=0.0, help=">0: clustered block means with this temperature")
    ap.add_argument("--coherent", type=int, default=0, metavar="SMOOTH",
                    help="SURVEY.md 8(d)'s second regime: K block means = centroid + noise with centroids smoothed SMOOTH "
                         "times over the Hilbert block-neighbour graph (spatially smooth features); Q of block m drawn "
                         "near the mean centroid of its Hilbert neighbours.  Adjacent query blocks then keep similar "
                         "lists, as a trained model's do; --gain sets the temperature so that top_k decides n")
    ap.add_argument("--gain", type=float, default=3.0, help="--coherent: centroid scale (pooled score ~ gain^2)")
    ap.add_argument("--sorted", action="store_true", help="kept-count-aware launch order (ATTN_SORTED)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--valid-text", type=int, default=64)
    ap.add_argument("--no-xcd", action="store_true")
    ap.add_argument("--same-list", action="store_true", help="every query block keeps the SAME blocks (perfect L2 reuse)")
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--l2-resident", type=int, default=0,
                    help="N>0: every query block reads the same N kv blocks repeatedly (same pair count): isolates MFMA/LDS work from L2-miss fill traffic")
    ap.add_argument("--window", type=int, default=0,
                    help="experiment: every query block keeps a random 31.6 %% of the kv blocks [0, WINDOW) only")
    ap.add_argument("--k-head-major", action="store_true", help="K (and Q) stored [B,H,S,D]: contiguous 16 KiB K tiles")
    ap.add_argument("--flags", type=int, default=None,
                    help="attention flags (_capi.ATTN_*): 1 = XCD remap, 4 = balanced launch, 8 = LP kernel, 16 = kept-count-aware "
                         "order (29 = the LP default), 64 = pair kernel (69 = its default), 0 / 1 = round-1 kernel")
    ap.add_argument("--also-flags", type=int, nargs="*", default=[],
                    help="more flag sets timed on the SAME tensors and lists in the same process (A/B on one box); each is "
                         "reported under also[<flags>] with its max |o - o_first|")
    ap.add_argument("--pair-overlap", type=float, default=-1.0,
                    help=">= 0: synthetic lists -- every odd query block shares this fraction of its list with the even "
                         "block in front of it (what Hilbert-adjacent blocks of a trained model look like); same counts")
    a = ap.parse_args()
    if a.dense:
        return dense_ab(a)
    if a.d64:
        return d64_ab(a)
    dev = torch.device("cuda:0")
    t, h, w = a.grid
    S_img, tb = t * h * w, 2
    assert S_img % 128 == 0
    nimg, nb = S_img // 128, S_img // 128 + tb
    S = nb * 128
    H = a.heads
    torch.manual_seed(0)
    nbm = G.gilbert_block_neighbor_mapping(t, h, w, as_tensor=True)
    q = torch.randn(1, S, H, 128, device=dev, dtype=torch.bfloat16)
    k = torch.randn(1, S, H, 128, device=dev, dtype=torch.bfloat16)
    v = torch.randn(1, S, H, 128, device=dev, dtype=torch.bfloat16)
    if a.peaky > 0:
        cent = torch.randn(1, nb, 1, H, 128, device=dev) * a.peaky
        k = (k.view(1, nb, 128, H, 128).float() + cent).to(torch.bfloat16).view(1, S, H, 128)
        pick = torch.randint(0, nimg, (nb,), device=dev)
        q = (q.view(1, nb, 128, H, 128).float() + cent[:, pick]).to(torch.bfloat16).view(1, S, H, 128)
    if a.coherent > 0:
        g = torch.Generator(device=dev).manual_seed(11)
        cent = torch.randn(nb, H, 128, device=dev, generator=g)
        A = torch.zeros(nb, nb, device=dev)
        A[:nimg, :nimg] = nbm.to(dev).float()
        A[nimg:, nimg:] = torch.eye(tb, device=dev)
        A = A / A.sum(-1, keepdim=True)
        for _ in range(a.coherent):
            cent = torch.einsum("mn,nhd->mhd", A, cent)
            cent = cent / cent.norm(dim=-1, keepdim=True) * (128 ** 0.5)      # keep |c|^2 = 128 like white noise
        qcent = torch.einsum("mn,nhd->mhd", A, cent)                          # mean centroid of the Hilbert neighbours
        qcent = qcent / qcent.norm(dim=-1, keepdim=True) * (128 ** 0.5)
        noise = lambda: torch.randn(1, nb, 128, H, 128, device=dev, generator=g)
        k = (noise() + a.gain * cent.view(1, nb, 1, H, 128)).to(torch.bfloat16).view(1, S, H, 128)
        q = (noise() + a.gain * qcent.view(1, nb, 1, H, 128)).to(torch.bfloat16).view(1, S, H, 128)
    top_k = int((1 - a.drop) * nimg)
    seqlens = torch.tensor([S_img + a.valid_text], dtype=torch.int32, device=dev)

    res = {"shape": dict(S=S, H=H, nb=nb, top_k=top_k, p=a.p, drop=a.drop, peaky=a.peaky)}
    ms, qpool = timed(lambda: _capi.block_pool(q, nimg), a.iters)
    ms2, kpool = timed(lambda: _capi.block_pool(k, nb), a.iters)
    res["pool_ms"] = ms + ms2
    res["pool_GBps"] = (q.numel() * 2 * (nimg / nb) + k.numel() * 2) / ((ms + ms2) * 1e-3) / 1e9
    ms, (mask, idx, cnt) = timed(lambda: _capi.block_select(qpool, kpool, nbm, nimg, tb, top_k, a.p), a.iters)
    res["select_ms"] = ms
    mk = _capi.block_select(qpool, kpool, nbm, nimg, tb, top_k, a.p, want_mask=True, want_lists=False)[0].bool()
    both = (mk[:, :, :-1, :nimg] & mk[:, :, 1:, :nimg]).sum(-1).float()
    res["adjacent_shared_frac"] = float((both / mk[:, :, :-1, :nimg].sum(-1).float()).mean().item())
    del mk, both
    ms, vt = timed(lambda: _capi.pack_v(v, nb), a.iters)
    res["pack_v_ms"] = ms
    res["pack_v_GBps"] = 2 * v.numel() * 2 / (ms * 1e-3) / 1e9
    if a.same_list:
        n = int(cnt.float().mean().item())
        idx = torch.arange(nb, device=dev, dtype=torch.int32).expand(1, H, nimg, nb).contiguous()
        idx[..., n - tb:n] = torch.arange(nimg, nb, device=dev, dtype=torch.int32)
        cnt = torch.full_like(cnt, n)
    if a.l2_resident:
        n = int(cnt.float().mean().item())
        idx = (torch.arange(nb, device=dev, dtype=torch.int32) % a.l2_resident).expand(1, H, nimg, nb).contiguous()
        cnt = torch.full_like(cnt, n)
    if a.window:
        n = max(1, int(0.316 * a.window))
        r = torch.rand(1, H, nimg, a.window, device=dev)
        sel = r.topk(n, dim=-1).indices.sort(dim=-1).values.to(torch.int32)
        idx = torch.zeros(1, H, nimg, nb, dtype=torch.int32, device=dev)
        idx[..., :n] = sel
        cnt = torch.full_like(cnt, n)
    if a.pair_overlap >= 0:
        n = int(cnt.float().mean().item())
        g = torch.Generator(device=dev).manual_seed(3)
        r = torch.rand(1, H, nimg, nimg, device=dev, generator=g)
        # odd rows reuse the even row's random keys for a fraction of the columns -> correlated top-n sets
        take = torch.rand(1, H, nimg, nimg, device=dev, generator=g) < a.pair_overlap
        r[:, :, 1::2] = torch.where(take[:, :, 1::2], r[:, :, 0:nimg - 1:2][:, :, : r[:, :, 1::2].shape[2]], r[:, :, 1::2])
        sel = r.topk(n - tb, dim=-1).indices.sort(dim=-1).values.to(torch.int32)
        idx = torch.zeros(1, H, nimg, nb, dtype=torch.int32, device=dev)
        idx[..., : n - tb] = sel
        idx[..., n - tb:n] = torch.arange(nimg, nb, device=dev, dtype=torch.int32)
        cnt = torch.full_like(cnt, n)
        ev, od = idx[:, :, 0:nimg - 1:2, : n - tb], idx[:, :, 1::2, : n - tb]
        ev = ev[:, :, : od.shape[2]]
        m_ev = torch.zeros(1, H, od.shape[2], nb, dtype=torch.bool, device=dev).scatter_(-1, ev.long(), True)
        res["pair_shared_frac"] = float(m_ev.gather(-1, od.long()).float().mean().item())
    if a.k_head_major:
        k = k.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        q = q.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    kept = int(cnt.sum().item())
    pairs = kept + H * tb * nb
    flops = 4 * 128 ** 3 * pairs
    res["pairs"] = pairs
    res["kept_mean"] = kept / (H * nimg)
    res["kept_min_max"] = [int(cnt.min()), int(cnt.max())]
    if a.fp8:
        return fp8_ab(a, q, k, vt, seqlens, idx, cnt, nimg, kpool, flops, res)
    fl = a.flags
    if a.sorted:
        fl = (_capi.ATTN_DEFAULT_FLAGS if fl is None else fl) | _capi.ATTN_SORTED
    res["flags"] = _capi.ATTN_DEFAULT_FLAGS if fl is None else fl
    ms, o = timed(lambda: _capi.bsattn_fwd(q, k, vt, seqlens, idx, cnt, nimg, 128 ** -0.5, 0.0, nimg,
                                           xcd_remap=not a.no_xcd, flags=fl), a.iters)
    res["attn_ms"] = ms
    res["attn_TFLOPs"] = flops / (ms * 1e-3) / 1e12
    res["attn_frac_of_2.5PF"] = res["attn_TFLOPs"] / 2500
    res["dense_equiv_TFLOPs"] = 4 * S * S * 128 * H / (ms * 1e-3) / 1e12
    res["finite"] = bool(torch.isfinite(o.float()).all().item())
    for fl2 in a.also_flags:
        ms2, o2 = timed(lambda: _capi.bsattn_fwd(q, k, vt, seqlens, idx, cnt, nimg, 128 ** -0.5, 0.0, nimg,
                                                 xcd_remap=not a.no_xcd, flags=fl2), a.iters)
        d = (o2.float() - o.float()).abs()
        res.setdefault("also", {})[str(fl2)] = dict(attn_ms=ms2, attn_TFLOPs=flops / (ms2 * 1e-3) / 1e12,
                                                    frac=flops / (ms2 * 1e-3) / 1e12 / 2500,
                                                    max_abs_diff_vs_first=float(d.max().item()),
                                                    mean_abs_diff_vs_first=float(d.mean().item()),
                                                    finite=bool(torch.isfinite(o2.float()).all().item()))
        del o2, d
    # second pass of the first set: the board reaches its power steady state over the run, order effects show here
    if a.also_flags:
        ms3, _ = timed(lambda: _capi.bsattn_fwd(q, k, vt, seqlens, idx, cnt, nimg, 128 ** -0.5, 0.0, nimg,
                                                xcd_remap=not a.no_xcd, flags=fl), a.iters)
        res["attn_ms_second_pass"] = ms3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
