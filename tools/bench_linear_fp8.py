#!/usr/bin/env python3
"""jenga_linear_fp8 (csrc/gemm8.hip) against jenga_linear in bf16 (hipBLASLt) on the six GEMM shapes of a HunyuanVideo block
(profiles/r05_gemm_own_vs_hipblaslt.json), operands uniform in [-1, 1), the two paths alternating; the activation quantiser is
timed on its own and added to the FP8 side.  GPU only.
  python tools/bench_linear_fp8.py [--out profiles/linear_fp8_ab.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jenga_amd import _capi  # noqa: E402

PEAK_BF16, PEAK_FP8 = 2500.0, 5000.0   # dense TFLOP/s of the MI355X
SHAPES = [("qkv (double block, img)", 115200, 9216, 3072), ("proj", 115200, 3072, 3072), ("fc1", 115200, 12288, 3072),
          ("fc2", 115200, 3072, 12288), ("linear1 MLP half", 115456, 12288, 3072), ("linear2", 115456, 3072, 15360)]

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--window", type=float, default=0.25, help="seconds of launches per timed window")
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def prepare(M, N, K):
    x = (torch.rand(M, K, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    w = (torch.rand(N, K, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
    o16, o8 = torch.empty(M, N, device=dev, dtype=torch.bfloat16), torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    x8 = torch.empty(M, K, device=dev, dtype=torch.uint8)
    w8, ws = _capi.quant_fp8_rows(w)
    _, xs = _capi.quant_fp8_rows(x, out=x8)
    fns = {"bf16": lambda: _capi.linear(x, w, out=o16), "fp8": lambda: _capi.linear_fp8(x8, xs, w8, ws, out=o8),
           "quant": lambda: _capi.quant_fp8_rows(x, out=x8)}
    for fn in fns.values():       # warm every shape first (plans, LDS attribute, clocks)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    return fns, (o8.float() - o16.float()).abs().max().item(), o16.float().abs().max().item()


cases = [(name, M, N, K) + prepare(M, N, K) for name, M, N, K in SHAPES]

rows = []
for name, M, N, K, fns, diff, ref in cases:
    ms = {}
    for _ in range(2):            # alternate the paths; the second pass is the record
        for k, fn in fns.items():
            n = max(3, int(a.window * 1e3 / max(timed(fn, 2), 1e-3)))
            ms[k] = timed(fn, n)
    tf = lambda t: 2.0 * M * N * K / t / 1e9
    rows.append({"shape": name, "M": M, "N": N, "K": K, "bf16_ms": round(ms["bf16"], 3), "fp8_ms": round(ms["fp8"], 3),
                 "quant_x_ms": round(ms["quant"], 3), "fp8_plus_quant_ms": round(ms["fp8"] + ms["quant"], 3),
                 "bf16_TFLOPs": round(tf(ms["bf16"]), 1), "bf16_frac_of_bf16_peak": round(tf(ms["bf16"]) / PEAK_BF16, 4),
                 "fp8_TFLOPs": round(tf(ms["fp8"]), 1), "fp8_frac_of_fp8_peak": round(tf(ms["fp8"]) / PEAK_FP8, 4),
                 "fp8_frac_of_bf16_peak": round(tf(ms["fp8"]) / PEAK_BF16, 4),
                 "speedup_with_quant": round(ms["bf16"] / (ms["fp8"] + ms["quant"]), 4),
                 "max_abs_diff_fp8_vs_bf16": diff, "max_abs_bf16": ref})
    print(json.dumps(rows[-1]), flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump({"what": "tools/bench_linear_fp8.py: jenga_linear (bf16, hipBLASLt) against jenga_quant_fp8_rows + "
                           "jenga_linear_fp8, alternating, device events, one box", "shapes": rows}, f, indent=1)
