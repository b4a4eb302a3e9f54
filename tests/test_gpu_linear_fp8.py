"""FP8 linear layers (csrc/gemm8.hip): jenga_quant_fp8_rows bit for bit against its recipe in torch on the CPU,
jenga_linear_fp8 against float64 on the dequantised operands, the refusals, and the JENGA_LINEAR_DTYPE routing of dit.py."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 0.0}
# |gelu_tanh evaluated in fp32 - in float64| <= 1.134e-7 * max(|v|, 1), measured on an MI355X over 4 M values of v in [-12, 12]
# (the device's tanhf, the formula of csrc/gemm8.hip; worst at v = 1.19); twice that for other inputs
GELU_EVAL = 2 * 1.134e-7
EPILOGUES = ["none", "bias16", "bias32_gate_res", "gelu_bias", "out32_gate_res"]


def _quant_cpu(x):
    """The recipe of jenga_quant_fp8_rows: x [rows, K] on the CPU -> (bytes uint8 [rows, K], scale fp32 [rows])."""
    xf = x.float()
    s = xf.abs().amax(dim=1).clamp(min=1e-30) / 448.0
    return (xf / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), s


@DTYPES
@pytest.mark.parametrize("strided", [False, True], ids=["contig", "strided"])
@pytest.mark.parametrize("rows,K", [(70, 256), (3, 16384 + 128)], ids=["regs", "twopass"])
def test_quantiser_is_bit_exact(dtype, strided, rows, K):
    from jenga_amd import _capi
    g = torch.Generator().manual_seed(rows + K)
    buf = (torch.randn(rows, K + 64, generator=g) * torch.rand(rows, 1, generator=g) * 8).to(dtype)
    buf[rows // 2] = 0                                   # a row of zeros: scale 1e-30 / 448, bytes 0
    x = buf[:, :K] if strided else buf[:, :K].contiguous()
    want8, want_s = _quant_cpu(x)
    out = torch.full((rows, K + 32), 7, dtype=torch.uint8, device="cuda")[:, :K] if strided else None
    x8, s = _capi.quant_fp8_rows(x.cuda(), out=out)
    assert torch.equal(x8.cpu(), want8) and torch.equal(s.cpu(), want_s)
    assert want_s[rows // 2].item() == torch.tensor(1e-30, dtype=torch.float32).div(448.0).item()


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """e4m3fn operands with their scales and the float64 product / absolute product of the dequantised values (CPU)."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    x8, xs = _quant_cpu(torch.randn(M, K, generator=g).bfloat16())
    w8, ws = _quant_cpu((torch.randn(N, K, generator=g) * 0.05).bfloat16())
    xd = x8.view(torch.float8_e4m3fn).double() * xs.double()[:, None]
    wd = w8.view(torch.float8_e4m3fn).double() * ws.double()[:, None]
    extra = {"bias": torch.randn(N, generator=g), "gate": torch.randn(N, generator=g) * 2, "res": torch.randn(M, N, generator=g)}
    return x8, xs, w8, ws, xd @ wd.T, xd.abs() @ wd.abs().T, extra


@DTYPES
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("K", [128, 384])          # the prologue only; an odd number of K steps (the LDS ring wraps)
@pytest.mark.parametrize("N", [8, 256 + 72])       # the narrowest legal N; a second, partial channel tile
@pytest.mark.parametrize("M", [1, 256 + 70])       # a single row; a second, partial token tile
def test_gemm_against_float64(dtype, epi, M, N, K):
    from jenga_amd import _capi
    x8, xs, w8, ws, prod, aprod, extra = _problem(M, N, K)
    odt = torch.float32 if epi.startswith("out32") else dtype
    bias = gate = res = None
    if "bias16" in epi or epi == "gelu_bias":
        bias = extra["bias"].to(dtype)
    if "bias32" in epi:
        bias = extra["bias"].clone()
    if "gate_res" in epi:
        gate, res = extra["gate"], extra["res"].to(odt)
    ref = prod * (gate.double() if gate is not None else 1.0)
    ref = ref + (bias.double() if bias is not None else 0.0) + (res.double() if res is not None else 0.0)
    acc_err = K * 2.0 ** -22 * aprod
    acc_err = acc_err + acc_err * (gate.double().abs() if gate is not None else 0.0)
    if epi == "gelu_bias":
        acc_err = 1.13 * acc_err + GELU_EVAL * ref.abs().clamp(min=1.0)
        ref = 0.5 * ref * (1.0 + torch.tanh(0.7978845608028654 * (ref + 0.044715 * ref ** 3)))
    bound = ULP[odt] * ref.abs() + acc_err

    xbuf = torch.zeros((M, K + 16), dtype=torch.uint8, device="cuda")      # x8 with a row stride larger than K
    xbuf[:, :K] = x8.cuda()
    obuf = torch.full((M, N + 16), 3.0, dtype=odt, device="cuda")          # out / res: column slices of wider buffers
    rbuf = torch.full((M, N + 16), 5.0, dtype=odt, device="cuda")
    if res is not None:
        rbuf[:, 8:8 + N] = res.cuda()
    out = _capi.linear_fp8(xbuf[:, :K], xs.cuda(), w8.cuda(), ws.cuda(), None if bias is None else bias.cuda(),
                           act=_capi.ACT_GELU_TANH if epi == "gelu_bias" else _capi.ACT_NONE,
                           gate=None if gate is None else gate.cuda(), res=rbuf[:, 8:8 + N] if res is not None else None,
                           out=obuf[:, 8:8 + N], dtype=dtype)
    assert out.data_ptr() == obuf[:, 8:8 + N].data_ptr()
    got = obuf.cpu()
    assert (got[:, :8] == 3.0).all() and (got[:, 8 + N:] == 3.0).all(), "columns beside the output were written"
    err = (got[:, 8:8 + N].double() - ref).abs()
    print(f"linear_fp8 {epi} M={M} N={N} K={K} {dtype}: worst error / bound = {(err / bound.clamp(min=1e-300)).max().item():.3f}, "
          f"max abs error {err.max().item():.3e}")
    assert (err <= bound).all()


def test_refusals():
    from jenga_amd import _capi
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")
    f = lambda n: torch.ones(n, dtype=torch.float32, device="cuda")
    with pytest.raises((ValueError, _capi.JengaError)):
        _capi.linear_fp8(z(4, 192), f(4), z(8, 192), f(8))                       # K not a multiple of 128
    with pytest.raises((ValueError, _capi.JengaError)):
        _capi.linear_fp8(z(4, 128), f(4), z(12, 128), f(12))                     # N not a multiple of 8
    with pytest.raises((ValueError, _capi.JengaError)):
        _capi.linear_fp8(z(4, 128), f(4), z(8, 128), f(8), act=_capi.ACT_GELU_TANH,
                         res=torch.zeros(4, 8, dtype=torch.bfloat16, device="cuda"))
    # the C entry itself refuses them too (nothing is launched)
    L, p = _capi.lib(), _capi._p
    x8, w8, o = z(4, 192), z(16, 192), torch.zeros(4, 16, dtype=torch.bfloat16, device="cuda")
    for N, K, act, res in ((16, 192, 0, None), (12, 128, 0, None), (16, 128, 1, o)):
        rc = L.jenga_linear_fp8(None, p(x8), p(f(4)), p(w8), p(f(16)), None, p(res), None, p(o), 4, N, K, 192, 192, 16, 16, act, 0)
        assert rc != 0 and b"jenga_linear_fp8" in L.jenga_last_error()


def test_dit_routing(monkeypatch):
    from jenga_amd import _capi, dit
    torch.manual_seed(0)
    mlp = dit.MLP(128, 256, dtype=torch.bfloat16, device="cuda")
    x = torch.randn(1, 200, 128, dtype=torch.bfloat16, device="cuda")
    gate = torch.randn(1, 128, dtype=torch.bfloat16, device="cuda")
    res = torch.randn(1, 200, 128, dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        h = mlp.hidden(x)
        assert torch.equal(h, _capi.linear(x, mlp.fc1.weight, mlp.fc1.bias, act=_capi.ACT_GELU_TANH))
        gbias = mlp.fc2.bias.float() * gate.reshape(-1).float()
        assert torch.equal(dit.linear_gate_residual(mlp.fc2, h, gate, res),
                           _capi.linear(h, mlp.fc2.weight, gbias, gate=gate.reshape(-1), res=res))
        monkeypatch.setattr(dit, "LINEAR_DTYPE", "fp8")
        h8 = mlp.hidden(x)
        w8, ws = _capi.quant_fp8_rows(mlp.fc1.weight)
        assert torch.equal(h8, _capi.linear_fp8(*_capi.quant_fp8_rows(x), w8, ws, mlp.fc1.bias, act=_capi.ACT_GELU_TANH))
        assert not torch.equal(h8, h)
        w8, ws = _capi.quant_fp8_rows(mlp.fc2.weight)
        assert torch.equal(dit.linear_gate_residual(mlp.fc2, h, gate, res),
                           _capi.linear_fp8(*_capi.quant_fp8_rows(h), w8, ws, gbias, gate=gate.reshape(-1), res=res))
        cached = mlp.fc1._jenga_fp8[1].data_ptr()
        mlp.hidden(x)
        assert mlp.fc1._jenga_fp8[1].data_ptr() == cached       # the weight is quantised once
