"""The FP8 linear wrappers without a GPU: no CPU path, and argument errors are found before any device is touched."""
import pytest
import torch

from jenga_amd import _capi


def _args(M=4, N=8, K=128):
    return (torch.zeros(M, K, dtype=torch.uint8), torch.ones(M), torch.zeros(N, K, dtype=torch.uint8), torch.ones(N))


def test_there_is_no_cpu_path():
    with pytest.raises(_capi.JengaError):
        _capi.quant_fp8_rows(torch.zeros(4, 128, dtype=torch.bfloat16))
    with pytest.raises(_capi.JengaError):
        _capi.linear_fp8(*_args())


@pytest.mark.parametrize("bad", ["K192", "N12", "w_K", "x_scale", "int8", "gelu_res", "quant_K8"])
def test_wrong_shapes_raise_value_error(bad):
    x8, xs, w8, ws = _args(K=192) if bad == "K192" else _args(N=12) if bad == "N12" else _args()
    kw = {}
    if bad == "w_K":
        w8 = torch.zeros(8, 256, dtype=torch.uint8)
    if bad == "x_scale":
        xs = torch.ones(5)
    if bad == "int8":
        x8 = x8.view(torch.int8)
    if bad == "gelu_res":
        kw = dict(act=_capi.ACT_GELU_TANH, res=torch.zeros(4, 8, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        if bad == "quant_K8":
            _capi.quant_fp8_rows(torch.zeros(4, 24, dtype=torch.bfloat16))
        else:
            _capi.linear_fp8(x8, xs, w8, ws, **kw)
