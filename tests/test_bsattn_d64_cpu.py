"""CPU: the argument checks of block_sparse_attention*(narrow_heads=...); nothing here reaches the library."""
import pytest
import torch

from jenga_amd import _capi
from jenga_amd.modules import attention_block_sparse as op


def _call(D, **kw):
    q, k, v = (torch.zeros(1, 256, 2, D, dtype=torch.bfloat16) for _ in range(3))
    cu = torch.tensor([0, 200, 256], dtype=torch.int32)
    return op.block_sparse_attention(q, k, v, 1, cu_seqlens_q=cu, cu_seqlens_kv=cu, text_blocks=1, **kw)


@pytest.mark.parametrize("D,kw,match", [
    (64, dict(narrow_heads="bogus"), "narrow_heads must be"),
    (128, dict(narrow_heads="native"), "needs head_dim 64"),
    (128, dict(narrow_heads="native", qk_dtype="fp8"), "native"),
    (64, dict(narrow_heads="native", qk_dtype="fp8"), "fp8"),
])
def test_bad_combinations_raise_value_error(D, kw, match):
    with pytest.raises(ValueError, match=match):
        _call(D, **kw)


@pytest.mark.parametrize("D", [64, 128])
def test_default_still_stops_at_the_first_kernel_on_cpu_tensors(D):
    with pytest.raises(_capi.JengaError, match="block_pool: tensors must live on the GPU"):
        _call(D)
    if D == 64:
        with pytest.raises(_capi.JengaError, match="block_pool_d64: tensors must live on the GPU"):
            _call(D, narrow_heads="native")
