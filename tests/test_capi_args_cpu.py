"""CPU: a table of bad-argument calls of the _capi wrappers on CPU tensors.  Every row runs twice:
  as given      -- the exception is the one the wrapper's own ORDER of checks gives for a CPU tensor: ValueError where the
                   argument is checked before `_need_gpu`, JengaError ("no CPU path") where `_need_gpu` comes first;
  checks only   -- `_need_gpu` switched off and `_stream`, which every launch evaluates as the library call's first argument,
                   replaced by a function that raises, so that the argument checks behind `_need_gpu` run on the CPU tensors
                   too and nothing can be launched: every row is a ValueError, and the unmodified base call of the same
                   wrapper gets as far as the launch.
Nothing here needs more than [1, 256, 2, 128]."""
import pytest
import torch

from jenga_amd import _capi

BF, F16, F32, I32 = torch.bfloat16, torch.float16, torch.float32, torch.int32
B, S, H = 1, 256, 2
VE, JE = ValueError, _capi.JengaError


def z(*shape, dtype=BF):
    return torch.zeros(*shape, dtype=dtype)


def _rope(**kw):
    a = dict(x=z(B, S, H, 128), weight=None, cos=z(S, 128, dtype=F32), sin=z(S, 128, dtype=F32), s_rope=None)
    a.update(kw)
    return _capi.rmsnorm_rope(**a)


def _pool(**kw):
    x = z(B, S, H, 128)
    a = dict(xq=x, xk=x, wq=None, wk=None, cos=z(S, 128, dtype=F32), sin=z(S, 128, dtype=F32), out_q=z(B, S, H, 128),
             out_k=z(B, S, H, 128), s_rope=None, qpool=z(B, H, 2, 128), kpool=z(B, H, 2, 128))
    a.update(kw)
    return _capi.qk_norm_rope_pool(**a)


def _sp(**kw):
    x = z(B, S, H, 128)
    a = dict(xq=x, xk=x, xv=x, wq=None, wk=None, cos=z(S, 128, dtype=F32), sin=z(S, 128, dtype=F32), out_q=z(B, S, H, 128),
             out_k=z(B, S, H, 128), out_v=z(B, S, H, 128), heads_per_peer=H)
    a.update(kw)
    return _capi.sp_qkv_prologue(**a)


def _linear(**kw):
    a = dict(x=z(4, 16), weight=z(8, 16))
    a.update(kw)
    return _capi.linear(**a)


def _linear_fp8(**kw):
    a = dict(x8=z(4, 128, dtype=torch.uint8), x_scale=torch.ones(4), w8=z(8, 128, dtype=torch.uint8), w_scale=torch.ones(8))
    a.update(kw)
    return _capi.linear_fp8(**a)


def _lists(**kw):
    """seqlens / idx / cnt of one image block and one text block"""
    a = dict(seqlens=z(B, dtype=I32), idx=z(B, H, 1, 2, dtype=I32), cnt=z(B, H, 1, dtype=I32), nq_img=1, sm_scale=1.0,
             text_amp=0.0, text_block_start=1)
    a.update(kw)
    return a


def _attn(**kw):
    return _capi.bsattn_fwd(**{**_lists(q=z(B, S, H, 128), k=z(B, S, H, 128), vt=z(B, H, 4, 128, 64)), **kw})


def _attn_fp8(**kw):
    q8 = z(B, S, H, 128, dtype=torch.uint8)
    sc = torch.ones(B, H, 2)
    return _capi.bsattn_fp8_fwd(**{**_lists(q8=q8, q_scale=sc, k8=q8, k_scale=sc, vt=z(B, H, 4, 128, 64)), **kw})


def _attn_d64(**kw):
    return _capi.bsattn_d64_fwd(**{**_lists(q=z(B, S, H, 64), k=z(B, S, H, 64), v=z(B, S, H, 64)), **kw})


GELU = _capi.ACT_GELU_TANH
# the RoPE tables of the three fp32 wrappers
ROPE = {
    "dtype": dict(cos=z(S, 128, dtype=torch.float64)),
    "sin_dtype": dict(sin=z(S, 128)),
    "width": dict(cos=z(S, 64, dtype=F32), sin=z(S, 64, dtype=F32)),
    "length": dict(cos=z(128, 128, dtype=F32), sin=z(128, 128, dtype=F32), s_rope=200),
    "beyond_S": dict(cos=z(2 * S, 128, dtype=F32), sin=z(2 * S, 128, dtype=F32)),
    "s_rope_beyond_S": dict(cos=z(2 * S, 128, dtype=F32), sin=z(2 * S, 128, dtype=F32), s_rope=S + 1),
}
# seqlens / idx / cnt of the three attention wrappers
LISTS = {
    "few_seqlens": dict(seqlens=z(0, dtype=I32)),
    "idx_dtype": dict(idx=z(B, H, 1, 2, dtype=torch.int64)),
    "idx_shape": dict(idx=z(B, H, 2, 2, dtype=I32)),
    "idx_row_length": dict(idx=z(B, H, 1, 3, dtype=I32)),
    "idx_strided": dict(idx=z(B, H, 1, 4, dtype=I32)[..., ::2]),
    "idx_missing": dict(idx=None),
    "cnt_dtype": dict(cnt=z(B, H, 1, dtype=torch.int64)),
    "cnt_shape": dict(cnt=z(B, H, 2, dtype=I32)),
    "cnt_missing": dict(cnt=None),
}
POOL = {
    "shape": z(B, H, 2, 64), "heads": z(B, H + 1, 2, 128), "rank": z(H, 2, 128), "dtype": z(B, H, 2, 128, dtype=F16),
    "strided": z(B, H, 4, 128)[:, :, ::2],
}

# (id, base call, its bad keyword arguments, the exception on CPU tensors as given)
ROWS = []
for fn in (_rope, _pool, _sp):
    ROWS += [(f"{fn.__name__}-{n}", fn, kw, JE) for n, kw in ROPE.items()]
for which in ("qpool", "kpool"):
    ROWS += [(f"_pool-{which}_{n}", _pool, {which: t}, JE) for n, t in POOL.items()]
ROWS += [
    # sp_qkv_prologue's None-combinations are checked before anything else
    ("_sp-nothing", _sp, dict(xq=None, xk=None, out_q=None, out_k=None, xv=None, out_v=None), VE),
    ("_sp-q_without_k", _sp, dict(xk=None), VE),
    ("_sp-q_without_out_q", _sp, dict(out_q=None), VE),
    ("_sp-q_without_out_k", _sp, dict(out_k=None), VE),
    ("_sp-k_without_q", _sp, dict(xq=None, out_q=None, out_k=None), VE),
    ("_sp-v_without_out_v", _sp, dict(out_v=None), VE),
    ("_linear-bias_size", _linear, dict(bias=z(7)), JE),
    ("_linear-bias32_size", _linear, dict(bias=z(7, dtype=F32)), JE),
    ("_linear-gate_size", _linear, dict(gate=z(1, 7)), JE),
    ("_linear-res_rows", _linear, dict(res=z(3, 8)), JE),
    ("_linear-res_width", _linear, dict(res=z(4, 7)), JE),
    ("_linear-res_dtype", _linear, dict(res=z(4, 8, dtype=F16)), JE),
    ("_linear-res_not_out_dtype", _linear, dict(res=z(4, 8), out=z(4, 8, dtype=F32)), JE),
    ("_linear-out_width", _linear, dict(out=z(4, 7)), JE),
    ("_linear-out_rows", _linear, dict(out=z(3, 8)), JE),
    ("_linear-out_dtype", _linear, dict(out=z(4, 8, dtype=F16)), JE),
    ("_linear-out_not_res_dtype", _linear, dict(res=z(4, 8, dtype=F32), out=z(4, 8)), JE),
    ("_linear-act_out32", _linear, dict(act=GELU, out=z(4, 8, dtype=F32)), JE),
    ("_linear-act_res32", _linear, dict(act=GELU, res=z(4, 8, dtype=F32)), JE),
    # linear_fp8 checks the activation rule before _need_gpu, the epilogue operands behind it
    ("_linear_fp8-act_out32", _linear_fp8, dict(act=GELU, out=z(4, 8, dtype=F32)), VE),
    ("_linear_fp8-act_gate", _linear_fp8, dict(act=GELU, gate=z(8)), VE),
    ("_linear_fp8-act_res", _linear_fp8, dict(act=GELU, res=z(4, 8)), VE),
    ("_linear_fp8-dtype", _linear_fp8, dict(dtype=F32), VE),
    ("_linear_fp8-bias_size", _linear_fp8, dict(bias=z(7)), JE),
    ("_linear_fp8-bias32_size", _linear_fp8, dict(bias=z(7, dtype=F32)), JE),
    ("_linear_fp8-gate_size", _linear_fp8, dict(gate=z(1, 7)), JE),
    ("_linear_fp8-res_rows", _linear_fp8, dict(res=z(3, 8)), JE),
    ("_linear_fp8-res_dtype", _linear_fp8, dict(res=z(4, 8, dtype=F16)), JE),
    ("_linear_fp8-res_stride", _linear_fp8, dict(res=z(4, 12)[:, :8]), JE),
    ("_linear_fp8-out_width", _linear_fp8, dict(out=z(4, 16)), JE),
    ("_linear_fp8-out_dtype", _linear_fp8, dict(out=z(4, 8, dtype=F16)), JE),
    ("_linear_fp8-out_stride", _linear_fp8, dict(out=z(4, 12)[:, :8]), JE),
    ("_linear_fp8-out_not_res_dtype", _linear_fp8, dict(res=z(4, 8, dtype=F32), out=z(4, 8)), JE),
]
for fn in (_attn, _attn_fp8, _attn_d64):
    ROWS += [(f"{fn.__name__}-{n}", fn, kw, JE) for n, kw in LISTS.items()]
ROWS += [
    ("_attn-vt_shape", _attn, dict(vt=z(B, H, 2, 128, 64)), JE),
    ("_attn-vt_dtype", _attn, dict(vt=z(B, H, 4, 128, 64, dtype=F16)), JE),
    ("_attn-k_shape", _attn, dict(k=z(B, S, H + 1, 128)), JE),
    ("_attn-out_shape", _attn, dict(out=z(B, S, H + 1, 128)), JE),
    ("_attn-order_with_pairs", _attn, dict(order=z(B, H, 1, dtype=I32), flags=_capi.ATTN_PAIR_FLAGS), JE),
    ("_attn_fp8-vt_shape", _attn_fp8, dict(vt=z(B, H, 2, 128, 64)), JE),
    ("_attn_fp8-vt_strided", _attn_fp8, dict(vt=z(B, H, 4, 128, 128)[..., ::2]), JE),
    ("_attn_fp8-scale_shape", _attn_fp8, dict(q_scale=torch.ones(B, H, 3)), JE),
    ("_attn_fp8-out_dtype", _attn_fp8, dict(out=z(B, S, H, 128, dtype=F16)), JE),
    ("_attn_fp8-nq_img_range", _attn_fp8, dict(nq_img=3, idx=z(B, H, 3, 2, dtype=I32), cnt=z(B, H, 3, dtype=I32)), JE),
    ("_attn_d64-v_shape", _attn_d64, dict(v=z(B, S, H, 128)), JE),
    ("_attn_d64-k_dtype", _attn_d64, dict(k=z(B, S, H, 64, dtype=F16)), JE),
    ("_attn_d64-nq_img_range", _attn_d64, dict(nq_img=3, idx=z(B, H, 3, 2, dtype=I32), cnt=z(B, H, 3, dtype=I32)), JE),
]
IDS = [r[0] for r in ROWS]
assert len(set(IDS)) == len(IDS)


class _Launched(Exception):
    """the call got past every argument check: it asked for the stream to launch on"""


@pytest.fixture
def checks_only(monkeypatch):
    def no_stream(device):
        raise _Launched()
    monkeypatch.setattr(_capi, "_need_gpu", lambda t, what: None)
    monkeypatch.setattr(_capi, "_stream", no_stream)
    monkeypatch.setattr(_capi, "_gemm_workspace", lambda device: z(1, dtype=torch.uint8))   # (needs a stream otherwise)


@pytest.mark.parametrize("name,fn,kw,exc", ROWS, ids=IDS)
def test_bad_argument_on_cpu_tensors(name, fn, kw, exc):
    with pytest.raises(exc) as e:
        fn(**kw)
    assert type(e.value) is exc


@pytest.mark.parametrize("name,fn,kw,exc", ROWS, ids=IDS)
def test_bad_argument_is_refused_before_the_launch(checks_only, name, fn, kw, exc):
    with pytest.raises(ValueError):
        fn(**kw)


@pytest.mark.parametrize("fn", sorted({r[1] for r in ROWS}, key=lambda f: f.__name__), ids=lambda f: f.__name__)
def test_base_call_reaches_the_launch(checks_only, fn):
    """the rows above fail for the argument they change, not for something else in the base call"""
    with pytest.raises(_Launched):
        fn()


def test_base_call_has_no_cpu_path():
    for fn in sorted({r[1] for r in ROWS}, key=lambda f: f.__name__):
        with pytest.raises(_capi.JengaError, match="no CPU path"):
            fn()
