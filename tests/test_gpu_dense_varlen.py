"""GPU (-m gpu): the dense varlen kernel (csrc/dattn.hip, jenga_dense_varlen_fwd) against softmax(Q K^T 128^-0.5) V in float64,
segment by segment, on the 16-bit inputs.  H = 2, D = 128, seeded randn."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 2
BOUND = {torch.bfloat16: 1e-2, torch.float16: 2e-3}
# (cu_q, cu_kv, Tq, Tk): Tq / Tk None = a few rows more than the last boundary
SETS = [
    ([0, 333, 590], [0, 333, 590], None, None),                         # ragged ends, a segment that starts mid-tile
    ([0, 1, 130, 130, 700], [0, 77, 78, 300, 1100], None, None),        # 1 row, 1 key, empty segment, Lq != Lkv, > 2 tiles
    ([0, 257], [0, 64], None, None),                                    # one row past a tile, exactly one kv tile
    ([0, 300], [0, 0], 384, 64),                                        # no keys + tail rows: all zeros
]


def _inputs(cu_q, cu_kv, Tq, Tk, dtype, seed=7):
    gen = torch.Generator().manual_seed(seed)
    Tq = cu_q[-1] + 3 if Tq is None else Tq
    Tk = cu_kv[-1] + 5 if Tk is None else Tk
    return [torch.randn(n, H, 128, generator=gen).to(dtype) for n in (Tq, Tk, Tk)]


def _ref(q, k, v, cu_q, cu_kv):
    o = torch.zeros(q.shape, dtype=torch.float64)
    for (a, b), (c, d) in zip(zip(cu_q, cu_q[1:]), zip(cu_kv, cu_kv[1:])):
        if b > a and d > c:
            s = torch.einsum("qhd,khd->hqk", q[a:b].double(), k[c:d].double()) * 128 ** -0.5
            o[a:b] = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v[c:d].double())
    return o


def _run(q, k, v, cu_q, cu_kv):
    from jenga_amd import _capi
    dev = torch.device("cuda:0")
    i32 = lambda c: torch.tensor(c, dtype=torch.int32, device=dev)
    return _capi.dense_varlen_fwd(q.to(dev), k.to(dev), v.to(dev), i32(cu_q), i32(cu_kv)).cpu()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", range(len(SETS)))
def test_accuracy(case, dtype):
    cu_q, cu_kv, Tq, Tk = SETS[case]
    q, k, v = _inputs(cu_q, cu_kv, Tq, Tk, dtype)
    o = _run(q, k, v, cu_q, cu_kv)
    ref = _ref(q, k, v, cu_q, cu_kv)
    err = (o.double() - ref).abs().max().item()
    print(f"case {case} {dtype}: max |o - ref| = {err:.3e}")
    assert err <= BOUND[dtype]
    assert not o[cu_q[-1]:].any()          # rows behind the last boundary: exact zeros
    if cu_kv[-1] == 0:
        assert not o.any()


@pytest.mark.parametrize("j", [1, 3])
def test_rows_of_a_segment_see_nothing_outside_it(j):
    """One leaked key moves the output by less than the accuracy bound: everything outside segment j is replaced by other
    random data (K / V rows behind cu_kv[-1] included) and the rows of segment j must not change by a bit."""
    cu_q, cu_kv, _, _ = SETS[1]
    q, k, v = _inputs(cu_q, cu_kv, None, None, torch.bfloat16)
    q2, k2, v2 = _inputs(cu_q, cu_kv, None, None, torch.bfloat16, seed=8)
    (a, b), (c, d) = cu_q[j:j + 2], cu_kv[j:j + 2]
    q2[a:b], k2[c:d], v2[c:d] = q[a:b], k[c:d], v[c:d]
    o, o2 = _run(q, k, v, cu_q, cu_kv), _run(q2, k2, v2, cu_q, cu_kv)
    assert o[a:b].abs().max() > 0.01 and torch.equal(o[a:b], o2[a:b])


@pytest.mark.parametrize("B,S_img", [(1, 512), (2, 500)])
def test_front_end_varlen_kernel_and_graph_capture(B, S_img):
    """attention(kernel="varlen") on the (valid | padding) segments of get_cu_seqlens, batch 2 and S % 128 != 0 included; then
    the same call captured in a graph (capture fails if anything reads cu_seqlens on the host) and replayed: bit-equal."""
    from jenga_amd.modules.attention import attention, get_cu_seqlens
    dev = torch.device("cuda:0")
    S_txt, valid = 256, [90, 20][:B]
    S = S_img + S_txt
    gen = torch.Generator().manual_seed(31)
    q, k, v = [torch.randn(B, S, H, 128, generator=gen).to(torch.bfloat16) for _ in range(3)]
    mask = (torch.arange(S_txt)[None, :] < torch.tensor(valid)[:, None]).to(torch.int64)
    cu = get_cu_seqlens(mask.to(dev), S_img)
    cu_list = [0] + [x for b in range(B) for x in (b * S + S_img + valid[b], (b + 1) * S)]
    assert cu.tolist() == cu_list
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    o = attention(qd, kd, vd, cu_seqlens_q=cu, cu_seqlens_kv=cu, kernel="varlen")
    assert o.shape == (B, S, H * 128)
    flat = lambda t: t.reshape(B * S, H, 128)
    ref = _ref(flat(q), flat(k), flat(v), cu_list, cu_list).reshape(B, S, H * 128)
    err = (o.cpu().double() - ref).abs().max().item()
    print(f"B {B} S {S}: max |o - ref| = {err:.3e}")
    assert err <= BOUND[torch.bfloat16]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        og = attention(qd, kd, vd, cu_seqlens_q=cu, cu_seqlens_kv=cu, kernel="varlen")
    for _ in range(2):
        og.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(og, o)
