"""GPU (-m gpu): the HIP path, called through the C ABI, against the golden fixtures and the oracle."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import inputs  # tests/golden/inputs.py
from helpers import assert_ulp_close, from_bits, hip_pooled, tie_tolerant_mask_equal, to_np

pytestmark = pytest.mark.gpu


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def lists_from_mask(mask_bool, device):
    """bool [B,H,nq,nk] -> (idx int32 [B,H,nq,nk] ascending kept columns, cnt int32 [B,H,nq])."""
    m = torch.as_tensor(mask_bool).to(device)
    nk = m.shape[-1]
    order = torch.argsort((~m).to(torch.int8), dim=-1, stable=True).to(torch.int32)
    return order.contiguous(), m.sum(-1).to(torch.int32).contiguous()


# ----------------------------------------------------------------------------------------------- geometry
def test_gilbert_small_verbatim(golden_dir, dev):
    from jenga_amd import gilbert as G
    g = np.load(os.path.join(golden_dir, "gilbert_small.npz"))
    for key in g.files:
        kind, t, h, w, what = key.split("_")
        t, h, w = int(t), int(h), int(w)
        mapping = G.gilbert_mapping if kind == "g" else G.sliced_gilbert_mapping
        if what in ("l2h", "h2l"):
            l2h, h2l = mapping(t, h, w)
            assert isinstance(l2h, list)
            got = np.asarray(l2h if what == "l2h" else h2l, dtype=np.int64)
        else:
            fn = G.gilbert_block_neighbor_mapping if kind == "g" else G.sliced_gilbert_block_neighbor_mapping
            got = fn(t, h, w, int(what[2:])).numpy()
        assert np.array_equal(got, g[key]), key


def test_gilbert_transposed_orders_verbatim(golden_dir, dev):
    """transpose_order through the three public entry points (gilbert.py:274-330, :436-438, :484-486) against goldens
    generated from the reference; the block-neighbour functions accept the argument and ignore it like the reference."""
    from jenga_amd import gilbert as G
    g = np.load(os.path.join(golden_dir, "gilbert_transposed.npz"))
    for key in g.files:
        _, t, h, w, o, what = key.split("_")
        dims, order = (int(t), int(h), int(w)), [int(c) for c in o[1:]]
        for fn in (lambda: G.transpose_gilbert_mapping(dims, order), lambda: G.gilbert_mapping(*dims, transpose_order=order),
                   lambda: G.sliced_gilbert_mapping(*dims, transpose_order=order)):
            l2h, h2l = fn()
            assert isinstance(l2h, list)
            assert np.array_equal(np.asarray(l2h if what == "l2h" else h2l, dtype=np.int64), g[key]), key
    nb_t = G.gilbert_block_neighbor_mapping(3, 4, 5, 8, transpose_order=[2, 1, 0])
    assert torch.equal(nb_t, G.gilbert_block_neighbor_mapping(3, 4, 5, 8))
    with pytest.raises(ValueError):
        G.transpose_gilbert_mapping((2, 2, 2), [0, 1, 1])


def test_gilbert_production_grids_sha(golden_dir, dev):
    from jenga_amd import gilbert as G
    d = json.load(open(os.path.join(golden_dir, "gilbert_big_digests.json")))
    for key, v in d.items():
        kind, t, h, w = key.split("_")
        t, h, w = int(t), int(h), int(w)
        if kind == "g":
            l2h, h2l = G.gilbert_mapping(t, h, w, as_tensor=True)
            nb = G.gilbert_block_neighbor_mapping(t, h, w)
        else:
            l2h, h2l = G.sliced_gilbert_mapping(t, h, w, as_tensor=True)
            nb = G.sliced_gilbert_block_neighbor_mapping(t, h, w)
        assert _sha(l2h.cpu().numpy()) == v["l2h_sha256"], key
        assert _sha(h2l.cpu().numpy()) == v["h2l_sha256"], key
        assert _sha(nb.numpy().astype(np.uint8)) == v["nb128_sha256"], key


def test_gather_scatter_roundtrip(dev):
    from jenga_amd import _capi, gilbert as G
    l2h, h2l = G.gilbert_mapping(4, 6, 10, as_tensor=True)
    x = torch.randn(2, 240, 3072, device=dev).to(torch.bfloat16)
    y = _capi.gather_rows(x, h2l)
    assert torch.equal(y, x[:, h2l])
    assert torch.equal(_capi.gather_rows(y, l2h), x)


# ----------------------------------------------------------------------------------------------- norm + rope
@pytest.mark.parametrize("tag,dt", [("bf16", "bfloat16"), ("fp16", "float16")])
def test_rmsnorm_rope_vs_reference_golden(golden_dir, dev, tag, dt):
    from jenga_amd.modules.norm_layers import RMSNorm
    from jenga_amd.modules.posemb_layers import apply_rotary_emb, get_nd_rotary_pos_embed, qk_norm_rope
    g = np.load(os.path.join(golden_dir, "norm_rope_cases.npz"))
    cos, sin = get_nd_rotary_pos_embed([16, 56, 56], [3, 4, 6], theta=256, use_real=True, theta_rescale_factor=1)
    assert np.array_equal(cos.numpy(), g["rope_3_4_6_cos"]) and np.array_equal(sin.numpy(), g["rope_3_4_6_sin"])
    tdt = getattr(torch, dt)
    xq, xk = from_bits(g[f"{tag}_xq"], dt).to(dev), from_bits(g[f"{tag}_xk"], dt).to(dev)
    wq, wk = from_bits(g[f"{tag}_wq"], dt).to(dev), from_bits(g[f"{tag}_wk"], dt).to(dev)
    nq = RMSNorm(128, dtype=tdt, device=dev)
    nq.weight.data.copy_(wq)
    y = nq(xq)
    # a 1-ulp flip of the normalised value (fp32 order of the 128-term mean) times a weight in [0.7,1.3] -> <= 2 ulp
    assert_ulp_close(to_np(y), to_np(from_bits(g[f"{tag}_nq"], dt)), dt, max_ulps=2)
    # RoPE alone on the reference's normed tensors: bit-exact
    rq, rk = apply_rotary_emb(from_bits(g[f"{tag}_nq"], dt).to(dev), from_bits(g[f"{tag}_nk"], dt).to(dev), (cos, sin))
    assert np.array_equal(to_np(rq), to_np(from_bits(g[f"{tag}_rq"], dt)))
    assert np.array_equal(to_np(rk), to_np(from_bits(g[f"{tag}_rk"], dt)))
    # fused path: same as the two steps
    fq, fk = qk_norm_rope(xq, xk, wq, wk, (cos, sin))
    assert_ulp_close(to_np(fq), to_np(from_bits(g[f"{tag}_rq"], dt)), dt, max_frac=2e-3, max_ulps=2, rowwise=True)
    assert_ulp_close(to_np(fk), to_np(from_bits(g[f"{tag}_rk"], dt)), dt, max_frac=2e-3, max_ulps=2, rowwise=True)


@pytest.mark.parametrize("tag,dt", [("bf16", "bfloat16"), ("fp16", "float16")])
def test_other_forms_of_the_pre_ops_vs_reference_golden(golden_dir, dev, tag, dt):
    """The forms of the reference's pre-ops no Jenga entry script uses (posemb_layers.py:181-229 head_first=True and a complex
    freqs_cis; norm_layers.py:5-59 at a width other than 128), against the reference's own outputs: RoPE bit for bit, RMSNorm
    <= 2 ulp (the order of the mean is free)."""
    from jenga_amd.modules.norm_layers import RMSNorm
    from jenga_amd.modules.posemb_layers import apply_rotary_emb
    g = np.load(os.path.join(golden_dir, "rope_forms_cases.npz"))
    tdt = getattr(torch, dt)
    xq, xk = from_bits(g[f"{tag}_xq"], dt).to(dev), from_bits(g[f"{tag}_xk"], dt).to(dev)
    cos, sin = torch.from_numpy(g["cos"]), torch.from_numpy(g["sin"])
    cis = torch.complex(torch.from_numpy(g["cis_real"]), torch.from_numpy(g["cis_imag"]))
    cq, ck = apply_rotary_emb(xq, xk, cis, head_first=False)
    assert np.array_equal(to_np(cq), to_np(from_bits(g[f"{tag}_complex_q"], dt)))
    assert np.array_equal(to_np(ck), to_np(from_bits(g[f"{tag}_complex_k"], dt)))
    hq, hk = apply_rotary_emb(xq.transpose(1, 2).contiguous(), xk.transpose(1, 2).contiguous(), (cos, sin), head_first=True)
    assert hq.shape == (1, 3, 72, 128) and hq.is_contiguous()
    assert np.array_equal(to_np(hq), to_np(from_bits(g[f"{tag}_headfirst_q"], dt)))
    assert np.array_equal(to_np(hk), to_np(from_bits(g[f"{tag}_headfirst_k"], dt)))
    for C in (256, 3072):
        x = from_bits(g[f"{tag}_rms{C}_x"], dt).to(dev)
        n = RMSNorm(C, dtype=tdt, device=dev)
        n.weight.data.copy_(from_bits(g[f"{tag}_rms{C}_w"], dt).to(dev))
        assert_ulp_close(to_np(n(x)), to_np(from_bits(g[f"{tag}_rms{C}_y"], dt)), dt, max_frac=2e-3, max_ulps=2)
        n0 = RMSNorm(C, elementwise_affine=False, eps=1e-5, dtype=tdt, device=dev)
        assert_ulp_close(to_np(n0(x)), to_np(from_bits(g[f"{tag}_rms{C}_y_noweight"], dt)), dt, max_frac=2e-3, max_ulps=2)
    with pytest.raises(ValueError):
        RMSNorm(100, dtype=tdt, device=dev)(torch.zeros(2, 100, dtype=tdt, device=dev))      # not a multiple of 8
    with pytest.raises(ValueError):
        RMSNorm(128, dtype=tdt, device=dev)(torch.zeros(2, 256, dtype=tdt, device=dev))      # width mismatch


def test_rmsnorm_rope_strided_qkv_vs_oracle(dev):
    """q/k as strided views of a fused QKV projection output, RoPE on the first s_rope tokens only."""
    from jenga_amd import _capi
    from oracle import norm_rope as onr
    torch.manual_seed(3)
    B, S, H, s_rope = 1, 40, 5, 24
    qkv = (torch.randn(B, S, 3 * H * 128) * 1.7).to(torch.bfloat16).to(dev)
    q = qkv.view(B, S, 3, H, 128)[:, :, 0]
    w = (1 + 0.1 * torch.randn(128)).to(torch.bfloat16).to(dev)
    cos, sin = onr.rope_tables([16, 56, 56], [2, 3, 4], 256.0)
    out = _capi.rmsnorm_rope(q, w, torch.from_numpy(cos).to(dev), torch.from_numpy(sin).to(dev), s_rope=s_rope)
    ref = onr.rmsnorm(to_np(q), to_np(w), "bfloat16")
    ref[:, :s_rope] = onr.apply_rotary_emb(ref[:, :s_rope], cos, sin, "bfloat16")
    assert_ulp_close(to_np(out), ref, "bfloat16", max_frac=2e-3, max_ulps=2, rowwise=True)


# ----------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("index", range(len(inputs.SELECT_SPECS)))
def test_select_vs_reference_golden(golden_dir, dev, index):
    from jenga_amd.modules.attention_block_sparse import build_block_index
    from oracle import attention as oa
    name, flav, dt, H, nb_img, tb, top_k, p, temp, ffb = inputs.SELECT_SPECS[index]
    g = np.load(os.path.join(golden_dir, "select_cases.npz"))
    q, k = inputs.select_inputs(index)          # [1,H,S,128]
    nbm = g["neighbors"]
    # the op takes [B,S,H,D]; q carries image tokens only -> append zero text rows (they are not pooled for q)
    qf = torch.cat([q, torch.zeros(1, H, tb * 128, 128, dtype=q.dtype)], dim=2) if tb else q
    mask, idx, cnt = build_block_index(qf.transpose(1, 2).to(dev), k.transpose(1, 2).to(dev), top_k, tb, p,
                                       torch.from_numpy(nbm), first_frame_blocks=ffb, want_mask=True)
    mask = mask.bool().cpu().numpy()
    ref = g[f"{name}_mask"]
    probs = g[f"{name}_probs_f32"][None]
    n = g[f"{name}_n"][None]
    forced = np.zeros_like(ref)
    forced[..., :nb_img] |= nbm[None, None, :nb_img, :nb_img]
    if ffb:
        forced[:, :, :ffb, :ffb] = True
    ok, msg = tie_tolerant_mask_equal(mask, ref, probs, n, nb_img, forced)
    ham = int((mask != ref).sum())
    # every recorded run of rounds 2-3 is tie-exact on all eight cases (profiles/r03_parity_select_hamming.json): the test
    # demands exactly that -- any differing entry must lie inside a group of equal bf16 probabilities at the cutoff
    assert ok, f"{msg}; hamming={ham}/{ref.size}"
    # lists agree with the mask
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    for h in range(H):
        for r in range(nb_img):
            c = cnt[0, h, r]
            assert c == mask[0, h, r].sum()
            assert np.array_equal(idx[0, h, r, :c], np.nonzero(mask[0, h, r])[0])


def test_select_vs_oracle_larger(dev):
    from jenga_amd.modules.attention_block_sparse import build_block_index
    from oracle import attention as oa
    from oracle import gilbert as og
    gen = torch.Generator().manual_seed(77)
    H, nb_img, tb = 3, 96, 2
    q, k = inputs.peaky_qk(gen, 1, H, nb_img, nb_img + tb, 128, 1.0)
    q, k = q.to(torch.bfloat16), k.to(torch.bfloat16)
    nbm = og.gilbert_block_neighbor_mapping(8, 16, 96, 128)   # 12288 tokens = 96 blocks
    ref = oa.build_block_mask(to_np(q), to_np(k), 10, nb_img, nb_img + tb, 0.3, tb, nbm, "bfloat16")
    qf = torch.cat([q, torch.zeros(1, H, tb * 128, 128, dtype=q.dtype)], dim=2)
    mask, idx, cnt = build_block_index(qf.transpose(1, 2).to(dev), k.transpose(1, 2).to(dev), 10, tb, 0.3,
                                       torch.from_numpy(nbm), want_mask=True)
    ham = int((mask.bool().cpu().numpy() != ref).sum())
    # (the oracle pools with numpy's summation order, the kernel with its own: a pooled mean may differ by one bf16 ulp and
    # move a boundary block; the realised distance goes to gpurun_out/parity_records/, the bound is a tenth of round 3's)
    try:
        rec_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_records")
        os.makedirs(rec_dir, exist_ok=True)
        import json
        json.dump({"hamming": ham, "of": int(ref.size)}, open(os.path.join(rec_dir, "select_vs_oracle_larger.json"), "w"))
    except OSError:
        pass
    assert ham <= ref.size // 5000, f"hamming {ham}/{ref.size}"


# ----------------------------------------------------------------------------------------------- sparse kernel
def _run_kernel(q_bhsd, k_bhsd, v_bhsd, mask, seqlen, amp, nb_img, dev, flags=None, sm_scale=None):
    """inputs in the reference kernel's [B,H,S,D] layout -> o [B,H,Sq_img,D] (image rows only)."""
    from jenga_amd import _capi
    B, H, Sq, D = q_bhsd.shape
    S = k_bhsd.shape[2]
    nb = S // 128
    qfull = torch.zeros(B, H, S, D, dtype=q_bhsd.dtype)
    qfull[:, :, :Sq] = q_bhsd
    q = qfull.transpose(1, 2).contiguous().to(dev)          # [B,S,H,D]
    k = k_bhsd.transpose(1, 2).contiguous().to(dev)
    v = v_bhsd.transpose(1, 2).contiguous().to(dev)
    idx, cnt = lists_from_mask(mask, dev)
    vt = _capi.pack_v(v, nb)
    seqlens = torch.tensor([seqlen] * B, dtype=torch.int32, device=dev)
    o = _capi.bsattn_fwd(q, k, vt, seqlens, idx, cnt, nb_img, D ** -0.5 if sm_scale is None else sm_scale, amp, nb_img,
                         flags=flags)
    torch.cuda.synchronize()
    return o.transpose(1, 2)[:, :, :Sq].float().cpu().numpy()


@pytest.mark.parametrize("index", range(len(inputs.KERNEL_SPECS)))
def test_sparse_kernel_vs_triton_interpreter_golden(golden_dir, dev, index):
    H, nb_img, tb, seqlen_txt, amp, seed = inputs.KERNEL_SPECS[index]
    g = np.load(os.path.join(golden_dir, "attn_cases.npz"))
    q, k, v, mask, seqlen, amp = inputs.kernel_inputs(index)
    o = _run_kernel(q, k, v, mask, seqlen, amp, nb_img, dev)
    ref = g[f"k{index}_o"].astype(np.float32)
    err = np.abs(o - ref)
    # fp16: identical rounding points; differences = fp32 summation order + v_exp_f32 (1 ulp) -> a few fp16 ulps
    assert err.max() <= 6e-3, err.max()
    assert (err > 2e-3).mean() < 2e-3


@pytest.mark.parametrize("flags", [None, 85], ids=["default", "pair"])
@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
@pytest.mark.parametrize("index", range(len(inputs.KERNEL_SPECS)))
def test_sparse_kernel_vs_reference_kernel_in_the_product_dtype(golden_dir, dev, index, dt, flags):
    """attn_exact_cases.npz = the reference Triton kernel itself (interpreter, fp32 `qk_scale` argument as compiled; the
    oracle matches it bit for bit, tests/test_oracle_golden.py).  The HIP kernels differ from it only in the order of the
    fp32 sums inside the MFMA dots and in v_exp_f32 (1 ulp): a few ulps of the storage type at |o| <= 2."""
    H, nb_img, tb, seqlen_txt, amp, seed = inputs.KERNEL_SPECS[index]
    tdt = getattr(torch, dt)
    g = np.load(os.path.join(golden_dir, "attn_exact_cases.npz"))
    q, k, v, mask, seqlen, amp = inputs.kernel_inputs(index, dtype=tdt)
    o = _run_kernel(q, k, v, mask, seqlen, amp, nb_img, dev, flags=flags)
    ref = torch.from_numpy(g[f"k{index}_o" + ("" if dt == "bfloat16" else "_fp16")]).view(tdt).float().numpy()
    err = np.abs(o - ref)
    tol = 1.6e-2 if dt == "bfloat16" else 4e-3            # 2 ulp (bf16: 2^-7 at |o| in [1,2)) / 4 ulp (fp16)
    assert err.max() <= tol, err.max()
    assert (err > tol / 4).mean() < 2e-3 and err.mean() < tol / 40


@pytest.mark.parametrize("flags", [None, 85], ids=["default", "pair"])
@pytest.mark.parametrize("D", inputs.NARROW_HEAD_DIMS)
def test_narrow_heads_kernel_vs_reference_kernel(golden_dir, dev, D, flags):
    """Head dims 64 / 32 / 16: the 128-channel kernels on zero-padded channels, sm_scale = D ** -0.5, against the reference
    kernel's own bf16 output at that head dim (attn_exact_cases.npz)."""
    g = np.load(os.path.join(golden_dir, "attn_exact_cases.npz"))
    q, k, v, mask, seqlen, amp = inputs.narrow_kernel_inputs(D)
    pad = lambda t: torch.nn.functional.pad(t, [0, 128 - D])
    o = _run_kernel(pad(q), pad(k), pad(v), mask, seqlen, amp, q.shape[2] // 128, dev, flags=flags, sm_scale=D ** -0.5)
    assert np.abs(o[..., D:]).max() == 0.0                 # zero V channels -> exact zeros
    ref = torch.from_numpy(g[f"d{D}_o"]).view(torch.bfloat16).float().numpy()
    err = np.abs(o[..., :D] - ref)
    assert err.max() <= 3.2e-2, err.max()                  # 2 bf16 ulp at |o| in [2,4)
    assert err.mean() < 1.5e-3                             # (a rounding flip of the bf16 output costs 2e-3 at |o| ~ 0.5)


@pytest.mark.parametrize("D", inputs.NARROW_HEAD_DIMS)
def test_narrow_heads_whole_op_vs_oracle(dev, D):
    """The op at head dims 64 / 32 / 16 (HY flavour): selection with head_dim ** -0.5 (JENGA_SELECT_HEAD_DIM), attention,
    text rows -- every row against the oracle run at the true head dim on the HIP pooling kernel's block means."""
    from jenga_amd import _capi
    from jenga_amd.modules import attention_block_sparse as op
    from oracle import attention as oa
    from oracle import gilbert as og
    gen = torch.Generator().manual_seed(50 + D)
    H, tb = 2, 2
    nbm = og.gilbert_block_neighbor_mapping(2, 8, 64, 128)   # 1024 tokens = 8 blocks
    S = 10 * 128
    q, k = inputs.peaky_qk(gen, 1, H, 10, 10, D, 0.8)
    q = q.transpose(1, 2).to(torch.bfloat16).contiguous()
    k = k.transpose(1, 2).to(torch.bfloat16).contiguous()
    v = torch.randn(1, S, H, D, generator=gen).to(torch.bfloat16)
    cu = torch.tensor([0, 8 * 128 + 60, S], dtype=torch.int32)
    o = op.block_sparse_attention(q.to(dev), k.to(dev), v.to(dev), 3, cu_seqlens_q=cu.to(dev), cu_seqlens_kv=cu.to(dev),
                                  text_blocks=tb, text_amp=0.2, block_neighbor_list=torch.from_numpy(nbm),
                                  p_remain_rates=0.3)
    assert o.shape == (1, S, H * D)
    pad = lambda t: torch.nn.functional.pad(t, [0, 128 - D]).to(dev)
    qp = _capi.block_pool(pad(q), 8).float().cpu().numpy()[..., :D]
    kp = _capi.block_pool(pad(k), 10).float().cpu().numpy()[..., :D]
    ref = oa.block_sparse_attention(to_np(q), to_np(k), to_np(v), 3, "bfloat16", cu_seqlens_q=cu.numpy(), text_blocks=tb,
                                    text_amp=0.2, block_neighbor_list=nbm, p_remain_rates=0.3, pooled=(qp, kp))
    err = np.abs(o.float().cpu().numpy().reshape(ref.shape) - ref)
    assert np.median(err) < 2e-3 and int((err.max(-1) > 3e-2).sum()) == 0, err.max()


@pytest.mark.parametrize("dt,flags", [("bfloat16", None), ("float16", None), ("bfloat16", 9), ("float16", 8), ("bfloat16", 25),
                                      ("bfloat16", 0), ("bfloat16", 1), ("float16", 1),
                                      ("bfloat16", 65), ("float16", 64), ("bfloat16", 69)])
def test_sparse_kernel_vs_oracle(dev, dt, flags):
    """flags None = the default: the LP kernel (JENGA_ATTN_LP, csrc/bsattn3.hip) with the XCD remap = 9; 8 = LP in plain
    workgroup order; 25 = LP with the kept-count-aware launch order (ATTN_SORTED); 0 / 1 = no kernel bit = the round-1
    kernel (csrc/bsattn.hip); 64 / 65 / 69 = the pair kernel (csrc/bsattn5.hip; plain order / XCD remap / balanced launch)
    -- all held to the same tolerance."""
    from jenga_amd import _capi
    from oracle import attention as oa
    gen = torch.Generator().manual_seed(11)
    H, nb_img, tb = 3, 9, 2
    S = (nb_img + tb) * 128
    tdt = getattr(torch, dt)
    q = (torch.randn(1, H, nb_img * 128, 128, generator=gen) * 1.5).to(tdt)
    k = (torch.randn(1, H, S, 128, generator=gen) * 1.5).to(tdt)
    v = torch.randn(1, H, S, 128, generator=gen).to(tdt)
    mask = torch.rand(1, H, nb_img, nb_img + tb, generator=gen) < 0.4
    mask[..., nb_img:] = True
    mask[..., 0] = True
    seqlen = nb_img * 128 + 37          # first text block partially valid, second fully masked
    o = _run_kernel(q, k, v, mask, seqlen, 0.431, nb_img, dev, flags=flags)
    ref = oa.sparse_rows(to_np(q), to_np(k), to_np(v), [seqlen], mask.numpy(), 128 ** -0.5, dt, 0.431, nb_img)
    tol = 2e-2 if dt == "bfloat16" else 4e-3     # 2-3 ulp of the storage dtype at |o| <= ~2
    assert np.abs(o - ref).max() <= tol, np.abs(o - ref).max()
    assert np.abs(o - ref).mean() <= tol / 20


def test_whole_op_vs_reference_golden(golden_dir, dev):
    from jenga_amd.modules.attention_block_sparse import block_sparse_attention
    s = inputs.OP_SPEC
    g = np.load(os.path.join(golden_dir, "attn_cases.npz"))
    q, k, v, cu = inputs.op_inputs()
    o = block_sparse_attention(q.to(dev), k.to(dev), v.to(dev), top_k=s["top_k"], cu_seqlens_q=cu.to(dev),
                               cu_seqlens_kv=cu.to(dev), text_blocks=s["text_blocks"], text_amp=s["text_amp"],
                               block_neighbor_list=torch.from_numpy(g["op_neighbors"]), p_remain_rates=s["p"])
    ref = g["op_o"].astype(np.float32)
    assert o.shape == ref.shape
    err = np.abs(o.float().cpu().numpy() - ref)
    assert err.max() <= 6e-3, err.max()


@pytest.mark.parametrize("flavour", ["hy", "i2v", "wan"])
def test_whole_op_flavours_vs_oracle(dev, flavour):
    from jenga_amd.modules import attention_block_sparse as op
    from oracle import attention as oa
    from oracle import gilbert as og
    gen = torch.Generator().manual_seed(5)
    H = 2
    nbm = og.gilbert_block_neighbor_mapping(2, 8, 64, 128)   # 1024 tokens = 8 blocks
    if flavour == "hy":
        S, tb = 10 * 128, 2
    elif flavour == "i2v":
        S, tb = 8 * 128 + 4 * 128 - 50, 4      # padded up to 12 blocks
    else:
        S, tb = 8 * 128 - 30, 0                # wan: 994 tokens padded to 8 blocks
    q, k = inputs.peaky_qk(gen, 1, H, 12, 12, 128, 0.8)
    q = q[:, :, :S].transpose(1, 2).to(torch.bfloat16).contiguous()
    k = k[:, :, :S].transpose(1, 2).to(torch.bfloat16).contiguous()
    v = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
    cu = torch.tensor([0, 8 * 128 + 60, S], dtype=torch.int32)
    if flavour == "hy":
        o = op.block_sparse_attention(q.to(dev), k.to(dev), v.to(dev), 3, cu_seqlens_q=cu.to(dev),
                                      cu_seqlens_kv=cu.to(dev), text_blocks=tb, text_amp=0.2,
                                      block_neighbor_list=torch.from_numpy(nbm), p_remain_rates=0.3)
        ref = oa.block_sparse_attention(to_np(q), to_np(k), to_np(v), 3, "bfloat16", cu_seqlens_q=cu.numpy(),
                                        text_blocks=tb, text_amp=0.2, block_neighbor_list=nbm, p_remain_rates=0.3,
                                        pooled=hip_pooled(q, k, tb, dev))
    elif flavour == "i2v":
        o = op.block_sparse_attention_i2v(q.to(dev), k.to(dev), v.to(dev), 3, cu_seqlens_q=cu.to(dev),
                                          cu_seqlens_kv=cu.to(dev), text_amp=0.2,
                                          block_neighbor_list=torch.from_numpy(nbm), p_remain_rates=0.3)
        ref = oa.block_sparse_attention(to_np(q), to_np(k), to_np(v), 3, "bfloat16", cu_seqlens_q=cu.numpy(),
                                        text_blocks=4, text_amp=0.2, block_neighbor_list=nbm, p_remain_rates=0.3,
                                        flavour="i2v", pooled=hip_pooled(q, k, 4, dev))
    else:
        o = op.block_sparse_attention_wan(q.to(dev), k.to(dev), v.to(dev), 3, block_neighbor_list=torch.from_numpy(nbm),
                                          p_remain_rates=0.5, first_frame_blocks=2)
        ref = oa.block_sparse_attention(to_np(q), to_np(k), to_np(v), 3, "bfloat16", text_blocks=0,
                                        block_neighbor_list=nbm, p_remain_rates=0.5, flavour="wan",
                                        first_frame_blocks=2, pooled=hip_pooled(q, k, 0, dev))
    o = o.float().cpu().numpy()
    assert o.shape == ref.shape
    err = np.abs(o - ref)
    # the oracle selects from the HIP kernel's own pooled means (helpers.hip_pooled): no selection flip is possible, EVERY
    # row has to agree (round 4 allowed 2 % of the rows to differ by a flipped block)
    assert (err.max(axis=-1) > 3e-2).sum() == 0, (int((err.max(axis=-1) > 3e-2).sum()), float(err.max()))
    assert np.median(err) <= 2e-3


# ----------------------------------------------------------------------------------------------- Wan flavour
def test_wan_preops_vs_reference_golden(golden_dir, dev):
    from jenga_amd.modules import wan as W
    g = np.load(os.path.join(golden_dir, "wan_cases.npz"))
    freqs = W.wan_freqs()
    assert np.array_equal(freqs.real[:8].numpy(), g["freqs_re_head"])
    x = from_bits(g["x"], "bfloat16").to(dev)
    grid = torch.tensor([[3, 4, 5]])
    r = W.rope_apply(x, grid, freqs)
    assert r.dtype == torch.float32 and np.array_equal(r.cpu().numpy(), g["rope"])           # fp64 math: bit-exact
    r2 = W.rope_apply(x, grid, freqs, torch.from_numpy(g["remap"]))
    assert np.array_equal(r2.cpu().numpy(), g["rope_remap"])
    rb = W.rope_apply(x, grid, freqs, out_dtype=torch.bfloat16)                               # fused cast
    assert torch.equal(rb.cpu(), torch.from_numpy(g["rope"]).to(torch.bfloat16))
    norm = W.WanRMSNorm(1536, eps=1e-6).to(dev)
    norm.weight.data.copy_(torch.from_numpy(g["norm_w"]))
    y = norm(from_bits(g["norm_x"], "bfloat16").to(dev))
    assert y.dtype == torch.float32
    assert_ulp_close(y.cpu().numpy(), g["norm_y"], "bfloat16", max_ulps=2)


@pytest.mark.parametrize("rate", [0.0, 0.7])
def test_wan_self_attention_vs_oracle_composition(dev, rate):
    """WanSelfAttention.forward: q/k/v linears (torch) -> WanRMSNorm -> fp64 RoPE -> dense (rate<=0.25) or AttenCarve."""
    from jenga_amd.modules import wan as W
    from oracle import attention as oa
    from oracle import gilbert as og
    from oracle import wan as ow
    torch.manual_seed(0)
    dim, heads, grid = 256, 2, (3, 16, 21)            # 1008 tokens -> padded to 8 blocks by the op
    S = grid[0] * grid[1] * grid[2]
    att = W.WanSelfAttention(dim, heads, dtype=torch.bfloat16, device=dev)
    for lin in (att.q, att.k, att.v, att.o):
        lin.weight.data.normal_(0, 0.08)
    x = torch.randn(1, S, dim, device=dev).to(torch.bfloat16)
    nbm = og.sliced_gilbert_block_neighbor_mapping(*grid, 128)
    l2h, h2l = og.sliced_gilbert_mapping(*grid)
    remap = torch.from_numpy(h2l)
    freqs = W.wan_freqs()
    out = att(x, torch.tensor([S]), torch.tensor([list(grid)]), freqs, sa_drop_rate=rate, p_remain_rates=0.8,
              freq_remap=remap, block_neighbor_list=torch.from_numpy(nbm))
    # oracle composition on the same linear outputs
    with torch.no_grad():
        q, k, v = att.q(x), att.k(x), att.v(x)
    wq, wk = att.norm_q.weight.detach().cpu().numpy(), att.norm_k.weight.detach().cpu().numpy()
    rnd = lambda a: torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    qn = ow.wan_rmsnorm(to_np(q), wq, "bfloat16", 1e-6).reshape(1, S, heads, 128)
    kn = ow.wan_rmsnorm(to_np(k), wk, "bfloat16", 1e-6).reshape(1, S, heads, 128)
    fr = ow.wan_freqs()
    qr, kr = rnd(ow.rope_apply(qn, grid, fr, h2l)), rnd(ow.rope_apply(kn, grid, fr, h2l))
    vv = to_np(v).reshape(1, S, heads, 128)
    nb = 8
    if rate <= 0.25:
        ref = oa.block_sparse_attention(qr, kr, vv, nb, "bfloat16", text_blocks=0, block_neighbor_list=None,
                                        p_remain_rates=2.0, flavour="wan")
    else:
        import math
        ref = oa.block_sparse_attention(qr, kr, vv, math.ceil(int(nb * (1 - rate))), "bfloat16", text_blocks=0,
                                        block_neighbor_list=nbm, p_remain_rates=0.8, flavour="wan",
                                        first_frame_blocks=math.ceil(nb // 21))
    with torch.no_grad():
        want = att.o(torch.from_numpy(ref).to(torch.bfloat16).to(dev))
    err = (out.float() - want.float()).abs()
    assert err.mean().item() <= 3e-3 and (err.max(-1).values > 0.08).float().mean().item() <= 0.02, \
        (err.max().item(), err.mean().item())


@pytest.mark.parametrize("dt", ["bfloat16", "float16"])
def test_sparse_kernel_running_max_jumps(dev, dt):
    """Forces the rare branches of the lazy running max: keys whose score exceeds everything seen before by ~30,
    ~100 and > 127 log2 units (the last one overflows exp2 against the stale reference), placed in late tiles and in
    both 64-key halves.  Bounded random data never takes these branches, so this test is the only thing guarding them."""
    from oracle import attention as oa
    gen = torch.Generator().manual_seed(23)
    H, nb_img, tb = 2, 8, 1
    S = (nb_img + tb) * 128
    tdt = getattr(torch, dt)
    q = torch.randn(1, H, nb_img * 128, 128, generator=gen)
    k = torch.randn(1, H, S, 128, generator=gen)
    v = torch.randn(1, H, S, 128, generator=gen)
    # (query row, key row, gain): key = gain * query  ->  score ~ gain * 128 * 0.1275 log2 units
    for (qr, kr, gain) in [(5, 3 * 128 + 7, 1.8), (200, 5 * 128 + 100, 6.0), (201, 6 * 128 + 2, 9.5),
                           (640, 7 * 128 + 70, 9.0), (641, 2 * 128 + 33, 2.5)]:
        k[0, :, kr] = gain * q[0, :, qr]
    q, k, v = q.to(tdt), k.to(tdt), v.to(tdt)
    mask = torch.ones(1, H, nb_img, nb_img + tb, dtype=torch.bool)
    seqlen = nb_img * 128 + 50
    o = _run_kernel(q, k, v, mask, seqlen, 0.0, nb_img, dev)
    ref = oa.sparse_rows(to_np(q), to_np(k), to_np(v), [seqlen], mask.numpy(), 128 ** -0.5, dt, 0.0, nb_img)
    assert np.isfinite(o).all()
    tol = 3e-2 if dt == "bfloat16" else 6e-3
    assert np.abs(o - ref).max() <= tol, np.abs(o - ref).max()
    for qr in (5, 200, 201, 640, 641):            # the spiked rows themselves: softmax collapses onto one key
        assert np.abs(o[0, :, qr] - ref[0, :, qr]).max() <= tol


def test_dense_path_vs_oracle(dev):
    """sa_drop_rate == 0 (attenion.py:108-121, flash_attn_varlen over the valid | padding segments): valid rows must
    match softmax over the valid keys, the padding rows softmax over the padding keys (both segments since round 6)."""
    from jenga_amd.modules.attention import attention, get_cu_seqlens
    from oracle import attention as oa
    gen = torch.Generator().manual_seed(31)
    H, S_img, S_txt, valid = 2, 512, 256, 90
    S = S_img + S_txt
    q = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
    k = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
    v = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
    mask = torch.zeros(1, S_txt, dtype=torch.int64)
    mask[:, :valid] = 1
    cu = get_cu_seqlens(mask.to(dev), S_img)
    assert cu.tolist() == [0, S_img + valid, S]
    o = attention(q.to(dev), k.to(dev), v.to(dev), cu_seqlens_q=cu, cu_seqlens_kv=cu).float().cpu().numpy()
    tr = lambda t: np.transpose(to_np(t), (0, 2, 1, 3))
    ref = oa.dense_varlen(tr(q), tr(k), tr(v), [0, S_img + valid, S], 128 ** -0.5, "bfloat16")
    ref = np.transpose(ref, (0, 2, 1, 3)).reshape(1, S, H * 128)
    n = S_img + valid
    assert np.abs(o[:, :n] - ref[:, :n]).max() <= 2e-2
    assert np.abs(o[:, n:] - ref[:, n:]).max() <= 2e-2 and np.abs(o[:, n:]).max() > 0.05
    # no padding at all, and a padding segment longer than one block
    for valid2 in (S_txt, 20):
        mask2 = torch.zeros(1, S_txt, dtype=torch.int64)
        mask2[:, :valid2] = 1
        cu2 = get_cu_seqlens(mask2.to(dev), S_img)
        o2 = attention(q.to(dev), k.to(dev), v.to(dev), cu_seqlens_q=cu2, cu_seqlens_kv=cu2).float().cpu().numpy()
        ref2 = oa.dense_varlen(tr(q), tr(k), tr(v), [0, S_img + valid2, S], 128 ** -0.5, "bfloat16")
        assert np.abs(o2 - np.transpose(ref2, (0, 2, 1, 3)).reshape(1, S, H * 128)).max() <= 2e-2


# ----------------------------------------------------------------------------------------------- DiT block glue
@pytest.mark.parametrize("C", [3072, 1024, 2560])     # 3072 / 1024: the wave-per-row kernel (round 4); 2560: block per row
def test_fused_elementwise_vs_eager_chain(dev, C):
    """jenga_ln_modulate / jenga_gate_residual / jenga_gelu_tanh against the eager torch chains of the reference blocks
    (every op result rounded to bf16), incl. the I2V token-replace selection and strided views."""
    import torch.nn.functional as F
    from jenga_amd import _capi
    g = torch.Generator(device=dev).manual_seed(9)
    S = 301
    x = (torch.randn(1, S, C, generator=g, device=dev) * 2 + 0.3).to(torch.bfloat16)
    vecs = [(0.2 * torch.randn(1, C, generator=g, device=dev)).to(torch.bfloat16) for _ in range(6)]
    sh, sc, gt, sh2, sc2, gt2 = vecs
    mask = torch.rand(S, generator=g, device=dev) < 0.3
    eager = lambda t, s_, c_: F.layer_norm(t, (C,), eps=1e-6) * (1 + c_.unsqueeze(1)) + s_.unsqueeze(1)
    y = _capi.ln_modulate(x, sh, sc)
    # x*(1+scale) and shift can cancel, so a one-ulp flip of an intermediate is measured at the row's scale
    assert_ulp_close(to_np(y), to_np(eager(x, sh, sc)), "bfloat16", max_frac=5e-3, max_ulps=2, rowwise=True)
    y2 = _capi.ln_modulate(x, sh, sc, shift2=sh2, scale2=sc2, mask=mask)
    ref2 = eager(x, sh, sc)
    ref2[:, mask] = eager(x, sh2, sc2)[:, mask]
    assert_ulp_close(to_np(y2), to_np(ref2), "bfloat16", max_frac=5e-3, max_ulps=2, rowwise=True)
    # gate + residual, y as a strided view
    big = torch.randn(1, S, 2 * C, generator=g, device=dev).to(torch.bfloat16)
    yv = big[..., C:]
    out = _capi.gate_residual(x, yv, gt)
    assert torch.equal(out, x + yv * gt.unsqueeze(1))
    out2 = _capi.gate_residual(x, yv, gt, gate2=gt2, mask=mask)
    ref = x + yv * gt.unsqueeze(1)
    ref[:, mask] = (x + yv * gt2.unsqueeze(1))[:, mask]
    assert torch.equal(out2, ref)
    # gelu into the right part of a concat buffer
    cat = torch.zeros(1, S, C + 512, device=dev, dtype=torch.bfloat16)
    src = big[..., :512]
    _capi.gelu_tanh(src, out=cat[..., C:])
    want = F.gelu(src, approximate="tanh")
    assert_ulp_close(to_np(cat[..., C:]), to_np(want), "bfloat16", max_frac=2e-3, max_ulps=1)
    assert torch.count_nonzero(cat[..., :C]) == 0


# ----------------------------------------------------------------------------------------------- full size (config 2)
def test_full_size_properties_and_sampled_rows(dev):
    """HunyuanVideo 720x1280x125f shape (S = 115200 + 256, real 32x45x80 curve neighbours), ALL 24 heads:
    (a) V == 1  ->  every output element is 1 (softmax weights sum to one through selection, kept lists, lazy max,
        both 64-key halves and the dense text rows) -- all heads, all rows;
    (b) EVERY kept list (24 x 900) is ascending, unique, contains the neighbours, the text blocks and at least top_k
        image blocks -- checked on the device;
    (c) 16 sampled (head, query block) rows against the oracle evaluated on exactly those rows' kept blocks."""
    from jenga_amd import _capi, gilbert as G
    from jenga_amd.modules import attention_block_sparse as op
    from oracle import attention as oa
    t, h, w = 32, 45, 80
    S_img, tb, H = t * h * w, 2, 24
    nimg, nb = S_img // 128, S_img // 128 + tb
    S = nb * 128
    nbm = G.gilbert_block_neighbor_mapping(t, h, w, as_tensor=True)
    g = torch.Generator(device=dev).manual_seed(77)
    cent = torch.randn(1, nb, 1, H, 128, generator=g, device=dev) * 0.9          # clustered block means: peaky rows
    q = (torch.randn(1, nb, 128, H, 128, generator=g, device=dev) + cent[:, torch.randint(0, nimg, (nb,), device=dev)])
    q = q.to(torch.bfloat16).view(1, S, H, 128)
    k = (torch.randn(1, nb, 128, H, 128, generator=g, device=dev) + cent).to(torch.bfloat16).view(1, S, H, 128)
    del cent
    top_k = int((1 - 0.75) * nimg)
    seqlens = torch.tensor([S], dtype=torch.int32, device=dev)
    # (a) rows of a softmax sum to one
    ones = torch.ones(1, S, H, 128, device=dev, dtype=torch.bfloat16)
    vt1 = _capi.pack_v(ones, nb)
    o1, idx, cnt = op.attencarve_packed(q, k, vt1, top_k, seqlens, tb, 0.2, 0.3, nbm, return_lists=True)
    assert torch.all((o1.float() - 1).abs() <= 2 ** -7), (o1.float() - 1).abs().max().item()
    del ones, vt1, o1
    # (b) list invariants, every row of every head
    valid = torch.arange(nb, device=dev)[None, None, None, :] < cnt[..., None]
    assert bool(((idx[..., 1:] > idx[..., :-1]) | ~valid[..., 1:]).all()), "a kept list is not strictly ascending"
    hit = torch.zeros(1, H, nimg, nb, dtype=torch.int32, device=dev)
    hit.scatter_add_(-1, torch.where(valid, idx, torch.zeros_like(idx)).long(), valid.to(torch.int32))
    assert bool((hit <= 1).all()) and bool((hit.sum(-1) == cnt).all()), "duplicate or out-of-range entries"
    assert bool((hit[..., nimg:] == 1).all()), "text blocks missing"
    assert bool(((hit[..., :nimg] == 1) | ~nbm.to(dev)[None, None]).all()), "a neighbour block is missing"
    assert int(cnt.min()) >= top_k + tb
    del hit, valid
    idx_c, cnt_c = idx.cpu(), cnt.cpu()
    # (c) sampled rows vs the oracle on their own kept blocks
    v = torch.randn(1, S, H, 128, generator=g, device=dev).to(torch.bfloat16)
    vt = _capi.pack_v(v, nb)
    o = op.attencarve_packed(q, k, vt, top_k, seqlens, tb, 0.2, 0.3, nbm)
    for (hh, m) in [(0, 0), (1, 449), (0, 899), (1, 77), (5, 1), (7, 898), (11, 300), (13, 601), (17, 112), (19, 113),
                    (23, 899), (23, 0), (2, 450), (9, 225), (21, 675), (15, 37)]:
        n = int(cnt_c[0, hh, m])
        blocks = idx_c[0, hh, m, :n].tolist()
        rows = slice(m * 128, (m + 1) * 128)
        kk = torch.cat([k[0, b * 128:(b + 1) * 128, hh] for b in blocks]).float().cpu().numpy()[None, None]
        vv = torch.cat([v[0, b * 128:(b + 1) * 128, hh] for b in blocks]).float().cpu().numpy()[None, None]
        qq = q[0, rows, hh].float().cpu().numpy()[None, None]
        mask = np.ones((1, 1, 1, n), bool)
        ref = oa.sparse_rows(qq, kk, vv, [n * 128], mask, 128 ** -0.5, "bfloat16", text_amp=0.2, text_block_start=n - tb)
        got = o[0, rows, hh].float().cpu().numpy()
        assert np.abs(got - ref[0, 0]).max() <= 2e-2, (hh, m, np.abs(got - ref[0, 0]).max())
    # (d) EVERY row of every head: the LP kernel (default launch order) against the round-1 kernel -- two independent
    #     kernels (different software pipelines, same lists): indexing at 900 blocks x 24 heads, both 64-key halves, the
    #     list-window reloads, the XCD remap and the count-sorted order.  Same arithmetic contract,
    #     different summation order of the running sums: a few bf16 ulps at |o| <= 1.
    o_r1 = _capi.bsattn_fwd(q, k, vt, seqlens, idx, cnt, nimg, 128 ** -0.5, 0.2, nimg,
                            flags=_capi.ATTN_XCD_REMAP | _capi.ATTN_LEGACY)
    d_all = (o.float() - o_r1.float()).abs()
    assert float(d_all.max()) <= 2e-2 and float(d_all.mean()) <= 5e-4, (float(d_all.max()), float(d_all.mean()))
    per_row = d_all.amax(dim=-1)                     # [1, S, H]: no query row (= no workgroup / wave) is off
    assert float((per_row > 8e-3).float().mean()) <= 1e-3
    del o_r1, d_all, per_row
    # text query rows: dense over everything (flash_attn semantics), one head
    ref_t = oa.text_rows(q[:, S_img:, 0:1].transpose(1, 2).float().cpu().numpy(), k[:, :, 0:1].transpose(1, 2).float().cpu().numpy(),
                         v[:, :, 0:1].transpose(1, 2).float().cpu().numpy(), 128 ** -0.5, "bfloat16")
    got_t = o[0, S_img:, 0].float().cpu().numpy()
    assert np.abs(got_t - ref_t[0, 0]).max() <= 2e-2


def test_full_size_gather_scatter_and_norm_rope_roundtrip(dev):
    """Config-2 sizes: scatter(gather(x)) == x on [1,115200,3072]; RoPE is a rotation: per-pair norms are preserved and
    applying the table built from (-angle) undoes it up to bf16 rounding."""
    from jenga_amd import _capi, gilbert as G
    from jenga_amd.modules.posemb_layers import get_nd_rotary_pos_embed
    t, h, w = 32, 45, 80
    l2h, h2l = G.gilbert_mapping(t, h, w, as_tensor=True)
    x = torch.randn(1, t * h * w, 3072, device=dev).to(torch.bfloat16)
    y = _capi.gather_rows(x, h2l)
    assert torch.equal(_capi.gather_rows(y, l2h), x) and not torch.equal(y, x)
    cos, sin = get_nd_rotary_pos_embed([16, 56, 56], [t, h, w], theta=256, use_real=True, theta_rescale_factor=1)
    cos, sin = cos.to(dev), sin.to(dev)
    qh = x.view(1, t * h * w, 24, 128)
    r = _capi.rmsnorm_rope(qh, None, cos, sin, eps=-1.0)
    back = _capi.rmsnorm_rope(r, None, cos, -sin, eps=-1.0)
    assert (back.float() - qh.float()).abs().max().item() <= 0.07          # two bf16 roundings at |x| <= ~5
    n0 = qh.float().view(-1, 64, 2).norm(dim=-1)
    n1 = r.float().view(-1, 64, 2).norm(dim=-1)
    assert (n0 - n1).abs().max().item() <= 0.05


# ----------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("valid_text,top_k", [(0, 3), (256, 0), (1, 1), (255, 11)])
def test_whole_op_edge_cases_vs_oracle(dev, valid_text, top_k):
    """No valid text token at all (every text key masked for image rows, text rows still dense), a fully valid text,
    top_k = 0 (the probability rule alone decides), top_k > number of image blocks (everything kept)."""
    from jenga_amd.modules.attention_block_sparse import block_sparse_attention
    from oracle import attention as oa
    from oracle import gilbert as og
    gen = torch.Generator().manual_seed(100 + valid_text + top_k)
    H, grid = 2, (2, 8, 32)
    S_img, S_txt = grid[0] * grid[1] * grid[2], 256
    S = S_img + S_txt
    q = (torch.randn(1, S, H, 128, generator=gen) * 1.3).to(torch.bfloat16)
    k = (torch.randn(1, S, H, 128, generator=gen) * 1.3).to(torch.bfloat16)
    v = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
    nbm = og.gilbert_block_neighbor_mapping(*grid, 128)
    cu = torch.tensor([0, S_img + valid_text, S], dtype=torch.int32)
    o = block_sparse_attention(q.to(dev), k.to(dev), v.to(dev), top_k=top_k, cu_seqlens_q=cu.to(dev),
                               cu_seqlens_kv=cu.to(dev), text_blocks=2, text_amp=0.25,
                               block_neighbor_list=torch.from_numpy(nbm), p_remain_rates=0.4)
    ref = oa.block_sparse_attention(to_np(q), to_np(k), to_np(v), top_k, "bfloat16", cu_seqlens_q=cu.numpy(),
                                    text_blocks=2, text_amp=0.25, block_neighbor_list=nbm, p_remain_rates=0.4)
    got = o.float().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 2e-2, np.abs(got - ref).max()


def test_c_abi_rejects_bad_arguments_on_device(dev):
    """The C entry points validate before launching: misaligned pointers / strides, bad dtype codes, missing lists."""
    from jenga_amd import _capi
    L = _capi.lib()
    st = _capi._stream(dev)
    q = torch.zeros(1, 256, 1, 128, device=dev, dtype=torch.bfloat16)
    vt = torch.zeros(1, 1, 4, 128, 64, device=dev, dtype=torch.bfloat16)
    o = torch.empty_like(q)
    sl = torch.tensor([256], dtype=torch.int32, device=dev)
    idx = torch.zeros(1, 1, 2, 2, dtype=torch.int32, device=dev)
    cnt = torch.ones(1, 1, 2, dtype=torch.int32, device=dev)
    p = _capi._p
    args = lambda qq=q, dtype=0, ss=128: (st, p(qq), p(q), p(vt), p(o), p(sl), p(idx), p(cnt), None, 1, 1, 2, 2, 256 * 128, ss,
                                          128, 256 * 128, 128, 128, 256 * 128, 128, 128, 0.088, 0.0, 2, dtype, 1)
    assert L.jenga_bsattn_fwd(*args()) == 0
    torch.cuda.synchronize()
    assert L.jenga_bsattn_fwd(*args(dtype=7)) != 0 and b"dtype" in L.jenga_last_error()
    assert L.jenga_bsattn_fwd(*args(ss=129)) != 0 and b"stride" in L.jenga_last_error()
    q_mis = torch.zeros(256 * 128 + 8, device=dev, dtype=torch.bfloat16)[4:]
    assert L.jenga_bsattn_fwd(*args(qq=q_mis)) != 0 and b"aligned" in L.jenga_last_error()
    bad = list(args())
    bad[6] = None
    assert L.jenga_bsattn_fwd(*bad) != 0 and b"idx" in L.jenga_last_error()

    # the other attention entries, same shapes (B = 1, H = 1, two blocks): one accepted call each, then the same kinds of bad
    # argument -- rejected under the entry's own name
    def rejected(fn, name, a):
        assert fn(*a) != 0, name
        assert L.jenga_last_error().startswith(name.encode()), (name, L.jenga_last_error())

    def without(a, i):
        a = list(a)
        a[i] = None
        return a

    pidx = torch.zeros(1, 1, 1, 2, dtype=torch.int32, device=dev)
    pcnt = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=dev).view(1, 1, 1, 4)    # one shared kv block
    pargs = lambda qq=q, dtype=0, ss=128: (st, p(qq), p(q), p(vt), p(o), p(sl), p(pidx), p(pcnt), None, 1, 1, 2, 2, 256 * 128,
                                           ss, 128, 256 * 128, 128, 128, 256 * 128, 128, 128, 0.088, 0.0, 2, dtype, 1)
    assert L.jenga_bsattn_pair_fwd(*pargs()) == 0, L.jenga_last_error()
    torch.cuda.synchronize()
    rejected(L.jenga_bsattn_pair_fwd, "jenga_bsattn_pair_fwd", pargs(dtype=7))
    rejected(L.jenga_bsattn_pair_fwd, "jenga_bsattn_pair_fwd", pargs(ss=129))
    rejected(L.jenga_bsattn_pair_fwd, "jenga_bsattn_pair_fwd", pargs(qq=q_mis))
    rejected(L.jenga_bsattn_pair_fwd, "jenga_bsattn_pair_fwd", without(pargs(), 6))

    xargs = lambda qq=q, dtype=0, ss=128: (st, p(qq), p(q), p(vt), p(o), 1, 1, 2, 2, 256, 256 * 128, ss, 128, 256 * 128, 128,
                                           128, 256 * 128, 128, 128, 0.088, dtype)
    assert L.jenga_cross_attn_fwd(*xargs()) == 0, L.jenga_last_error()
    torch.cuda.synchronize()
    rejected(L.jenga_cross_attn_fwd, "jenga_cross_attn_fwd", xargs(dtype=7))
    rejected(L.jenga_cross_attn_fwd, "jenga_cross_attn_fwd", xargs(ss=129))
    rejected(L.jenga_cross_attn_fwd, "jenga_cross_attn_fwd", xargs(qq=q_mis))     # (no lists in this entry)

    q8 = torch.zeros(1, 256, 1, 128, device=dev, dtype=torch.uint8)
    q8_mis = torch.zeros(256 * 128 + 16, device=dev, dtype=torch.uint8)[8:]
    sc8 = torch.ones(1, 1, 2, device=dev, dtype=torch.float32)
    fargs = lambda qq=q8, dtype=0, ss=128: (st, p(qq), p(sc8), p(q8), p(sc8), p(vt), p(o), p(sl), p(idx), p(cnt), 1, 1, 2, 2,
                                            256 * 128, ss, 128, 256 * 128, 128, 128, 256 * 128, 128, 128, 0.088, 0.0, 2, dtype, 1)
    assert L.jenga_bsattn_fp8_fwd(*fargs()) == 0, L.jenga_last_error()
    torch.cuda.synchronize()
    rejected(L.jenga_bsattn_fp8_fwd, "jenga_bsattn_fp8_fwd", fargs(dtype=7))
    rejected(L.jenga_bsattn_fp8_fwd, "jenga_bsattn_fp8_fwd", fargs(ss=136))      # q8 / k8 strides: multiples of 16
    rejected(L.jenga_bsattn_fp8_fwd, "jenga_bsattn_fp8_fwd", fargs(qq=q8_mis))
    rejected(L.jenga_bsattn_fp8_fwd, "jenga_bsattn_fp8_fwd", without(fargs(), 8))
    # host wrapper: one kv length per sample is required (the reference would read past cu_seqlens_q[1:2] for B = 2)
    q2 = torch.zeros(2, 256, 1, 128, device=dev, dtype=torch.bfloat16)
    vt2 = torch.zeros(2, 1, 4, 128, 64, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        _capi.bsattn_fwd(q2, q2, vt2, sl, idx.expand(2, -1, -1, -1).contiguous(), cnt.expand(2, -1, -1).contiguous(),
                         2, 0.088, 0.0, 2)


def test_two_streams_and_graph_capture(dev):
    """The library only enqueues work on the stream it is given: (a) two different problems on two streams at the same
    time give the results of running them one after the other; (b) the whole op (pool, select, pack_v, attention) can be
    captured into a HIP graph and replayed on new inputs."""
    from jenga_amd.modules.attention_block_sparse import block_sparse_attention
    from oracle import gilbert as og
    grid = (2, 8, 32)
    S = grid[0] * grid[1] * grid[2] + 256
    nbm = torch.from_numpy(og.gilbert_block_neighbor_mapping(*grid, 128)).to(dev)
    cu = torch.tensor([0, S - 100, S], dtype=torch.int32, device=dev)

    def make(seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return [torch.randn(1, S, 2, 128, generator=g, device=dev).to(torch.bfloat16) for _ in range(3)]

    run = lambda q, k, v: block_sparse_attention(q, k, v, top_k=2, cu_seqlens_q=cu, cu_seqlens_kv=cu, text_blocks=2,
                                                 text_amp=0.1, block_neighbor_list=nbm, p_remain_rates=0.3)
    a, b = make(1), make(2)
    ref_a, ref_b = run(*a), run(*b)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    outs = []
    for _ in range(3):
        with torch.cuda.stream(s1):
            oa = run(*a)
        with torch.cuda.stream(s2):
            ob = run(*b)
        outs.append((oa, ob))
    torch.cuda.synchronize()
    for oa, ob in outs:
        assert torch.equal(oa, ref_a) and torch.equal(ob, ref_b)
    # graph capture: static input buffers, replay after overwriting them
    sq, sk, sv = [t.clone() for t in a]
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        so = run(sq, sk, sv)
    for src, ref in ((b, ref_b), (a, ref_a)):
        sq.copy_(src[0]); sk.copy_(src[1]); sv.copy_(src[2])
        gph.replay()
        torch.cuda.synchronize()
        assert torch.equal(so, ref)


@pytest.mark.parametrize("seed", range(32))
def test_op_randomized_shapes_vs_oracle(dev, seed):
    """Differential test over random small configurations: heads, image / text block counts (text_blocks 0 included),
    valid length, top_k, probability threshold, text_amp, neighbours, dtype."""
    from jenga_amd.modules.attention_block_sparse import block_sparse_attention
    from oracle import attention as oa
    rng = np.random.RandomState(1000 + seed)
    H = int(rng.randint(1, 4))
    nimg = int(rng.randint(1, 11))
    tb = int(rng.choice([0, 1, 2, 4]))
    dt = "bfloat16" if seed % 3 else "float16"
    S_img, S_txt = nimg * 128, tb * 128
    S = S_img + S_txt
    valid = int(rng.randint(0, S_txt + 1)) if tb else 0
    top_k = int(rng.randint(0, nimg + 3))
    p = float(rng.choice([0.0, 0.2, 0.5, 0.9, 1.0]))
    amp = float(rng.choice([0.0, 0.25, 0.431]))
    gen = torch.Generator().manual_seed(seed)
    tdt = getattr(torch, dt)
    scale = float(rng.choice([0.5, 1.0, 1.6]))
    q = (torch.randn(1, S, H, 128, generator=gen) * scale).to(tdt)
    k = (torch.randn(1, S, H, 128, generator=gen) * scale).to(tdt)
    v = torch.randn(1, S, H, 128, generator=gen).to(tdt)
    nbm = (torch.rand(nimg, nimg, generator=gen) < 0.2) | torch.eye(nimg, dtype=torch.bool)
    cu = torch.tensor([0, S_img + valid, S], dtype=torch.int32)
    o = block_sparse_attention(q.to(dev), k.to(dev), v.to(dev), top_k=top_k, cu_seqlens_q=cu.to(dev),
                               cu_seqlens_kv=cu.to(dev), text_blocks=tb, text_amp=amp, block_neighbor_list=nbm,
                               p_remain_rates=p)
    ref = oa.block_sparse_attention(to_np(q), to_np(k), to_np(v), top_k, dt, cu_seqlens_q=cu.numpy(), text_blocks=tb,
                                    text_amp=amp, block_neighbor_list=nbm.numpy(), p_remain_rates=p,
                                    pooled=hip_pooled(q, k, tb, dev))
    got = o.float().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), (H, nimg, tb, valid, top_k, p, amp, dt)
    tol = 2.5e-2 if dt == "bfloat16" else 5e-3
    bad = np.abs(got - ref) > tol
    # the oracle selects from the HIP pooled means: every element must agree
    assert bad.sum() == 0, (H, nimg, tb, valid, top_k, p, amp, dt, np.abs(got - ref).max(), bad.mean())


@pytest.mark.parametrize("seed", range(16))
def test_padded_flavours_randomized_vs_oracle(dev, seed):
    """I2V (text_blocks = 4, ragged S padded to 128) and Wan (text_blocks = 0, first-frame blocks, bf16 forced, ragged S)
    flavours over random lengths / top_k / thresholds."""
    from jenga_amd.modules import attention_block_sparse as op
    from oracle import attention as oa
    rng = np.random.RandomState(500 + seed)
    wan = bool(seed % 2)
    H = int(rng.randint(1, 3))
    nimg = int(rng.randint(2, 9))
    gen = torch.Generator().manual_seed(50 + seed)
    top_k = int(rng.randint(1, nimg + 1))
    p = float(rng.choice([0.3, 0.5, 0.8, 0.9]))
    nbm = (torch.rand(nimg + 1, nimg + 1, generator=gen) < 0.25) | torch.eye(nimg + 1, dtype=torch.bool)
    if wan:
        S = nimg * 128 + int(rng.randint(1, 128))                     # ragged tail -> one more (padded) block
        ffb = int(rng.randint(0, 3))
        q = (torch.randn(1, S, H, 128, generator=gen) * 1.2).to(torch.bfloat16)
        k = (torch.randn(1, S, H, 128, generator=gen) * 1.2).to(torch.bfloat16)
        v = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
        o = op.block_sparse_attention_wan(q.to(dev), k.to(dev), v.to(dev), top_k, block_neighbor_list=nbm,
                                          p_remain_rates=p, first_frame_blocks=ffb)
        ref = oa.block_sparse_attention(to_np(q), to_np(k), to_np(v), top_k, "bfloat16", text_blocks=0,
                                        block_neighbor_list=nbm.numpy(), p_remain_rates=p, flavour="wan",
                                        first_frame_blocks=ffb, pooled=hip_pooled(q, k, 0, dev))
    else:
        S_img = nimg * 128
        S = S_img + 4 * 128 - int(rng.randint(1, 128))                 # ragged text tail, padded up to 4 text blocks
        valid = int(rng.randint(1, S - S_img))
        q = (torch.randn(1, S, H, 128, generator=gen) * 1.2).to(torch.bfloat16)
        k = (torch.randn(1, S, H, 128, generator=gen) * 1.2).to(torch.bfloat16)
        v = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
        cu = torch.tensor([0, S_img + valid, S], dtype=torch.int32)
        o = op.block_sparse_attention_i2v(q.to(dev), k.to(dev), v.to(dev), top_k, cu_seqlens_q=cu.to(dev),
                                          cu_seqlens_kv=cu.to(dev), text_amp=0.2, block_neighbor_list=nbm[:nimg, :nimg],
                                          p_remain_rates=p)
        ref = oa.block_sparse_attention(to_np(q), to_np(k), to_np(v), top_k, "bfloat16", cu_seqlens_q=cu.numpy(),
                                        text_blocks=4, text_amp=0.2, block_neighbor_list=nbm[:nimg, :nimg].numpy(),
                                        p_remain_rates=p, flavour="i2v", pooled=hip_pooled(q, k, 4, dev))
    got = o.float().cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got - ref)
    assert (err.max(axis=-1) > 3e-2).sum() == 0, (wan, H, nimg, S, top_k, p, err.max())


def test_wan_dense_branch_masks_keys_beyond_seq_lens(dev):
    """WanSelfAttention's dense branch (sa_drop_rate <= 0.25) is flash_attention(..., k_lens=seq_lens)
    (wan/modules/model_mul.py:153-159): when teacache_forward padded the tokens, keys at or beyond the real length must
    not be attended.  Valid rows must equal dense attention over the first seq_len keys only."""
    from jenga_amd.modules.attention_block_sparse import block_sparse_attention_wan
    from oracle import attention as oa
    gen = torch.Generator().manual_seed(3)
    S, L, H = 640, 601, 2                                   # 39 padding tokens at the tail
    q = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
    k = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
    v = torch.randn(1, S, H, 128, generator=gen).to(torch.bfloat16)
    k[:, L:] = k[:, :S - L] * 3.0                           # make the padding keys attractive: a missing mask shows
    out = block_sparse_attention_wan(q.to(dev), k.to(dev), v.to(dev), top_k=5, text_blocks=0, p_remain_rates=2.0,
                                     shape_xfuse=True, kv_lens=torch.tensor([L]))
    qn, kn, vn = (to_np(t.transpose(1, 2)) for t in (q, k, v))
    ref = oa.sparse_rows(qn, kn, vn, [L], np.ones((1, H, 5, 5), bool), 128 ** -0.5, "bfloat16", 0.0, 5)
    got = out.transpose(1, 2).float().cpu().numpy()
    assert np.abs(got[:, :, :L] - ref[:, :, :L]).max() <= 2e-2
    unmasked = block_sparse_attention_wan(q.to(dev), k.to(dev), v.to(dev), top_k=5, text_blocks=0, p_remain_rates=2.0,
                                          shape_xfuse=True).transpose(1, 2).float().cpu().numpy()
    assert np.abs(unmasked[:, :, :L] - ref[:, :, :L]).max() > 0.1      # the test input does discriminate
