// FP8 Q.K block-sparse attention for gfx950: the block quantiser (jenga_quant_fp8_blocks) and the attention kernel that
// multiplies e4m3fn Q by e4m3fn K with v_mfma_f32_32x32x64_f8f6f4 (jenga_bsattn_fp8_fwd).  P.V stays 16-bit on the
// jenga_pack_v workspace.  DESIGN.md section "FP8 Q.K kernel" has the budget and the measurements.
//
// Quantiser.  One 256-thread workgroup per (b, h, 128-token block): the 32 KiB tile is read once into registers (thread t
// holds the 16-channel chunk t & 7 of rows (t >> 3) + 32 j, j = 0..3: eight 16-byte loads), |x - offset| is reduced in the
// wave by cross-lane moves and between the four waves through 16 bytes of LDS, every value is divided by the block scale
// (true fp32 division: the result is reproducible bit for bit in torch) and converted with v_cvt_pk_fp8_f32; a thread writes
// its 16 bytes per row with one 16-byte store.
//
// Attention.  Decomposition, C layout, lane-local softmax, P packing and the P.V product are those of csrc/bsattn.hip:
// workgroup = 4 waves = one 128-row query block of one (b, h); wave w owns rows 32 w .. 32 w + 31, lane (lq, hi) owns row lq.
//   S^T[key][q] = sum_d K8[key][d] Q8[q][d]: two 32x32x64 FP8 MFMAs per 32 keys (eight 32x32x16 in 16 bit).  MFMA j takes,
//   from lane (lq, hi), the 32 bytes "channels 64 j + 32 hi .. + 31" of key lq (A, two ds_read_b128 of one LDS row) and of
//   query row lq (B, 2 x 8 VGPRs loaded once).  A dot product does not care which k-slot a channel sits in as long as A and
//   B agree, and both operands map (lane >> 5, byte) to k the same way.
//   The fp32 scores are scaled by ONE wave-uniform scalar per kv block: q_scale[b,h,m] * k_scale[b,h,j] * sm_scale * log2 e.
// LDS: K8 ring of 3 slots x 8 KiB (64 keys x 128 B; tile t in slot t % 3, fetched two tiles ahead) + V^T ring of 2 slots x
// 16 KiB (fetched one tile ahead) = 56 KiB: two workgroups per CU.  A K8 row has eight 16-byte chunks, XOR-swizzled by
// (key >> 1) & 7: 16 consecutive keys reading one logical chunk touch 16 different 16-byte bank groups (even keys the low
// 128 bytes of the 256-byte bank line, odd keys the high ones).  Both tiles move by LDS-DMA (1 KiB per wave instruction:
// 4 V^T pieces + 2 K8 pieces per wave and tile), the swizzle is applied on the global side, the waits are counted
// (vmcnt(2) leaves the K8 pieces of tile t + 2 in flight), one barrier per tile.
#include <math.h>

#include "attn_launch.h"

namespace jenga {
namespace {

// ------------------------------------------------------------------------------------------------ quantiser
struct QuantParams {
    const uint16_t* x;
    unsigned char* x8;
    float* scale;
    const float* offset;
    long long x_sb, x_ss, x_sh;
    int H, nb;
};

// two floats -> two e4m3fn bytes in the low half of a dword (no word select: the high half is merged with a shift)
__device__ __forceinline__ uint32_t cvt2_fp8(float a, float b) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}

template <typename T>
__global__ void __launch_bounds__(256) quant_fp8_kernel(QuantParams P) {
    __shared__ float wmax[4];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x % P.nb;
    const int bh = blockIdx.x / P.nb;
    const int h = bh % P.H, b = bh / P.H;
    const int c16 = tid & 7, r0 = tid >> 3;

    float off[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) off[i] = 0.f;
    if (P.offset) {
        const float4* op = reinterpret_cast<const float4*>(P.offset + ((long long)b * P.H + h) * 128 + c16 * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 f = op[i];
            off[4 * i] = f.x; off[4 * i + 1] = f.y; off[4 * i + 2] = f.z; off[4 * i + 3] = f.w;
        }
    }

    float xf[4][16];
    float amax = 0.f;
    const uint16_t* xp = P.x + b * P.x_sb + ((long long)blk * 128 + r0) * P.x_ss + h * P.x_sh + c16 * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint4* p = reinterpret_cast<const uint4*>(xp + (long long)j * 32 * P.x_ss);
        const uint4 lo = p[0], hi = p[1];
        float f[8], g[8];
        unpack8<T>(lo, f);
        unpack8<T>(hi, g);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            xf[j][i] = P.offset ? f[i] - off[i] : f[i];
            xf[j][8 + i] = P.offset ? g[i] - off[8 + i] : g[i];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(xf[j][i]));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
    if ((tid & 63) == 0) wmax[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const float s = __fdiv_rn(fmaxf(amax, 1e-30f), 448.0f);
    if (tid == 0) P.scale[(long long)bh * P.nb + blk] = s;

    unsigned char* yp = P.x8 + ((((long long)b * P.nb + blk) * 128 + r0) * P.H + h) * 128 + c16 * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t lo = cvt2_fp8(__fdiv_rn(xf[j][4 * i], s), __fdiv_rn(xf[j][4 * i + 1], s));
            const uint32_t hi = cvt2_fp8(__fdiv_rn(xf[j][4 * i + 2], s), __fdiv_rn(xf[j][4 * i + 3], s));
            w[i] = lo | (hi << 16);
        }
        *reinterpret_cast<uint4*>(yp + (long long)j * 32 * P.H * 128) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ------------------------------------------------------------------------------------------------ attention
struct QaParams {
    const unsigned char* q8;
    const unsigned char* k8;
    const float* q_scale;
    const float* k_scale;
    const uint16_t* vt;
    uint16_t* o;
    const int32_t* seqlens;
    const int32_t* idx;
    const int32_t* cnt;
    AttnGeom g;   // strides of q8 / k8 in bytes
};

constexpr int QA_KT = 64;                        // keys per LDS tile
constexpr int QA_K_TILE = QA_KT * 128;           // 8 KiB of e4m3fn
constexpr int QA_V_TILE = 128 * QA_KT * 2;       // 16 KiB, the jenga_pack_v image
constexpr int QA_V_RING = 3 * QA_K_TILE;
constexpr int QA_LDS_BYTES = 3 * QA_K_TILE + 2 * QA_V_TILE;   // 56 KiB

typedef int qa_i8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma_fp8(const uint4& a0, const uint4& a1, const qa_i8& b, const f32x16& c) {
    const qa_i8 a = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
    // cbsz = blgp = 0: both operands e4m3; zero scale operands select the unscaled v_mfma_f32_32x32x64_f8f6f4
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
}

// One tile's staging of one wave: 4 V^T pieces, THEN 2 K8 pieces (loads retire in order: vmcnt(2) retires everything up to
// and including this call's V^T pieces and leaves its K8 pieces, needed one tile later, in flight).  M0 is saved and restored.
__device__ __forceinline__ void qa_stage(const void* kbase, const void* vbase, unsigned lds_k, unsigned lds_v, unsigned k0,
                                         unsigned k1, unsigned v0, unsigned v1, unsigned v2, unsigned v3) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %7, %4\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "global_load_lds_dwordx4 %8, %4\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "global_load_lds_dwordx4 %9, %4\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "global_load_lds_dwordx4 %10, %4\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %5, %3\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "global_load_lds_dwordx4 %6, %3\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(lds_k), "s"(lds_v), "s"(kbase), "s"(vbase), "v"(k0), "v"(k1), "v"(v0), "v"(v1), "v"(v2), "v"(v3)
        : "memory", "scc");
}
#define QA_WAIT_ALL() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define QA_WAIT_KEEP_K() asm volatile("s_waitcnt vmcnt(2)" ::: "memory")
// vmcnt(0) as a builtin right behind the (rare) reload of a list chunk: see LIST_LOAD_WAIT in bsattn.hip
#define QA_LIST_WAIT() __builtin_amdgcn_s_waitcnt(0x0F70)

template <typename T, bool TEXT>
__device__ __forceinline__ void qa_block(const QaParams& P, unsigned char* smem, int b, int h, int m) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 31, hi = lane >> 5;
    const int seqlen = P.seqlens ? P.seqlens[b] : P.g.n_blocks * 128;
    const long long bh = (long long)b * P.g.H + h;

    // ---- kept-block list ----
    const int32_t* list = nullptr;
    int nkept;
    if (TEXT) {
        nkept = P.g.n_blocks;
    } else {
        const long long row = bh * P.g.nq_img + m;
        list = P.idx + row * P.g.n_blocks;
        nkept = __builtin_amdgcn_readfirstlane(P.cnt[row]);
        nkept = nkept < 0 ? 0 : (nkept > P.g.n_blocks ? P.g.n_blocks : nkept);
    }
    const float* const ksc = P.k_scale + bh * P.g.n_blocks;
    const float sc_q = P.q_scale[bh * P.g.n_blocks + m] * P.g.qk_scale;

    // ---- Q8 fragments: lane (lq, hi) keeps channels 64 j + 32 hi .. + 31 of its row for MFMA j ----
    const long long qrow = (long long)m * 128 + wave_u * 32 + lq;
    qa_i8 qf[2];
    {
        const unsigned char* qp = P.q8 + b * P.g.q_sb + qrow * P.g.q_ss + h * P.g.q_sh + hi * 32;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint4 a = *reinterpret_cast<const uint4*>(qp + j * 64);
            const uint4 c = *reinterpret_cast<const uint4*>(qp + j * 64 + 16);
            qf[j] = qa_i8{(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)c.x, (int)c.y, (int)c.z, (int)c.w};
        }
    }
    uint16_t* const op = P.o + b * P.g.o_sb + qrow * P.g.o_ss + h * P.g.o_sh + hi * 4;

    f32x16 oacc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float l_i = 0.f;          // this lane's share of the row sum (the other half-wave holds the other keys of every tile)
    float m_i = -INFINITY;    // running maximum of the scaled scores (whole row: identical in both half-waves)
    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;

    const unsigned char* kbh = P.k8 + b * P.g.k_sb + h * P.g.k_sh;
    const uint16_t* vbh = P.vt + bh * (long long)P.g.n_blocks * 2 * (128 * QA_KT);

    // ---- loop-invariant LDS read addresses ----
    int k_addr[4], v_addr[4];   // K8: chunk c = 4 j + 2 hi + e of key lq, index 2 j + e
#pragma unroll
    for (int c = 0; c < 4; ++c)
        k_addr[c] = lq * 128 + ((((c >> 1) * 4 + hi * 2 + (c & 1)) ^ ((lq >> 1) & 7)) << 4);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        v_addr[ks] = lq * 128 + ((((ks >> 1) * 4 + hi * 2 + (ks & 1)) ^ ((lq >> 1) & 7)) << 4);
    // ---- per-lane source offsets (bytes) of the pieces this wave stages per tile ----
    // K8 piece 2 wave + p: tile rows 16 wave + 8 p + (lane >> 3), LDS chunk lane & 7 <- source chunk ^ ((row >> 1) & 7)
    // V^T piece 4 wave + i: rows 32 wave + 8 i + (lane >> 3), same rule (the layout of bsattn.hip)
    const unsigned smem_base =
        __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem);
    const int pr_ = lane >> 3, pc_ = lane & 7, psw_ = lane >> 4;
    const unsigned kss_b = (unsigned)P.g.k_ss;   // 64 rows x stride < 2^31, checked on the host
    const unsigned k_src0 = (unsigned)(16 * wave_u + pr_) * kss_b + ((pc_ ^ psw_) << 4);
    const unsigned k_src1 = (unsigned)(16 * wave_u + 8 + pr_) * kss_b + ((pc_ ^ (4 + psw_)) << 4);
    const int vr_ = 32 * wave_u + pr_;
    const unsigned v_src0 = (unsigned)(vr_ + 0) * 128 + ((pc_ ^ ((0 + psw_) & 7)) << 4);
    const unsigned v_src1 = (unsigned)(vr_ + 8) * 128 + ((pc_ ^ ((4 + psw_) & 7)) << 4);
    const unsigned v_src2 = (unsigned)(vr_ + 16) * 128 + ((pc_ ^ ((8 + psw_) & 7)) << 4);
    const unsigned v_src3 = (unsigned)(vr_ + 24) * 128 + ((pc_ ^ ((12 + psw_) & 7)) << 4);
    // Q8 is awaited HERE, in front of the first LDS-DMA: left to the compiler, its vmcnt(0) for these loads lands in front
    // of the first MFMA inside the kv loop and drains the staging pipeline
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(qf[j][i]));

    auto stage = [&](int kblk, int khalf, int vblk, int vhalf, int kslot, int vslot) {
        qa_stage(kbh + ((long long)kblk * 128 + khalf * QA_KT) * P.g.k_ss, vbh + ((long long)vblk * 2 + vhalf) * (128 * QA_KT),
                 smem_base + kslot * QA_K_TILE + wave_u * 2048, smem_base + QA_V_RING + vslot * QA_V_TILE + wave_u * 4096,
                 k_src0, k_src1, v_src0, v_src1, v_src2, v_src3);
    };

    // one 64-key tile of kv block `blk` (HALF = which half of it) with the block's score scale `sc`
    auto compute = [&](int kslot, int vslot, int blk, int half, float sc) {
        const int key0 = blk * 128 + half * QA_KT;
        if (!TEXT && key0 >= seqlen) return;   // wholly behind the valid length: contributes nothing (wave-uniform)
        const unsigned char* cur = smem + kslot * QA_K_TILE;
        const unsigned char* curv = smem + QA_V_RING + vslot * QA_V_TILE;
        f32x16 s0, s1;
        {
            uint4 ka[4], kb[4];
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                ka[c] = *reinterpret_cast<const uint4*>(cur + k_addr[c]);
                kb[c] = *reinterpret_cast<const uint4*>(cur + k_addr[c] + 4096);
            }
            s0 = mfma_fp8(ka[0], ka[1], qf[0], zero16);
            s1 = mfma_fp8(kb[0], kb[1], qf[0], zero16);
            s0 = mfma_fp8(ka[2], ka[3], qf[1], s0);
            s1 = mfma_fp8(kb[2], kb[3], qf[1], s1);
            __builtin_amdgcn_s_setprio(0);
        }
        const float amp = (!TEXT && blk >= P.g.text_block_start) ? P.g.text_amp : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s0[r] = fmaf(s0[r], sc, amp);
            s1[r] = fmaf(s1[r], sc, amp);
        }
        if (!TEXT && key0 + QA_KT > seqlen) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kk = key0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (kk >= seqlen) s0[r] = -INFINITY;
                if (kk + 32 >= seqlen) s1[r] = -INFINITY;
            }
        }
        float tmax = fmaxf(s0[0], s1[0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, fmaxf(s0[r], s1[r]));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float m_new = fmaxf(m_i, tmax);   // finite: key0 is a valid key of every row
        if (__builtin_amdgcn_ballot_w64(m_new > m_i) != 0ull) {
            const float alpha = __builtin_amdgcn_exp2f(m_i - m_new);   // exactly 1 where the maximum stayed
            l_i *= alpha;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
            m_i = m_new;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s0[r] = __builtin_amdgcn_exp2f(s0[r] - m_i);
            s1[r] = __builtin_amdgcn_exp2f(s1[r] - m_i);
            l_i += s0[r] + s1[r];   // the row sum takes the unrounded p
        }
        // P -> 16-bit B operands: k-step ks = 2 g + s uses C registers 8 s .. 8 s + 7 of 32-key group g
        uint4 pf[4];
        pf[0] = make_uint4(pack2<T>(s0[0], s0[1]), pack2<T>(s0[2], s0[3]), pack2<T>(s0[4], s0[5]), pack2<T>(s0[6], s0[7]));
        pf[1] = make_uint4(pack2<T>(s0[8], s0[9]), pack2<T>(s0[10], s0[11]), pack2<T>(s0[12], s0[13]),
                           pack2<T>(s0[14], s0[15]));
        pf[2] = make_uint4(pack2<T>(s1[0], s1[1]), pack2<T>(s1[2], s1[3]), pack2<T>(s1[4], s1[5]), pack2<T>(s1[6], s1[7]));
        pf[3] = make_uint4(pack2<T>(s1[8], s1[9]), pack2<T>(s1[10], s1[11]), pack2<T>(s1[12], s1[13]),
                           pack2<T>(s1[14], s1[15]));
        // O^T += V^T P^T: four independent accumulator chains per k-step, the reads of k-step ks + 1 in front of the MFMAs of ks
        {
            uint4 va[4][4];
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int db = 0; db < 4; ++db) va[ks][db] = *reinterpret_cast<const uint4*>(curv + v_addr[ks] + db * 4096);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int db = 0; db < 4; ++db) oacc[db] = mfma32<T>(va[ks][db], pf[ks], oacc[db]);
            __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
            for (int g_ = 0; g_ < 2; ++g_) {
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
            __builtin_amdgcn_s_setprio(0);
        }
    };

    // The list and the key scales of its blocks are read 64 entries at a time into two VGPRs (lane j holds entry base + j)
    // and pulled out with v_readlane: a per-iteration load would put a vmcnt(0) into every iteration and drain the DMA queue.
    int lchunk = 0;
    float schunk = 0.f;
    auto list_get = [&](int j, int& blk, float& sc) {
        if ((j & 63) == 0) {
            int e = j + lane;
            if (!TEXT) {
                e = e < nkept ? list[e] : 0;
                e = e < 0 ? 0 : (e >= P.g.n_blocks ? P.g.n_blocks - 1 : e);   // whatever the list holds: inside the tensors
            } else {
                e = e < nkept ? e : 0;
            }
            lchunk = e;
            schunk = ksc[e] * sc_q;
            QA_LIST_WAIT();
        }
        blk = __builtin_amdgcn_readlane(lchunk, j & 63);
        sc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, schunk), j & 63));
    };

    // Tile t (= 2 i + half of kept block i) reads K8 slot t % 3 and V^T slot t % 2.  At the start of tile t the DMA of
    // V(t+1) and K(t+2) goes out; at its end vmcnt(2) retires V(t+1) (and K(t+1), issued a tile earlier) and leaves K(t+2)
    // in flight across the barrier.
    int blk = 0, ks_cur = 0, ks_p2 = 2;
    float sc = 0.f;
    if (nkept > 0) {
        list_get(0, blk, sc);
        stage(blk, 0, blk, 0, 0, 0);   // K(0), V(0)
        stage(blk, 1, blk, 1, 1, 1);   // K(1) and V(1) early (V(1) goes out again with tile 0, into the same slot)
    }
    QA_WAIT_KEEP_K();
    __syncthreads();
    for (int i = 0; i < nkept; ++i) {
        int nblk = blk;
        float nsc = sc;
        if (i + 1 < nkept) list_get(i + 1, nblk, nsc);
        stage(nblk, 0, blk, 1, ks_p2, 1);
        compute(ks_cur, 0, blk, 0, sc);
        QA_WAIT_KEEP_K();
        __syncthreads();
        ks_cur = ks_cur == 2 ? 0 : ks_cur + 1;
        ks_p2 = ks_p2 == 2 ? 0 : ks_p2 + 1;
        stage(nblk, 1, nblk, 0, ks_p2, 0);
        compute(ks_cur, 1, blk, 1, sc);
        QA_WAIT_KEEP_K();
        __syncthreads();
        ks_cur = ks_cur == 2 ? 0 : ks_cur + 1;
        ks_p2 = ks_p2 == 2 ? 0 : ks_p2 + 1;
        blk = nblk;
        sc = nsc;
    }
    QA_WAIT_ALL();   // drain the last (unused) prefetch before the workgroup's LDS is released

    // ---- epilogue: o = acc / l, one rounding; image rows >= seqlen and rows without a valid key are zeros ----
    const float l_tot = l_i + __shfl_xor(l_i, 32);
    const bool row_ok = (TEXT || qrow < seqlen) && l_tot > 0.f;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            uint2 w = make_uint2(0u, 0u);
            if (row_ok) {
                w.x = pack2<T>(__fdiv_rn(oacc[db][rq * 4 + 0], l_tot), __fdiv_rn(oacc[db][rq * 4 + 1], l_tot));
                w.y = pack2<T>(__fdiv_rn(oacc[db][rq * 4 + 2], l_tot), __fdiv_rn(oacc[db][rq * 4 + 3], l_tot));
            }
            *reinterpret_cast<uint2*>(op + db * 32 + rq * 8) = w;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256, 2) bsattn_fp8_kernel(QaParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n_text = P.g.n_blocks - P.g.nq_img;
    const int id = blockIdx.x;
    if (id < P.g.n_text_wg_pad) {   // text query blocks first: the longest work items start earliest
        if (id >= P.g.B * P.g.H * n_text) return;
        const int m = P.g.nq_img + id % n_text;
        const int bh = id / n_text;
        qa_block<T, true>(P, smem, bh / P.g.H, bh % P.g.H, m);
        return;
    }
    const int li = id - P.g.n_text_wg_pad;
    const int bh = li / P.g.img_per_head;
    const int r = li % P.g.img_per_head;
    int m;
    if (P.g.xcd_chunk) {   // workgroup id -> XCD is id % 8: give each XCD a contiguous range of query blocks
        m = (r & 7) * P.g.xcd_chunk + (r >> 3);
        if ((r >> 3) >= P.g.xcd_chunk || m >= P.g.nq_img) return;
    } else {
        m = r;
    }
    qa_block<T, false>(P, smem, bh / P.g.H, bh % P.g.H, m);
}

bool bad16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace
}  // namespace jenga

using namespace jenga;

extern "C" int jenga_quant_fp8_blocks(void* stream, const void* x, void* x8, float* scale, const float* offset, int64_t B,
                                      int64_t H, int64_t n_blocks, int64_t x_sb, int64_t x_ss, int64_t x_sh, int dtype) {
    if (!x || !x8 || !scale || B <= 0 || H <= 0 || n_blocks <= 0 || bad16(x) || bad16(x8) || bad16(offset) ||
        ((uintptr_t)scale & 3) || (x_sb & 7) || (x_ss & 7) || (x_sh & 7) || B * H * n_blocks > 0x7fffffffLL ||
        n_blocks * 128 >= (1LL << 31)) {
        set_error("jenga_quant_fp8_blocks: bad arguments (non-null 16-B aligned x / x8, offset NULL or 16-B aligned, B, H, "
                  "n_blocks >= 1, strides of x multiples of 8 elements)");
        return JENGA_EINVAL;
    }
    if (dtype != JENGA_BF16 && dtype != JENGA_FP16) {
        set_error("jenga_quant_fp8_blocks: dtype must be bf16 or fp16");
        return JENGA_EUNSUPPORTED;
    }
    QuantParams P;
    P.x = (const uint16_t*)x; P.x8 = (unsigned char*)x8; P.scale = scale; P.offset = offset;
    P.x_sb = x_sb; P.x_ss = x_ss; P.x_sh = x_sh;
    P.H = (int)H; P.nb = (int)n_blocks;
    const dim3 grid((unsigned)(B * H * n_blocks));
    if (dtype == JENGA_BF16) hipLaunchKernelGGL(quant_fp8_kernel<BF16>, grid, dim3(256), 0, (hipStream_t)stream, P);
    else hipLaunchKernelGGL(quant_fp8_kernel<FP16>, grid, dim3(256), 0, (hipStream_t)stream, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("jenga_quant_fp8_blocks: %s", hipGetErrorString(e));
        return JENGA_ELAUNCH;
    }
    return JENGA_OK;
}

extern "C" int jenga_bsattn_fp8_fwd(void* stream, const void* q8, const float* q_scale, const void* k8, const float* k_scale,
                                    const void* vt, void* o, const int32_t* seqlens, const int32_t* idx, const int32_t* cnt,
                                    int64_t B, int64_t H, int64_t n_blocks, int64_t nq_img, int64_t q_sb, int64_t q_ss,
                                    int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh, int64_t o_sb, int64_t o_ss,
                                    int64_t o_sh, float sm_scale, float text_amp, int64_t text_block_start, int dtype,
                                    int flags) {
    if (!q8 || !k8 || !q_scale || !k_scale || !vt || !o || B <= 0 || H <= 0 || n_blocks <= 0 || nq_img < 0 ||
        nq_img > n_blocks || n_blocks * 128 >= (1LL << 31) || (nq_img > 0 && (!idx || !cnt)) || bad16(q8) || bad16(k8) ||
        bad16(vt) || bad16(o) || ((uintptr_t)q_scale & 3) || ((uintptr_t)k_scale & 3) || ((uintptr_t)seqlens & 3) ||
        ((uintptr_t)idx & 3) || ((uintptr_t)cnt & 3) || ((q_sb | q_ss | q_sh | k_sb | k_ss | k_sh) & 15) ||
        ((o_sb | o_ss | o_sh) & 7) || k_ss <= 0 || k_ss > (1 << 24)) {
        set_error("jenga_bsattn_fp8_fwd: bad arguments (non-null 16-B aligned q8 / k8 / vt / o, fp32 q_scale / k_scale, idx / "
                  "cnt when nq_img > 0, strides of q8 / k8 multiples of 16 elements and of o multiples of 8, 0 < k_ss <= 2^24)");
        return JENGA_EINVAL;
    }
    if (dtype != JENGA_BF16 && dtype != JENGA_FP16) {
        set_error("jenga_bsattn_fp8_fwd: dtype (of vt and o) must be bf16 or fp16");
        return JENGA_EUNSUPPORTED;
    }
    if (flags & ~JENGA_ATTN_XCD_REMAP) {
        set_error("jenga_bsattn_fp8_fwd: flags %d: only 0 and JENGA_ATTN_XCD_REMAP are supported", flags);
        return JENGA_EUNSUPPORTED;
    }
    if (!(sm_scale > 0.f) || !(sm_scale < INFINITY)) {
        set_error("jenga_bsattn_fp8_fwd: sm_scale must be positive and finite");
        return JENGA_EINVAL;
    }
    const AttnArgs a = {(hipStream_t)stream, q8, k8, vt, o, seqlens, idx, cnt, nullptr, B, H, n_blocks, nq_img, q_sb, q_ss, q_sh,
                        k_sb, k_ss, k_sh, o_sb, o_ss, o_sh, sm_scale, text_amp, text_block_start, dtype, flags};
    QaParams P;
    P.q8 = (const unsigned char*)q8; P.k8 = (const unsigned char*)k8; P.q_scale = q_scale; P.k_scale = k_scale;
    P.vt = (const uint16_t*)vt; P.o = (uint16_t*)o;
    P.seqlens = seqlens; P.idx = idx; P.cnt = cnt;
    attn_fill_geom(P.g, a);
    // this kernel's own: the list entries index the scale arrays, so text_block_start is clamped; log2(e) to full precision
    P.g.text_block_start = (int)(text_block_start < 0 ? 0 : (text_block_start > n_blocks ? n_blocks : text_block_start));
    P.g.qk_scale = (float)((double)sm_scale * 1.4426950408889634);
    const long long grid = attn_plan_grid("jenga_bsattn_fp8_fwd", P.g, B * H, n_blocks - nq_img, nq_img, flags);
    if (!grid) return JENGA_EINVAL;
    return attn_launch_result("jenga_bsattn_fp8_fwd",
                              ATTN_LAUNCH(dtype, bsattn_fp8_kernel, QA_LDS_BYTES, P, grid, a.stream));
}
