// Block-sparse attention forward for 64-channel heads (jenga_bsattn_d64_fwd) and the block pooling that feeds its selection
// (jenga_block_pool_d64).  Same semantics as jenga_bsattn_fwd (csrc/bsattn.hip), on [B, S, H, 64] rows as they lie in memory:
// no zero padding to 128 channels, no jenga_pack_v workspace, no output slice.  DESIGN.md section 3.10 has the budget.
//
// Work split.  One 4-wave workgroup per 128-row query block of one (b, h); wave w owns rows 32 w .. 32 w + 31, a lane owns ONE
// query row (lq = lane & 31), the two half-waves (hi = lane >> 5) split the channel / key index inside every MFMA.  The Q
// fragments (4 x uint4) and the O accumulators (2 x 16 fp32) stay in registers over the whole kept list.  Three workgroups fit a
// CU (3 x 48 KiB LDS, <= 168 VGPRs): a wave's softmax runs under the MFMAs of the two other waves of its SIMD.
//
// Per 64-key tile and wave (v_mfma_f32_32x32x16_{bf16,f16}; C layout col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 hi):
//   S^T = K . Q^T   2 halves of 32 keys x 4 MFMA; A = K rows (ds_read_b128), B = Q registers: the scores of a query row sit
//                   in one lane column, the softmax is lane-local and P is packed from the score registers in the k-order the
//                   next MFMA wants as its B operand;
//   O^T += V^T . P^T   2 d-blocks x 4 k-steps of 16 keys; A = 8 KEYS of one channel per lane, read from the natural-layout V
//                   tile with the transposing ds_read_b64_tr_b16: lane j of a 16-lane group gets element j of each of the four
//                   16-element rows that the group's lanes 4 e .. 4 e + 3 address, so the four rows of a group are the four
//                   keys 4 hi + e (+ 8 for the second read) that the P fragment holds at that position.
//
// LDS: rings of 3 K slots + 3 V slots of 64 keys x 128 B = 8 KiB each, 48 KiB.  A row is 128 B = eight 16-byte chunks, two
// rows span the 64 banks.  K: chunk c of key r lies at c ^ ((r >> 1) & 7) -- the 16 lanes of a ds_read_b128 phase read one
// chunk of 16 consecutive keys and land on 16 different 16-byte bank groups.  V: chunk c of key r lies at
// c ^ (((r >> 1) & 1) << 2) -- the 32 lanes of a transposing-read phase cover 4 keys x 64 bytes, keys 4 hi + {0, 1} and
// {2, 3} take opposite halves of the row pair.  The LDS-DMA (global_load_lds_dwordx4) writes 1 KiB = 8 rows per wave
// instruction linearly, so both swizzles are applied on the GLOBAL side (lane -> which chunk of which row it fetches).
//
// Pipeline: tile t + 2 is issued behind the barrier that ends tile t - 1's reads of the slot it overwrites; a wave's own four
// pieces (2 K + 2 V) of tile t are awaited with a counted s_waitcnt vmcnt(4), then the barrier publishes all waves' pieces.
// One barrier per tile.  The tile sequence is the kept list, two tiles per block, WITHOUT the tiles wholly behind seqlens[b].
#include <math.h>

#include "attn_launch.h"

namespace jenga {
namespace {

constexpr int D6_TILE = 8192;              // 64 keys x 64 channels x 2 bytes
constexpr int D6_K_RING = 0;               // 3 slots: tile t in slot t % 3
constexpr int D6_V_RING = 3 * D6_TILE;     // 3 slots
constexpr int D6_LDS_BYTES = 6 * D6_TILE;  // 48 KiB: three workgroups in the CU's 160 KiB

struct D6Params {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    uint16_t* o;
    const int32_t* seqlens;
    const int32_t* idx;
    const int32_t* cnt;
    long long v_sb, v_ss, v_sh;
    AttnGeom g;
};

// one 1-KiB piece: 64 lanes x 16 bytes from base + off[lane] to LDS [lds, lds + 1024)
__device__ __forceinline__ void d6_dma(const void* base, unsigned lds, unsigned off) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1"
                 :
                 : "s"(lds), "s"(base), "v"(off)
                 : "memory", "m0");
}
#define D6_WAIT_ALL() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define D6_WAIT_KEEP4() asm volatile("s_waitcnt vmcnt(4)" ::: "memory")
// vmcnt(0) as a builtin right behind the (rare) reload of the kept-list chunk, see bsattn.hip
#define D6_LIST_WAIT() __builtin_amdgcn_s_waitcnt(0x0F70)

typedef short d6_s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) d6_s4 d6_lds_s4;
__device__ __forceinline__ uint2 d6_read_tr(const unsigned char* p) {
    const d6_s4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((d6_lds_s4*)p);
    return __builtin_bit_cast(uint2, r);
}

template <typename T, bool TEXT>
__device__ __forceinline__ void d6_block(const D6Params& P, unsigned char* smem, int b, int h, int m) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 31, hi = lane >> 5;
    const int n_blocks = P.g.n_blocks;
    const int seqlen = __builtin_amdgcn_readfirstlane(P.seqlens ? P.seqlens[b] : n_blocks * 128);

    // ---- kept-block list (text rows: every block) ----
    const int32_t* list = nullptr;
    int nkept = n_blocks;
    if (!TEXT) {
        const long long row = ((long long)b * P.g.H + h) * P.g.nq_img + m;
        list = P.idx + row * n_blocks;
        const int c = P.cnt[row];
        nkept = __builtin_amdgcn_readfirstlane(c < 0 ? 0 : (c > n_blocks ? n_blocks : c));
    }

    // ---- Q fragments: lane (lq, hi) holds channels 16 ds + 8 hi .. + 7 of its row ----
    const long long qrow = (long long)m * 128 + wave * 32 + lq;
    uint4 qf[4];
    {
        const uint16_t* qp = P.q + b * P.g.q_sb + qrow * P.g.q_ss + h * P.g.q_sh + hi * 8;
#pragma unroll
        for (int ds = 0; ds < 4; ++ds) {
            uint4 raw = *reinterpret_cast<const uint4*>(qp + ds * 16);
            if (!TEXT) {   // q~ = dtype(float(q) * (sm_scale * log2 e))
                float f[8];
                unpack8<T>(raw, f);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = f[e] * P.g.qk_scale;
                raw = pack8<T>(f);
            }
            qf[ds] = raw;
        }
        // awaited HERE, in front of the first LDS-DMA: a compiler-placed vmcnt(0) inside the loop would drain the staging
#pragma unroll
        for (int ds = 0; ds < 4; ++ds)
            asm volatile("" : "+v"(qf[ds].x), "+v"(qf[ds].y), "+v"(qf[ds].z), "+v"(qf[ds].w));
    }
    uint16_t* const op = P.o + b * P.g.o_sb + qrow * P.g.o_ss + h * P.g.o_sh + 4 * hi;

    // ---- staging: wave `wave`, piece p (0, 1) moves tile rows 32 p + 8 wave + (lane >> 3), LDS chunk lane & 7 ----
    const unsigned smem_base =
        __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem);
    const unsigned char* const kbh = reinterpret_cast<const unsigned char*>(P.k + b * P.g.k_sb + h * P.g.k_sh);
    const unsigned char* const vbh = reinterpret_cast<const unsigned char*>(P.v + b * P.v_sb + h * P.v_sh);
    const unsigned kss_b = (unsigned)P.g.k_ss * 2u, vss_b = (unsigned)P.v_ss * 2u;   // host: 64 rows x stride x 2 < 2^31
    const int st_row = 8 * wave + (lane >> 3);
    const unsigned k_chunk = (unsigned)(((lane & 7) ^ ((st_row >> 1) & 7)) << 4);
    const unsigned v_chunk = (unsigned)(((lane & 7) ^ (((st_row >> 1) & 1) << 2)) << 4);
    const unsigned k_off0 = (unsigned)st_row * kss_b + k_chunk, k_off1 = (unsigned)(st_row + 32) * kss_b + k_chunk;
    const unsigned v_off0 = (unsigned)st_row * vss_b + v_chunk, v_off1 = (unsigned)(st_row + 32) * vss_b + v_chunk;
    auto issue = [&](int key0, int slot) {
        const unsigned char* const kt = kbh + (long long)key0 * (long long)kss_b;
        const unsigned char* const vt = vbh + (long long)key0 * (long long)vss_b;
        const unsigned lds = smem_base + slot * D6_TILE + wave * 1024;
        d6_dma(kt, lds + D6_K_RING, k_off0);
        d6_dma(kt, lds + D6_K_RING + 4096, k_off1);
        d6_dma(vt, lds + D6_V_RING, v_off0);
        d6_dma(vt, lds + D6_V_RING + 4096, v_off1);
    };

    // ---- LDS read addresses ----
    int k_addr[4];   // K fragment ds of key lq (+ 32 per half): chunk 2 ds + hi
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) k_addr[ds] = D6_K_RING + lq * 128 + (((ds * 2 + hi) ^ ((lq >> 1) & 7)) << 4);
    // V: 16-lane group g = lane >> 4 reads channels 32 db + 16 (g & 1) ..; lane 4 e + c of the group addresses channels
    // + 4 c .. 4 c + 3 of key 4 hi + e (+ 32 half + 16 s + 8 j for the j-th 64-bit half of the fragment)
    int v_addr[2];
    {
        const int e = (lane >> 2) & 3, c = lane & 3, g1 = (lane >> 4) & 1;
#pragma unroll
        for (int db = 0; db < 2; ++db)
            v_addr[db] = D6_V_RING + (4 * hi + e) * 128 + ((((db ^ (e >> 1)) * 4) + g1 * 2 + (c >> 1)) << 4) + (c & 1) * 8;
    }

    // ---- the tile sequence: entry tt >> 1 of the list, half tt & 1; -> first key of the next tile with a valid key, or -1.
    // The list is fetched 64 entries at a time into one VGPR and read with v_readlane (bsattn.hip: a per-entry load is a
    // vector load whose wait drains the LDS-DMA every tile); entries are clamped into [0, n_blocks)
    int tt = 0, lchunk = 0;
    auto next_tile = [&]() -> int {
        while (tt < 2 * nkept) {
            const int j = tt >> 1;
            int blk = j;
            if (!TEXT) {
                if ((tt & 127) == 0) {
                    lchunk = (j + lane < nkept) ? list[j + lane] : 0;
                    D6_LIST_WAIT();
                }
                blk = __builtin_amdgcn_readlane(lchunk, j & 63);
                blk = blk < 0 ? 0 : (blk >= n_blocks ? n_blocks - 1 : blk);
            }
            const int key0 = blk * 128 + (tt & 1) * 64;
            ++tt;
            if (TEXT || key0 < seqlen) return key0;
        }
        return -1;
    };

    f32x16 o[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float l = 0.f;          // this lane's share of the row sum (the other half-wave holds the other 32 keys of every tile)
    float mrow = -INFINITY; // running maximum of the base-2 logits (whole row: identical in both half-waves)
    const float sc = P.g.qk_scale;

    int k0a = next_tile();
    int k0b = k0a >= 0 ? next_tile() : -1;
    if (k0a >= 0) issue(k0a, 0);
    if (k0b >= 0) issue(k0b, 1);
    int slot = 0;
    while (k0a >= 0) {
        if (k0b >= 0) D6_WAIT_KEEP4();
        else D6_WAIT_ALL();
        __syncthreads();   // tile t is complete; every wave is done with tile t - 1
        const int k0c = k0b >= 0 ? next_tile() : -1;
        if (k0c >= 0) issue(k0c, slot == 0 ? 2 : slot - 1);

        const unsigned char* const ts = smem + slot * D6_TILE;
        f32x16 s[2];
        {
            uint4 kf[2][4];   // all eight fragments in flight before the first MFMA
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int ds = 0; ds < 4; ++ds)
                    kf[half][ds] = *reinterpret_cast<const uint4*>(ts + k_addr[ds] + half * 4096);
#pragma unroll
            for (int r = 0; r < 16; ++r) s[0][r] = s[1][r] = 0.f;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ds = 0; ds < 4; ++ds) {   // two independent accumulator chains
                s[0] = mfma32<T>(kf[0][ds], qf[ds], s[0]);
                s[1] = mfma32<T>(kf[1][ds], qf[ds], s[1]);
            }
        }
        float amp = 0.f;
        if (!TEXT) {
            if ((k0a >> 7) >= P.g.text_block_start) amp = P.g.text_amp;
            if (k0a + 64 > seqlen) {   // keys past the valid length
#pragma unroll
                for (int half = 0; half < 2; ++half)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = k0a + half * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        if (key >= seqlen) s[half][r] = -INFINITY;
                    }
            }
        }
        float tmax = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, fmaxf(s[0][r], s[1][r]));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        // finite: the tile's first key is valid.  Image rows: the logits are already in base 2 (q~), text rows: s * sc
        const float m_new = fmaxf(mrow, TEXT ? tmax * sc : tmax + amp);
        if (__builtin_amdgcn_ballot_w64(m_new > mrow) != 0ull) {
            const float alpha = __builtin_amdgcn_exp2f(mrow - m_new);   // exactly 1 where the maximum stayed
            l *= alpha;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
            mrow = m_new;
        }
        const float cadd = amp - mrow;
        uint4 pf[2][2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float e[16], ls = 0.f;   // (a sum per half: two dependent chains of 16 adds instead of one of 32)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                e[r] = __builtin_amdgcn_exp2f(TEXT ? fmaf(s[half][r], sc, cadd) : s[half][r] + cadd);
                ls += e[r];   // the row sum takes the unrounded p
            }
            l += ls;
            pf[half][0] = make_uint4(pack2<T>(e[0], e[1]), pack2<T>(e[2], e[3]), pack2<T>(e[4], e[5]), pack2<T>(e[6], e[7]));
            pf[half][1] = make_uint4(pack2<T>(e[8], e[9]), pack2<T>(e[10], e[11]), pack2<T>(e[12], e[13]),
                                     pack2<T>(e[14], e[15]));
        }
        {
            uint4 vf[4][2];   // k-step ks = 2 half + s, d-block db; all in flight before the first MFMA
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const unsigned char* vp = ts + v_addr[db] + ks * 16 * 128;
                    const uint2 a = d6_read_tr(vp), c = d6_read_tr(vp + 8 * 128);
                    vf[ks][db] = make_uint4(a.x, a.y, c.x, c.y);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int db = 0; db < 2; ++db) o[db] = mfma32<T>(vf[ks][db], pf[ks >> 1][ks & 1], o[db]);
        }
        k0a = k0b;
        k0b = k0c;
        slot = slot == 2 ? 0 : slot + 1;
    }

    // ---- epilogue: o = acc / l, one rounding; lane (lq, hi) holds channels 32 db + 8 j + 4 hi .. + 3 of its row.  Image rows
    // >= seqlen and rows without a single valid kept key are written as zeros ----
    const float l_tot = l + __shfl_xor(l, 32);
    const bool row_ok = (TEXT || qrow < seqlen) && l_tot > 0.f;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint2 w = make_uint2(0u, 0u);
            if (row_ok) {
                w.x = pack2<T>(__fdiv_rn(o[db][4 * j], l_tot), __fdiv_rn(o[db][4 * j + 1], l_tot));
                w.y = pack2<T>(__fdiv_rn(o[db][4 * j + 2], l_tot), __fdiv_rn(o[db][4 * j + 3], l_tot));
            }
            *reinterpret_cast<uint2*>(op + db * 32 + j * 8) = w;
        }
}

// the second argument is waves per SIMD: three 4-wave workgroups per CU
template <typename T>
__global__ void __launch_bounds__(256, 3) bsattn_d64_kernel(D6Params P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int n_text = P.g.n_blocks - P.g.nq_img;
    const int id = blockIdx.x;
    if (id < P.g.n_text_wg_pad) {  // text query blocks first: the longest work items start earliest
        if (id >= P.g.B * P.g.H * n_text) return;
        const int m = P.g.nq_img + id % n_text;
        const int bh = id / n_text;
        d6_block<T, true>(P, smem, bh / P.g.H, bh % P.g.H, m);
        return;
    }
    const int li = id - P.g.n_text_wg_pad;
    const int bh = li / P.g.img_per_head;
    const int r = li % P.g.img_per_head;
    int m;
    if (P.g.xcd_chunk) {  // workgroup id -> XCD is id % 8: give each XCD a contiguous range of query blocks
        m = (r & 7) * P.g.xcd_chunk + (r >> 3);
        if ((r >> 3) >= P.g.xcd_chunk || m >= P.g.nq_img) return;
    } else {
        m = r;
    }
    d6_block<T, false>(P, smem, bh / P.g.H, bh % P.g.H, m);
}

// ---- block pooling of 64-channel rows into the 128-channel pooled layout of jenga_block_select ----
// One 128-thread workgroup per (b, h, block): thread -> (token group tg = t / 8, slice = t % 8).  The summation order is
// block_pool_kernel's (rowops.hip): 8 tokens per thread in fp32, the 16 partial sums added in ascending order, s / 128, one
// rounding -- bit-identical to jenga_block_pool of the zero-padded rows; channels 64..127 are written as zeros.
template <typename T>
__global__ void __launch_bounds__(128) block_pool_d64_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ pooled,
                                                             long long B, long long H, long long nb, long long x_sb,
                                                             long long x_ss, long long x_sh) {
    __shared__ float red[16][65];
    const int sub = threadIdx.x & 7, tg = threadIdx.x >> 3;
    for (long long blk = blockIdx.x; blk < B * H * nb; blk += gridDim.x) {
        const long long j = blk % nb, h = (blk / nb) % H, b = blk / (nb * H);
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint16_t* base = x + b * x_sb + (j * 128) * x_ss + h * x_sh + sub * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float f[8];
            unpack8<T>(*reinterpret_cast<const uint4*>(base + (long long)(tg * 8 + i) * x_ss), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += f[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[tg][sub * 8 + e] = acc[e];
        __syncthreads();
        uint16_t out = 0;
        if (threadIdx.x < 64) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 16; ++g) s += red[g][threadIdx.x];
            out = from_f32<T>(s / 128.0f);
        }
        pooled[((b * H + h) * nb + j) * 128 + threadIdx.x] = out;
        __syncthreads();
    }
}

}  // namespace
}  // namespace jenga

using namespace jenga;

extern "C" int jenga_block_pool_d64(void* stream, const void* x, void* pooled, int64_t B, int64_t H, int64_t n_blocks,
                                    int64_t x_sb, int64_t x_ss, int64_t x_sh, int dtype) {
    if (!x || !pooled || B < 0 || H < 0 || n_blocks < 0 || ((x_sb | x_ss | x_sh) & 7) || ((uintptr_t)x & 15)) {
        set_error("jenga_block_pool_d64: bad arguments (non-null x / pooled, x 16-byte aligned, strides multiples of 8 elements)");
        return JENGA_EINVAL;
    }
    if (dtype != JENGA_BF16 && dtype != JENGA_FP16) {
        set_error("jenga_block_pool_d64: dtype must be bf16 or fp16");
        return JENGA_EUNSUPPORTED;
    }
    const long long n = (long long)B * H * n_blocks;
    if (n == 0) return JENGA_OK;
    const unsigned grid = (unsigned)(n > 65536 ? 65536 : n);
#define LAUNCH_BP64(T)                                                                                                 \
    hipLaunchKernelGGL(block_pool_d64_kernel<T>, dim3(grid), dim3(128), 0, (hipStream_t)stream, (const uint16_t*)x,   \
                       (uint16_t*)pooled, (long long)B, (long long)H, (long long)n_blocks, (long long)x_sb,           \
                       (long long)x_ss, (long long)x_sh)
    if (dtype == JENGA_BF16) LAUNCH_BP64(BF16); else LAUNCH_BP64(FP16);
#undef LAUNCH_BP64
    return attn_launch_result("jenga_block_pool_d64", hipGetLastError());
}

extern "C" int jenga_bsattn_d64_fwd(void* stream, const void* q, const void* k, const void* v, void* o,
                                    const int32_t* seqlens, const int32_t* idx, const int32_t* cnt, int64_t B, int64_t H,
                                    int64_t n_blocks, int64_t nq_img, int64_t q_sb, int64_t q_ss, int64_t q_sh, int64_t k_sb,
                                    int64_t k_ss, int64_t k_sh, int64_t v_sb, int64_t v_ss, int64_t v_sh, int64_t o_sb,
                                    int64_t o_ss, int64_t o_sh, float sm_scale, float text_amp, int64_t text_block_start,
                                    int dtype, int flags) {
    const char* const who = "jenga_bsattn_d64_fwd";
    const AttnArgs a = {(hipStream_t)stream, q, k, v, o, seqlens, idx, cnt, nullptr, B, H, n_blocks, nq_img, q_sb, q_ss, q_sh,
                        k_sb, k_ss, k_sh, o_sb, o_ss, o_sh, sm_scale, text_amp, text_block_start, dtype, flags};
    // k_ss, v_ss: per-lane 32-bit byte offsets inside a 64-row tile
    if (const int rc = attn_check_args(who, a, "idx/cnt", 1, 1 << 23, "key sequence")) return rc;
    if ((v_sb | v_ss | v_sh) & 7) {
        set_error("%s: strides must be multiples of 8 elements (16-byte rows)", who);
        return JENGA_EINVAL;
    }
    if (v_ss < 1 || v_ss > (1 << 23)) {
        set_error("%s: value sequence stride %lld out of range", who, (long long)v_ss);
        return JENGA_EINVAL;
    }
    if (n_blocks > (1 << 23)) {
        set_error("%s: n_blocks %lld out of range", who, (long long)n_blocks);
        return JENGA_EINVAL;
    }
    if (!(sm_scale > 0.f) || !(sm_scale < INFINITY)) {
        set_error("%s: sm_scale must be positive and finite", who);
        return JENGA_EINVAL;
    }
    if (flags & ~JENGA_ATTN_XCD_REMAP) {
        set_error("%s: flags must be 0 or JENGA_ATTN_XCD_REMAP (got %d)", who, flags);
        return JENGA_EUNSUPPORTED;
    }
    D6Params P;
    P.q = (const uint16_t*)q;
    P.k = (const uint16_t*)k;
    P.v = (const uint16_t*)v;
    P.o = (uint16_t*)o;
    P.seqlens = seqlens;
    P.idx = idx;
    P.cnt = cnt;
    P.v_sb = v_sb; P.v_ss = v_ss; P.v_sh = v_sh;
    attn_fill_geom(P.g, a);
    const long long grid = attn_plan_grid(who, P.g, B * H, n_blocks - nq_img, nq_img, flags);
    if (!grid) return JENGA_EINVAL;
    return attn_launch_result(who, ATTN_LAUNCH(dtype, bsattn_d64_kernel, D6_LDS_BYTES, P, grid, a.stream));
}
