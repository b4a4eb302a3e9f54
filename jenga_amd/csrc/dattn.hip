// Dense variable-length attention forward (jenga_dense_varlen_fwd): the counterpart of the reference's dense call,
// flash_attn_varlen_func over cu_seqlens (hyvideo/modules/attenion.py:108-121).  No kept-block lists, no packed-V
// workspace, nothing read back by the host.  DESIGN.md section "Dense varlen kernel" has the budget and the measurements.
//
// Decomposition.  One 8-wave workgroup owns a 256-row query tile of one (segment, head); wave w owns rows 32 w .. 32 w + 31
// and keeps their Q fragments (8 x uint4) and the O accumulators (4 x 16 fp32) in registers for the whole kv loop.  The kv
// sequence of the segment is walked in 64-key tiles.  Every K tile and every V tile is staged into LDS ONCE per workgroup
// (global_load_lds_dwordx4, each wave moves 8 of the 64 rows of either tile) and serves all 256 query rows: half the K/V
// bytes per FLOP of the 128-row LP kernel.  Rings: 3 K slots + 3 V slots of 16 KiB = 96 KiB, one workgroup per CU.
//
// Per tile and wave:  S^T = K . Q^T  (2 halves of 32 keys x 8 MFMA 32x32x16: A = K rows from LDS, B = Q registers), the
// scores of a query row end up in ONE lane column (16 keys per register set and half-wave) -> online softmax in fp32 in the
// exp2 domain without any transposition, P packed to 16 bit in exactly the k-order the next MFMA wants as its B operand,
// O^T += V^T . P^T (4 d-blocks x 4 MFMA).  V is staged in its natural [key][d] layout; the A operand of the P.V product needs
// 8 KEYS of one d per lane, which is what gfx950's transposing LDS read delivers: ds_read_b64_tr_b16 hands lane j of a 16-lane
// group element j of each of the four 16-element rows that the group's lanes 4e .. 4e+3 address (e = 0..3), so the four row
// addresses of a group are simply the four keys that the P fragment holds at that position.
//
// LDS layout (both rings): row = key, 256 bytes, the sixteen 16-byte chunks of a row XOR-swizzled -- K by (key & 15): the 16
// lanes of a ds_read_b128 phase read the same chunk of 16 consecutive keys; V by (key & 3) << 2: the 32 lanes of a transposing
// read cover 4 keys x 64 bytes.  The LDS-DMA writes 1 KiB per wave instruction linearly, so the swizzle is applied on the
// GLOBAL side (lane -> which chunk of which row it fetches).
//
// Pipeline: tile t+2 is issued behind the barrier that ends tile t-1's reads of the slot it overwrites; a wave's own pieces of
// tile t are awaited with a COUNTED s_waitcnt vmcnt(4) (the four DMA instructions of tile t+1 stay in flight), then the barrier
// publishes all eight waves' pieces.  One barrier per tile.
//
// Tile -> segment mapping.  The grid is (ceil(Tq / 256) + n_segments) x H, rounded up to 8.  Segment i (and, as segment n, the
// tail rows [cu_q[n], Tq) that have no keys) owns the tile ids [start_i, start_i + ceil(len_i / 256)) with
// start_i = floor(cu_q[i] / 256) + i: strictly increasing in i, never overlapping, never beyond the grid.  A workgroup
// binary-searches cu_seqlens_q for the last start_i <= its id; ids in the gaps exit.
// Launch order: a workgroup's XCD is blockIdx & 7; XCD x takes the x-th eighth of the (head-major) tile list, so the
// workgroups that are resident together on an XCD are consecutive query tiles of one head and share its K/V stream in that L2.
#include <math.h>

#include "common.h"

namespace jenga {
namespace {

constexpr int DV_THREADS = 512;
constexpr int DV_QTILE = 256;
constexpr int DV_TILE = 16384;             // 64 keys x 128 channels x 2 bytes
constexpr int DV_K_RING = 0;               // 3 slots: tile t in slot t % 3
constexpr int DV_V_RING = 3 * DV_TILE;     // 3 slots
constexpr int DV_LDS_BYTES = 6 * DV_TILE;  // 96 KiB of gfx950's 160: one workgroup per CU

struct DvParams {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    uint16_t* o;
    const int32_t* cu_q;
    const int32_t* cu_kv;
    long long q_ss, q_sh, k_ss, k_sh, v_ss, v_sh, o_ss, o_sh;
    int n_seg, Tq, Tk, H;
    int n_tiles;   // tile ids per head: ceil(Tq / 256) + n_seg
    int total;     // n_tiles * H
    int chunk;     // ceil(total / 8): one XCD's share
    float qk_scale;
};

// one 1-KiB piece: 64 lanes x 16 bytes from base + off[lane] to LDS [lds, lds + 1024)
__device__ __forceinline__ void dv_dma(const void* base, unsigned lds, unsigned off) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %1"
                 :
                 : "s"(lds), "s"(base), "v"(off)
                 : "memory", "m0");
}
#define DV_WAIT_ALL() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define DV_WAIT_KEEP4() asm volatile("s_waitcnt vmcnt(4)" ::: "memory")

typedef short dv_s4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) dv_s4 dv_lds_s4;
// 4 keys x 16 channels per 16-lane group, transposed: see the header
__device__ __forceinline__ uint2 dv_read_tr(const unsigned char* p) {
    const dv_s4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((dv_lds_s4*)p);
    return __builtin_bit_cast(uint2, r);
}

template <typename T>
__global__ void __launch_bounds__(DV_THREADS) dense_varlen_kernel(DvParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lq = lane & 31, hi = lane >> 5;

    // ---- which (head, segment, tile) ----
    const int bid = blockIdx.x;
    const int logical = (bid & 7) * P.chunk + (bid >> 3);
    if ((bid >> 3) >= P.chunk || logical >= P.total) return;
    const int h = logical / P.n_tiles;
    const int w = logical - h * P.n_tiles;
    int lo = 0, up = P.n_seg;
    while (lo < up) {   // the last segment whose first tile id is <= w
        const int mid = (lo + up + 1) >> 1;
        int c = P.cu_q[mid];
        c = c < 0 ? 0 : (c > P.Tq ? P.Tq : c);
        if ((c >> 8) + mid <= w) lo = mid;
        else up = mid - 1;
    }
    const int seg = __builtin_amdgcn_readfirstlane(lo);
    // segment bounds, clamped into the tensors whatever the device arrays hold
    int q0 = P.cu_q[seg], q1 = seg < P.n_seg ? P.cu_q[seg + 1] : P.Tq;
    int kv0 = 0, kv1 = 0;
    if (seg < P.n_seg) {
        kv0 = P.cu_kv[seg];
        kv1 = P.cu_kv[seg + 1];
    }
    q0 = q0 < 0 ? 0 : (q0 > P.Tq ? P.Tq : q0);
    q1 = q1 < q0 ? q0 : (q1 > P.Tq ? P.Tq : q1);
    kv0 = kv0 < 0 ? 0 : (kv0 > P.Tk ? P.Tk : kv0);
    kv1 = kv1 < kv0 ? kv0 : (kv1 > P.Tk ? P.Tk : kv1);
    q0 = __builtin_amdgcn_readfirstlane(q0);
    q1 = __builtin_amdgcn_readfirstlane(q1);
    kv0 = __builtin_amdgcn_readfirstlane(kv0);
    const int kvlen = __builtin_amdgcn_readfirstlane(kv1 - kv0);
    const int tq = w - ((q0 >> 8) + seg);
    if (tq < 0) return;
    const long long row0 = (long long)q0 + (long long)tq * DV_QTILE;
    if (row0 >= q1) return;

    const long long qrow = row0 + wave * 32 + lq;
    const bool row_ok = qrow < q1;
    const bool wave_on = row0 + wave * 32 < q1;   // a wave without rows still stages its share of K / V
    uint16_t* const op = P.o + qrow * P.o_ss + (long long)h * P.o_sh + 4 * hi;

    if (kvlen == 0) {   // no keys: zeros
        if (row_ok) {
#pragma unroll
            for (int i = 0; i < 16; ++i) *reinterpret_cast<uint2*>(op + (i >> 2) * 32 + (i & 3) * 8) = make_uint2(0u, 0u);
        }
        return;
    }

    // ---- Q fragments: lane (lq, hi) holds channels 16 ds + 8 hi .. + 7 of its row (rows past the segment: the last row) ----
    uint4 qf[8];
    {
        const long long qr = row_ok ? qrow : (long long)q1 - 1;
        const uint16_t* qp = P.q + qr * P.q_ss + (long long)h * P.q_sh + hi * 8;
#pragma unroll
        for (int ds = 0; ds < 8; ++ds) qf[ds] = *reinterpret_cast<const uint4*>(qp + ds * 16);
        // Q is awaited HERE, in front of the first LDS-DMA: left to the compiler, its vmcnt(0) for these loads lands in front of
        // the first MFMA inside the kv loop and drains the staging pipeline on every tile
#pragma unroll
        for (int ds = 0; ds < 8; ++ds)
            asm volatile("" : "+v"(qf[ds].x), "+v"(qf[ds].y), "+v"(qf[ds].z), "+v"(qf[ds].w));
    }

    // ---- staging: wave `wave`, piece p (0, 1) moves tile rows 32 p + 4 wave + (lane >> 4) ----
    const unsigned smem_base =
        __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem);
    const unsigned char* const kb =
        reinterpret_cast<const unsigned char*>(P.k + (long long)kv0 * P.k_ss + (long long)h * P.k_sh);
    const unsigned char* const vb =
        reinterpret_cast<const unsigned char*>(P.v + (long long)kv0 * P.v_ss + (long long)h * P.v_sh);
    const unsigned kss_b = (unsigned)P.k_ss * 2u, vss_b = (unsigned)P.v_ss * 2u;   // launcher: Tk * stride * 2 < 2^32
    const int st_row = 4 * wave + (lane >> 4);                                     // (+ 32 p) row inside the tile
    const unsigned k_chunk = (unsigned)(((lane & 15) ^ (st_row & 15)) << 4);
    const unsigned v_chunk = (unsigned)(((lane & 15) ^ ((st_row & 3) << 2)) << 4);
    auto issue = [&](int t, int slot) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int r = t * 64 + p * 32 + st_row;
            r = r < kvlen ? r : kvlen - 1;   // rows past the segment end: a valid row again, masked in the softmax
            const unsigned lds = smem_base + slot * DV_TILE + (p * 8 + wave) * 1024;
            dv_dma(kb, lds + DV_K_RING, (unsigned)r * kss_b + k_chunk);
            dv_dma(vb, lds + DV_V_RING, (unsigned)r * vss_b + v_chunk);
        }
    };

    // ---- LDS read addresses ----
    int k_addr[8];   // K fragment ds of key lq (+ 32 per half): chunk 2 ds + hi
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) k_addr[ds] = DV_K_RING + lq * 256 + (((ds * 2 + hi) ^ (lq & 15)) << 4);
    // V: 16-lane group g = lane >> 4 reads channels 32 db + 16 (g & 1) ..; lane i = 4 e + c of the group addresses
    // channels + 4 c .. 4 c + 3 of key 4 hi + e (+ 32 half + 16 s + 8 j for the j-th 64-bit half of the fragment)
    int v_addr[4];
    {
        const int e = (lane >> 2) & 3, c = lane & 3, g1 = (lane >> 4) & 1;
#pragma unroll
        for (int db = 0; db < 4; ++db)
            v_addr[db] = DV_V_RING + (4 * hi + e) * 256 + (((db ^ e) * 4 + g1 * 2 + (c >> 1)) << 4) + (c & 1) * 8;
    }

    f32x16 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
    float l = 0.f;          // this lane's share of the row sum (the other half-wave holds the other 32 keys of every tile)
    float m = -INFINITY;    // running maximum of the scaled scores (whole row: identical in both half-waves)
    const float sc = P.qk_scale;

    const int ntiles = (kvlen + 63) >> 6;
    issue(0, 0);
    if (ntiles > 1) issue(1, 1);
    int slot = 0;
    for (int t = 0; t < ntiles; ++t) {
        if (t + 1 < ntiles) DV_WAIT_KEEP4();
        else DV_WAIT_ALL();
        __syncthreads();   // tile t is complete; every wave is done with tile t - 1
        if (t + 2 < ntiles) issue(t + 2, slot == 0 ? 2 : slot - 1);
        if (wave_on) {
            const unsigned char* const ts = smem + slot * DV_TILE;
            f32x16 s[2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[half][r] = 0.f;
                uint4 kf[8];   // all eight fragments in flight before the first MFMA (left alone, hipcc reads one, waits, multiplies)
#pragma unroll
                for (int ds = 0; ds < 8; ++ds) kf[ds] = *reinterpret_cast<const uint4*>(ts + k_addr[ds] + half * 8192);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ds = 0; ds < 8; ++ds) s[half] = mfma32<T>(kf[ds], qf[ds], s[half]);
            }
            if (t * 64 + 64 > kvlen) {   // ragged last tile: keys past the segment end
#pragma unroll
                for (int half = 0; half < 2; ++half)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = t * 64 + half * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                        if (key >= kvlen) s[half][r] = -INFINITY;
                    }
            }
            float tmax = -INFINITY;
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[half][r]);
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float m_new = fmaxf(m, tmax * sc);   // finite: key 64 t is inside the segment
            if (__builtin_amdgcn_ballot_w64(m_new > m) != 0ull) {
                const float alpha = __builtin_amdgcn_exp2f(m - m_new);   // exactly 1 where the maximum stayed
                l *= alpha;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
                m = m_new;
            }
            uint4 pf[2][2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                float e[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    e[r] = __builtin_amdgcn_exp2f(fmaf(s[half][r], sc, -m));
                    l += e[r];   // the row sum takes the unrounded p
                }
                pf[half][0] = make_uint4(pack2<T>(e[0], e[1]), pack2<T>(e[2], e[3]), pack2<T>(e[4], e[5]), pack2<T>(e[6], e[7]));
                pf[half][1] = make_uint4(pack2<T>(e[8], e[9]), pack2<T>(e[10], e[11]), pack2<T>(e[12], e[13]),
                                         pack2<T>(e[14], e[15]));
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                uint4 vf[8];   // fragment i: d-block i & 3, 16-key step i >> 2; all in flight before the first MFMA
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned char* vp = ts + v_addr[i & 3] + (half * 32 + (i >> 2) * 16) * 256;
                    const uint2 a = dv_read_tr(vp), b = dv_read_tr(vp + 8 * 256);
                    vf[i] = make_uint4(a.x, a.y, b.x, b.y);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i & 3] = mfma32<T>(vf[i], pf[half][i >> 2], o[i & 3]);
            }
        }
        slot = slot == 2 ? 0 : slot + 1;
    }

    // ---- epilogue: o / l, one rounding; lane (lq, hi) holds channels 32 db + 8 j + 4 hi .. + 3 of its row ----
    if (row_ok) {
        const float inv = 1.0f / (l + __shfl_xor(l, 32));
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<uint2*>(op + db * 32 + j * 8) =
                    make_uint2(pack2<T>(o[db][4 * j] * inv, o[db][4 * j + 1] * inv),
                               pack2<T>(o[db][4 * j + 2] * inv, o[db][4 * j + 3] * inv));
    }
}

template <typename T>
hipError_t dv_launch(const DvParams& P, int grid, hipStream_t stream) {
    static bool attr_done[64] = {};
    lp_set_smem_once(reinterpret_cast<const void*>(&dense_varlen_kernel<T>), DV_LDS_BYTES, attr_done);
    hipLaunchKernelGGL(dense_varlen_kernel<T>, dim3(grid), dim3(DV_THREADS), DV_LDS_BYTES, stream, P);
    return hipGetLastError();
}

}  // namespace
}  // namespace jenga

using namespace jenga;

extern "C" int jenga_dense_varlen_fwd(void* stream, const void* q, const void* k, const void* v, void* o,
                                      const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_kv, int64_t n_segments,
                                      int64_t Tq, int64_t Tk, int64_t H, int64_t q_ss, int64_t q_sh, int64_t k_ss,
                                      int64_t k_sh, int64_t v_ss, int64_t v_sh, int64_t o_ss, int64_t o_sh, float sm_scale,
                                      int dtype) {
    auto bad8 = [](int64_t a, int64_t b) { return (a & 7) || (b & 7); };
    auto bad16 = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
    const int64_t lim = (1LL << 32) - 256;   // the staging offsets are 32-bit byte offsets from the segment's first key
    if (!q || !o || !cu_seqlens_q || !cu_seqlens_kv || (Tk > 0 && (!k || !v)) || n_segments <= 0 || Tq <= 0 || Tk < 0 ||
        H <= 0 || Tq >= (1LL << 31) || Tk >= (1LL << 31) || n_segments >= (1LL << 24) || bad8(q_ss, q_sh) ||
        bad8(k_ss, k_sh) || bad8(v_ss, v_sh) || bad8(o_ss, o_sh) || bad16(q) || bad16(k) || bad16(v) || bad16(o) ||
        ((uintptr_t)cu_seqlens_q & 3) || ((uintptr_t)cu_seqlens_kv & 3) || k_ss < 0 || v_ss < 0 ||
        k_ss >= (1LL << 31) || v_ss >= (1LL << 31) || Tk * k_ss * 2 > lim || Tk * v_ss * 2 > lim) {
        set_error("jenga_dense_varlen_fwd: bad arguments (non-null 16-B aligned q / k / v / o, device int32 cu_seqlens, "
                  "n_segments >= 1, Tq >= 1, Tk >= 0, strides multiples of 8 elements, Tk * row stride of k / v below 4 GiB)");
        return JENGA_EINVAL;
    }
    if (dtype != JENGA_BF16 && dtype != JENGA_FP16) {
        set_error("jenga_dense_varlen_fwd: dtype must be bf16 or fp16");
        return JENGA_EUNSUPPORTED;
    }
    if (!(sm_scale > 0.f) || !(sm_scale < INFINITY)) {
        set_error("jenga_dense_varlen_fwd: sm_scale must be positive and finite");
        return JENGA_EINVAL;
    }
    DvParams P;
    P.q = (const uint16_t*)q; P.k = (const uint16_t*)k; P.v = (const uint16_t*)v; P.o = (uint16_t*)o;
    P.cu_q = cu_seqlens_q; P.cu_kv = cu_seqlens_kv;
    P.q_ss = q_ss; P.q_sh = q_sh; P.k_ss = k_ss; P.k_sh = k_sh;
    P.v_ss = v_ss; P.v_sh = v_sh; P.o_ss = o_ss; P.o_sh = o_sh;
    P.n_seg = (int)n_segments; P.Tq = (int)Tq; P.Tk = (int)Tk; P.H = (int)H;
    const long long n_tiles = (Tq + DV_QTILE - 1) / DV_QTILE + n_segments;
    const long long total = n_tiles * H;
    if (total > 0x7ffffff0LL) {
        set_error("jenga_dense_varlen_fwd: grid size %lld out of range", total);
        return JENGA_EINVAL;
    }
    P.n_tiles = (int)n_tiles;
    P.total = (int)total;
    P.chunk = (int)((total + 7) / 8);
    P.qk_scale = (float)((double)sm_scale * 1.4426950408889634);
    const hipError_t e = dtype == JENGA_BF16 ? dv_launch<BF16>(P, P.chunk * 8, (hipStream_t)stream)
                                             : dv_launch<FP16>(P, P.chunk * 8, (hipStream_t)stream);
    if (e != hipSuccess) {
        set_error("jenga_dense_varlen_fwd: %s", hipGetErrorString(e));
        return JENGA_ELAUNCH;
    }
    return JENGA_OK;
}
