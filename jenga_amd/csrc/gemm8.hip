// FP8 linear layers for gfx950: the per-row e4m3fn quantiser (jenga_quant_fp8_rows) and a hand-written FP8 GEMM with
// jenga_linear's epilogues (jenga_linear_fp8).  DESIGN.md section 3.11 has the design notes, the error and the timing record.
//
// Quantiser.  One 256-thread workgroup per row.  Thread t holds the 16-element chunks t, t + 256, t + 512, t + 768 of the row
// in registers (two 16-byte loads per chunk; rows up to 16384 elements), |x| is reduced in the wave by cross-lane moves and
// between the four waves through 16 bytes of LDS, every value is divided by the row scale (true fp32 division: the result is
// reproducible bit for bit in torch) and converted with v_cvt_pk_fp8_f32 (low-word form); a chunk leaves with one 16-byte
// store.  Longer rows take the two-pass form of the same kernel (the row is read a second time for the conversion).
//
// GEMM.  out[m, n] = act(gate[n] * (xs[m] * ws[n] * sum_k x8[m,k] w8[n,k]) + bias[n] + res[m, n]).
//   Workgroup = 8 waves on a 256 (tokens) x 256 (channels) output tile, one workgroup per CU; wave (wm, wn) owns tokens
//   [128 wm, +128) x channels [64 wn, +64): 2 x 4 fragments of 32 x 32, 128 fp32 accumulators per lane.
//   v_mfma_f32_32x32x64_f8f6f4 with A = W rows and B = X rows: D[n][m], so a lane holds, per register quad, 4 CONSECUTIVE
//   channels of ONE token -- the per-token scale is one value per lane and fragment, the store is 8 bytes (16 bit) or 16 bytes (fp32).
//   K step = 128 bytes = one LDS row = two MFMAs deep per fragment pair.  MFMA j takes, from lane (lr, hi), the 32 bytes
//   "k 64 j + 32 hi .. + 31" of row lr of both operands (two ds_read_b128 each): A and B map (lane >> 5, byte) to k alike, which
//   is all a dot product asks for.
//   LDS: 2 stages x (X tile 32 KiB + W tile 32 KiB) = 128 KiB.  A tile row has eight 16-byte chunks, XOR-swizzled by
//   (row >> 1) & 7: the 32 rows of a fragment read one logical chunk from 16 different 16-byte bank groups, even rows in the
//   low half of the 256-byte bank line and odd rows in the high one.  Tiles move by LDS-DMA (global_load_lds_dwordx4, 1 KiB =
//   8 rows per wave instruction, 4 X + 4 W pieces per wave and K step); the swizzle is applied on the DMA's SOURCE address.
//   Rows behind M / N are clamped to the last valid row on the source side (never read outside the operands), their results
//   are not stored.  The DMA of K step t + 2 goes out in the middle of step t and has a whole step to land; one barrier per K step; fragments are
//   double-buffered in registers (the reads of MFMA group j + 1 are issued in front of the MFMAs of group j, across the barrier).
//   Workgroup ids are remapped so that each XCD (id % 8) gets a contiguous range of tiles, ordered in groups of 4 token tiles
//   x all channel tiles: a W panel is shared by 4 consecutive workgroups of one L2, an X panel stays for a whole sweep over N.
#include <math.h>

#include <type_traits>

#include "common.h"

namespace jenga {
namespace {

// ------------------------------------------------------------------------------------------------ quantiser
struct RowQuantParams {
    const uint16_t* x;
    unsigned char* x8;
    float* scale;
    long long x_rs, x8_rs;
    int nchunks;   // K / 16
};

constexpr int RQ_CHUNKS = 4;   // 16-element chunks a thread keeps in registers

__device__ __forceinline__ uint32_t cvt2_fp8(float a, float b) {
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}

template <typename T>
__device__ __forceinline__ void rq_load(const uint16_t* p, float (&f)[16]) {
    const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
    float a[8], b[8];
    unpack8<T>(lo, a);
    unpack8<T>(hi, b);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f[i] = a[i];
        f[8 + i] = b[i];
    }
}

__device__ __forceinline__ void rq_store(unsigned char* p, const float (&f)[16], float s) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = cvt2_fp8(__fdiv_rn(f[4 * i], s), __fdiv_rn(f[4 * i + 1], s));
        const uint32_t hi = cvt2_fp8(__fdiv_rn(f[4 * i + 2], s), __fdiv_rn(f[4 * i + 3], s));
        w[i] = lo | (hi << 16);
    }
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}

// IN_REGS: the row fits RQ_CHUNKS chunks per thread and is read once; otherwise it is read twice
template <typename T, bool IN_REGS>
__global__ void __launch_bounds__(256) quant_fp8_rows_kernel(RowQuantParams P) {
    __shared__ float wmax[4];
    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const uint16_t* xp = P.x + row * P.x_rs;
    unsigned char* yp = P.x8 + row * P.x8_rs;

    float xf[RQ_CHUNKS][16];
    float amax = 0.f;
    if (IN_REGS) {
#pragma unroll
        for (int j = 0; j < RQ_CHUNKS; ++j) {
            const int c = tid + 256 * j;
            if (c < P.nchunks) {
                rq_load<T>(xp + c * 16, xf[j]);
#pragma unroll
                for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(xf[j][i]));
            }
        }
    } else {
        for (int c = tid; c < P.nchunks; c += 256) {
            rq_load<T>(xp + (long long)c * 16, xf[0]);
#pragma unroll
            for (int i = 0; i < 16; ++i) amax = fmaxf(amax, fabsf(xf[0][i]));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
    if ((tid & 63) == 0) wmax[tid >> 6] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const float s = __fdiv_rn(fmaxf(amax, 1e-30f), 448.0f);
    if (tid == 0) P.scale[row] = s;

    if (IN_REGS) {
#pragma unroll
        for (int j = 0; j < RQ_CHUNKS; ++j) {
            const int c = tid + 256 * j;
            if (c < P.nchunks) rq_store(yp + c * 16, xf[j], s);
        }
    } else {
        for (int c = tid; c < P.nchunks; c += 256) {
            rq_load<T>(xp + (long long)c * 16, xf[0]);
            rq_store(yp + (long long)c * 16, xf[0], s);
        }
    }
}

// ------------------------------------------------------------------------------------------------ GEMM
struct Gemm8Params {
    const unsigned char* x8;
    const unsigned char* w8;
    const float* xs;
    const float* ws;
    const void* bias;
    const void* res;
    const float* gate;
    void* out;
    long long M, N;
    long long x_rs, w_rs, res_rs, out_rs;   // x8 / w8 in bytes, res / out in elements
    int KT;                                 // K / 128
    int mt_n, nt_n;                         // tiles along M and N
    int act, bias32;
};

constexpr int G8_BM = 256, G8_BN = 256, G8_BK = 128, G8_THREADS = 512;
constexpr int G8_TILE = 256 * G8_BK;        // one operand tile: 32 KiB
constexpr int G8_STAGE = 2 * G8_TILE;       // X tile, then W tile
constexpr int G8_LDS_BYTES = 2 * G8_STAGE;  // 128 KiB

typedef int g8_i8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x16 g8_mfma(const g8_i8& a, const g8_i8& b, const f32x16& c) {
    // cbsz = blgp = 0: both operands e4m3; zero scale operands select the unscaled v_mfma_f32_32x32x64_f8f6f4
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
}

__device__ __forceinline__ g8_i8 g8_frag(const unsigned char* row, int c0, int c1) {
    const uint4 a = *reinterpret_cast<const uint4*>(row + c0);
    const uint4 b = *reinterpret_cast<const uint4*>(row + c1);
    return g8_i8{(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y, (int)b.z, (int)b.w};
}

__device__ __forceinline__ float g8_gelu_tanh(float v) {
    const float inner = 0.7978845608028654f * (v + 0.044715f * v * v * v);
    return 0.5f * v * (1.0f + tanhf(inner));
}

// One K step's staging of one wave: 4 X pieces, then 4 W pieces (1 KiB each, 8 KiB apart; the W tile lies 32 KiB behind the X
// tile).  Inline asm, so that the compiler puts no vmcnt(0) in front of the fragment reads of the OTHER stage: the waits are
// counted by hand in the main loop.  M0 is saved and restored.
__device__ __forceinline__ void g8_stage(const void* xbase, const void* wbase, unsigned lds, const unsigned (&xo)[4],
                                         const unsigned (&wo)[4]) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %4, %2\n\t"
        "s_add_u32 m0, m0, 0x2000\n\t"
        "global_load_lds_dwordx4 %5, %2\n\t"
        "s_add_u32 m0, m0, 0x2000\n\t"
        "global_load_lds_dwordx4 %6, %2\n\t"
        "s_add_u32 m0, m0, 0x2000\n\t"
        "global_load_lds_dwordx4 %7, %2\n\t"
        "s_add_u32 m0, m0, 0x2000\n\t"
        "global_load_lds_dwordx4 %8, %3\n\t"
        "s_add_u32 m0, m0, 0x2000\n\t"
        "global_load_lds_dwordx4 %9, %3\n\t"
        "s_add_u32 m0, m0, 0x2000\n\t"
        "global_load_lds_dwordx4 %10, %3\n\t"
        "s_add_u32 m0, m0, 0x2000\n\t"
        "global_load_lds_dwordx4 %11, %3\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(lds), "s"(xbase), "s"(wbase), "v"(xo[0]), "v"(xo[1]), "v"(xo[2]), "v"(xo[3]), "v"(wo[0]), "v"(wo[1]), "v"(wo[2]),
          "v"(wo[3])
        : "memory", "scc");
}
#define G8_WAIT_ALL() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#define G8_WAIT_KEEP_STAGE() asm volatile("s_waitcnt vmcnt(8)" ::: "memory")

template <typename T, bool OUT32>
__global__ void __launch_bounds__(G8_THREADS, 2) linear_fp8_kernel(Gemm8Params P) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    // XCD-aware remap (bijective for any grid size): the hardware deals workgroup ids round robin over 8 XCDs
    const int nwg = P.mt_n * P.nt_n;
    const int orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
    const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
    // tile order inside the range: groups of 4 token tiles, inside a group channel-tile major, token-tile minor
    const int per_group = 4 * P.nt_n, grp = wgid / per_group, in_g = wgid % per_group;
    const int g_m = (P.mt_n - grp * 4) < 4 ? (P.mt_n - grp * 4) : 4;
    const int mt = grp * 4 + in_g % g_m, nt = in_g / g_m;
    const long long m0 = (long long)mt * G8_BM, n0 = (long long)nt * G8_BN;
    const unsigned char* xg = P.x8 + m0 * P.x_rs;
    const unsigned char* wg = P.w8 + n0 * P.w_rs;

    // ---- per-lane source offsets of the 4 + 4 DMA pieces of this wave: piece p = 8 i + wave covers tile rows 8 p .. 8 p + 7,
    // lane -> row 8 p + (lane >> 3), LDS chunk lane & 7 <- source chunk (lane & 7) ^ ((row >> 1) & 7); rows clamped into the operand
    const int m_last = (int)((P.M - m0 < G8_BM ? P.M - m0 : G8_BM) - 1);
    const int n_last = (int)((P.N - n0 < G8_BN ? P.N - n0 : G8_BN) - 1);
    unsigned xoff[4], woff[4];   // < 256 * row stride <= 2^32 (row strides <= 2^24, checked on the host)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (8 * i + wave) * 8 + (lane >> 3);
        const unsigned c = (unsigned)(((lane & 7) ^ ((row >> 1) & 7)) << 4);
        xoff[i] = (unsigned)(row < m_last ? row : m_last) * (unsigned)P.x_rs + c;
        woff[i] = (unsigned)(row < n_last ? row : n_last) * (unsigned)P.w_rs + c;
    }
    const unsigned smem_base =
        __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem);
    auto stage = [&](int kt, int buf) {
        g8_stage(xg + (long long)kt * G8_BK, wg + (long long)kt * G8_BK, smem_base + buf * G8_STAGE + wave * 1024, xoff, woff);
    };

    // ---- fragment read addresses: row lr of a 32-row fragment, logical chunks 4 j + 2 hi and 4 j + 2 hi + 1 ----
    const int lr = lane & 31, hi = lane >> 5;
    const int sw = (lr >> 1) & 7;   // = (row >> 1) & 7: fragment bases are multiples of 32 rows
    int cb[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) cb[j][e] = ((4 * j + 2 * hi + e) ^ sw) << 4;
    const int xrow = (wm * 128 + lr) * G8_BK;
    const int wrow = G8_TILE + (wn * 64 + lr) * G8_BK;

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    g8_i8 wf[2][2], xf[2][4];
    auto load_frags = [&](const unsigned char* base, int j, int slot) {
#pragma unroll
        for (int i = 0; i < 2; ++i) wf[slot][i] = g8_frag(base + wrow + i * 32 * G8_BK, cb[j][0], cb[j][1]);
#pragma unroll
        for (int i = 0; i < 4; ++i) xf[slot][i] = g8_frag(base + xrow + i * 32 * G8_BK, cb[j][0], cb[j][1]);
    };
    auto mfmas = [&](int slot) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = g8_mfma(wf[slot][i], xf[slot][j], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
    };

    // Step t reads stage t % 2.  In the middle of step t (behind its barrier) the DMA of step t + 2 goes out into the stage that
    // step t has just finished reading; it has a whole step to land: the wait in front of the barrier of step t + 1 retires it.
    stage(0, 0);
    if (P.KT > 1) {
        stage(1, 1);
        G8_WAIT_KEEP_STAGE();   // loads retire in order: step 0's eight pieces have landed, step 1's stay in flight
    } else {
        G8_WAIT_ALL();
    }
    __syncthreads();
    load_frags(smem, 0, 0);
    for (int kt = 0; kt < P.KT; ++kt) {
        const int buf = kt & 1;
        load_frags(smem + buf * G8_STAGE, 1, 1);
        mfmas(0);
        G8_WAIT_ALL();     // this wave's pieces of step kt + 1 have landed, its reads of this stage have returned ...
        __syncthreads();   // ... and so have everybody's: the stage may be overwritten, the other one may be read
        if (kt + 2 < P.KT) stage(kt + 2, buf);
        if (kt + 1 < P.KT) load_frags(smem + (buf ^ 1) * G8_STAGE, 0, 0);
        mfmas(1);
    }

    // ---- epilogue.  D[n][m]: lane -> token lr of fragment j, register 4 rq + e -> channel 8 rq + 4 hi + e of fragment i ----
    float xsc[4];
    long long mrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mrow[j] = m0 + wm * 128 + j * 32 + lr;
        xsc[j] = mrow[j] < P.M ? P.xs[mrow[j]] : 0.f;
    }
    typedef typename std::conditional<OUT32, float, uint16_t>::type OutT;
    OutT* const outp = reinterpret_cast<OutT*>(P.out);
    const OutT* const resp = reinterpret_cast<const OutT*>(P.res);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            const long long n = n0 + wn * 64 + i * 32 + rq * 8 + 4 * hi;
            if (n >= P.N) continue;   // N is a multiple of 8: a quad is inside or outside as a whole
            const f32x4 wsc = *reinterpret_cast<const f32x4*>(P.ws + n);
            f32x4 gt = {1.f, 1.f, 1.f, 1.f}, bs = {0.f, 0.f, 0.f, 0.f};
            if (P.gate) gt = *reinterpret_cast<const f32x4*>(P.gate + n);
            if (P.bias) {
                if (P.bias32) {
                    bs = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(P.bias) + n);
                } else {
                    const uint2 b = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(P.bias) + n);
                    bs[0] = to_f32<T>((uint16_t)(b.x & 0xffffu));
                    bs[1] = to_f32<T>((uint16_t)(b.x >> 16));
                    bs[2] = to_f32<T>((uint16_t)(b.y & 0xffffu));
                    bs[3] = to_f32<T>((uint16_t)(b.y >> 16));
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (mrow[j] >= P.M) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = acc[i][j][rq * 4 + e] * (xsc[j] * wsc[e]);
                    if (P.gate) v[e] *= gt[e];
                    v[e] += bs[e];
                }
                if (P.res) {
                    const OutT* rp = resp + mrow[j] * P.res_rs + n;
                    if (OUT32) {
                        const f32x4 rv = *reinterpret_cast<const f32x4*>(rp);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += rv[e];
                    } else {
                        const uint2 rv = *reinterpret_cast<const uint2*>(rp);
                        v[0] += to_f32<T>((uint16_t)(rv.x & 0xffffu));
                        v[1] += to_f32<T>((uint16_t)(rv.x >> 16));
                        v[2] += to_f32<T>((uint16_t)(rv.y & 0xffffu));
                        v[3] += to_f32<T>((uint16_t)(rv.y >> 16));
                    }
                }
                if (P.act == JENGA_ACT_GELU_TANH) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = g8_gelu_tanh(v[e]);
                }
                OutT* op = outp + mrow[j] * P.out_rs + n;
                if (OUT32) {
                    const f32x4 o = {v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(op) = o;
                } else {
                    *reinterpret_cast<uint2*>(op) = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
                }
            }
        }
    }
}

template <typename T, bool OUT32>
hipError_t g8_launch(const Gemm8Params& P, unsigned grid, hipStream_t stream) {
    static bool done[64] = {};   // the per-kernel "dynamic LDS size set" flag, per device
    lp_set_smem_once((const void*)linear_fp8_kernel<T, OUT32>, G8_LDS_BYTES, done);
    hipLaunchKernelGGL((linear_fp8_kernel<T, OUT32>), dim3(grid), dim3(G8_THREADS), G8_LDS_BYTES, stream, P);
    return hipGetLastError();
}

bool bad16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace
}  // namespace jenga

using namespace jenga;

extern "C" int jenga_quant_fp8_rows(void* stream, const void* x, void* x8, float* scale, int64_t rows, int64_t K,
                                    int64_t x_row_stride, int64_t x8_row_stride, int dtype) {
    if (!x || !x8 || !scale || rows < 1 || K < 1 || (K & 15) || bad16(x) || bad16(x8) || ((uintptr_t)scale & 3) ||
        x_row_stride < K || (x_row_stride & 7) || x8_row_stride < K || (x8_row_stride & 15) || rows > 0x7fffffffLL ||
        K >= (1LL << 31)) {
        set_error("jenga_quant_fp8_rows: bad arguments (non-null 16-B aligned x / x8, rows >= 1, K a positive multiple of 16, "
                  "row stride of x a multiple of 8 and of x8 a multiple of 16, both >= K)");
        return JENGA_EINVAL;
    }
    if (dtype != JENGA_BF16 && dtype != JENGA_FP16) {
        set_error("jenga_quant_fp8_rows: dtype must be bf16 or fp16");
        return JENGA_EUNSUPPORTED;
    }
    RowQuantParams P;
    P.x = (const uint16_t*)x; P.x8 = (unsigned char*)x8; P.scale = scale;
    P.x_rs = x_row_stride; P.x8_rs = x8_row_stride; P.nchunks = (int)(K / 16);
    const dim3 grid((unsigned)rows);
    const bool in_regs = P.nchunks <= 256 * RQ_CHUNKS;
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == JENGA_BF16) {
        if (in_regs) hipLaunchKernelGGL((quant_fp8_rows_kernel<BF16, true>), grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL((quant_fp8_rows_kernel<BF16, false>), grid, dim3(256), 0, st, P);
    } else {
        if (in_regs) hipLaunchKernelGGL((quant_fp8_rows_kernel<FP16, true>), grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL((quant_fp8_rows_kernel<FP16, false>), grid, dim3(256), 0, st, P);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("jenga_quant_fp8_rows: %s", hipGetErrorString(e));
        return JENGA_ELAUNCH;
    }
    return JENGA_OK;
}

extern "C" int jenga_linear_fp8(void* stream, const void* x8, const float* x_scale, const void* w8, const float* w_scale,
                                const void* bias, const void* res, const float* gate, void* out, int64_t M, int64_t N,
                                int64_t K, int64_t x_row_stride, int64_t w_row_stride, int64_t res_row_stride,
                                int64_t out_row_stride, int act, int dtype) {
    const bool bias32 = (act & JENGA_BIAS_F32) != 0;
    const bool out32 = (act & JENGA_OUT_F32) != 0;
    const int flags = act & ~0xff;
    act &= 0xff;
    if (!x8 || !w8 || !x_scale || !w_scale || !out || M < 1 || N < 1 || K < 1 ||
        (act != JENGA_ACT_NONE && act != JENGA_ACT_GELU_TANH) || (flags & ~(JENGA_BIAS_F32 | JENGA_OUT_F32))) {
        set_error("jenga_linear_fp8: bad arguments (non-null x8 / x_scale / w8 / w_scale / out, M, N, K >= 1, act in {0, 1})");
        return JENGA_EINVAL;
    }
    if (K % 128 || N % 8) {
        set_error("jenga_linear_fp8: K must be a multiple of 128 and N a multiple of 8 (got K = %lld, N = %lld)", (long long)K,
                  (long long)N);
        return JENGA_EINVAL;
    }
    if (x_row_stride < K || w_row_stride < K || (x_row_stride & 15) || (w_row_stride & 15) || x_row_stride > (1 << 24) ||
        w_row_stride > (1 << 24) || out_row_stride < N || (out_row_stride & 7) ||
        (res && (res_row_stride < N || (res_row_stride & 7)))) {
        set_error("jenga_linear_fp8: row strides of x8 / w8 must be multiples of 16 bytes in [K, 2^24], those of res / out "
                  "multiples of 8 elements >= N");
        return JENGA_EINVAL;
    }
    if (bad16(x8) || bad16(w8) || bad16(out) || bad16(res) || bad16(bias) || bad16(gate) || bad16(w_scale) ||
        ((uintptr_t)x_scale & 3)) {
        set_error("jenga_linear_fp8: x8, w8, w_scale, bias, gate, res and out must be 16-byte aligned");
        return JENGA_EINVAL;
    }
    if (out32 && act != JENGA_ACT_NONE) {
        set_error("jenga_linear_fp8: JENGA_OUT_F32 is for the gate / residual form (no activation epilogue)");
        return JENGA_EUNSUPPORTED;
    }
    if (act != JENGA_ACT_NONE && (res || gate)) {
        set_error("jenga_linear_fp8: the activation epilogue cannot be combined with gate / residual");
        return JENGA_EUNSUPPORTED;
    }
    if (dtype != JENGA_BF16 && dtype != JENGA_FP16) {
        set_error("jenga_linear_fp8: dtype must be bf16 or fp16");
        return JENGA_EUNSUPPORTED;
    }
    const long long mt_n = (M + G8_BM - 1) / G8_BM, nt_n = (N + G8_BN - 1) / G8_BN;
    if (mt_n * nt_n > 0x7fffffffLL || K / G8_BK > 0x7fffffffLL) {
        set_error("jenga_linear_fp8: problem too large (%lld x %lld tiles)", mt_n, nt_n);
        return JENGA_EINVAL;
    }
    Gemm8Params P;
    P.x8 = (const unsigned char*)x8; P.w8 = (const unsigned char*)w8; P.xs = x_scale; P.ws = w_scale;
    P.bias = bias; P.res = res; P.gate = gate; P.out = out;
    P.M = M; P.N = N;
    P.x_rs = x_row_stride; P.w_rs = w_row_stride; P.res_rs = res_row_stride; P.out_rs = out_row_stride;
    P.KT = (int)(K / G8_BK); P.mt_n = (int)mt_n; P.nt_n = (int)nt_n;
    P.act = act; P.bias32 = bias32 ? 1 : 0;
    const unsigned grid = (unsigned)(mt_n * nt_n);
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (dtype == JENGA_BF16) e = out32 ? g8_launch<BF16, true>(P, grid, st) : g8_launch<BF16, false>(P, grid, st);
    else e = out32 ? g8_launch<FP16, true>(P, grid, st) : g8_launch<FP16, false>(P, grid, st);
    if (e != hipSuccess) {
        set_error("jenga_linear_fp8: %s", hipGetErrorString(e));
        return JENGA_ELAUNCH;
    }
    return JENGA_OK;
}
