// Host side of the block-sparse attention entries (jenga_bsattn_fwd, jenga_bsattn_pair_fwd, jenga_cross_attn_fwd,
// jenga_bsattn_fp8_fwd): the argument record, the checks the 16-bit entries share, the grid layout and the launch itself.
// What differs between the entries (the key-stride bound, the scale constant, fp8's alignment rules) stays with the entry.
#pragma once
#include "common.h"

namespace jenga {

// the arguments of jenga_bsattn_fwd / jenga_bsattn_pair_fwd, in the order of the C signature
struct AttnArgs {
    hipStream_t stream;
    const void *q, *k, *vt;
    void* o;
    const int32_t *seqlens, *idx, *cnt, *order;   // (pair entry: pidx, pcnt)
    int64_t B, H, n_blocks, nq_img;
    int64_t q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, o_sb, o_ss, o_sh;
    float sm_scale, text_amp;
    int64_t text_block_start;
    int dtype, flags;
};

// bsattn3.hip: the launcher behind jenga_bsattn_fwd(..., flags & JENGA_ATTN_LP); arguments already validated
int jenga_bsattn_lp_launch(const AttnArgs& a);

// the checks of the 16-bit list entries; `lists` names the two list arguments in the message, k_ss must lie in
// [kss_min, kss_max] (the bound is the kernel's: per-lane 32-bit byte offsets inside a 64-row K tile)
inline int attn_check_args(const char* who, const AttnArgs& a, const char* lists, int64_t kss_min, int64_t kss_max,
                           const char* kss_name) {
    if (!a.q || !a.k || !a.vt || !a.o || a.B <= 0 || a.H <= 0 || a.n_blocks <= 0 || a.nq_img < 0 ||
        a.nq_img > a.n_blocks) {
        set_error("%s: bad arguments", who);
        return JENGA_EINVAL;
    }
    if (a.nq_img > 0 && (!a.idx || !a.cnt)) {
        set_error("%s: %s are required when nq_img > 0", who, lists);
        return JENGA_EINVAL;
    }
    if ((a.q_sb | a.q_ss | a.q_sh | a.k_sb | a.k_ss | a.k_sh | a.o_sb | a.o_ss | a.o_sh) & 7) {
        set_error("%s: strides must be multiples of 8 elements (16-byte rows)", who);
        return JENGA_EINVAL;
    }
    if (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.vt | (uintptr_t)a.o) & 15) {
        set_error("%s: pointers must be 16-byte aligned", who);
        return JENGA_EINVAL;
    }
    if (a.dtype != JENGA_BF16 && a.dtype != JENGA_FP16) {
        set_error("%s: dtype must be bf16 or fp16", who);
        return JENGA_EUNSUPPORTED;
    }
    if (a.k_ss < kss_min || a.k_ss > kss_max) {
        set_error("%s: %s stride %lld out of range", who, kss_name, (long long)a.k_ss);
        return JENGA_EINVAL;
    }
    return JENGA_OK;
}

// strides, sizes and score constants of a launch into `g`: an AttnGeom, or the parameter struct of a kernel that keeps
// those fields flat (the LP and pair kernels); the grid layout comes from attn_plan_grid.  qk_scale is the 16-bit kernels'
// constant (the fp8 entry overwrites it with its own)
template <typename G>
void attn_fill_geom(G& g, const AttnArgs& a) {
    g.q_sb = a.q_sb; g.q_ss = a.q_ss; g.q_sh = a.q_sh;
    g.k_sb = a.k_sb; g.k_ss = a.k_ss; g.k_sh = a.k_sh;
    g.o_sb = a.o_sb; g.o_ss = a.o_ss; g.o_sh = a.o_sh;
    g.B = (int)a.B; g.H = (int)a.H; g.n_blocks = (int)a.n_blocks; g.nq_img = (int)a.nq_img;
    g.text_block_start = (int)a.text_block_start;
    g.qk_scale = (float)((double)a.sm_scale * 1.44269504);
    g.text_amp = a.text_amp;
    g.n_text_wg_pad = g.img_per_head = g.xcd_chunk = 0;
}

// Grid layout: the text items of all bh = B * H heads first (padded to a multiple of 8 workgroups), then img_per_head
// slots per head.  Items are query blocks, or pairs of them for the pair kernel.  With JENGA_ATTN_XCD_REMAP and at least
// 64 image items per head every XCD (workgroup id % 8) gets a contiguous range of xcd_chunk items.
// -> the grid size, or 0 after set_error (out of range)
template <typename G>
long long attn_plan_grid(const char* who, G& g, long long bh, long long n_text_items, long long n_img_items, int flags) {
    g.n_text_wg_pad = (int)((bh * n_text_items + 7) / 8 * 8);
    if ((flags & JENGA_ATTN_XCD_REMAP) && n_img_items >= 64) {
        g.xcd_chunk = (int)((n_img_items + 7) / 8);
        g.img_per_head = g.xcd_chunk * 8;
    } else {
        g.xcd_chunk = 0;
        g.img_per_head = (int)n_img_items;
    }
    const long long grid = (bh * n_text_items + 7) / 8 * 8 + bh * (long long)g.img_per_head;
    if (grid <= 0 || grid > 0x7fffffffLL) {
        set_error("%s: grid size %lld out of range", who, grid);
        return 0;
    }
    return grid;
}

// One launch of KERNEL (256 threads, LDS bytes of dynamic LDS).  hipFuncSetAttribute(MaxDynamicSharedMemorySize) runs
// once per kernel instantiation and device: `done` is a static of this function's instantiation, i.e. of the kernel
template <auto KERNEL, int LDS, typename P>
hipError_t attn_launch(const P& p, long long grid, hipStream_t stream) {
    static bool done[64] = {};
    lp_set_smem_once((const void*)KERNEL, LDS, done);
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)grid), dim3(256), LDS, stream, p);
    return hipGetLastError();
}
// the same for a kernel template whose first parameter is the storage type tag: ATTN_LAUNCH(dtype, kernel, LDS, P, grid,
// stream) or, with further template arguments, ATTN_LAUNCH_V(dtype, kernel, VARIANT, LDS, P, grid, stream)
#define ATTN_LAUNCH(DTYPE_, K_, LDS_, ...)                                                                             \
    ((DTYPE_) == JENGA_BF16 ? attn_launch<K_<BF16>, LDS_>(__VA_ARGS__) : attn_launch<K_<FP16>, LDS_>(__VA_ARGS__))
#define ATTN_LAUNCH_V(DTYPE_, K_, V_, LDS_, ...)                                                                       \
    ((DTYPE_) == JENGA_BF16 ? attn_launch<K_<BF16, V_>, LDS_>(__VA_ARGS__)                                             \
                            : attn_launch<K_<FP16, V_>, LDS_>(__VA_ARGS__))

// how an entry ends: the launch error (if any) under the entry's name
inline int attn_launch_result(const char* who, hipError_t e) {
    if (e == hipSuccess) return JENGA_OK;
    set_error("%s: %s", who, hipGetErrorString(e));
    return JENGA_ELAUNCH;
}

}  // namespace jenga
