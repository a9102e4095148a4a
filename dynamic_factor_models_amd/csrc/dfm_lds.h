// dfm_lds.h -- the LDS vocabulary of the hand-written kernels, written once: address-space aliases and the vector types behind
// them, the LDS-DMA statement, the counted waits and the LDS-only barrier.  Reached through dfm_device.h by every kernel file.
#pragma once
#include <hip/hip_runtime.h>

// cache-policy modifiers of the streaming LDS-DMA loads (development A/B: -DDFM_DMA_MOD='" nt"', '" sc1"', ...); default: none
#ifndef DFM_DMA_MOD
#define DFM_DMA_MOD ""
#endif
// the PANEL rows of collapse_wide2_kernel (development A/B: -DDFM_W2_PANEL_MOD='" nt"' puts a modifier on them alone -- the W / R
// tables of a replicate are re-read from L2 by every CU of its XCD and must stay cacheable)
#ifndef DFM_W2_PANEL_MOD
#define DFM_W2_PANEL_MOD DFM_DMA_MOD
#endif
// the PANEL rows of mstep_wide_kernel (development A/B: -DDFM_MW_PANEL_MOD='" nt"'); the factor rows are re-read by the 8 series
// blocks of a replicate
#ifndef DFM_MW_PANEL_MOD
#define DFM_MW_PANEL_MOD ""
#endif

namespace dfm {

typedef double v4d __attribute__((ext_vector_type(4)));   // also the accumulator of v_mfma_f64_16x16x4_f64
typedef double v2d __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

using lds_char_ptr = __attribute__((address_space(3))) char*;
using lds_double_ptr = __attribute__((address_space(3))) double*;
using lds_cvd_ptr = const volatile __attribute__((address_space(3))) double*;
using lds_cv2_ptr = const __attribute__((address_space(3))) v2d*;
using lds_cu4_ptr = const __attribute__((address_space(3))) v4u*;
using lds_cu2_ptr = const __attribute__((address_space(3))) v2u*;
using lds_cu1_ptr = const __attribute__((address_space(3))) unsigned*;

// One LDS-DMA: every active lane moves 16 B from its own global address to lds_dst + 16 * lane -- 1 KB back to back per wave,
// asynchronous, never passing through a VGPR, counted by vmcnt (hipcc does not count this load: the waits are the kernel's).
// M0 carries the wave-uniform LDS byte address; it is compiler-reserved, so it is saved and restored inside the statement, and
// the s_nop covers the hazard between the write of M0 and the load that reads it (cdna_hip_programming.md §5.7).
// MOD is the cache-policy suffix of the instruction: it has to be a string literal inside the asm text, hence a macro.
#define DFM_LDS_DMA16(MOD, gsrc, lds_dst)                 \
    do {                                                  \
        unsigned keep_m0_;                                \
        asm volatile(                                     \
            "s_mov_b32 %0, m0\n\t"                        \
            "s_mov_b32 m0, %2\n\t"                        \
            "s_nop 0\n\t"                                 \
            "global_load_lds_dwordx4 %1, off" MOD "\n\t"  \
            "s_mov_b32 m0, %0"                            \
            : "=&s"(keep_m0_)                             \
            : "v"(gsrc), "s"(lds_dst)                     \
            : "memory");                                  \
    } while (0)

__device__ __forceinline__ void dma16(const void* gsrc, unsigned lds_dst) { DFM_LDS_DMA16("", gsrc, lds_dst); }
__device__ __forceinline__ void dma16_nt(const void* gsrc, unsigned lds_dst) { DFM_LDS_DMA16(" nt", gsrc, lds_dst); }
__device__ __forceinline__ void dma16_mod(const void* gsrc, unsigned lds_dst) { DFM_LDS_DMA16(DFM_DMA_MOD, gsrc, lds_dst); }
__device__ __forceinline__ void dma16_w2_panel(const void* gsrc, unsigned lds_dst) { DFM_LDS_DMA16(DFM_W2_PANEL_MOD, gsrc, lds_dst); }
__device__ __forceinline__ void dma16_mw_panel(const void* gsrc, unsigned lds_dst) { DFM_LDS_DMA16(DFM_MW_PANEL_MOD, gsrc, lds_dst); }
// nt: the non-temporal hint on the panel stream.  The panel is read ONCE per pass; with the hint its lines do not displace the
// rest of the pass's working set from the 256-MB Infinity Cache -- the outputs (P_smooth, f_smooth: 180 MB per 1024 replicates),
// which the next pass or the M-step behind this one overwrites or reads again, and the covariance tables.  Measured in one
// process (profiles/r04/ab_dma_nt_*.txt): +12 % at B = 512, +13..15 % at 1024, +8 % at 1536, +6 % at 2048, +1 % at 4096, -2 % at
// 8192 (nothing of a 6.6-GB batch stays on chip, and the hint costs the L2 its write-combining of neighbouring rows): the
// launcher sets it for batches whose panels are <= 2 GiB.
__device__ __forceinline__ void dma16_stream(const void* gsrc, unsigned lds_dst, bool nt) {
    if (nt) dma16_nt(gsrc, lds_dst);                           // (wave-uniform)
    else dma16_mod(gsrc, lds_dst);
}
// The base-plus-offset form: lane l copies 16 bytes from gbase + voff to LDS byte lds_dst + 16 l.  gbase, lds_dst wave-uniform.
__device__ __forceinline__ void dma16_base(const void* gbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(gbase), "s"(lds_dst) : "memory");
}
// ... lanes 0 .. 15 only (a 256-byte row): exec is masked inside the statement
__device__ __forceinline__ void dma16_base_row16(const void* gbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    unsigned long long ex;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b64 %1, exec\n\ts_mov_b32 m0, %4\n\ts_mov_b64 exec, 0xffff\n\tglobal_load_lds_dwordx4 %2, %3\n\t"
                 "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep), "=&s"(ex) : "v"(voff), "s"(gbase), "s"(lds_dst) : "memory");
}

// One ring BLOCK of LDS-DMAs in one statement: 4 rows x NDR pieces of 1 KB.  Row k comes from the wave-uniform pointer rk and
// lands at lds_dst + k * slot_stride; piece p of a row is the instruction's immediate offset 1024 p, which the hardware adds to
// the global AND to the LDS address.  Lane l moves the 16 bytes at voff (= 16 l) of its piece.  M0 is saved and restored ONCE and
// walks the slots by addition; exec changes ONCE, for the last piece of every row, which only the lanes of last_mask move (a row
// need not fill its last KB).  Two pieces: up the rows with the full-width piece, back down with the last one.  One piece: up
// the rows under the mask.  The s_nop behind each write of M0 covers the hazard between that write and the load that reads M0
// (cdna_hip_programming.md §5.7); behind the first write the save of exec stands in that place.  vmcnt counts exactly 4 NDR
// loads per statement; their order inside the block is free, the kernels' counted waits are block-granular.
// PRECONDITION: all 64 lanes active on entry (a wave-uniform call site).  The full-width pieces go out under the exec they find
// and the last pieces under last_mask itself, not under its intersection with the caller's exec.
#define DFM_GLDS_(MOD, R, P) "global_load_lds_dwordx4 %2, " R " offset:" P MOD "\n\t"
#define DFM_M0_UP_ "s_add_u32 m0, m0, %8\n\ts_nop 0\n\t"
#define DFM_M0_DOWN_ "s_sub_u32 m0, m0, %8\n\ts_nop 0\n\t"
#define DFM_BLOCK_ROWS1_(MOD)                                                                                               \
    "s_mov_b64 exec, %9\n\t"                                                                                                \
    DFM_GLDS_(MOD, "%3", "0") DFM_M0_UP_ DFM_GLDS_(MOD, "%4", "0") DFM_M0_UP_ DFM_GLDS_(MOD, "%5", "0") DFM_M0_UP_          \
    DFM_GLDS_(MOD, "%6", "0")
#define DFM_BLOCK_ROWS2_(MOD)                                                                                               \
    DFM_GLDS_(MOD, "%3", "0") DFM_M0_UP_ DFM_GLDS_(MOD, "%4", "0") DFM_M0_UP_ DFM_GLDS_(MOD, "%5", "0") DFM_M0_UP_          \
    DFM_GLDS_(MOD, "%6", "0")                                                                                               \
    "s_mov_b64 exec, %9\n\t"                                                                                                \
    DFM_GLDS_(MOD, "%6", "1024") DFM_M0_DOWN_ DFM_GLDS_(MOD, "%5", "1024") DFM_M0_DOWN_ DFM_GLDS_(MOD, "%4", "1024")        \
    DFM_M0_DOWN_ DFM_GLDS_(MOD, "%3", "1024")
#define DFM_LDS_DMA_BLOCK(ROWS, voff, r0, r1, r2, r3, lds_dst, slot_stride, last_mask)                                      \
    do {                                                                                                                    \
        unsigned keep_m0_;                                                                                                  \
        unsigned long long keep_ex_;                                                                                        \
        asm volatile(                                                                                                       \
            "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %7\n\ts_mov_b64 %1, exec\n\t"                                                \
            ROWS                                                                                                            \
            "s_mov_b64 exec, %1\n\ts_mov_b32 m0, %0"                                                                        \
            : "=&s"(keep_m0_), "=&s"(keep_ex_)                                                                              \
            : "v"(voff), "s"(r0), "s"(r1), "s"(r2), "s"(r3), "s"(lds_dst), "s"(slot_stride), "s"(last_mask)                 \
            : "memory", "scc");                                                                                             \
    } while (0)
#define DFM_LDS_DMA_BLOCK_NDR(MOD, ...)                                                       \
    do {                                                                                      \
        if constexpr (NDR == 1) DFM_LDS_DMA_BLOCK(DFM_BLOCK_ROWS1_(MOD), __VA_ARGS__);        \
        else DFM_LDS_DMA_BLOCK(DFM_BLOCK_ROWS2_(MOD), __VA_ARGS__);                           \
    } while (0)
// nt: the panel stream's non-temporal hint (dma16_stream above), chosen once per block
template <int NDR>
__device__ __forceinline__ void dma16_block_stream(unsigned voff, const void* r0, const void* r1, const void* r2, const void* r3,
                                                   unsigned lds_dst, unsigned slot_stride, unsigned long long last_mask, bool nt) {
    static_assert(NDR == 1 || NDR == 2, "rows of at most 2 KB (the MFMA collapse: N <= 256); a longer row needs its own ROWS text");
    if (nt) DFM_LDS_DMA_BLOCK_NDR(" nt", voff, r0, r1, r2, r3, lds_dst, slot_stride, last_mask);      // (wave-uniform)
    else DFM_LDS_DMA_BLOCK_NDR(DFM_DMA_MOD, voff, r0, r1, r2, r3, lds_dst, slot_stride, last_mask);
}
// the lanes that move 16 bytes of the last piece of a row of row_bytes (a multiple of 16)
__device__ __forceinline__ unsigned long long dma16_last_mask(unsigned row_bytes) {
    const unsigned nl = ((row_bytes + 1023u) % 1024u + 1u) / 16u;    // 1 .. 64 lanes
    return nl >= 64u ? ~0ull : (1ull << nl) - 1ull;
}

// at most K vector-memory operations of this wave (LDS-DMAs among them) still in flight; K = 0: all have landed
template <int K>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(K) : "memory");
}
// the wave's LDS operations are complete.  A wave's own LDS writes are visible to its later reads anyway (one in-order queue):
// between them this is only the fence that keeps the compiler from moving them.
__device__ __forceinline__ void wait_lgkmcnt0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// Workgroup barrier for data that travels through LDS only.  __syncthreads() also drains vmcnt: it would wait for every
// outstanding global access of the wave -- prefetched operands, table stores, the asynchronous staging.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// one ds_read_b64 (never merged into ds_read2_b64, never moved relative to other volatile accesses) of LDS byte address a
__device__ __forceinline__ double lds_read64(unsigned a) { return *(lds_cvd_ptr)(size_t)a; }

}  // namespace dfm
