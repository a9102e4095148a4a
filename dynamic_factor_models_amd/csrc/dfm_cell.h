// dfm_cell.h -- the text the post-estimation cell kernels share (forecast.hip, filter.hip, filter_ar.hip, structural.hip, proxy.hip,
// simsmooth.hip, news.hip).  A cell kernel writes a [rows][N] panel from per-series loadings held in registers and per-row vectors staged in LDS
// (DESIGN.md section 10).  No kernels here: the chunk decode, the row staging, the lane map, the loadings holder with its dot
// product, the packed quadratic form, the 16-byte-or-scalar cell I/O and the twin launchers, each written once.  The first part is
// plain C++ behind DFM_CELL_FN, so that tests/host/cell_host.cpp compiles the holder and the quadratic form for the CPU.
#pragma once
#include <math.h>

#include "dfm_cellgeom.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DFM_CELL_FN __device__ __forceinline__
#else
#define DFM_CELL_FN inline
#endif

namespace dfm {

// ---- chunk decode -------------------------------------------------------------------------------------------------------------
// Series block s, chunk c of the rows [t0, t1) of `outer` (a replicate, a pass replicate, a slab).
struct CellChunk {
    int s, c;
    size_t outer;
    int t0, t1;
};

// The kernels on a 3-D grid pass their block indices.
DFM_CELL_FN CellChunk cell_chunk(const CellGeom& geo, int s, int c, size_t outer, int rows) {
    const int t0 = c * geo.RC;
    return CellChunk{s, c, outer, t0, t0 + geo.RC < rows ? t0 + geo.RC : rows};
}

// 1-D grids: blk = (outer nchunk + c) nsblk + s.
DFM_CELL_FN CellChunk cell_chunk(const CellGeom& geo, unsigned blk, int rows) {
    const int s = (int)(blk % (unsigned)geo.nsblk);
    blk /= (unsigned)geo.nsblk;
    return cell_chunk(geo, s, (int)(blk % (unsigned)geo.nchunk), (size_t)(blk / (unsigned)geo.nchunk), rows);
}

// ---- lane map -----------------------------------------------------------------------------------------------------------------
// Lane tid of series block s: row group g, first series i0 of its SP, and n of them inside the panel (0: the lane idles -- it
// returns, or stays for the barriers).  The SP kernels run SP = 2 for even N only (n = SP on a live lane); the pair kernels
// always give a lane a column pair, and the last pair of an odd N has n = 1.
struct CellLane {
    int g, i0, n;
    bool live;
};

template <int SP>
DFM_CELL_FN CellLane cell_lane(const CellGeom& geo, int tid, int s, int N) {
    const int j = tid % geo.NPB, g = tid / geo.NPB, i0 = (s * geo.NPB + j) * SP;
    const bool live = g < geo.G && i0 < N;
    return CellLane{g, i0, live ? (i0 + SP <= N ? SP : N - i0) : 0, live};
}

// ---- loadings -----------------------------------------------------------------------------------------------------------------
// The loadings of SP adjacent series in RB registers each.  RB = r known at compile time: every m < r below folds away.
template <int SP, int RB>
struct CellLam {
    double l[SP][RB];

    // Series i0 .. i0 + SP - 1 of replicate b: zero beyond r, all zero for the series q >= present; times scale[series] when given.
    DFM_CELL_FN void load(const double* Lam, size_t b, int N, int i0, int r, int present = SP, const double* scale = nullptr) {
#pragma unroll
        for (int q = 0; q < SP; ++q) {
            const size_t bi = b * N + i0 + q;
            const bool have = q < present;
            const double sc = (scale && have) ? scale[bi] : 1.0;
#pragma unroll
            for (int m = 0; m < RB; ++m) l[q][m] = (have && m < r) ? sc * Lam[bi * r + m] : 0.0;
        }
    }

    // lam_q' row: one fma chain over m = 0 .. r - 1.
    DFM_CELL_FN double dot(int q, const double* row, int r) const {
        double v = 0.0;
#pragma unroll
        for (int m = 0; m < RB; ++m)
            if (m < r) v = fma(l[q][m], row[m], v);
        return v;
    }

    // v[q] = lam_q' row for every q at once: one read of row[m] and one m < r test serve all SP chains (the pair kernels, whose r
    // is a run-time value inside the bucket: a dot per series would test and read twice).
    DFM_CELL_FN void dots(const double* row, int r, double (&v)[SP]) const {
#pragma unroll
        for (int q = 0; q < SP; ++q) v[q] = 0.0;
#pragma unroll
        for (int m = 0; m < RB; ++m)
            if (m < r) {
                const double x = row[m];
#pragma unroll
                for (int q = 0; q < SP; ++q) v[q] = fma(l[q][m], x, v[q]);
            }
    }
};

// qf += lam' P lam for a symmetric r x r P packed row-wise lower, P[j (j + 1) / 2 + k] = P_jk (k <= j): the terms
// lam_j (P_jj lam_j + 2 u_j), u_j = sum_{k<j} P_jk lam_k, join qf in the order of j.  lam: double[RB], zero beyond r.  The diagonal
// product is kept out of contraction: it is rounded on its own and 2 u_j joins it in one fma, which is how this expression has
// always been compiled -- left to the compiler, a rewrite of the surrounding text fused P_jj lam_j instead and moved xvar / vstd by
// a bit.  A statement macro (no semicolon after it) and not a function: as a function the exact-R instances of
// forecast_fill_kernel lose a wave per SIMD to another order of the LDS reads; in place it compiles as before.
#define DFM_CELL_QUAD(qf, lam, P, RB, r)                                                                  \
    _Pragma("unroll") for (int j_ = 0; j_ < (RB); ++j_)                                                   \
        if (j_ < (r)) {                                                                                   \
            double u_ = 0.0;                                                                              \
            _Pragma("unroll") for (int k_ = 0; k_ < j_; ++k_) u_ += (P)[j_ * (j_ + 1) / 2 + k_] * (lam)[k_]; \
            double d_;                                                                                    \
            {                                                                                             \
                _Pragma("clang fp contract(off)")                                                         \
                d_ = (P)[j_ * (j_ + 1) / 2 + j_] * (lam)[j_];                                             \
            }                                                                                             \
            (qf) += (lam)[j_] * (d_ + 2.0 * u_);                                                          \
        }

#if defined(__HIPCC__)
// ---- row staging --------------------------------------------------------------------------------------------------------------
// The workgroup copies n doubles into LDS; the caller's barrier publishes them.
__device__ __forceinline__ void cell_stage(double* dst, const double* src, int n) {
    for (int e = threadIdx.x; e < n; e += blockDim.x) dst[e] = src[e];
}
// The first w doubles of each of nrows source rows `stride` apart, packed.
__device__ __forceinline__ void cell_stage(double* dst, const double* src, int nrows, int w, int stride) {
    for (int e = threadIdx.x; e < nrows * w; e += blockDim.x) dst[e] = src[(size_t)(e / w) * stride + e % w];
}

// ---- cell I/O -----------------------------------------------------------------------------------------------------------------
// The cells of a lane's SP series in one row: one 16-byte access for SP = 2 (the launcher has checked N's parity and the pointer).
template <int SP>
__device__ __forceinline__ void cell_ld(const double* p, double (&x)[SP]) {
    if constexpr (SP == 2) {
        const double2 v = *reinterpret_cast<const double2*>(p);
        x[0] = v.x; x[1] = v.y;
    } else {
        x[0] = p[0];
    }
}
template <int SP>
__device__ __forceinline__ void cell_st(double* p, const double (&x)[SP]) {
    if constexpr (SP == 2) *reinterpret_cast<double2*>(p) = double2{x[0], x[1]};
    else p[0] = x[0];
}

// The pair kernels: VEC as above; otherwise two scalar accesses, the second only where the pair has its second column (x[1] is
// left as it is where not).
template <bool VEC>
__device__ __forceinline__ void cell_ld_pair(const double* p, bool two, double (&x)[2]) {
    if constexpr (VEC) {
        cell_ld<2>(p, x);
    } else {
        x[0] = p[0];
        if (two) x[1] = p[1];
    }
}
template <bool VEC>
__device__ __forceinline__ void cell_st_pair(double* p, bool two, const double (&x)[2]) {
    if constexpr (VEC) {
        cell_st<2>(p, x);
    } else {
        p[0] = x[0];
        if (two) p[1] = x[1];
    }
}
// The pair of a row that may lie behind the chunk (NaN then): issued one row ahead, in flight while the current row is computed.
template <bool VEC>
__device__ __forceinline__ void cell_prefetch_pair(const double* p, bool in_range, bool two, double (&x)[2]) {
    x[0] = x[1] = __longlong_as_double(0x7FF8000000000000ll);
    if (in_range) cell_ld_pair<VEC>(p, two, x);
}

// ---- launch tails -------------------------------------------------------------------------------------------------------------
// The SP twins of a kernel on a 1-D grid: k2 runs when SP = 2 (cell_sp, dfm_cellgeom.h).  Above RB = 16 there is no <RB, 2>
// instance: the caller names <RB, cell_sp_max(RB)> for k2, and the branch is not compiled.
constexpr int cell_sp_max(int RB) { return RB <= 16 ? 2 : 1; }

template <int RB, class Args>
inline hipError_t cell_launch_sp(void (*k1)(Args), void (*k2)(Args), int SP, size_t blocks, int threads, size_t lds,
                                 hipStream_t s, const Args& a) {
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    void (*k)(Args) = k1;
    if constexpr (RB <= 16) {
        if (SP == 2) k = k2;
    }
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(threads), lds, s, a);
    return hipGetLastError();
}

// The VEC twins of a pair kernel on its own grid.
template <class Args>
inline hipError_t cell_launch_vec(void (*kscalar)(Args), void (*kvec)(Args), bool vec, dim3 grid, int threads, size_t lds,
                                  hipStream_t s, const Args& a) {
    hipLaunchKernelGGL(vec ? kvec : kscalar, grid, dim3(threads), lds, s, a);
    return hipGetLastError();
}
#endif  // __HIPCC__

}  // namespace dfm
