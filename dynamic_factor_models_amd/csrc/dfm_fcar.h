// dfm_fcar.h -- the text the series recursions of the model with AR(q) idiosyncratic terms share (forecast_ar.hip,
// simsmooth_ar.hip): the lane's series (loadings, AR coefficients, innovation variance in registers) and, for the path draws of
// dfm_simsmooth_ar_batch, the lane's simulated idiosyncratic path e+ -- a pure function of the call's counters, so that the kernel
// which writes the difference panel and the kernel which assembles the draw run the SAME recursion and x+ is never stored.
#pragma once
#include "dfm_cell.h"
#include "dfm_kernels.h"
#include "dfm_philox.h"

namespace dfm {

// The lane's series: loadings, AR coefficients, innovation variance.  An idle lane (behind the block's last series) walks series
// N - 1 beside the others and stores nothing: it stays for the barriers.
template <int Q, int RB>
struct FcArSeries {
    CellLam<1, RB> lam;
    double rho[Q], sig2;
    int i;
    bool live;
    __device__ __forceinline__ void load(const FcArArgs& a, size_t b, const CellLane& ln) {
        live = ln.live;
        i = live ? ln.i0 : a.N - 1;
        lam.load(a.Lam, b, a.N, i, a.r);
        const size_t bi = b * a.N + i;
#pragma unroll
        for (int l = 0; l < Q; ++l) rho[l] = a.rho[bi * Q + l];
        sig2 = a.sig2[bi];
    }
};

// ---- path draws (dfm_simsmooth_ar_batch; the streams are those of include/dfm_hip.h) ------------------------------------------
enum : uint64_t { kSsArZ0 = 1, kSsArEta = 2, kSsArEpsPlus = 3, kSsArPre = 5 };
constexpr int kSsArLdsTail = 64;              // doubles behind the staged rows: the q lag blocks of z+ (32) and its normals (32)

__device__ __forceinline__ uint64_t ssar_key(uint64_t seed, int64_t first_draw, int d) {
    return seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(first_draw + d + 1));
}

// The workgroup forms rows 0 .. q r - 1 of z+ = mu0 + L_P0 n (lag blocks f+_{q-1} .. f+_0) in sz, the sums in the order of
// simsmooth_path_kernel, which starts the factor path from the same z+.  sn: 32 doubles of scratch.  Barriers inside.
__device__ __forceinline__ void ssar_stage_z(const SsArDraw& dr, size_t b, uint64_t key, int qr, double* sz, double* sn) {
    const int k = dr.k, tid = threadIdx.x;
    if (tid < k) {
        double z0, z1;
        normal2(key, 16 * b + kSsArZ0, (uint64_t)(tid / 2), z0, z1);
        sn[tid] = (tid & 1) ? z1 : z0;
    }
    __syncthreads();
    if (tid < qr) {
        double v = dr.mu0[b * k + tid];
        for (int m = 0; m <= tid; ++m) v = fma(dr.LP0[(b * k + tid) * k + m], sn[m], v);
        sz[tid] = v;
    }
    __syncthreads();
}

// e+ of the lane's series: e[l] = e+_{t-1-l} before step(t).  A Philox block holds the normals of two adjacent series in one row.
// Where the series block starts at an even series (`paired`: wave-uniform) the lanes 2k, 2k + 1 of a wave are such a pair, idle
// lanes included, and share the work over two rows: at an even row the even lane evaluates the block of row t, the odd lane that of
// row t + 1, and each hands the other the component it does not use; the odd row takes the kept one.  One Box-Muller per lane and
// two rows instead of two.  A block that starts at an odd series evaluates every row's block in both lanes.
template <int Q, int RB>
struct SsArIdio {
    double e[Q], ssig, kept;
    uint64_t key, stream, hN, half;
    bool odd, paired;

    // The q terms before output row 0: the residual of the observed panel cell against f+ (x+ equals X there), a N(0, v0) draw
    // where the cell is missing.
    // i0: the first series of the lane's block (lane tid stands at series i0 + tid, which is se.i on a live lane).
    // HASX = false (simulate_ar_cells_kernel without a panel, simulate.hip): dr.X is null and every term is such a draw.
    template <bool HASX = true>
    __device__ __forceinline__ void start(const FcArArgs& a, const SsArDraw& dr, const FcArSeries<Q, RB>& se, size_t b, uint64_t key_,
                                          const double* sz, int i0) {
        key = key_;
        hN = (uint64_t)(a.N + 1) / 2;
        paired = (i0 & 1) == 0;
        const int li = paired ? i0 + (int)threadIdx.x : se.i;
        half = (uint64_t)(li / 2);
        odd = (li & 1) != 0;
        kept = 0.0;
        stream = 16 * b + kSsArEpsPlus;
        ssig = sqrt(se.sig2);
        const double sv0 = sqrt(a.v0 ? a.v0[b * a.N + se.i] : se.sig2);
#pragma unroll
        for (int l = 1; l <= Q; ++l) {
            double x = __longlong_as_double(0x7FF8000000000000ll);
            if constexpr (HASX) x = dr.X[(b * dr.T + (Q - l)) * a.N + se.i];
            const bool obs = x == x;
            double z0 = 0.0, z1 = 0.0;
            if (__any(!obs)) normal2(key, 16 * b + kSsArPre, (uint64_t)(l - 1) * hN + (uint64_t)(se.i / 2), z0, z1);
            e[l - 1] = obs ? x - se.lam.dot(0, sz + (l - 1) * a.r, a.r) : sv0 * ((se.i & 1) ? z1 : z0);
        }
    }

    // e+_t of output row t; the state moves on.  Rows are taken in order from 0, by every lane of the workgroup.
    __device__ __forceinline__ double step(const FcArSeries<Q, RB>& se, int t) {
        double z;
        if (!paired) {
            double z0, z1;
            normal2(key, stream, (uint64_t)t * hN + half, z0, z1);
            z = odd ? z1 : z0;
        } else if ((t & 1) == 0) {
            double z0, z1;
            normal2(key, stream, (uint64_t)(t + (odd ? 1 : 0)) * hN + half, z0, z1);
            const double got = __shfl_xor(odd ? z0 : z1, 1);
            z = odd ? got : z0;
            kept = odd ? z1 : got;
        } else {
            z = kept;
        }
        double en = ssig * z;
#pragma unroll
        for (int l = 0; l < Q; ++l) en = fma(se.rho[l], e[l], en);
#pragma unroll
        for (int l = Q - 1; l > 0; --l) e[l] = e[l - 1];
        e[0] = en;
        return en;
    }
};

}  // namespace dfm
