// simulate.hip -- panels simulated from a given model (dfm_simulate_batch, dfm_simulate_ar_batch, capi.hip): the x+ the simulation
// smoothers build and never store, written out.  For pass replicate j = b D + d the roots and the factor path f+ come from
// simsmooth_prep_kernel and simsmooth_path_kernel as they stand (simsmooth.hip); the two kernels here are the cell side:
//   plain  x+_ti = lam_i' f+_t + sqrt(R_i) eps+_ti, the normals of stream 3 at the indices of simsmooth_diff_kernel, NaN where the
//          mask panel is NaN (no mask panel: every cell)                                                  (simulate_cells_kernel)
//   AR     e+ by the SsArIdio recursion of dfm_fcar.h (streams 3 and 5), x+_ti = lam_i' f+_t + e+_ti on panel rows q .. T-1, NaN
//          where the panel is; rows < q are the panel's own (a bootstrap conditional on them), or lam_i' f+ of the lag blocks of
//          z+ plus the pre-sample term where there is no panel                                         (simulate_ar_cells_kernel)
// simulate_cells_kernel is a write-bound stream over B D T N cells on the geometry of the other pair kernels (cell_geometry: a lane
// per column pair, the chunk's f+ rows in LDS, loadings in registers, one Philox counter per pair, 16 bytes per lane where N is
// even, the mask row one step ahead).  simulate_ar_cells_kernel is B D N dependent recursions: one lane per series as in
// simsmooth_ar_diff_kernel, rows in lockstep, one coalesced store per row.
#include "dfm_fcar.h"

namespace dfm {

constexpr int kSimMaxThreads = 512;
constexpr size_t kSimLds = 32 * 1024;         // f+ rows staged per workgroup (the cap of the smoother's cell kernels)
constexpr size_t kSimArLds = 48 * 1024;

// RB >= r: loadings in registers; VEC: N even and 16-byte aligned pointers.  blockIdx = (pass replicate of the slice, chunk, series block).
template <int RB, bool VEC>
__global__ __launch_bounds__(kSimMaxThreads) void simulate_cells_kernel(SsArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sfr[];
    const int r = a.r, N = a.N, T = a.T, tid = threadIdx.x;
    const int s = blockIdx.x;
    const CellChunk ch = cell_chunk(a.geo, blockIdx.z, blockIdx.y, s, T);
    const long long j = a.j0 + s;
    const size_t b = (size_t)(j / a.D);
    const int d = (int)(j % a.D);
    const int t0 = ch.t0, t1 = ch.t1;
    cell_stage(sfr, a.f_draw + ((size_t)j * T + t0) * r, (t1 - t0) * r);
    __syncthreads();
    const CellLane ln = cell_lane<2>(a.geo, tid, ch.s, N);
    if (!ln.live) return;
    const int i0 = ln.i0, gr = ln.g;
    const bool two = ln.n == 2;                              // (VEC: N even, always)
    CellLam<2, RB> lam;
    lam.load(a.Lam, b, N, i0, r, ln.n);
    const double sr0 = sqrt(a.R[b * N + i0]), sr1 = two ? sqrt(a.R[b * N + i0 + 1]) : 0.0;
    const uint64_t key = ssar_key(a.seed, a.first_draw, d), stream = 16 * b + kSsArEpsPlus;
    const uint64_t hN = (uint64_t)(N + 1) / 2;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const bool masked = a.panel != nullptr;
    const double* px = masked ? a.panel + b * T * N + i0 : nullptr;
    double* po = a.x_draw + (size_t)j * T * N + i0;
    double nx[2] = {0.0, 0.0};                               // the next row's mask cells, in flight while this row is computed
    if (masked) cell_prefetch_pair<VEC>(px + (size_t)(t0 + gr) * N, t0 + gr < t1, two, nx);
    for (int t = t0 + gr; t < t1; t += a.geo.G) {
        const double* f = sfr + (size_t)(t - t0) * r;
        const double x0 = nx[0], x1 = nx[1];
        const int tn = t + a.geo.G;
        if (masked) cell_prefetch_pair<VEC>(px + (size_t)tn * N, tn < t1, two, nx);
        double m[2];
        lam.dots(f, r, m);
        const bool o0 = x0 == x0, o1 = two && x1 == x1;
        double e0 = 0.0, e1 = 0.0;
        if (o0 || o1) normal2(key, stream, (uint64_t)t * hN + (uint64_t)(i0 / 2), e0, e1);
        double y[2];
        y[0] = o0 ? m[0] + sr0 * e0 : nan;
        y[1] = o1 ? m[1] + sr1 * e1 : nan;
        cell_st_pair<VEC>(po + (size_t)t * N, two, y);
    }
}

template <int RB>
static hipError_t launch_sim_rb(const SsArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((unsigned)a.S, (unsigned)a.geo.nchunk, (unsigned)a.geo.nsblk);
    const size_t lds = (size_t)a.geo.RC * a.r * sizeof(double);
    return cell_launch_vec(simulate_cells_kernel<RB, false>, simulate_cells_kernel<RB, true>, vec, grid, a.geo.threads, lds, s, a);
}

// A lane per column pair; a staged row is f+_t (cell_geometry, dfm_cellgeom.h); a 3-D grid: its y and z extents are checked.
hipError_t launch_simulate_cells(SsArgs a, hipStream_t s) {
    if (a.r < 1 || a.r > 32 || a.S < 1 || a.H != 0) return hipErrorInvalidValue;
    a.geo = cell_geometry((a.N + 1) / 2, a.r, a.T, kSimMaxThreads, kSimLds);
    if (a.geo.nchunk > 65535 || a.geo.nsblk > 65535) return hipErrorInvalidValue;
    const bool vec = cell_vec(a.N, a.panel, a.x_draw);
    return dispatch_r_bucket(a.r, [&](auto RB) { return launch_sim_rb<decltype(RB)::value>(a, vec, s); });
}

// One lane per series, a workgroup per (pass replicate, series block), as simsmooth_ar_diff_kernel: the same staging, the same
// generator from the same counters.  Output row t is panel row q + t.
template <int Q, int RB>
__global__ __launch_bounds__(kCellBlockLanes) void simulate_ar_cells_kernel(SsArArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = a.n, N = a.N, r = a.r, T = a.dr.T, tid = threadIdx.x;
    const int s = (int)(blockIdx.x % (unsigned)a.geo.nsblk);
    const size_t bl = blockIdx.x / (unsigned)a.geo.nsblk, j = (size_t)a.dr.j0 + bl, b = j / (size_t)a.dr.D;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double* sz = sm + (size_t)a.geo.RC * r;
    FcArSeries<Q, RB> se;
    se.load(a, b, cell_lane<1>(a.geo, tid, s, N));
    const uint64_t key = ssar_key(a.dr.seed, a.dr.first_draw, (int)(j % (size_t)a.dr.D));
    ssar_stage_z(a.dr, b, key, Q * r, sz, sz + 32);
    const bool hasx = a.dr.X != nullptr;                                     // (uniform over the launch)
    SsArIdio<Q, RB> gen;
    if (hasx) gen.template start<true>(a, a.dr, se, b, key, sz, s * a.geo.NPB);
    else gen.template start<false>(a, a.dr, se, b, key, sz, s * a.geo.NPB);
    const double* xcol = hasx ? a.dr.X + b * (size_t)T * N + se.i : nullptr;  // panel row t of the lane's series: xcol[t N]
    double* ocol = a.dr.x_draw + j * (size_t)T * N + se.i;
    // rows < q: the panel's own cells, or lam' f+ of lag block l - 1 of z+ (panel row q - l) plus the pre-sample term
#pragma unroll
    for (int l = 1; l <= Q; ++l) {
        const double v = hasx ? xcol[(size_t)(Q - l) * N] : se.lam.dot(0, sz + (l - 1) * r, r) + gen.e[l - 1];
        if (se.live) ocol[(size_t)(Q - l) * N] = v;
    }
    double xn = hasx ? xcol[(size_t)Q * N] : 0.0;                            // (T > q)
    for (int ck = 0; ck < a.geo.nchunk; ++ck) {
        const int t0 = ck * a.geo.RC, t1 = t0 + a.geo.RC < n ? t0 + a.geo.RC : n;
        __syncthreads();
        cell_stage(sm, a.dr.fplus + (j * n + t0) * r, (t1 - t0) * r);
        __syncthreads();
        for (int t = t0; t < t1; ++t) {
            const double x = xn;
            xn = (hasx && t + 1 + Q < T) ? xcol[(size_t)(t + 1 + Q) * N] : 0.0;   // one row ahead
            const double mp = se.lam.dot(0, sm + (size_t)(t - t0) * r, r);
            const double ep = gen.step(se, t);
            if (se.live) ocol[(size_t)(Q + t) * N] = x == x ? mp + ep : nan;
        }
    }
}

template <int Q>
static hipError_t launch_simar_q(SsArArgs a, hipStream_t s) {
    constexpr size_t tail = kSsArLdsTail * sizeof(double);
    a.geo = series_geometry(a.N, a.r, a.n, kSimArLds - tail);
    const size_t blocks = (size_t)a.S * a.geo.nsblk, lds = (size_t)a.geo.RC * a.r * sizeof(double) + tail;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    void (*k)(SsArArgs) = simulate_ar_cells_kernel<Q, 16>;
    if (a.r <= 4) k = simulate_ar_cells_kernel<Q, 4>;
    else if (a.r <= 8) k = simulate_ar_cells_kernel<Q, 8>;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(a.geo.threads), lds, s, a);
    return hipGetLastError();
}

// (r <= 16: the state holds q + 1 >= 2 lags of the factors)
hipError_t launch_simulate_ar_cells(const SsArArgs& a, hipStream_t s) {
    if (a.r < 1 || a.r > 16 || a.n < 1 || a.S < 1 || a.dr.T != a.n + a.q) return hipErrorInvalidValue;
    switch (a.q) {
        case 1: return launch_simar_q<1>(a, s);
        case 2: return launch_simar_q<2>(a, s);
        case 3: return launch_simar_q<3>(a, s);
        case 4: return launch_simar_q<4>(a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace dfm
