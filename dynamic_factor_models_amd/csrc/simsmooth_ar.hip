// simsmooth_ar.hip -- the series-side generator of dfm_simsmooth_ar_batch (capi.hip): posterior draws of factor and panel paths from
// the model with AR(q) idiosyncratic terms,  x_it = lam_i' f_t + e_it,  e_it = rho_i1 e_i,t-1 + .. + rho_iq e_i,t-q + eps_it, by the
// simulation smoother of Durbin and Koopman (2002).  xhat of dfm_forecast_ar_batch is an affine map L of the observed cells, so
// x+ + L (X - x+) with x+ simulated from the model has mean xhat and the covariance of xhat's error.  For pass replicate j = b D + d:
//   1. z+ = mu0 + L_P0 n and the factor path f+ of the n = T + H - q output rows          (simsmooth_prep / _path_kernel, m lags)
//   2. the simulated series e+, x+ = lam' f+ + e+ and the difference panel D = X - x+             (simsmooth_ar_diff_kernel, here)
//   3. g = E[f | D] with mu0 = 0: the AR pass on the slice's difference panels                                        (capi.hip)
//   4. the backward messages of the residuals D - lam' g                                (forecast_ar_back_kernel, unchanged)
//   5. the forward filter with the message join, x_draw = lam' (f+ + g) + e+ + ehat*      (simsmooth_ar_fwd_kernel, forecast_ar.hip)
//   6. f_draw = f+ + g                                                                           (simsmooth_ar_finish_kernel)
// B D N dependent recursions with one normal per cell: ONE LANE PER SERIES as in forecast_ar.hip, a workgroup per (pass replicate,
// series block) that walks the rows forward in lockstep, the chunk's f+ rows staged in LDS, lam_i / rho_i / sig2_i in registers, one
// coalesced store of the difference panel per row.  x+ is never stored: step 5 runs the same recursion (SsArIdio, dfm_fcar.h) from
// the same counters.  A Philox block serves two adjacent series: the two lanes of a pair split the Box-Muller work over two rows and
// exchange components where the series block starts at an even series (SsArIdio).
#include "dfm_fcar.h"

namespace dfm {

constexpr size_t kSsArLds = 48 * 1024;

template <int Q, int RB>
__global__ __launch_bounds__(kCellBlockLanes) void simsmooth_ar_diff_kernel(SsArArgs a) {
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
    SsArIdio<Q, RB> gen;
    gen.start(a, a.dr, se, b, key, sz, s * a.geo.NPB);
    const double* xcol = a.dr.X + b * (size_t)T * N + se.i;                  // panel row t of the lane's series: xcol[t N]
    double* dcol = a.dr.diff + bl * (size_t)(n + Q) * N + se.i;
    bool bad = false;
    // rows < q: x+ equals X where X is observed
#pragma unroll
    for (int l = 0; l < Q; ++l) {
        const double x = xcol[(size_t)l * N];
        bad = bad || x != x;
        if (se.live) dcol[(size_t)l * N] = x == x ? 0.0 : nan;
    }
    double xn = xcol[(size_t)Q * N];                                         // (T > q)
    for (int ck = 0; ck < a.geo.nchunk; ++ck) {
        const int t0 = ck * a.geo.RC, t1 = t0 + a.geo.RC < n ? t0 + a.geo.RC : n;
        __syncthreads();
        cell_stage(sm, a.dr.fplus + (j * n + t0) * r, (t1 - t0) * r);
        __syncthreads();
        for (int t = t0; t < t1; ++t) {
            const double x = xn;
            xn = t + 1 + Q < T ? xcol[(size_t)(t + 1 + Q) * N] : nan;       // one row ahead; the horizon rows are NaN
            bad = bad || (x != x && t + Q < T);
            const double mp = se.lam.dot(0, sm + (size_t)(t - t0) * r, r);
            const double ep = gen.step(se, t);
            if (se.live) dcol[(size_t)(Q + t) * N] = x - (mp + ep);          // NaN where X is
        }
    }
    if (a.dr.check_nan && se.live && bad) atomicOr(a.dr.status, 1);
}

template <int Q>
static hipError_t launch_ssar_diff_q(SsArArgs a, hipStream_t s) {
    constexpr size_t tail = kSsArLdsTail * sizeof(double);
    a.geo = series_geometry(a.N, a.r, a.n, kSsArLds - tail);
    const size_t blocks = (size_t)a.S * a.geo.nsblk, lds = (size_t)a.geo.RC * a.r * sizeof(double) + tail;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    void (*k)(SsArArgs) = simsmooth_ar_diff_kernel<Q, 16>;
    if (a.r <= 4) k = simsmooth_ar_diff_kernel<Q, 4>;
    else if (a.r <= 8) k = simsmooth_ar_diff_kernel<Q, 8>;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(a.geo.threads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_simsmooth_ar_diff(const SsArArgs& a, hipStream_t s) {
    if (a.r < 1 || a.r > 16 || a.n < 1 || a.S < 1) return hipErrorInvalidValue;
    switch (a.q) {
        case 1: return launch_ssar_diff_q<1>(a, s);
        case 2: return launch_ssar_diff_q<2>(a, s);
        case 3: return launch_ssar_diff_q<3>(a, s);
        case 4: return launch_ssar_diff_q<4>(a, s);
    }
    return hipErrorInvalidValue;
}

// ---- the small kernels around it ----------------------------------------------------------------------------------------------
// [A_1 .. A_p] on the state of m = max(p, q + 1) lags: zero blocks behind lag p.
__global__ __launch_bounds__(256) void simsmooth_ar_params_kernel(size_t n, int rp, int rm, const double* Avar, double* Apad) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const size_t row = e / rm;
    const int c = (int)(e % rm);
    Apad[e] = c < rp ? Avar[row * rp + c] : 0.0;
}

// dst [S][per] = src [(j0 + s) / D][per]: the per-series parameters simsmooth_expand_kernel does not know (rho).
__global__ __launch_bounds__(256) void simsmooth_ar_expand_kernel(size_t n, long long j0, int D, size_t per, const double* src,
                                                                  double* dst) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const size_t s = e / per, b = (size_t)((j0 + (long long)s) / D);
    dst[e] = src[b * per + e % per];
}

__global__ __launch_bounds__(256) void simsmooth_ar_finish_kernel(size_t n, const double* g, double* f_draw) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) f_draw[e] += g[e];
}

static unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_simsmooth_ar_params(int B, int r, int p, int m, const double* Avar, double* Apad, hipStream_t s) {
    const size_t n = (size_t)B * r * r * m;
    hipLaunchKernelGGL(simsmooth_ar_params_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, r * p, r * m, Avar, Apad);
    return hipGetLastError();
}

hipError_t launch_simsmooth_ar_expand(int S, long long j0, int D, size_t per, const double* src, double* dst, hipStream_t s) {
    const size_t n = (size_t)S * per;
    hipLaunchKernelGGL(simsmooth_ar_expand_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, j0, D, per, src, dst);
    return hipGetLastError();
}

hipError_t launch_simsmooth_ar_finish(size_t n, const double* g, double* f_draw, hipStream_t s) {
    hipLaunchKernelGGL(simsmooth_ar_finish_kernel, dim3(blocks256(n)), dim3(256), 0, s, n, g, f_draw);
    return hipGetLastError();
}

}  // namespace dfm
