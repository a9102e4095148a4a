// gibbs_ar.hip -- the series block "rho_i, sig2_i, lam_i | factor path" of the Gibbs sampler of the model with AR(q) idiosyncratic
// terms (dfm_gibbs_ar_batch, capi.hip; include/dfm_hip.h),  x_it = lam_i' f_t + e_it,  e_it = rho_i1 e_i,t-1 + .. + rho_iq e_i,t-q + eps_it.
// For chain b and the path F the simulation smoother drew for this sweep (n output rows = panel rows q .. T-1), with
// U_i = { t >= q : cells t, t-1, .. t-q of series i observed }:
//   walk 1 (the entry lam_i)  e_t = X_ti - lam_i' F_t, w_t = (e_t-1 .. e_t-q): sum w w', sum w e_t over U_i; then
//          S = tau_rho I + sum w w' / sig2_i = L L', y = L^-1 sum w e_t / sig2_i, candidates L^-T (y + n) until one is stationary
//   walk 2 (the new rho_i)    x~_t = X_t - sum rho_l X_t-l, f~_t = F_t - sum rho_l F_t-l: sum f~ f~', sum f~ x~, sum x~^2, n_i over U_i;
//          then the conjugate draw of gibbs_load_kernel<RB, true> (gibbs.hip) on them, with the loadings' normals on stream 10.
// N regressions per chain that share nothing (each series quasi-differences with its own rho_i): ONE LANE PER SERIES, a workgroup
// per (chain, series block) on series_geometry, lam_i / rho_i / sig2_i in registers (FcArSeries), the chunk's F rows in LDS behind
// their q preceding rows and zero-padded to RB columns (those coordinates decouple, the loops run to RB at compile time), the panel
// read coalesced across the series one row ahead.  "Observed" is a select and a run-length counter of consecutive observed rows:
// t is in U_i when the run exceeds q.  A masked row adds exact zeros, every sum runs over t in ascending order and nothing is
// combined across lanes, so two runs agree bit for bit.
#include "dfm_fcar.h"
#include "dfm_gibbs.h"
#include "dfm_smallmat.h"

namespace dfm {

constexpr size_t kGbArLds = 48 * 1024;
constexpr int kGbArRhoCap = 32;               // candidates of one rho draw

// S = tau I + G = L L' in place in the packed lower triangle (row-major: G[j (j + 1) / 2 + m], m <= j); psd_root's rule on the
// first r coordinates: a pivot <= kPsdTol trace(S) fails.  Coordinates r .. NB-1 hold tau alone.
template <int NB>
__device__ __forceinline__ bool gb_chol_packed(double (&G)[NB * (NB + 1) / 2], int r, double tau) {
    bool bad = false;
    double tr = 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j)
        if (j < r) tr += G[j * (j + 1) / 2 + j] + tau;
    const double tol = kPsdTol * tr;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        double dj = G[j * (j + 1) / 2 + j] + tau;
#pragma unroll
        for (int m = 0; m < j; ++m) dj = fma(-G[j * (j + 1) / 2 + m], G[j * (j + 1) / 2 + m], dj);
        bad |= j < r && !(dj > tol);
        const double ljj = sqrt(dj), inv = 1.0 / ljj;
        G[j * (j + 1) / 2 + j] = ljj;
#pragma unroll
        for (int i2 = j + 1; i2 < NB; ++i2) {
            double v = G[i2 * (i2 + 1) / 2 + j];
#pragma unroll
            for (int m = 0; m < j; ++m) v = fma(-G[i2 * (i2 + 1) / 2 + m], G[j * (j + 1) / 2 + m], v);
            G[i2 * (i2 + 1) / 2 + j] = v * inv;
        }
    }
    return bad;
}
// s <- L^-1 s; returns s's squared length
template <int NB>
__device__ __forceinline__ double gb_fwd_packed(const double (&L)[NB * (NB + 1) / 2], double (&s)[NB]) {
    double yy = 0.0;
#pragma unroll
    for (int p = 0; p < NB; ++p) {
        double v = s[p];
#pragma unroll
        for (int q = 0; q < p; ++q) v = fma(-L[p * (p + 1) / 2 + q], s[q], v);
        v = v / L[p * (p + 1) / 2 + p];
        s[p] = v;
        yy = fma(v, v, yy);
    }
    return yy;
}
// s <- L^-T s
template <int NB>
__device__ __forceinline__ void gb_back_packed(const double (&L)[NB * (NB + 1) / 2], double (&s)[NB]) {
#pragma unroll
    for (int pp = 0; pp < NB; ++pp) {
        const int p = NB - 1 - pp;
        double v = s[p];
#pragma unroll
        for (int q = p + 1; q < NB; ++q) v = fma(-L[q * (q + 1) / 2 + p], s[q], v);
        s[p] = v / L[p * (p + 1) / 2 + p];
    }
}

// The step-down (Levinson) recursion: phi is stationary when every reflection coefficient lies inside (-1, 1).
template <int Q>
__device__ __forceinline__ bool gb_stationary(const double (&phi)[Q]) {
    double c[Q];
#pragma unroll
    for (int l = 0; l < Q; ++l) c[l] = phi[l];
    bool ok = true;
#pragma unroll
    for (int kk = 0; kk < Q; ++kk) {
        const int k = Q - kk;
        const double kap = c[k - 1];
        ok = ok && fabs(kap) < 1.0;
        const double den = 1.0 - kap * kap;
#pragma unroll
        for (int j = 1; 2 * j <= k - 1; ++j) {                // the pair (j, k - j) moves together; the middle one alone
            const double u = c[j - 1], w = c[k - j - 1];
            c[j - 1] = (u + kap * w) / den;
            c[k - j - 1] = (w + kap * u) / den;
        }
        if (k > 1 && (k - 1) % 2 == 1) c[k / 2 - 1] = (c[k / 2 - 1] + kap * c[k / 2 - 1]) / den;
    }
    return ok;
}

// Rows t0 - lag .. t0 + nrow - 1 of F into sm, RB doubles each: zero beyond column r and before row 0.
template <int RB>
__device__ __forceinline__ void gb_ar_stage(double* sm, const double* F, int t0, int nrow, int lag, int r) {
    for (int e = threadIdx.x; e < (nrow + lag) * RB; e += blockDim.x) {
        const int t = t0 - lag + e / RB, m = e % RB;
        sm[e] = (t >= 0 && m < r) ? F[(size_t)t * r + m] : 0.0;
    }
}

template <int Q, int RB>
__global__ __launch_bounds__(kCellBlockLanes) void gibbs_ar_series_kernel(GbArArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int NP = RB * (RB + 1) / 2, NQ = Q * (Q + 1) / 2;
    const int n = a.n, N = a.N, r = a.r, tid = threadIdx.x;
    const int sb = (int)(blockIdx.x % (unsigned)a.geo.nsblk);
    const size_t b = blockIdx.x / (unsigned)a.geo.nsblk;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    FcArArgs v{};
    v.N = N; v.r = r; v.Lam = a.Lam; v.sig2 = a.sig2; v.rho = a.rho;
    FcArSeries<Q, RB> se;
    se.load(v, b, cell_lane<1>(a.geo, tid, sb, N));          // (an idle lane walks series N - 1 and stores nothing)
    const double* xcol = a.panel + (b * (size_t)(n + Q) + Q) * N + se.i;     // output row t of the lane's series: xcol[t N]
    const double* F = a.f + b * (size_t)n * r;
    const uint64_t key = gb_key(a.seed, a.sweep);
    bool fail = false;

    // ---- walk 1: rho_i | lam_i, sig2_i, F
    {
        double W[NQ], we[Q], e[Q];
#pragma unroll
        for (int c = 0; c < NQ; ++c) W[c] = 0.0;
#pragma unroll
        for (int l = 0; l < Q; ++l) { we[l] = 0.0; e[l] = 0.0; }
        int run = 0;
        double xn = xcol[0];
        for (int ck = 0; ck < a.geo.nchunk; ++ck) {
            const int t0 = ck * a.geo.RC, t1 = t0 + a.geo.RC < n ? t0 + a.geo.RC : n;
            __syncthreads();
            gb_ar_stage<RB>(sm, F, t0, t1 - t0, 0, r);
            __syncthreads();
            for (int t = t0; t < t1; ++t) {
                const double x = xn;
                xn = t + 1 < n ? xcol[(size_t)(t + 1) * N] : nan;
                const bool obs = x == x;
                const double et = obs ? x - se.lam.dot(0, sm + (size_t)(t - t0) * RB, RB) : 0.0;
                run = obs ? run + 1 : 0;
                const bool use = run > Q;
#pragma unroll
                for (int j = 0; j < Q; ++j) {
                    const double wv = use ? e[j] : 0.0;
                    we[j] = fma(wv, et, we[j]);
#pragma unroll
                    for (int m = 0; m <= j; ++m) W[j * (j + 1) / 2 + m] = fma(wv, e[m], W[j * (j + 1) / 2 + m]);
                }
#pragma unroll
                for (int l = Q - 1; l > 0; --l) e[l] = e[l - 1];
                e[0] = et;
            }
        }
#pragma unroll
        for (int c = 0; c < NQ; ++c) W[c] = W[c] / se.sig2;
#pragma unroll
        for (int l = 0; l < Q; ++l) we[l] = we[l] / se.sig2;
        const bool bad = gb_chol_packed<Q>(W, Q, a.tau_rho);
        gb_fwd_packed<Q>(W, we);
        constexpr int hq = (Q + 1) / 2;
        bool done = bad;
        // one Philox block per trip: trip it draws pair l2 = it % hq of attempt it / hq; the last pair completes the candidate
        double c[Q];
#pragma unroll
        for (int l = 0; l < Q; ++l) c[l] = we[l];
        for (int it = 0; it < kGbArRhoCap * hq && !done; ++it) {
            const int k = it / hq, l2 = it % hq;
            double z0, z1;
            normal2(key, 16 * b + kGbArRhoN, ((uint64_t)k * (uint64_t)N + (uint64_t)se.i) * hq + l2, z0, z1);
#pragma unroll
            for (int l = 0; l < Q; ++l) c[l] = (l / 2 == l2) ? we[l] + ((l & 1) ? z1 : z0) : c[l];
            if (l2 == hq - 1) {
                gb_back_packed<Q>(W, c);
                done = gb_stationary<Q>(c);
#pragma unroll
                for (int l = 0; l < Q; ++l) se.rho[l] = done ? c[l] : se.rho[l];
            }
        }
        fail = bad || !done;                                  // a failed root or 32 rejected candidates leave rho_i as it was
        if (se.live && !fail) {
#pragma unroll
            for (int l = 0; l < Q; ++l) a.rho[(b * N + se.i) * Q + l] = se.rho[l];
        }
    }

    // ---- walk 2: sig2_i, lam_i | rho_i, F
    double G[NP], s[RB], xr[Q];
    double xx = 0.0, cnt = 0.0;
#pragma unroll
    for (int c = 0; c < NP; ++c) G[c] = 0.0;
#pragma unroll
    for (int m = 0; m < RB; ++m) s[m] = 0.0;
#pragma unroll
    for (int l = 0; l < Q; ++l) xr[l] = 0.0;
    {
        int run = 0;
        double xn = xcol[0];
        for (int ck = 0; ck < a.geo.nchunk; ++ck) {
            const int t0 = ck * a.geo.RC, t1 = t0 + a.geo.RC < n ? t0 + a.geo.RC : n;
            __syncthreads();
            gb_ar_stage<RB>(sm, F, t0, t1 - t0, Q, r);
            __syncthreads();
            for (int t = t0; t < t1; ++t) {
                const double x = xn;
                xn = t + 1 < n ? xcol[(size_t)(t + 1) * N] : nan;
                const bool obs = x == x;
                const double x0 = obs ? x : 0.0;
                run = obs ? run + 1 : 0;
                const bool use = run > Q;
                const double* fr = sm + (size_t)(t - t0 + Q) * RB;             // F_t; F_t-l is RB l doubles before it
                double xt = x0, ft[RB];
#pragma unroll
                for (int l = 0; l < Q; ++l) xt = fma(-se.rho[l], xr[l], xt);
#pragma unroll
                for (int m = 0; m < RB; ++m) {
                    double w = fr[m];
#pragma unroll
                    for (int l = 0; l < Q; ++l) w = fma(-se.rho[l], fr[m - (l + 1) * RB], w);
                    ft[m] = w;
                }
                const double xv = use ? xt : 0.0;
                xx = fma(xv, xt, xx);
                cnt += use ? 1.0 : 0.0;
#pragma unroll
                for (int m = 0; m < RB; ++m) {
                    const double fv = use ? ft[m] : 0.0;
                    s[m] = fma(fv, xt, s[m]);
#pragma unroll
                    for (int c = 0; c <= m; ++c) G[m * (m + 1) / 2 + c] = fma(fv, ft[c], G[m * (m + 1) / 2 + c]);
                }
#pragma unroll
                for (int l = Q - 1; l > 0; --l) xr[l] = xr[l - 1];
                xr[0] = x0;
            }
        }
    }
    bool bad = gb_chol_packed<RB>(G, r, a.tau_lam);
    const double yy = gb_fwd_packed<RB>(G, s);                // y = L^-1 sum f~ x~; m' S m = y'y
    bool capped = false;
    const double ga = 0.5 * (a.nu_R + cnt), gbb = 0.5 * (a.nu_R * a.s_R + xx - yy);
    const double g = gb_gamma(key, 16 * b + kGbRGam, se.i, N, ga, capped);
    const double Si = gbb / g;
    bad |= !(Si > 0.0);
    const double sr = sqrt(Si);
    const int hr = (r + 1) / 2;
#pragma unroll
    for (int q2 = 0; q2 < (RB + 1) / 2; ++q2) {               // lam = L^-T (y + sqrt(sig2_i) z)
        double z0 = 0.0, z1 = 0.0;
        if (q2 < hr) normal2(key, 16 * b + kGbArLamN, (uint64_t)se.i * hr + q2, z0, z1);
        s[2 * q2] = fma(sr, z0, s[2 * q2]);
        if (2 * q2 + 1 < RB && 2 * q2 + 1 < r) s[2 * q2 + 1] = fma(sr, z1, s[2 * q2 + 1]);
    }
    gb_back_packed<RB>(G, s);
    if (!se.live) return;
    if (fail || bad || capped) atomicOr(a.status, kGbFailBit);
    if (bad) return;                                          // a failed draw leaves the series' lam_i, sig2_i as they were
#pragma unroll
    for (int m = 0; m < RB; ++m)
        if (m < r) a.Lam[(b * N + se.i) * r + m] = s[m];
    a.sig2[b * N + se.i] = Si;
}

template <int Q>
static hipError_t launch_gibbs_ar_q(GbArArgs a, hipStream_t s) {
    const int RB = a.r <= 4 ? 4 : 8;
    const size_t lag = (size_t)Q * RB * sizeof(double);
    a.geo = series_geometry(a.N, RB, a.n, kGbArLds - lag);
    const size_t blocks = (size_t)a.B * a.geo.nsblk, lds = (size_t)a.geo.RC * RB * sizeof(double) + lag;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    void (*k)(GbArArgs) = gibbs_ar_series_kernel<Q, 8>;
    if (RB == 4) k = gibbs_ar_series_kernel<Q, 4>;
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(a.geo.threads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_gibbs_ar_series(const GbArArgs& a, hipStream_t s) {
    if (a.r < 1 || a.r > 8 || a.n < 1 || a.B < 1 || a.N < 1) return hipErrorInvalidValue;
    switch (a.q) {
        case 1: return launch_gibbs_ar_q<1>(a, s);
        case 2: return launch_gibbs_ar_q<2>(a, s);
        case 3: return launch_gibbs_ar_q<3>(a, s);
        case 4: return launch_gibbs_ar_q<4>(a, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace dfm
