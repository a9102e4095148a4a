// proxy.hip -- impulse responses identified by an external instrument (dfm_proxyirf_batch, capi.hip; semantics in include/dfm_hip.h).
// sv_prep_kernel (structural.hip, named = null) supplies S = chol(Q), S^-1 and the tables Theta_h = Psi_h S of every replicate; the
// smoother pass supplies f_t|T.  Slot 0 of a replicate is the sample of its n used rows, slots 1 .. D are moving block draws.  Then
//   px_rows_kernel        one workgroup per replicate: etahat_t = f_t - sum_j A_j f_{t-j} and z_t of the used rows, [n][r+1]
//   px_moment_kernel      the hot path: a workgroup owns a replicate and kPxLanes slots, one slot per lane, the replicate's row table in
//                         LDS with an odd row stride (lanes gather different rows); a table over kPxTabLds is read from global
//                         memory instead (through L2).  A lane draws its block starts (one Philox block gives four), keeps 2 r + 2
//                         running sums over its n rows, forms the centred moments m and v, solves S y = m by forward substitution
//                         (S from LDS: a broadcast), kappa = y'y, hvec = m / sqrt(kappa), w = S^-1 hvec = y / sqrt(kappa), flips the
//                         sign on lam_norm' hvec < 0 and writes impact, rel and w.  r <= 8: R = r, all in registers.  r > 8: R = 0,
//                         the same text with run-time loops -- correct, not fast.
//   px_slot_table_kernel  Theta_h w and Theta^c_h w of every slot, [B][D+1][H][r], and the unit-effect divisor of the slot
//   px_den_kernel         1 / (sum_k num_k + idio) of dfm_irf_batch, [B][H][N]: a per-replicate table that the D + 1 slots share
//   px_fill_kernel        streams irf / fevd [B][D+1][H][N]: a workgroup owns a slot and a block of series, a lane one series (or two
//                         adjacent ones, 16-byte stores), walks h in order with the slot's rows in LDS (a broadcast), one response and
//                         one running sum of squares per series; the den loads of kPxDenAhead rows are in flight together, and the
//                         workgroup ids are remapped so that the slots of a replicate run on one XCD
//   px_shock_kernel       u_t = w_0' S^-1 etahat_t of slot 0, all t at once
// No atomics; every sum runs in a fixed order, so two identical calls agree bit for bit.
#include "dfm_cell.h"
#include "dfm_kernels.h"
#include "dfm_philox.h"

namespace dfm {

constexpr int kPxFillLanes = 128;             // px_fill_kernel: lanes (series, or pairs of series) per workgroup
constexpr size_t kPxFillLds = 48 * 1024;
constexpr int kPxDenAhead = 8;               // px_fill_kernel: rows whose den loads are in flight together
constexpr uint64_t kPxStream = 11;            // stream word 16 b + 11 (1-10 are taken)

__host__ __device__ inline int px_stride(int r) { return (r + 1) | 1; }
size_t proxy_row_stride(int r) { return (size_t)px_stride(r); }

__device__ __forceinline__ double px_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(256) void px_rows_kernel(PxArgs a) {
    __shared__ double sA[1024];
    const size_t b = blockIdx.x;
    const int r = a.r, p = a.p, k = a.r * a.p, r1 = a.r + 1, tid = threadIdx.x, nth = blockDim.x;
    const double* f = a.f + b * a.T * r;
    for (int e = tid; e < r * k; e += nth) sA[e] = a.A[b * r * k + e];
    __syncthreads();
    for (int e = tid; e < a.n * r1; e += nth) {
        const int t = a.U[e / r1], c = e % r1;
        double v;
        if (c == r) {
            v = a.z[t];
        } else {
            v = f[(size_t)t * r + c];
            for (int j = 1; j <= p; ++j)
                for (int m = 0; m < r; ++m) v = fma(-sA[c * k + (j - 1) * r + m], f[(size_t)(t - j) * r + m], v);
        }
        a.rows[b * a.n * r1 + e] = v;
    }
}

// The 2 r + 2 sums of slot s over its n source rows: se = sum eta, sez = sum eta z, sz = sum z, szz = sum z^2.
// tab: the row table, ts doubles per row (LDS or global: the call sites are inlined, each with its own address space).
template <int RM>
__device__ __forceinline__ void px_sums(const double* tab, int ts, int r, int n, int L, int s, uint64_t key, uint64_t stream,
                                        double (&se)[RM], double (&sez)[RM], double& sz, double& szz) {
    auto add = [&](int row) {
        const double* q = tab + (size_t)row * ts;
        const double z = q[r];
        sz += z;
        szz = fma(z, z, szz);
#pragma unroll
        for (int c = 0; c < RM; ++c)
            if (c < r) {
                se[c] += q[c];
                sez[c] = fma(q[c], z, sez[c]);
            }
    };
    if (s == 0) {
        for (int j = 0; j < n; ++j) add(j);
        return;
    }
    const int nb = (n + L - 1) / L;
    const uint64_t span = (uint64_t)(n - L + 1);
    for (int k0 = 0; k0 < nb; k0 += 4) {
        uint32_t o[4];
        Philox::block(key, (uint64_t)(k0 / 4), stream, o);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + q;
            if (k < nb) {
                const int start = (int)(((uint64_t)o[q] * span) >> 32);        // 0 .. n - L
                const int len = n - k * L < L ? n - k * L : L;
                for (int j = 0; j < len; ++j) add(start + j);
            }
        }
    }
}

// R in 1..8: r = R, the sums in registers.  R = 0: any r <= 32, run-time loops.
template <int R>
__global__ __launch_bounds__(kPxLanes) void px_moment_kernel(PxArgs a) {
    constexpr int RM = R ? R : 32;
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, r = R ? R : a.r, rr = r * r, n = a.n, D1 = a.D + 1, r1 = r + 1, st = px_stride(r);
    const unsigned nblk = (unsigned)((D1 + kPxLanes - 1) / kPxLanes);
    const size_t b = blockIdx.x / nblk;
    const int s = (int)(blockIdx.x % nblk) * kPxLanes + tid;
    const bool in_lds = (size_t)n * st * sizeof(double) <= kPxTabLds;
    double* sS = sm;                                                 // [r][r] the root of Q
    double* sl = sm + rr;                                            // [r] lam_norm
    double* stab = sm + rr + r;                                      // [n][st]
    const double* grows = a.rows + b * n * r1;
    for (int e = tid; e < rr; e += blockDim.x) sS[e] = a.S[b * rr + e];
    for (int e = tid; e < r; e += blockDim.x) sl[e] = a.Lam[(b * a.N + a.norm) * r + e];
    if (in_lds)
        for (int e = tid; e < n * r1; e += blockDim.x) stab[(e / r1) * st + e % r1] = grows[e];
    __syncthreads();
    if (s >= D1) return;
    const uint64_t key = a.seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(a.first_draw + s));      // g + 1 = first_draw + (s - 1) + 1
    double se[RM], sez[RM], sz = 0.0, szz = 0.0;
#pragma unroll
    for (int c = 0; c < RM; ++c) { se[c] = 0.0; sez[c] = 0.0; }
    if (in_lds) px_sums<RM>(stab, st, r, n, a.L, s, key, 16 * (uint64_t)b + kPxStream, se, sez, sz, szz);
    else px_sums<RM>(grows, r1, r, n, a.L, s, key, 16 * (uint64_t)b + kPxStream, se, sez, sz, szz);
    const double dn = (double)n, zbar = sz / dn, v = (szz - zbar * sz) / dn;
    // m (in sez), then y = S^-1 m by forward substitution (in se); a zero pivot leaves a zero component, as sv_prep_kernel has it
    double kappa = 0.0;
#pragma unroll
    for (int i = 0; i < RM; ++i)
        if (i < r) {
            sez[i] = (sez[i] - zbar * se[i]) / dn;
            double y = sez[i];
#pragma unroll
            for (int j = 0; j < RM; ++j)
                if (j < i) y = fma(-sS[i * r + j], se[j], y);
            const double piv = sS[i * r + i];
            y = piv > 0.0 ? y / piv : 0.0;
            se[i] = y;
            kappa = fma(y, y, kappa);
        }
    const bool ok = kappa > 0.0;
    const double sq = sqrt(kappa);
    double dot = 0.0;
#pragma unroll
    for (int c = 0; c < RM; ++c)
        if (c < r) {
            sez[c] = sez[c] / sq;
            se[c] = se[c] / sq;
            dot = fma(sl[c], sez[c], dot);
        }
    const bool flip = dot < 0.0;
    const size_t o = b * D1 + s;
    const double nan = px_nan();
#pragma unroll
    for (int c = 0; c < RM; ++c)
        if (c < r) {
            a.impact[o * r + c] = ok ? (flip ? -sez[c] : sez[c]) : nan;
            a.w[o * r + c] = ok ? (flip ? -se[c] : se[c]) : nan;
        }
    a.rel[o] = ok ? kappa / v : nan;
}

// A thread per (slot, h, component); the threads of (h = 0, component 0) also write the slot's unit-effect divisor, in the fill's own
// arithmetic so that its quotient is exactly 1.
__global__ __launch_bounds__(256) void px_slot_table_kernel(PxArgs a) {
    const int r = a.r, rr = r * r, H = a.H, D1 = a.D + 1;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x, tot = (size_t)a.B * D1 * H * r;
    if (e >= tot) return;
    const int i = (int)(e % r), h = (int)((e / r) % H);
    const size_t sl = e / ((size_t)r * H), b = sl / D1;
    const double* w = a.w + sl * r;
    const double* T = a.Th + (b * H + h) * rr;                       // T[k r + i] = (Theta_h)_ik
    double v = 0.0;
    for (int k = 0; k < r; ++k) v = fma(T[k * r + i], w[k], v);
    a.tk[e] = v;
    if (a.tkc) {
        const double* Tc = a.Thc + (b * H + h) * rr;
        double vc = 0.0;
        for (int k = 0; k < r; ++k) vc = fma(Tc[k * r + i], w[k], vc);
        a.tkc[e] = vc;
    }
    if (a.scale && h == 0 && i == 0) {
        const size_t bi = b * a.N + a.norm;
        double x = 0.0;
        for (int m = 0; m < r; ++m) {
            double t0 = 0.0;
            for (int k = 0; k < r; ++k) t0 = fma(T[k * r + m], w[k], t0);
            x = fma(a.Lam[bi * r + m], t0, x);
        }
        x = a.sd ? a.sd[bi] * x : 1.0 * x;
        a.scale[sl] = x == 0.0 ? px_nan() : x;
    }
}

// 1 / (sum_k num_k + idio) for a block of series of one replicate, h in order: the arithmetic of sv_irf_fill_kernel.
template <int RB>
__global__ __launch_bounds__(256) void px_den_kernel(PxArgs a) {
    __shared__ double sT[RB * RB], sTc[RB * RB];
    const size_t b = blockIdx.x;
    const int r = a.r, rr = r * r, H = a.H, N = a.N, tid = threadIdx.x;
    const int i = blockIdx.y * blockDim.x + tid;
    const bool live = i < N, hasc = a.Thc != nullptr;
    const size_t bi = b * N + (live ? i : 0);
    double lam[RB], ssq[RB];
#pragma unroll
    for (int m = 0; m < RB; ++m) { lam[m] = m < r ? a.Lam[bi * r + m] : 0.0; ssq[m] = 0.0; }
    const double Rv = a.R[bi];
    const bool cm = a.cum != nullptr && a.cum[live ? i : 0] != 0;
    for (int e = tid; e < RB * RB; e += blockDim.x) { sT[e] = 0.0; sTc[e] = 0.0; }
    for (int h = 0; h < H; ++h) {
        __syncthreads();
        for (int e = tid; e < rr; e += blockDim.x) {
            sT[(e / r) * RB + e % r] = a.Th[(b * H + h) * rr + e];
            if (hasc) sTc[(e / r) * RB + e % r] = a.Thc[(b * H + h) * rr + e];
        }
        __syncthreads();
        if (!live) continue;
        const double* Tq = cm ? sTc : sT;
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < RB; ++k)
            if (k < r) {
                double v = 0.0;
#pragma unroll
                for (int m = 0; m < RB; ++m) v = fma(lam[m], Tq[k * RB + m], v);
                ssq[k] = fma(v, v, ssq[k]);
                tot += ssq[k];
            }
        const double idio = cm ? (double)(h + 1) * Rv : Rv;
        a.den[(b * H + h) * N + i] = 1.0 / (tot + idio);
    }
}

template <int RB, int SP>
__global__ __launch_bounds__(kPxFillLanes) void px_fill_kernel(PxArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x, r = a.r, H = a.H, N = a.N, D1 = a.D + 1;
    // Workgroups are dealt round-robin over the 8 XCDs: the ids that share an XCD take a contiguous run of (slot, series block) pairs,
    // so that the D + 1 slots of a replicate read its loadings and its den table through one L2 (a bijection for any grid size)
    const unsigned nwg = gridDim.x, xcd = blockIdx.x % 8u, wq = nwg / 8u, wr = nwg % 8u;
    const unsigned wg = (xcd < wr ? xcd * (wq + 1u) : wr * (wq + 1u) + (xcd - wr) * wq) + blockIdx.x / 8u;
    const int s = (int)(wg % (unsigned)a.geo.nsblk);
    const size_t sl = wg / (unsigned)a.geo.nsblk, b = sl / (unsigned)D1;
    const bool hasc = a.tkc != nullptr, wantV = a.fevd != nullptr, wantI = a.irf != nullptr;
    double* sT = sm;                                                 // [RC][RB], columns r .. RB - 1 zero
    double* sTc = sm + (size_t)a.geo.RC * RB;
    const CellLane ln = cell_lane<SP>(a.geo, tid, s, N);             // (G = 1: an idle lane stays for the barriers)
    const int i0 = ln.i0;
    const bool live = ln.live;
    CellLam<SP, RB> lam;
    lam.load(a.Lam, b, N, i0, r, ln.n);
    double ssq[SP], sdv[SP];
    bool cm[SP];
#pragma unroll
    for (int q = 0; q < SP; ++q) {
        const size_t bi = b * N + (live ? i0 + q : 0);
        ssq[q] = 0.0;
        sdv[q] = a.sd ? a.sd[bi] : 1.0;
        cm[q] = a.cum != nullptr && a.cum[live ? i0 + q : 0] != 0;
    }
    const bool unit = a.scale != nullptr;
    const double sc = unit ? a.scale[sl] : 1.0;
    for (int h0 = 0; h0 < H; h0 += a.geo.RC) {
        const int nh = H - h0 < a.geo.RC ? H - h0 : a.geo.RC;
        __syncthreads();
        for (int e = tid; e < nh * RB; e += blockDim.x) {
            const int m = e % RB, hh = e / RB;
            sT[e] = m < r ? a.tk[(sl * H + h0 + hh) * r + m] : 0.0;
            if (hasc) sTc[e] = m < r ? a.tkc[(sl * H + h0 + hh) * r + m] : 0.0;
        }
        __syncthreads();
        if (!live) continue;
        // kPxDenAhead rows at a time: their den loads are issued together, ahead of the rows' arithmetic and stores (a load per row
        // in front of its stores left the lane waiting on L2 once per row)
        for (int hq = 0; hq < nh; hq += kPxDenAhead) {
            double dn[kPxDenAhead][SP];
#pragma unroll
            for (int u = 0; u < kPxDenAhead; ++u) {
                const int h = h0 + hq + u;
#pragma unroll
                for (int q = 0; q < SP; ++q) dn[u][q] = 0.0;
                if (wantV) cell_ld<SP>(a.den + (b * H + (h < H ? h : H - 1)) * N + i0, dn[u]);
            }
#pragma unroll
            for (int u = 0; u < kPxDenAhead; ++u) {
                const int hh = hq + u, h = h0 + hh;
                if (hh >= nh) break;
                double x[SP];
#pragma unroll
                for (int q = 0; q < SP; ++q) {
                    const double* Tq = (cm[q] ? sTc : sT) + (size_t)hh * RB;
                    const double v = lam.dot(q, Tq, RB);          // (the staged rows are zero beyond r, as the loadings are)
                    ssq[q] = fma(v, v, ssq[q]);
                    x[q] = unit ? sdv[q] * v / sc : sdv[q] * v;
                }
                const size_t o = (sl * H + h) * N + i0;
                if (wantI) cell_st<SP>(a.irf + o, x);
                if (!wantV) continue;
#pragma unroll
                for (int q = 0; q < SP; ++q) x[q] = ssq[q] * dn[u][q];
                cell_st<SP>(a.fevd + o, x);
            }
        }
    }
}

// u_t of slot 0: g = S^-T w_0, u_t = g' etahat_t.  A thread per period.
__global__ __launch_bounds__(256) void px_shock_kernel(PxArgs a) {
    __shared__ double sA[1024], sg[32];
    const size_t b = blockIdx.x;
    const int r = a.r, p = a.p, k = a.r * a.p, T = a.T, tid = threadIdx.x, nth = blockDim.x;
    const double* f = a.f + b * T * r;
    const double* w = a.w + b * (a.D + 1) * r;
    for (int e = tid; e < r * k; e += nth) sA[e] = a.A[b * r * k + e];
    if (tid < r) {
        double v = 0.0;
        for (int m = 0; m < r; ++m) v = fma(a.Sinv[b * r * r + m * r + tid], w[m], v);
        sg[tid] = v;
    }
    __syncthreads();
    const int t = blockIdx.y * nth + tid;
    if (t >= T) return;
    double u = 0.0;
    if (t >= p)
        for (int c = 0; c < r; ++c) {
            double v = f[(size_t)t * r + c];
            for (int j = 1; j <= p; ++j)
                for (int m = 0; m < r; ++m) v = fma(-sA[c * k + (j - 1) * r + m], f[(size_t)(t - j) * r + m], v);
            u = fma(sg[c], v, u);
        }
    a.shock[b * T + t] = u;
}

hipError_t launch_px_rows(const PxArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(px_rows_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

// Fewer than kPxLanes slots per replicate: whole waves for the slots there are (the slot index still counts in kPxLanes).
template <int R>
static hipError_t launch_moment_r(const PxArgs& a, unsigned blocks, size_t lds, hipStream_t s) {
    const int lanes = a.D + 1 < kPxLanes ? (a.D + 1 + 63) / 64 * 64 : kPxLanes;
    hipLaunchKernelGGL((px_moment_kernel<R>), dim3(blocks), dim3(lanes), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_px_moment(const PxArgs& a, hipStream_t s) {
    const size_t blocks = (size_t)a.B * ((a.D + 1 + kPxLanes - 1) / kPxLanes);
    if (a.r < 1 || a.r > 32 || a.n < 1 || a.L < 1 || a.L > a.n || blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const size_t tab = (size_t)a.n * px_stride(a.r) * sizeof(double);
    const size_t lds = ((size_t)a.r * a.r + a.r) * sizeof(double) + (tab <= kPxTabLds ? tab : 0);
    switch (a.r) {
        case 1: return launch_moment_r<1>(a, (unsigned)blocks, lds, s);
        case 2: return launch_moment_r<2>(a, (unsigned)blocks, lds, s);
        case 3: return launch_moment_r<3>(a, (unsigned)blocks, lds, s);
        case 4: return launch_moment_r<4>(a, (unsigned)blocks, lds, s);
        case 5: return launch_moment_r<5>(a, (unsigned)blocks, lds, s);
        case 6: return launch_moment_r<6>(a, (unsigned)blocks, lds, s);
        case 7: return launch_moment_r<7>(a, (unsigned)blocks, lds, s);
        case 8: return launch_moment_r<8>(a, (unsigned)blocks, lds, s);
        default: return launch_moment_r<0>(a, (unsigned)blocks, lds, s);
    }
}

hipError_t launch_px_slot_table(const PxArgs& a, hipStream_t s) {
    const size_t blocks = ((size_t)a.B * (a.D + 1) * a.H * a.r + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(px_slot_table_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_px_den(const PxArgs& a, hipStream_t s) {
    if (a.r < 1 || a.r > 32 || a.N > 65535 * 256) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.B, (unsigned)((a.N + 255) / 256));
    return dispatch_r_bucket(a.r, [&](auto RB) {
        hipLaunchKernelGGL((px_den_kernel<decltype(RB)::value>), grid, dim3(256), 0, s, a);
        return hipGetLastError();
    });
}

// Series blocks and rows per LDS chunk from irf_geometry (dfm_cellgeom.h), as sv_irf_fill_kernel: a staged row here is RB doubles
// (two with the cumulated table), which the geometry's r x r rows bound from above.
template <int RB>
static hipError_t launch_fill_rb(PxArgs a, hipStream_t s) {
    const int SP = cell_sp(a.N, RB, a.irf, a.fevd);
    const bool hasc = a.tkc != nullptr;
    a.geo = irf_geometry(a.N, RB, SP, a.H, hasc, kPxFillLanes, kPxFillLds);
    const size_t lds = (size_t)a.geo.RC * RB * (hasc ? 2 : 1) * sizeof(double);
    return cell_launch_sp<RB>(px_fill_kernel<RB, 1>, px_fill_kernel<RB, cell_sp_max(RB)>, SP,
                              (size_t)a.B * (a.D + 1) * a.geo.nsblk, a.geo.threads, lds, s, a);
}

hipError_t launch_px_fill(PxArgs a, hipStream_t s) {
    if (a.r < 1 || a.r > 32 || a.H < 1) return hipErrorInvalidValue;
    return dispatch_r_bucket(a.r, [&](auto RB) { return launch_fill_rb<decltype(RB)::value>(a, s); });
}

hipError_t launch_px_shock(const PxArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(px_shock_kernel, dim3((unsigned)a.B, (unsigned)((a.T + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace dfm
