// dfm_argeom.h -- launch geometry of the series step of the AR-idiosyncratic ECM (mstep_ar.hip: mmw_vec_kernel, ar_moments_kernel<R, Q1>,
// ar_solve_kernel<R, Q1>).  Plain C++17 with no HIP include: the kernels and their launcher read it, and tests/host/argeom_host.cpp
// compiles it for the CPU, where tests/test_ar_geometry_cpu.py holds the Python restatement of tests/ar_geometry.py against it.
#pragma once
#include <stddef.h>

namespace dfm {

// R = the model's number of factors (exact), Q1 = q + 1.  The moments of a series are 16-column tiles of OUT: NTM tiles of
// W = sum E[z z'] (the packed leading K1 x K1 block) and, per lag l' of the panel, NZF tiles of ZX[l'] = sum x z; TT tiles in all,
// TPW to a wave (four waves), and SGW groups of 16 series per workgroup, fewer where a wave holds more accumulator tiles.
template <int R, int Q1>
struct ArGeo {
    static constexpr int K1 = R * Q1, NPR = K1 * (K1 + 1) / 2, NTM = (NPR + 15) / 16, NZF = (K1 + 15) / 16;
    static constexpr int TT = NTM + Q1 * NZF, TPW = (TT + 3) / 4;
    static constexpr int SGW = TPW <= 6 ? 3 : (TPW <= 9 ? 2 : 1);
    static constexpr int NXX = Q1 * (Q1 + 1) / 2;
};
constexpr int kArTC = 128;                                     // periods per staged chunk of the panel block
constexpr int kArPF = 3;                                       // B operands in flight: steps ahead
constexpr int kArSolveSeries = 64;                             // series per workgroup of ar_solve_kernel (four lanes each)

// tiles of wave W: tiles W TPW .. W TPW + TPW - 1 of the TT, as far as there are any
constexpr int ar_wave_tiles(int TT, int TPW, int W) {
    return (TT - W * TPW) < TPW ? ((TT - W * TPW) > 0 ? (TT - W * TPW) : 0) : TPW;
}

// The workspace of the moment form, V | OUT | SM (doubles): a row of V is 16 ntm columns of vec(E z z') and the Rk states rounded up
// to 16; OUT and SM are stored series-fastest with Ns = N rounded up to 16.
struct ArWs {
    int VW, ntm16, Ns, TT;
    size_t nV, nOUT, nSM;
};
inline ArWs ar_ws_geometry(int B, int T, int N, int r, int q, int Rk) {
    const int k1 = r * (q + 1), npr = k1 * (k1 + 1) / 2, ntm = (npr + 15) / 16, nzf = (k1 + 15) / 16;
    ArWs w;
    w.VW = 16 * ntm + 16 * ((Rk + 15) / 16);
    w.ntm16 = 16 * ntm;
    w.Ns = (N + 15) & ~15;
    w.TT = ntm + (q + 1) * nzf;
    w.nV = (size_t)B * (T - q) * w.VW;
    w.nOUT = (size_t)B * 16 * w.TT * w.Ns;
    w.nSM = (size_t)B * 16 * w.Ns;
    return w;
}

// workgroups per replicate: ar_moments_kernel<R, Q1> takes 16 SGW series, ar_solve_kernel kArSolveSeries
template <int R, int Q1>
constexpr int ar_moment_blocks(int N) { return (N + 16 * ArGeo<R, Q1>::SGW - 1) / (16 * ArGeo<R, Q1>::SGW); }
constexpr int ar_solve_blocks(int N) { return (N + kArSolveSeries - 1) / kArSolveSeries; }

}  // namespace dfm
