// dfm_msgeom.h -- launch geometry of the loadings half of the M-step on a balanced panel: mstep_mfma.hip (mstep_mfma_kernel<R, STEPS,
// NDR>, mstep_finish_kernel<R>), the segments make_plan (capi.hip) deals to its waves, and mstep_wide.hip (mstep_wide_kernel<R, NX>,
// mstep_finish_wide_kernel<R>).  Plain C++17 with no HIP include (constexpr functions: the device code reads them too): the
// kernels, their launchers and make_plan read it, and tests/host/msgeom_host.cpp compiles it for the CPU, where
// tests/test_mstep_geometry_cpu.py holds the Python restatement of tests/mstep_geometry.py against it.
#pragma once
#include <stddef.h>

namespace dfm {

// ---- mstep_mfma.hip: R = the padded state width (4 | 8) --------------------------------------------------------------------------
template <int R>
struct MsGeo {
    static constexpr int NFG = (R + 3) / 4;                 // factor groups of 4
    static constexpr int FPI = NFG < 4 ? NFG : 4;
    static constexpr int NCG = 4 / FPI;                     // series groups per instruction
    static constexpr int CS = 4 * NCG;                      // series per step
};
constexpr unsigned ms_slot_bytes(int N) {                   // as collapse_mfma.hip: 4 consecutive slots 64 B apart mod 256
    unsigned sb = (unsigned)N * 8u;
    while ((sb & 255u) != 64u && (sb & 255u) != 192u) sb += 16u;
    return sb;
}
constexpr int kMsMaxSteps = 32;
// the instance <R, STEPS, NDR> of a cross-section: STEPS steps of CS series, NDR 1-KB pieces of a panel row; the NDR an instance
// <R, S, .> can meet lie in ms_ndr_lo .. ms_ndr_hi (N = CS (S - 1) + 1 .. CS S)
constexpr int ms_steps(int N, int CS) { return (N + CS - 1) / CS; }
constexpr int ms_ndr(int N) { return (N * 8 + 1023) / 1024; }
constexpr int ms_ndr_lo(int CS, int S) { return (CS * (S - 1) * 8 + 8 + 1023) / 1024; }
constexpr int ms_ndr_hi(int CS, int S) { return (CS * S * 8 + 1023) / 1024; }
// balanced panels, Rp in {4, 8} (the shapes of the fused E-step), even N, ceil(N / CS) <= 32, 8N <= 4096
constexpr bool ms_supported(int Rpad, int N) {
    if ((N & 1) != 0 || N * 8 > 4096 || N < 4) return false;
    if (Rpad == 4) return ms_steps(N, MsGeo<4>::CS) <= kMsMaxSteps;
    if (Rpad == 8) return ms_steps(N, MsGeo<8>::CS) <= kMsMaxSteps;
    return false;
}
// waves (period segments) per replicate (make_plan): 3072 / B, 1 .. 8, lowered while a segment would hold fewer than 8 periods
constexpr int ms_wpr(int B, int T) {
    int w = (256 * 12) / B;
    w = w < 1 ? 1 : (w > 8 ? 8 : w);
    while (w > 1 && T / w < 8) --w;
    return w;
}
// segment segi of wpr: periods ta .. tb - 1; the segment length tq is rounded up so that every segment starts on a 128-byte line
struct MsSeg {
    int tq, ta, tb, nrows;
};
constexpr MsSeg ms_segment(int N, int T, int wpr, int segi) {
    int tq = (T + wpr - 1) / wpr;
    {
        unsigned gg = ((unsigned)N * 8u) & 127u;
        gg = gg == 0 ? 128u : (gg & (~gg + 1u));
        const int m = (int)(128u / gg);
        tq = ((tq + m - 1) / m) * m;
    }
    const int ta = (segi * tq < T) ? segi * tq : T;
    const int tb = (ta + tq < T) ? ta + tq : T;
    return MsSeg{tq, ta, tb, tb - ta};
}
// workgroups of the streaming launch: nfront of four transition-step waves (one replicate each), then four segments each
constexpr int ms_front_blocks(int B) { return (B + 3) / 4; }
constexpr int ms_stream_blocks(int B, int wpr) { return (B * wpr + 3) / 4; }

// ---- mstep_wide.hip ---------------------------------------------------------------------------------------------------------------
constexpr int kMwSer = 128;                              // series per item: 8 consumer waves x 16
constexpr int kMwPer = 32;                               // periods per stage
constexpr int kMwNBuf = 3;
// r = the caller's factor count: column groups of 4 past the first 16 (Rp = 32: mstep_wide_kernel<32, NX>)
constexpr int mw_nx(int r) { return r <= 16 ? 1 : (r + 3 - 16) / 4; }
constexpr int mw_nsb(int N) { return (N + kMwSer - 1) / kMwSer; }           // series blocks (items) per replicate
constexpr int mw_stages(int T) { return (T + kMwPer - 1) / kMwPer; }        // stages per item
constexpr int mw_xcd_map(int B) { return B >= 16; }                         // a queue per XCD, replicate b on XCD b % 8
// Rp = 16 | 32 with an even N; narrower states (computed 16 wide) where mstep_mfma's 4-KB row ring ends
constexpr bool mw_supported(int Rpad, int N) {
    if ((N & 1) != 0 || N < 2) return false;
    return Rpad == 32 || Rpad == 16 || (Rpad >= 2 && Rpad <= 8 && N * 8 > 4096);
}
// persistent workgroups: one per CU, a multiple of 8; no more than there are items unless the queues are per XCD
constexpr int mw_grid(int B, int nsb, int num_cu) {
    const long long NI = (long long)B * nsb;
    int G = num_cu > 0 ? num_cu : 256;
    G = (G / 8) * 8;
    if (G < 8) G = 8;
    if (!mw_xcd_map(B) && NI < G) G = (int)NI;
    return G;
}

}  // namespace dfm
