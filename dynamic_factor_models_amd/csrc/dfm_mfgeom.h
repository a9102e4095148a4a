// dfm_mfgeom.h -- launch geometry of the series step of the mixed-frequency EM (mstep_mf.hip: mf_loadings_kernel, mf_table_kernel,
// mf_moments_kernel<TT>, mf_solve_kernel<R>; mstep_mf_blocks.hip: mf_solve_blocks_kernel<R>) and the host-side dealing of the series
// into weight classes and class-pure tiles (capi.hip: mf_classes).  Plain C++17 with no HIP include (constexpr functions: the device
// code reads them too): the kernels, their launchers and mf_plan read it, and tests/host/mfgeom_host.cpp compiles it for the CPU,
// where tests/test_mf_geometry_cpu.py holds the Python restatement of tests/mf_geometry.py against it.
#pragma once
#include <stddef.h>

#include <cmath>
#include <vector>

namespace dfm {

constexpr int kMfMaxClasses = 8, kMfMaxLags = 5;
constexpr int kMfTile = 16;                                    // series per tile (one wave), columns per table tile
constexpr int kMfWaves = 4;                                    // tiles (waves) per workgroup of mf_moments_kernel
constexpr int kMfGroup = 16;                                   // periods per group of mf_moments_kernel: 4 matrix steps of 4 periods
constexpr int kMfBlock = 256;                                  // threads per workgroup of every kernel of the step

// ---- a class row of the table V, a series row of OUT: [vech(E g g') (packed lower), zeros to VW - 16 | E g (r columns), zeros] ----
constexpr int mf_vech_cols(int r) { return r * (r + 1) / 2; }
constexpr int mf_row_width(int r) { return 16 * ((mf_vech_cols(r) + 15) / 16) + 16; }
constexpr int mf_row_tiles(int VW) { return VW / 16; }         // TT: TT - 1 tiles of vech against the mask, the last (E g) against the panel
constexpr int mf_vech_col(int c, int d) { return c * (c + 1) / 2 + d; }     // c >= d
constexpr int mf_mean_col0(int VW) { return VW - 16; }
constexpr int mf_mean_col(int VW, int c) { return mf_mean_col0(VW) + c; }
// what column col holds: 1 an entry of vech, 2 an entry of the mean, 0 a zero
constexpr int mf_col_kind(int r, int VW, int col) {
    return col < mf_vech_cols(r) ? 1 : ((col >= mf_mean_col0(VW) && col < mf_mean_col0(VW) + r) ? 2 : 0);
}

// ---- workgroups (x; y = the replicate, but for mf_loadings_kernel, whose threads run over the whole batch) ------------------------
constexpr size_t mf_loadings_blocks(int B, int N, int Rk) { return ((size_t)B * N * Rk + kMfBlock - 1) / kMfBlock; }
constexpr int mf_table_blocks(int T, int VW) { return (T * VW + kMfBlock - 1) / kMfBlock; }
constexpr int mf_moment_blocks(int ntiles) { return (ntiles + kMfWaves - 1) / kMfWaves; }
constexpr int mf_solve_blocks(int N) { return (N + kMfBlock - 1) / kMfBlock; }
constexpr int mf_groups(int T) { return (T + kMfGroup - 1) / kMfGroup; }   // of 16 periods; the last may hold 1 .. 16 live ones

// ---- the classes and the tiles ----------------------------------------------------------------------------------------------------
// The distinct rows of W [N][L] (exact comparison) in the order of their first series, and the series dealt by index, class after
// class, into tiles of 16 of ONE class each; the last tile of a class is padded with -1.
struct MfDeal {
    int C = 0, ntiles = 0;
    std::vector<double> Wc;            // [C][L]
    std::vector<int> tile_class;       // [ntiles]
    std::vector<int> tile_series;      // [ntiles][16], -1 = padding
};
constexpr int kMfDealOk = 0, kMfDealNotFinite = 1, kMfDealTooManyClasses = 2;
inline int mf_deal(int N, int L, const double* W, MfDeal* mc) {
    std::vector<int> cls(N);
    for (int i = 0; i < N; ++i) {
        for (int l = 0; l < L; ++l)
            if (!std::isfinite(W[(size_t)i * L + l])) return kMfDealNotFinite;
        int c = 0;
        for (; c < mc->C; ++c) {
            bool same = true;
            for (int l = 0; l < L; ++l) same = same && mc->Wc[(size_t)c * L + l] == W[(size_t)i * L + l];
            if (same) break;
        }
        if (c == mc->C) {
            if (mc->C == kMfMaxClasses) return kMfDealTooManyClasses;
            mc->Wc.insert(mc->Wc.end(), W + (size_t)i * L, W + (size_t)(i + 1) * L);
            ++mc->C;
        }
        cls[i] = c;
    }
    for (int c = 0; c < mc->C; ++c) {
        int fill = 0;
        for (int i = 0; i < N; ++i) {
            if (cls[i] != c) continue;
            if (fill == 0) mc->tile_class.push_back(c);
            mc->tile_series.push_back(i);
            fill = (fill + 1) & (kMfTile - 1);
        }
        while (fill) { mc->tile_series.push_back(-1); fill = (fill + 1) & (kMfTile - 1); }
    }
    mc->ntiles = (int)mc->tile_class.size();
    return kMfDealOk;
}

}  // namespace dfm
