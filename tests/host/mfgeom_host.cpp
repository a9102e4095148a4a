// Host driver of csrc/dfm_mfgeom.h, the launch geometry of the series step of the mixed-frequency EM (mstep_mf.hip,
// mstep_mf_blocks.hip) and the dealing of the series into weight classes and tiles (capi.hip: mf_classes): reads requests and prints
// the numbers the launchers, the kernels and mf_plan take from the header, so that the Python restatement of tests/mf_geometry.py is
// checked against the text the library executes (tests/test_mf_geometry_cpu.py).  TEST INFRASTRUCTURE ONLY.
//   N L r T B Rk  w_00 .. w_0,L-1  ..  w_N-1,L-1      (the weight rows, series after series)
// ->  VW TT ngroups  gl gt gm gs  rc C ntiles  kind_0 .. kind_VW-1  vech(0,0) vech(1,0) .. vech(r-1,r-1)  mean_0 .. mean_r-1
//     tile_class_0 ..  tile_series_0 .. tile_series_16 ntiles-1  the C class rows as 1e6 w, rounded
// gl, gt, gm, gs = the workgroups (x) of mf_loadings_kernel, mf_table_kernel, mf_moments_kernel and mf_solve_kernel /
// mf_solve_blocks_kernel; ngroups = the groups of 16 periods mf_moments_kernel walks; rc = mf_deal's status (not 0: C = ntiles = 0
// and no lists).  A request it cannot read ends the run with exit status 1.
#include <cstdio>
#include <vector>

#include "../../dynamic_factor_models_amd/csrc/dfm_mfgeom.h"

int main() {
    int N, L, r, T, B, Rk;
    for (;;) {
        const int got = scanf("%d %d %d %d %d %d", &N, &L, &r, &T, &B, &Rk);
        if (got == EOF) return 0;
        if (got != 6 || N < 1 || L < 1 || r < 1 || r > 8 || T < 1 || B < 1 || Rk < 1) return 1;
        std::vector<double> W((size_t)N * L);
        for (double& w : W)
            if (scanf("%lf", &w) != 1) return 1;
        const int VW = dfm::mf_row_width(r);
        printf("%d %d %d %zu %d", VW, dfm::mf_row_tiles(VW), dfm::mf_groups(T), dfm::mf_loadings_blocks(B, N, Rk),
               dfm::mf_table_blocks(T, VW));
        dfm::MfDeal d;
        const int rc = dfm::mf_deal(N, L, W.data(), &d);
        if (rc != dfm::kMfDealOk) d = dfm::MfDeal();
        printf(" %d %d %d %d %d", dfm::mf_moment_blocks(d.ntiles), dfm::mf_solve_blocks(N), rc, d.C, d.ntiles);
        for (int col = 0; col < VW; ++col) printf(" %d", dfm::mf_col_kind(r, VW, col));
        for (int c = 0; c < r; ++c)
            for (int e = 0; e <= c; ++e) printf(" %d", dfm::mf_vech_col(c, e));
        for (int c = 0; c < r; ++c) printf(" %d", dfm::mf_mean_col(VW, c));
        for (int c : d.tile_class) printf(" %d", c);
        for (int i : d.tile_series) printf(" %d", i);
        if (rc == dfm::kMfDealOk)                                  // the class rows themselves, as 1e6 w rounded (the tests' weights are exact in it)
            for (double w : d.Wc) printf(" %lld", (long long)(w * 1e6 + (w < 0 ? -0.5 : 0.5)));
        printf("\n");
    }
}
