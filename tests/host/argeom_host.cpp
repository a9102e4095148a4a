// Host driver of csrc/dfm_argeom.h, the launch geometry of the AR-idiosyncratic series step (mstep_ar.hip): reads one request per
// line and prints the numbers the launcher and the kernels take from the header, so that the Python restatement of
// tests/ar_geometry.py is checked against the text the library executes (tests/test_ar_geometry_cpu.py).  TEST INFRASTRUCTURE ONLY.
//   r q N T Rk   ->   K1 NTM NZF TT TPW SGW NT0 NT1 NT2 NT3   VW ntm16 Ns   gv gm gs
// NT0..3 = the tiles of the four waves; gv, gm, gs = the workgroups per replicate of mmw_vec_kernel (16 periods each: launch_mmw_vec
// of mstep_miss.hip, called with T - q periods), ar_moments_kernel and ar_solve_kernel.  The template instance is chosen as
// launch_mstep_ar chooses it: a switch over the 38 supported (r, q).  A line it cannot read, or an unsupported (r, q), ends the run
// with exit status 1.
#include <cstdio>

#include "../../dynamic_factor_models_amd/csrc/dfm_argeom.h"

template <int R, int Q1>
static int print(int N, int T, int Rk) {
    using G = dfm::ArGeo<R, Q1>;
    const dfm::ArWs w = dfm::ar_ws_geometry(1, T, N, R, Q1 - 1, Rk);
    if (w.TT != G::TT || w.ntm16 != 16 * G::NTM) return 1;         // the two statements of the tile counts agree
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", G::K1, G::NTM, G::NZF, G::TT, G::TPW, G::SGW,
           dfm::ar_wave_tiles(G::TT, G::TPW, 0), dfm::ar_wave_tiles(G::TT, G::TPW, 1), dfm::ar_wave_tiles(G::TT, G::TPW, 2),
           dfm::ar_wave_tiles(G::TT, G::TPW, 3), w.VW, w.ntm16, w.Ns, (T - (Q1 - 1) + 15) / 16, dfm::ar_moment_blocks<R, Q1>(N),
           dfm::ar_solve_blocks(N));
    return 0;
}

static int one(int r, int q, int N, int T, int Rk) {
    switch (8 * q + r - 1) {
#define RQ(R, Q) case 8 * Q + R - 1: return print<R, Q + 1>(N, T, Rk);
        RQ(1, 0) RQ(2, 0) RQ(3, 0) RQ(4, 0) RQ(5, 0) RQ(6, 0) RQ(7, 0) RQ(8, 0)
        RQ(1, 1) RQ(2, 1) RQ(3, 1) RQ(4, 1) RQ(5, 1) RQ(6, 1) RQ(7, 1) RQ(8, 1)
        RQ(1, 2) RQ(2, 2) RQ(3, 2) RQ(4, 2) RQ(5, 2) RQ(6, 2) RQ(7, 2) RQ(8, 2)
        RQ(1, 3) RQ(2, 3) RQ(3, 3) RQ(4, 3) RQ(5, 3) RQ(6, 3) RQ(7, 3) RQ(8, 3)
        RQ(1, 4) RQ(2, 4) RQ(3, 4) RQ(4, 4) RQ(5, 4) RQ(6, 4)
#undef RQ
        default: return 1;
    }
}

int main() {
    char line[256];
    int r, q, N, T, Rk;
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%d %d %d %d %d", &r, &q, &N, &T, &Rk) != 5) return 1;
        if (r < 1 || r > 8 || q < 0 || q > 4 || N < 1 || T <= q || Rk < 1) return 1;
        if (one(r, q, N, T, Rk)) return 1;
    }
    return 0;
}
