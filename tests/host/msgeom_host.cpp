// Host driver of csrc/dfm_msgeom.h, the launch geometry of the balanced loadings step (mstep_mfma.hip, mstep_wide.hip, make_plan of
// capi.hip): reads one request per line and prints the numbers the launchers, the kernels and make_plan take from the header, so that
// the Python restatement of tests/mstep_geometry.py is checked against the text the library executes
// (tests/test_mstep_geometry_cpu.py).  TEST INFRASTRUCTURE ONLY.
//   M B N T Rp          ->   ok CS STEPS NDR lo hi slot wpr tq nfront gstream n0 .. n7
//   W B N T r Rp ncu    ->   ok R NX rd nsb last_series nst last_rows xcd_map grid gy nbuf
// M: ok = mstep_mfma_supported; the instance is chosen as launch_ms_pick chooses it (STEPS from N, the NDR of N, lo .. hi = the NDR
// the instance <Rp, STEPS, .> exists for); slot = ms_slot_bytes; n0 .. n7 = the rows of segment 0 .. 7 (-1 past wpr).
// W: ok = mstep_wide_supported; R, NX = the instance of mstep_wide_kernel, rd = the width of the caller's arrays (and the instance of
// mstep_finish_wide_kernel), gy = its blocks of 256 series.  An unsupported shape prints ok = 0 alone.  A line it cannot read ends
// the run with exit status 1.
#include <cstdio>

#include "../../dynamic_factor_models_amd/csrc/dfm_msgeom.h"

template <int R>
static int mfma(int B, int N, int T) {
    constexpr int CS = dfm::MsGeo<R>::CS;
    const int steps = dfm::ms_steps(N, CS), ndr = dfm::ms_ndr(N), wpr = dfm::ms_wpr(B, T);
    printf("1 %d %d %d %d %d %u %d %d %d %d", CS, steps, ndr, dfm::ms_ndr_lo(CS, steps), dfm::ms_ndr_hi(CS, steps), dfm::ms_slot_bytes(N),
           wpr, dfm::ms_segment(N, T, wpr, 0).tq, dfm::ms_front_blocks(B), dfm::ms_stream_blocks(B, wpr));
    for (int s = 0; s < 8; ++s) printf(" %d", s < wpr ? dfm::ms_segment(N, T, wpr, s).nrows : -1);
    printf("\n");
    return steps <= dfm::kMsMaxSteps ? 0 : 1;
}

static int wide(int B, int N, int T, int r, int Rp, int ncu) {
    const int R = Rp <= 16 ? 16 : 32, nx = Rp <= 16 ? 0 : dfm::mw_nx(r), nsb = dfm::mw_nsb(N), nst = dfm::mw_stages(T);
    printf("1 %d %d %d %d %d %d %d %d %d %d %d\n", R, nx, Rp, nsb, N - (nsb - 1) * dfm::kMwSer, nst, T - (nst - 1) * dfm::kMwPer,
           dfm::mw_xcd_map(B), dfm::mw_grid(B, nsb, ncu), (N + 255) / 256, dfm::kMwNBuf);
    return 0;
}

int main() {
    char line[256];
    int B, N, T, r, Rp, ncu;
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == 'M') {
            if (sscanf(line + 1, "%d %d %d %d", &B, &N, &T, &Rp) != 4 || B < 1 || N < 1 || T < 1) return 1;
            if (!dfm::ms_supported(Rp, N)) { printf("0\n"); continue; }
            if (Rp == 4 ? mfma<4>(B, N, T) : mfma<8>(B, N, T)) return 1;
        } else if (line[0] == 'W') {
            if (sscanf(line + 1, "%d %d %d %d %d %d", &B, &N, &T, &r, &Rp, &ncu) != 6 || B < 1 || N < 1 || T < 1 || r < 1 || r > Rp) return 1;
            if (!dfm::mw_supported(Rp, N)) { printf("0\n"); continue; }
            if (wide(B, N, T, r, Rp, ncu)) return 1;
        } else {
            return 1;
        }
    }
    return 0;
}
