// Host driver of what launch_filter_ar_fill (csrc/filter_ar.hip) takes from csrc/dfm_cellgeom.h: the loadings' register bucket of the
// observation width w, SP at that bucket, the doubles of a staged row and the geometry they give, so that the restatement of
// tests/filter_ar_expect.py is checked against the text the library executes (tests/test_filter_ar_cpu.py).  TEST INFRASTRUCTURE ONLY.
//   N w rows aligned      ->  SP WB row_doubles NPB G RC nchunk nsblk threads
// A line it cannot read ends the run with exit status 1.
#include <cstdio>

#include "../../dynamic_factor_models_amd/csrc/dfm_cellgeom.h"

int main() {
    char line[256];
    int N, w, rows, aligned;
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%d %d %d %d", &N, &w, &rows, &aligned) != 4) return 1;
        alignas(16) static double cells[4];
        const double* none = nullptr;
        const int WB = dfm::dispatch_r_bucket(w, [](auto c) -> int { return decltype(c)::value; });
        const int SP = dfm::cell_sp(N, WB, aligned ? cells + 2 : cells + 1, none);
        const dfm::CellGeom g = dfm::filter_ar_fill_geometry(N, SP, w, rows);
        printf("%d %d %d %d %d %d %d %d %d\n", SP, WB, dfm::filter_ar_row_doubles(w), g.NPB, g.G, g.RC, g.nchunk, g.nsblk, g.threads);
    }
    return 0;
}
