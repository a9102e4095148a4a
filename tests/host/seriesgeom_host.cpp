// Host driver of series_geometry (csrc/dfm_cellgeom.h), the launch geometry of the series recursions of csrc/forecast_ar.hip: reads
// one request per line and prints the fields of the result, so that the Python restatement of tests/forecast_ar_expect.py is
// checked against the text the library executes (tests/test_forecast_ar_cpu.py).  TEST INFRASTRUCTURE ONLY.
//   N row_doubles rows lds_bytes      ->  NPB G RC nchunk nsblk threads
// A line it cannot read ends the run with exit status 1.
#include <cstdio>

#include "../../dynamic_factor_models_amd/csrc/dfm_cellgeom.h"

int main() {
    char line[256];
    long long v[4];
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%lld %lld %lld %lld", v, v + 1, v + 2, v + 3) != 4) return 1;
        const dfm::CellGeom g = dfm::series_geometry((int)v[0], (int)v[1], (int)v[2], (size_t)v[3]);
        printf("%d %d %d %d %d %d\n", g.NPB, g.G, g.RC, g.nchunk, g.nsblk, g.threads);
    }
    return 0;
}
