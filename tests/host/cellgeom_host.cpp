// Host driver of csrc/dfm_cellgeom.h, the launch geometry the post-estimation launchers call: reads one request per line and prints
// the fields of the result, so that the Python restatement of tests/post_geometry.py and tests/structural_geometry.py is checked
// against the text the library executes (tests/test_post_geometry_cpu.py, tests/test_structural_cpu.py).  TEST INFRASTRUCTURE ONLY.
//   cell lanes row_doubles rows max_threads lds_bytes      ->  NPB G RC nchunk nsblk threads
//   irf  N R SP H hasc max_lanes lds_bytes                 ->  NPB G RC nchunk nsblk threads
//   path r p max_threads lds_bytes                         ->  CP TC groups threads lds
//   sp   N RB aligned                                      ->  SP   (cell_sp with one pointer, 16 or 8 bytes off a 16-byte line, and
//                                                               a null one beside it, which counts as aligned)
// A line it cannot read ends the run with exit status 1.
#include <cstdio>
#include <cstring>

#include "../../dynamic_factor_models_amd/csrc/dfm_cellgeom.h"

static void print(const dfm::CellGeom& g) { printf("%d %d %d %d %d %d\n", g.NPB, g.G, g.RC, g.nchunk, g.nsblk, g.threads); }

int main() {
    char line[256], kind[8];
    long long v[7];
    while (fgets(line, sizeof line, stdin)) {
        kind[0] = 0;
        const int n = sscanf(line, "%7s %lld %lld %lld %lld %lld %lld %lld", kind, v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6) - 1;
        if (!strcmp(kind, "cell") && n == 5) {
            print(dfm::cell_geometry((int)v[0], (int)v[1], (int)v[2], (int)v[3], (size_t)v[4]));
        } else if (!strcmp(kind, "irf") && n == 7) {
            print(dfm::irf_geometry((int)v[0], (int)v[1], (int)v[2], (int)v[3], v[4] != 0, (int)v[5], (size_t)v[6]));
        } else if (!strcmp(kind, "path") && n == 4) {
            const dfm::PathGeom g = dfm::path_geometry((int)v[0], (int)v[1], (int)v[2], (size_t)v[3]);
            printf("%d %d %d %d %zu\n", g.CP, g.TC, g.groups, g.threads, g.lds);
        } else if (!strcmp(kind, "sp") && n == 3) {
            alignas(16) static double cells[4];
            const double* none = nullptr;
            printf("%d\n", dfm::cell_sp((int)v[0], (int)v[1], v[2] != 0 ? cells + 2 : cells + 1, none));
        } else {
            return 1;
        }
    }
    return 0;
}
