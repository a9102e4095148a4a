// Host driver of the arithmetic of csrc/dfm_cell.h that needs no device: the loadings holder (its zero-padded load, its dot product
// and the pair kernels' dots) and the packed quadratic form, compiled for the CPU in the register bucket the launchers would pick
// for r, so that tests/test_cell_cpu.py holds them against NumPy.  TEST INFRASTRUCTURE ONLY.  One request per line, numbers as hex
// floats:
//   dot  r  lam[r]  f[r]                        ->  lam' f
//   quad r  lam[r]  P[r (r + 1) / 2]            ->  lam' P lam, P symmetric, packed row-wise lower
//   dots r  present  lam[2][r]  sd[2]  f[r]     ->  sd_0 lam_0' f  and  sd_1 lam_1' f of the pair holder loaded with `present`
//                                                   (1 | 2) series: an absent second series gives exactly 0
// A line it cannot read ends the run with exit status 1; a loaded register beyond r, or of an absent series, that is not zero
// gives NaN.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../dynamic_factor_models_amd/csrc/dfm_cell.h"

template <int RB>
static double run(bool quad, int r, const double* lam, const double* v) {
    dfm::CellLam<1, RB> h;
    h.load(lam, 0, 1, 0, r);                      // Lam [1][1][r]: replicate 0 of a one-series panel
    for (int m = r; m < RB; ++m)
        if (h.l[0][m] != 0.0) return __builtin_nan("");
    if (!quad) return h.dot(0, v, r);
    double qf = 0.0;
    DFM_CELL_QUAD(qf, h.l[0], v, RB, r)
    return qf;
}

template <int RB>
static void run_pair(int r, int present, const double* lam, const double* sd, const double* f, double (&y)[2]) {
    dfm::CellLam<2, RB> h;
    h.load(lam, 0, 2, 0, r, present, sd);         // Lam [1][2][r], sd [1][2]
    h.dots(f, r, y);
    for (int q = 0; q < 2; ++q)
        for (int m = 0; m < RB; ++m)
            if ((m >= r || q >= present) && h.l[q][m] != 0.0) y[q] = __builtin_nan("");
}

static bool read(std::vector<double>& v) {
    for (double& x : v)
        if (scanf("%la", &x) != 1) return false;
    return true;
}

int main() {
    char kind[8];
    int r;
    while (scanf("%7s %d", kind, &r) == 2) {
        if (r < 1 || r > 32) return 1;
        if (!strcmp(kind, "dots")) {
            int present;
            std::vector<double> lam(2 * r), sd(2), f(r);
            if (scanf("%d", &present) != 1 || present < 1 || present > 2 || !read(lam) || !read(sd) || !read(f)) return 1;
            double y[2];
            dfm::dispatch_r_bucket(r, [&](auto RB) { run_pair<decltype(RB)::value>(r, present, lam.data(), sd.data(), f.data(), y); return 0; });
            printf("%a %a\n", y[0], y[1]);
            continue;
        }
        const bool quad = !strcmp(kind, "quad");
        if (!quad && strcmp(kind, "dot")) return 1;
        std::vector<double> lam(r), v(quad ? r * (r + 1) / 2 : r);
        if (!read(lam) || !read(v)) return 1;
        printf("%a\n", dfm::dispatch_r_bucket(r, [&](auto RB) { return run<decltype(RB)::value>(quad, r, lam.data(), v.data()); }));
    }
    return 0;
}
