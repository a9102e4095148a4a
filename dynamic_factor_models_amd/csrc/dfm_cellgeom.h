// dfm_cellgeom.h -- launch geometry of the post-estimation cell kernels (forecast.hip, filter.hip, filter_ar.hip, simsmooth.hip,
// news.hip, structural.hip, proxy.hip) and of the series recursions of forecast_ar.hip (series_geometry; tests/host/seriesgeom_host.cpp,
// tests/test_forecast_ar_cpu.py), the rule for the 16-byte cell path (cell_vec, cell_sp) and the two dispatchers the launchers
// share.  Plain C++17 with no HIP include: the launchers call it, the kernels read the CellGeom it returns through their argument
// struct, and tests/host/cellgeom_host.cpp compiles it for the CPU, where tests/test_post_geometry_cpu.py, tests/test_filter_cpu.py
// and tests/test_structural_cpu.py hold the Python restatements of tests/post_geometry.py, tests/filter_expect.py and
// tests/structural_geometry.py against it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace dfm {

// One kernel's launch geometry: nsblk series blocks of NPB lanes, G row groups per workgroup (threads = G x NPB rounded up to whole
// waves), RC rows staged in LDS per chunk, nchunk chunks.
struct CellGeom {
    int NPB, G, RC, nchunk, nsblk, threads;
};

constexpr int kCellBlockLanes = 256;          // lanes of one series block, at most

inline bool al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// The 16-byte cell path: N even and every pointer the kernel moves cells through 16-byte aligned (a null pointer -- an output not
// asked for -- counts as aligned).  cell_vec: the VEC of the pair kernels.  cell_sp: the series per lane of the SP kernels, two on
// that path while the loadings' register bucket RB is at most 16.
template <class... P>
inline bool cell_vec(int N, const P*... ptrs) { return (N & 1) == 0 && (al16(ptrs) && ...); }
template <class... P>
inline int cell_sp(int N, int RB, const P*... ptrs) { return RB <= 16 && cell_vec(N, ptrs...) ? 2 : 1; }

// A cell kernel streams a [rows][N] output from loadings in registers and rows of row_doubles doubles staged in LDS.  `lanes` (one
// series or one pair of series each) are split into blocks of at most 256; the workgroup is G x NPB lanes rounded up to whole
// waves, G chosen so that the fewest lanes idle (100 lanes: 5 x 100 of 512; 139 lanes: 3 x 139 of 448); a workgroup takes 8 rows
// per row group, fewer under the LDS cap or when there are no more.  rows >= 1.
inline CellGeom cell_geometry(int lanes, int row_doubles, int rows, int max_threads, size_t lds_bytes) {
    CellGeom g;
    g.nsblk = (lanes + kCellBlockLanes - 1) / kCellBlockLanes;
    g.NPB = (lanes + g.nsblk - 1) / g.nsblk;
    g.G = 1;
    double best = -1.0;
    for (int G = 1; G * g.NPB <= max_threads; ++G) {
        const int th = (G * g.NPB + 63) / 64 * 64;
        if (th > max_threads) break;
        const double eff = (double)(G * g.NPB) / th;
        if (eff > best + 1e-9) { best = eff; g.G = G; }
    }
    g.threads = (g.G * g.NPB + 63) / 64 * 64;
    int rc = g.G * 8;
    const int cap = (int)(lds_bytes / ((size_t)row_doubles * sizeof(double)));
    if (rc > cap) rc = cap;
    if (rc > rows) rc = rows;
    if (rc < 1) rc = 1;
    g.RC = rc;
    g.nchunk = (rows + rc - 1) / rc;
    return g;
}

// The series recursions of forecast_ar.hip: ONE lane per series and one row group (every lane walks every row, in order), so a
// workgroup is a series block of at most 256 lanes in whole waves and owns all the rows of its replicate; it stages them in LDS
// kSeriesChunkRows at a time, fewer under the LDS cap or when there are no more.  rows >= 1.
constexpr int kSeriesChunkRows = 32;

inline CellGeom series_geometry(int N, int row_doubles, int rows, size_t lds_bytes) {
    CellGeom g;
    g.nsblk = (N + kCellBlockLanes - 1) / kCellBlockLanes;
    g.NPB = (N + g.nsblk - 1) / g.nsblk;
    g.G = 1;
    g.threads = (g.NPB + 63) / 64 * 64;
    int rc = kSeriesChunkRows;
    const int cap = (int)(lds_bytes / ((size_t)row_doubles * sizeof(double)));
    if (rc > cap) rc = cap;
    if (rc > rows) rc = rows;
    if (rc < 1) rc = 1;
    g.RC = rc;
    g.nchunk = (rows + rc - 1) / rc;
    return g;
}

// filter_ar_fill_kernel (filter_ar.hip), a cell kernel of the model with AR(q) idiosyncratic terms: the observation loads on the
// first w = r (q + 1) entries of the state, so a staged row is the first w of z_pred and the packed leading w x w block of P_pred;
// the loadings' register bucket is dispatch_r_bucket's of w, and SP follows cell_sp at it.  tests/host/filter_ar_geom_host.cpp.
constexpr int kFtArFillMaxThreads = 512;
constexpr size_t kFtArFillLds = 48 * 1024;

inline int filter_ar_row_doubles(int w) { return w + w * (w + 1) / 2; }
inline CellGeom filter_ar_fill_geometry(int N, int SP, int w, int rows) {
    return cell_geometry((N + SP - 1) / SP, filter_ar_row_doubles(w), rows, kFtArFillMaxThreads, kFtArFillLds);
}

// sv_irf_fill_kernel: series blocks of at most max_lanes lanes of SP series and the rows of the Theta tables (one, or two with the
// cumulated table) per LDS chunk; 32 doubles of the LDS hold the unit-effect scales.
inline CellGeom irf_geometry(int N, int R, int SP, int H, bool hasc, int max_lanes, size_t lds_bytes) {
    CellGeom g;
    const int lanes = (N + SP - 1) / SP;
    g.nsblk = (lanes + max_lanes - 1) / max_lanes;
    g.NPB = (lanes + g.nsblk - 1) / g.nsblk;
    g.threads = (g.NPB + 63) / 64 * 64;
    const size_t row_bytes = (size_t)R * R * (hasc ? 2 : 1) * sizeof(double);
    int rc = (int)((lds_bytes - 32 * sizeof(double)) / row_bytes);
    if (rc > H) rc = H;
    g.RC = rc;
    g.nchunk = (H + rc - 1) / rc;
    g.G = 1;
    return g;
}

// sv_path_kernel: chains per workgroup (CP, each r p lanes wide), workgroups per replicate (groups) and rows staged between two
// write-outs (TC, under the LDS cap).
struct PathGeom {
    int CP, TC, groups, threads;
    size_t lds;
};

inline PathGeom path_geometry(int r, int p, int max_threads, size_t lds_bytes) {
    PathGeom g;
    const int k = r * p;
    int cp = max_threads / k;
    if (cp > r + 1) cp = r + 1;
    g.CP = cp;
    g.groups = (r + 1 + cp - 1) / cp;
    const int words = (int)(lds_bytes / sizeof(double)) - 2 * cp * k;
    int tc = words / (cp * r + r);
    g.TC = tc > 32 ? 32 : (tc < 1 ? 1 : tc);
    g.threads = (cp * k + 63) / 64 * 64;
    g.lds = ((size_t)2 * cp * k + (size_t)g.TC * (cp * r + r)) * sizeof(double);
    return g;
}

// f(std::integral_constant<int, R>{}) for the R in 1..32 equal to r (a kernel instance per r), `none` when there is none.
template <class T, class F, int... Rs>
inline T dispatch_r_exact(int r, T none, F&& f, std::integer_sequence<int, Rs...>) {
    T e = none;
    (void)((r == Rs + 1 ? (e = f(std::integral_constant<int, Rs + 1>{}), true) : false) || ...);
    return e;
}
template <class T, class F>
inline T dispatch_r_exact(int r, T none, F&& f) {
    return dispatch_r_exact(r, none, f, std::make_integer_sequence<int, 32>{});
}

// f(std::integral_constant<int, RB>{}) for the register bucket RB = 4 | 8 | 16 | 32 that holds r <= 32 loadings.
template <class F>
inline auto dispatch_r_bucket(int r, F&& f) {
    if (r <= 4) return f(std::integral_constant<int, 4>{});
    if (r <= 8) return f(std::integral_constant<int, 8>{});
    if (r <= 16) return f(std::integral_constant<int, 16>{});
    return f(std::integral_constant<int, 32>{});
}

}  // namespace dfm
