// dfm_filter.h -- what the two forward recursions in covariance form share (filter.hip: filter_kernel; filter_ar.hip:
// filter_ar_kernel): the constants of the family and the positive semi-definite root of one wave's workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace dfm {

constexpr int kFtFillMaxThreads = 512;
constexpr size_t kFtFillLds = 48 * 1024;
constexpr int kFtEvalChunk = 64;                  // origins whose states a workgroup of the evaluation advances together
constexpr int kFtFailBit = 32;

// Lower root L L' = M (leading n x n block of a matrix with rows ld apart, lower triangle read) of one wave's workgroup, as
// psd_root: a pivot <= tol_rel trace(M) gives a zero column.  Returns 1 when a pivot is below -tol_rel trace(M) or not finite
// (M is not positive semi-definite), else 0.  L: [n][n].
__device__ inline int filter_root(const double* M, int ld, int n, double* L, double tol_rel) {
    const int tid = threadIdx.x;
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += M[i * ld + i];
    const double tol = tol_rel * tr;
    for (int e = tid; e < n * n; e += blockDim.x) L[e] = 0.0;
    __syncthreads();
    int bad = (tr == tr && fabs(tr) <= 1.79e308) ? 0 : 1;
    for (int j = 0; j < n; ++j) {
        double dj = M[j * ld + j];
        for (int m = 0; m < j; ++m) dj -= L[j * n + m] * L[j * n + m];
        const bool keep = dj > tol;
        if (!(dj >= -tol)) bad = 1;
        const double ljj = keep ? sqrt(dj) : 0.0;
        for (int i = j + tid; i < n; i += blockDim.x) {
            if (i == j) {
                L[j * n + j] = ljj;
            } else {
                double v = M[i * ld + j];
                for (int m = 0; m < j; ++m) v -= L[i * n + m] * L[j * n + m];
                L[i * n + j] = keep ? v / ljj : 0.0;
            }
        }
        __syncthreads();
    }
    return bad;
}

}  // namespace dfm
