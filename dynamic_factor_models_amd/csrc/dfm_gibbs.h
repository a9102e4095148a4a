// dfm_gibbs.h -- what the parameter blocks of the two Gibbs samplers share (gibbs.hip: dfm_gibbs_batch; gibbs_ar.hip:
// dfm_gibbs_ar_batch): the sweep's key, the status bit, the Gamma sampler and the stream words of include/dfm_hip.h.
#pragma once
#include "dfm_kernels.h"
#include "dfm_philox.h"

namespace dfm {

constexpr int kGbFailBit = 64;                // status word: a Cholesky failed or a rejection sampler ran into its cap
constexpr int kGbGammaCap = 32;               // attempts of one Gamma draw
enum : uint64_t { kGbLamN = 5, kGbRGam = 6, kGbVarE = 7, kGbBartN = 8, kGbBartG = 9, kGbArLamN = 10, kGbArRhoN = 11 };

__device__ __forceinline__ uint64_t gb_key(uint64_t seed, int64_t sweep) {
    return seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(sweep + 1));
}
__device__ __forceinline__ double gb_uniform1(uint64_t key, uint64_t stream, uint64_t idx) {
    uint32_t o[4];
    Philox::block(key, idx, stream, o);
    return u01(o[0], o[1]);
}
// Gamma(a, 1), a >= 1; item `item` of n_items on stream word `word`
__device__ __forceinline__ double gb_gamma(uint64_t key, uint64_t word, int item, int n_items, double a, bool& capped) {
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (int k = 0; k < kGbGammaCap; ++k) {
        const uint64_t m = (uint64_t)k * (uint64_t)n_items + (uint64_t)item;
        double z, z1;
        normal2(key, word, 2 * m, z, z1);
        const double u = gb_uniform1(key, word, 2 * m + 1);
        const double t = 1.0 + c * z, v = t * t * t;
        if (v > 0.0 && log(u) < 0.5 * z * z + d - d * v + d * log(v)) return d * v;
    }
    capped = true;
    return d;
}

}  // namespace dfm
