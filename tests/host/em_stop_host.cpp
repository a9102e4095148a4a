// Host driver of em_improved (csrc/dfm_em_epilogue.h), the comparison of the EM stop rule every kernel calls: reads (ll, llp, tol)
// triples and answers one byte each -- 1 = go on, 0 = stop -- so that the text the GPU executes is checked against the expression of
// oracle/kalman_oracle.py em() on the CPU (tests/test_em_stop_rule_cpu.py).  TEST INFRASTRUCTURE ONLY.
// stdin (binary): double [n][3]; stdout (binary): unsigned char [n]
#include <cstdio>
#include "../../dynamic_factor_models_amd/csrc/dfm_em_epilogue.h"

int main() {
    double v[3];
    while (fread(v, sizeof(double), 3, stdin) == 3) {
        const unsigned char go = dfm::em_improved(v[0], v[1], v[2]) ? 1 : 0;
        if (fwrite(&go, 1, 1, stdout) != 1) return 1;
    }
    return 0;
}
