// Host build (g++) of getdist_amd/csrc/colexpr.hpp for tests/test_colexpr_cpu.py: the program check of gd_expr_eval and
// its interpreter step, run row by row over host columns.
#include "../../getdist_amd/csrc/colexpr.hpp"

extern "C" {

// nullptr when gd_expr_eval would accept the program for a sample set of `ncols` addressable columns, else the complaint
const char* colexpr_check(const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int64_t ncols) {
    gdex::Program P;
    return gdex::ex_pack(code, ncode, consts, nconst, ncols, &P);
}

// the deepest the stack gets, or -1 for a program that does not pass the check
int32_t colexpr_depth(const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int64_t ncols) {
    gdex::Program P;
    return gdex::ex_pack(code, ncode, consts, nconst, ncols, &P) ? -1 : P.depth;
}

// out[r] = the program's value at row r; column j of the row is cols[j * n + r], the weights are `weights` (NULL: 1.0).
// Returns 0, or -1 for a program that does not pass the check.
int32_t colexpr_run(const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int64_t ncols, const double* cols,
                    const double* weights, int64_t n, double* out) {
    gdex::Program P;
    if (gdex::ex_pack(code, ncode, consts, nconst, ncols, &P)) return -1;
    double vals[GD_EX_MAX_COLS];
    for (int64_t r = 0; r < n; ++r) {
        for (int k = 0; k < P.nsrc; ++k)
            vals[k] = P.src[k] == GD_EX_WEIGHT ? (weights ? weights[r] : 1.0) : cols[(int64_t)P.src[k] * n + r];
        out[r] = gdex::ex_run_row(P, vals);
    }
    return 0;
}

}  // extern "C"
