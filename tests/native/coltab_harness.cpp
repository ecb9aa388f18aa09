// Host build (g++) of getdist_amd/csrc/colexpr.hpp for tests/test_coltab_cpu.py: the table look-ups of gd_expr_eval_tab --
// the checks the entry point runs before any launch, the three row functions on their own, and whole programs with tables
// run row by row over host columns.
#include "../../getdist_amd/csrc/colexpr.hpp"

extern "C" {

// nullptr when gd_expr_eval_tab would accept the program and its tables, else the complaint
const char* coltab_check(const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int64_t ncols,
                         const gd_expr_table* tables, int32_t ntab) {
    gdex::Program P;
    return gdex::ex_pack(code, ncode, consts, nconst, ncols, &P, tables, ntab);
}

// the deepest the stack gets, or -1 for a program that does not pass the check
int32_t coltab_depth(const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int64_t ncols,
                     const gd_expr_table* tables, int32_t ntab) {
    gdex::Program P;
    return gdex::ex_pack(code, ncode, consts, nconst, ncols, &P, tables, ntab) ? -1 : P.depth;
}

// colexpr_run of colexpr_harness.cpp for a program with tables
int32_t coltab_run(const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int64_t ncols, const double* cols,
                   const double* weights, int64_t n, double* out, const gd_expr_table* tables, int32_t ntab) {
    gdex::Program P;
    if (gdex::ex_pack(code, ncode, consts, nconst, ncols, &P, tables, ntab)) return -1;
    double vals[GD_EX_MAX_COLS];
    for (int64_t r = 0; r < n; ++r) {
        for (int k = 0; k < P.nsrc; ++k)
            vals[k] = P.src[k] == GD_EX_WEIGHT ? (weights ? weights[r] : 1.0) : cols[(int64_t)P.src[k] * n + r];
        out[r] = gdex::ex_run_row(P, vals, tables);
    }
    return 0;
}

// one look-up on its own, WITHOUT the table check (so that knots the entry point refuses, infinite ones, can be put to the
// row function): out[i] = the table at x[i] (and y[i] for a SPLINE2 table, else y is not read)
void coltab_rows(const gd_expr_table* table, const double* x, const double* y, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = gdex::tab_apply(table->kind, *table, table->p0, table->p1, x[i], table->kind == GD_TAB_SPLINE2 ? y[i] : x[i]);
}

// np.searchsorted(t[lo:hi], x, side="right") + lo
int32_t coltab_upper(const double* t, int32_t lo, int32_t hi, double x) { return gdex::tab_upper(t, lo, hi, x); }

}  // extern "C"
