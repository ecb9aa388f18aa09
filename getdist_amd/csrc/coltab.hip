// gd_expr_eval_tab: column expressions with table look-ups (GD_TAB_INTERP / SPLINE1 / SPLINE2).  Kernel and launch code are in
// colexpr_kernel.hpp; this unit instantiates them with tables (k_expr_eval<true>), colexpr.hip without.
#include "colexpr_kernel.hpp"

extern "C" {

int gd_expr_eval_tab(gd_ctx* ctx, const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int32_t dst,
                     int32_t dst_arg, int64_t lo, int64_t hi, void* host_out, double* stats_out, const gd_expr_table* tables,
                     int32_t ntab) {
    GD_REQUIRE(ntab >= 0 && ntab <= GD_TAB_MAX_TABLES && (ntab == 0 || tables), "number of tables out of range");
    if (ntab == 0)  // the table-free kernel, which then refuses the table ops as unknown
        return gd_expr_eval(ctx, code, ncode, consts, nconst, dst, dst_arg, lo, hi, host_out, stats_out);
    return ex_eval<true>(ctx, code, ncode, consts, nconst, dst, dst_arg, lo, hi, host_out, stats_out, tables, ntab);
}

}  // extern "C"
