// gd_expr_eval: column expressions without table look-ups.  Kernel and launch code are in colexpr_kernel.hpp; this unit
// instantiates them without tables (k_expr_eval<false>), coltab.hip with.
#include "colexpr_kernel.hpp"

extern "C" {

int gd_expr_eval(gd_ctx* ctx, const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int32_t dst,
                 int32_t dst_arg, int64_t lo, int64_t hi, void* host_out, double* stats_out) {
    return ex_eval<false>(ctx, code, ncode, consts, nconst, dst, dst_arg, lo, hi, host_out, stats_out, nullptr, 0);
}

}  // extern "C"
