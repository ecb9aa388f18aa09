// Host-only build (g++) of the scalar tail of gd_prepare_params (getdist_amd/csrc/batch2d.hpp: prepare_tail) for the CPU
// test-suite: records in, records out, exactly as inside libgdhip.so.  Test infrastructure only.
#include "../../getdist_amd/csrc/batch2d.hpp"

extern "C" {

// q: m x 11, minmax: m x 2, limits: m x 2; recs arrive with the prior limit flags and leave final
void gdt_prepare_tail(int32_t m, const double* q, const double* minmax, const double* err, const double* limits,
                      gd_prepared_param* recs) {
    for (int c = 0; c < m; ++c)
        gdb::prepare_tail(q + (size_t)11 * c, minmax[2 * c], minmax[2 * c + 1], err[c], limits[2 * c], limits[2 * c + 1], &recs[c]);
}
}
