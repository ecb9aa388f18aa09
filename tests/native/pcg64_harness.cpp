// Host build (g++) of getdist_amd/csrc/pcg64.hpp for tests/test_pcg64_native.py: 128-bit words cross the C boundary as
// {hi, lo} pairs of uint64.
#include "../../getdist_amd/csrc/pcg64.hpp"

using gdpcg::make_u128;
using gdpcg::u128;

static gdpcg::Pcg64 gen(const uint64_t* st) { return gdpcg::Pcg64{make_u128(st[0], st[1]), make_u128(st[2], st[3])}; }

extern "C" {

// the double numpy's Generator.random() returns as draw number `offset` (0-based): advance(offset), then next_double
double pcg64_double_at(const uint64_t* st, uint64_t offset) {
    gdpcg::Pcg64 g = gen(st);
    g.advance((u128)offset);
    return g.next_double();
}

// out[i] = next_double() of n consecutive draws from the given state
void pcg64_doubles(const uint64_t* st, int64_t n, double* out) {
    gdpcg::Pcg64 g = gen(st);
    for (int64_t i = 0; i < n; ++i) out[i] = g.next_double();
}

// state_out = {hi, lo} of the state after advance(delta)
void pcg64_advance(const uint64_t* st, uint64_t delta, uint64_t* state_out) {
    gdpcg::Pcg64 g = gen(st);
    g.advance((u128)delta);
    state_out[0] = gdpcg::hi64(g.state), state_out[1] = gdpcg::lo64(g.state);
}

// out[k] = output of the state after (k + 1) applications of stride(inc, T), starting from the given state
void pcg64_stride_walk(const uint64_t* st, uint64_t T, int64_t steps, uint64_t* out) {
    gdpcg::Pcg64 g = gen(st);
    const gdpcg::Affine hop = gdpcg::stride(g.inc, (u128)T);
    u128 s = g.state;
    for (int64_t k = 0; k < steps; ++k) {
        s = hop(s);
        out[k] = gdpcg::output(s);
    }
}

// out[i] = next_u64() of n consecutive single steps
void pcg64_single_steps(const uint64_t* st, int64_t n, uint64_t* out) {
    gdpcg::Pcg64 g = gen(st);
    for (int64_t i = 0; i < n; ++i) out[i] = g.next_u64();
}

}  // extern "C"
