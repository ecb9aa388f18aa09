// The interpreter step of gd_expr_eval (colexpr.hip), written so that the SAME source runs inside the HIP kernel and in a
// plain C++ harness (tests/native), where the exact class of ops is checked bit for bit against numpy.
//
// A program is postfix: (op, arg) pairs over a stack of doubles.  Booleans are the doubles 0.0 / 1.0; an operand of a
// logical op or of WHERE's condition counts as true when it is != 0 (so NaN is true, as in numpy).  Every op is one small
// function; ex_apply1 / ex_apply2 dispatch on the opcode, which in the kernel is wave-uniform (the program lives in the
// kernel arguments), so the switch is a scalar branch.
//
// Exactness: + - * / sqrt are the IEEE operations as long as nothing is contracted into an fma (-ffp-contract=off, here
// and in the harness); NEG / ABS touch the sign bit only (NaN payloads survive); MIN / MAX are numpy's minimum / maximum,
// isnan(a) ? a : (a < b ? a : b) -- a NaN in either operand comes out, which fmin / fmax would swallow.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/gdhip.h"

#ifndef GD_HD
#ifdef __HIPCC__
#define GD_HD __host__ __device__
#else
#define GD_HD
#endif
#endif

namespace gdex {

GD_HD inline double from_bool(bool b) { return b ? 1.0 : 0.0; }

// ---- unary
GD_HD inline double op_neg(double x) { return -x; }
GD_HD inline double op_abs(double x) { return __builtin_fabs(x); }
GD_HD inline double op_sqrt(double x) { return ::sqrt(x); }
GD_HD inline double op_square(double x) { return x * x; }
GD_HD inline double op_recip(double x) { return 1.0 / x; }
GD_HD inline double op_exp(double x) { return ::exp(x); }
GD_HD inline double op_log(double x) { return ::log(x); }
GD_HD inline double op_log10(double x) { return ::log10(x); }
GD_HD inline double op_log2(double x) { return ::log2(x); }
GD_HD inline double op_sin(double x) { return ::sin(x); }
GD_HD inline double op_cos(double x) { return ::cos(x); }
GD_HD inline double op_tan(double x) { return ::tan(x); }
GD_HD inline double op_atan(double x) { return ::atan(x); }
GD_HD inline double op_tanh(double x) { return ::tanh(x); }
GD_HD inline double op_not(double x) { return from_bool(x == 0.0); }

// ---- binary (a below b on the stack)
GD_HD inline double op_add(double a, double b) { return a + b; }
GD_HD inline double op_sub(double a, double b) { return a - b; }
GD_HD inline double op_mul(double a, double b) { return a * b; }
GD_HD inline double op_div(double a, double b) { return a / b; }
GD_HD inline double op_pow(double a, double b) { return ::pow(a, b); }
GD_HD inline double op_atan2(double a, double b) { return ::atan2(a, b); }
GD_HD inline double op_min(double a, double b) { return a != a ? a : (a < b ? a : b); }
GD_HD inline double op_max(double a, double b) { return a != a ? a : (a > b ? a : b); }
GD_HD inline double op_lt(double a, double b) { return from_bool(a < b); }
GD_HD inline double op_le(double a, double b) { return from_bool(a <= b); }
GD_HD inline double op_gt(double a, double b) { return from_bool(a > b); }
GD_HD inline double op_ge(double a, double b) { return from_bool(a >= b); }
GD_HD inline double op_eq(double a, double b) { return from_bool(a == b); }
GD_HD inline double op_ne(double a, double b) { return from_bool(a != b); }
GD_HD inline double op_and(double a, double b) { return from_bool(a != 0.0 && b != 0.0); }
GD_HD inline double op_or(double a, double b) { return from_bool(a != 0.0 || b != 0.0); }

// ---- ternary
GD_HD inline double op_where(double c, double a, double b) { return c != 0.0 ? a : b; }

GD_HD inline bool is_unary(int op) { return op >= GD_EX_NEG && op <= GD_EX_NOT; }
GD_HD inline bool is_binary(int op) { return op >= GD_EX_ADD && op <= GD_EX_OR; }

// A stack entry is one row's value (the harness) or the values of the two rows a lane owns (the kernel): one dispatch on
// the opcode serves both rows.
struct Pair {
    double x, y;
};
template <double (*F)(double)>
GD_HD inline double map1(double v) {
    return F(v);
}
template <double (*F)(double)>
GD_HD inline Pair map1(const Pair& v) {
    return Pair{F(v.x), F(v.y)};
}
template <double (*F)(double, double)>
GD_HD inline double map2(double a, double b) {
    return F(a, b);
}
template <double (*F)(double, double)>
GD_HD inline Pair map2(const Pair& a, const Pair& b) {
    return Pair{F(a.x, b.x), F(a.y, b.y)};
}
GD_HD inline double map_where(double c, double a, double b) { return op_where(c, a, b); }
GD_HD inline Pair map_where(const Pair& c, const Pair& a, const Pair& b) {
    return Pair{op_where(c.x, a.x, b.x), op_where(c.y, a.y, b.y)};
}

template <class V>
GD_HD inline V ex_apply1(int op, const V& x) {
    switch (op) {
        case GD_EX_NEG: return map1<op_neg>(x);
        case GD_EX_ABS: return map1<op_abs>(x);
        case GD_EX_SQRT: return map1<op_sqrt>(x);
        case GD_EX_SQUARE: return map1<op_square>(x);
        case GD_EX_RECIP: return map1<op_recip>(x);
        case GD_EX_EXP: return map1<op_exp>(x);
        case GD_EX_LOG: return map1<op_log>(x);
        case GD_EX_LOG10: return map1<op_log10>(x);
        case GD_EX_LOG2: return map1<op_log2>(x);
        case GD_EX_SIN: return map1<op_sin>(x);
        case GD_EX_COS: return map1<op_cos>(x);
        case GD_EX_TAN: return map1<op_tan>(x);
        case GD_EX_ATAN: return map1<op_atan>(x);
        case GD_EX_TANH: return map1<op_tanh>(x);
        default: return map1<op_not>(x);
    }
}

template <class V>
GD_HD inline V ex_apply2(int op, const V& a, const V& b) {
    switch (op) {
        case GD_EX_ADD: return map2<op_add>(a, b);
        case GD_EX_SUB: return map2<op_sub>(a, b);
        case GD_EX_MUL: return map2<op_mul>(a, b);
        case GD_EX_DIV: return map2<op_div>(a, b);
        case GD_EX_POW: return map2<op_pow>(a, b);
        case GD_EX_ATAN2: return map2<op_atan2>(a, b);
        case GD_EX_MIN: return map2<op_min>(a, b);
        case GD_EX_MAX: return map2<op_max>(a, b);
        case GD_EX_LT: return map2<op_lt>(a, b);
        case GD_EX_LE: return map2<op_le>(a, b);
        case GD_EX_GT: return map2<op_gt>(a, b);
        case GD_EX_GE: return map2<op_ge>(a, b);
        case GD_EX_EQ: return map2<op_eq>(a, b);
        case GD_EX_NE: return map2<op_ne>(a, b);
        case GD_EX_AND: return map2<op_and>(a, b);
        default: return map2<op_or>(a, b);
    }
}

// The program as the kernel receives it: one 32-bit word per step, op | arg << 8 (a word, not two bytes: gfx950 has no scalar
// byte load, so the compiler reads a byte array in the kernel arguments with a VECTOR load per step), GD_EX_COL arguments
// renumbered to entries of the table of distinct sources (`src`: the caller's column indices, GD_EX_WEIGHT included).
struct Program {
    double consts[GD_EX_MAX_CONST];
    int32_t src[GD_EX_MAX_COLS];
    int32_t ncode, nsrc, depth;  // depth = the deepest the stack gets
    uint32_t ins[GD_EX_MAX_CODE];
    GD_HD int op(int pc) const { return (int)(ins[pc] & 0xffu); }
    GD_HD int arg(int pc) const { return (int)(ins[pc] >> 8); }
};

// Checks a program by simulating its stack and packs it; `ncols` = the number of addressable columns (spare ones
// included).  Returns nullptr when the program is valid, else what is wrong with it.
inline const char* ex_pack(const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int64_t ncols, Program* P) {
    if (!code || ncode < 1 || ncode > GD_EX_MAX_CODE) return "program length out of range";
    if (nconst < 0 || nconst > GD_EX_MAX_CONST || (nconst > 0 && !consts)) return "number of constants out of range";
    P->ncode = ncode, P->nsrc = 0, P->depth = 0;
    for (int i = 0; i < GD_EX_MAX_CONST; ++i) P->consts[i] = i < nconst ? consts[i] : 0.0;
    for (int i = 0; i < GD_EX_MAX_COLS; ++i) P->src[i] = 0;
    int depth = 0;
    for (int pc = 0; pc < ncode; ++pc) {
        const int32_t op = code[2 * pc], arg = code[2 * pc + 1];
        int a = 0;
        if (op == GD_EX_COL) {
            if (arg != GD_EX_WEIGHT && (arg < 0 || arg >= ncols)) return "column out of range";
            for (a = 0; a < P->nsrc && P->src[a] != arg; ++a) {
            }
            if (a == P->nsrc) {
                if (P->nsrc == GD_EX_MAX_COLS) return "too many distinct columns";
                P->src[P->nsrc++] = arg;
            }
            ++depth;
        } else if (op == GD_EX_CONST) {
            if (arg < 0 || arg >= nconst) return "constant out of range";
            a = arg;
            ++depth;
        } else if (is_unary(op)) {
            if (depth < 1) return "stack underflow";
        } else if (is_binary(op)) {
            if (depth < 2) return "stack underflow";
            --depth;
        } else if (op == GD_EX_WHERE) {
            if (depth < 3) return "stack underflow";
            depth -= 2;
        } else {
            return "unknown op";
        }
        if (depth > GD_EX_MAX_STACK) return "stack deeper than GD_EX_MAX_STACK";
        if (depth > P->depth) P->depth = depth;
        P->ins[pc] = (uint32_t)op | ((uint32_t)a << 8);
    }
    if (depth != 1) return "the program must leave exactly one value";
    return nullptr;
}

// One row on the host (the harness; the kernel has its own loop over the same ops with the stack in LDS):
// vals[k] = the row's value of source k.
inline double ex_run_row(const Program& P, const double* vals) {
    double st[GD_EX_MAX_STACK];
    int d = 0;
    for (int pc = 0; pc < P.ncode; ++pc) {
        const int op = P.op(pc);
        if (op == GD_EX_COL)
            st[d++] = vals[P.arg(pc)];
        else if (op == GD_EX_CONST)
            st[d++] = P.consts[P.arg(pc)];
        else if (is_unary(op))
            st[d - 1] = ex_apply1(op, st[d - 1]);
        else if (is_binary(op))
            st[d - 2] = ex_apply2(op, st[d - 2], st[d - 1]), --d;
        else
            st[d - 3] = op_where(st[d - 3], st[d - 2], st[d - 1]), d -= 2;
    }
    return st[0];
}

}  // namespace gdex
