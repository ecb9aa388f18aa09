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

// ---- table look-ups (gd_expr_eval_tab): the row arithmetic of GD_TAB_INTERP / SPLINE1 / SPLINE2 over pointers to the table
// (host pointers in the harness, the scratch copy in the kernel; the knot arrays are passed on their own).  Each is the reference's evaluation in its operation
// order -- numpy's arr_interp, densities.NotAKnotSpline.__call__, FITPACK's fpbisp + fpbspl for one point -- so that with
// nothing contracted the values are theirs bit for bit.

// The first i in [lo, hi) with x < t[i], else hi (np.searchsorted(side="right") on t[lo:hi]; a NaN x gives hi).  A
// bisection whose trip count depends on hi - lo only: the lanes of a wave hold different x but run the same steps, each
// with one load from the knot array.
GD_HD inline int tab_upper(const double* t, int lo, int hi, double x) {
    int base = lo, len = hi - lo;
    if (len <= 0) return lo;
    while (len > 1) {
        const int half = len >> 1;
        if (!(x < t[base + half - 1])) base += half;
        len -= half;
    }
    return base + (x < t[base] ? 0 : 1);
}

// np.interp(x, xp, fp, left, right), numpy/_core/src/multiarray/compiled_base.c (arr_interp)
GD_HD inline double tab_interp(const gd_expr_table& T, const double* xp, double x) {
    const double* fp = T.p1;
    const int n = T.nx;
    if (n == 1) return x < xp[0] ? T.left : (x > xp[0] ? T.right : fp[0]);  // (a NaN x gives fp[0] there)
    const int hit = tab_upper(xp, 0, n, x) - 1;  // the largest j with xp[j] <= x; -1 below the knots, n - 1 for NaN
    const int j = hit < 0 ? 0 : (hit > n - 2 ? n - 2 : hit);
    const double x0 = xp[j], x1 = xp[j + 1], f0 = fp[j], f1 = fp[j + 1];
    const double slope = (f1 - f0) / (x1 - x0);
    double r = slope * (x - x0) + f0;
    if (r != r) {  // "if we get nan in one direction, try the other"
        r = slope * (x - x1) + f1;
        if (r != r && f0 == f1) r = f0;
    }
    if (x0 == x) r = f0;  // no arithmetic at a knot
    if (hit == n - 1) r = f1;
    if (x < xp[0]) r = T.left;
    if (x > xp[n - 1]) r = T.right;
    return x != x ? x : r;
}

// densities.NotAKnotSpline.__call__(x, deriv): p1 holds {y[k], c1, c2, c3} of interval k, t = x - knot[k]
GD_HD inline double tab_spline1(const gd_expr_table& T, const double* kn, double x) {
    const int n = T.nx;
    int k = tab_upper(kn, 0, n, x) - 1;
    k = k < 0 ? 0 : (k > n - 2 ? n - 2 : k);
    const double t = x - kn[k];
    const double* c = T.p1 + 4 * (int64_t)k;
    double out;
    if (T.deriv == 0)
        out = c[0] + t * (c[1] + t * (c[2] + t * c[3]));
    else if (T.deriv == 1)
        out = c[1] + t * (2.0 * c[2] + 3.0 * t * c[3]);
    else if (T.deriv == 2)
        out = 2.0 * c[2] + 6.0 * t * c[3];
    else
        out = 6.0 * c[3];
    return (x < kn[0] || x > kn[n - 1]) ? 0.0 : out;
}

// one step of fpbspl's inner loop: h(i) = h(i) + f (t(li) - x), h(i + 1) = f (x - t(lj)) with f = hh(i) / (t(li) - t(lj)),
// or h(i + 1) = 0 where the two knots are equal
GD_HD inline void tab_bspl_step(double hh, double tli, double tlj, double x, double& hi, double& hi1) {
    if (tli == tlj) {
        hi1 = 0.0;
    } else {
        const double f = hh / (tli - tlj);
        hi = hi + f * (tli - x);
        hi1 = f * (x - tlj);
    }
}

// fpbisp's first half for one argument of one axis (kx = 3): clamp to [t[3], t[n - 4]], find the knot interval l
// (1-based as in the Fortran: t(l) <= arg < t(l + 1), l <= n - 4) and fpbspl's four non-zero B-splines h there -- its
// loops over j = 1 .. 3 and i = 1 .. j written out, so that h stays in registers.  Returns l - 4, the first coefficient
// of the axis.
GD_HD inline int tab_bspl(const double* t, int n, double arg, double* h) {
    const double tb = t[3], te = t[n - 4];
    if (arg < tb) arg = tb;
    if (arg > te) arg = te;
    const int l = tab_upper(t, 4, n - 4, arg);  // the Fortran's linear search: the first l >= 4 with arg < t(l + 1), else n - 4
    const double* u = t + l;  // u[k] = t(l + 1 + k)
    double h0, h1 = 0.0, h2 = 0.0, h3 = 0.0, a, b;
    h0 = 0.0;  // j = 1: hh = {1}
    tab_bspl_step(1.0, u[0], u[-1], arg, h0, h1);
    a = h0, h0 = 0.0;  // j = 2: hh = {a, b}
    b = h1;
    tab_bspl_step(a, u[0], u[-2], arg, h0, h1);
    tab_bspl_step(b, u[1], u[-1], arg, h1, h2);
    a = h0, h0 = 0.0;  // j = 3: hh = {a, b, c}
    b = h1;
    const double c = h2;
    tab_bspl_step(a, u[0], u[-3], arg, h0, h1);
    tab_bspl_step(b, u[1], u[-2], arg, h1, h2);
    tab_bspl_step(c, u[2], u[-1], arg, h2, h3);
    h[0] = h0, h[1] = h1, h[2] = h2, h[3] = h3;
    return l - 4;
}

// FITPACK fpbisp for the single point (x, y): what scipy's RectBivariateSpline.ev / bispeu computes
GD_HD inline double tab_spline2(const gd_expr_table& T, const double* tx, const double* ty, double x, double y) {
    double hx[4], hy[4];
    const int nky1 = T.ny - 4;
    const int lx = tab_bspl(tx, T.nx, x, hx), ly = tab_bspl(ty, T.ny, y, hy);
    const double* c = T.p2 + (int64_t)lx * nky1 + ly;
    double sp = 0.0;
#pragma unroll
    for (int i1 = 0; i1 < 4; ++i1)
#pragma unroll
        for (int j1 = 0; j1 < 4; ++j1) sp = sp + c[(int64_t)i1 * nky1 + j1] * hx[i1] * hy[j1];
    return sp;
}

GD_HD inline bool is_table_op(int op) { return op >= GD_TAB_INTERP && op <= GD_TAB_SPLINE2; }

// one table op on one row: b is the top of the stack, a the entry below it (read by SPLINE2 only).  k0 / k1 are the knot
// arrays, T.p0 / T.p1 or a copy of them that is nearer (the kernel stages them in LDS)
GD_HD inline double tab_apply(int op, const gd_expr_table& T, const double* k0, const double* k1, double a, double b) {
    if (op == GD_TAB_INTERP) return tab_interp(T, k0, b);
    if (op == GD_TAB_SPLINE1) return tab_spline1(T, k0, b);
    return tab_spline2(T, k0, k1, a, b);
}

// the number of doubles of a table whose sizes passed tab_check
inline int64_t tab_doubles(const gd_expr_table& T, int part) {
    if (T.kind == GD_TAB_INTERP) return part < 2 ? T.nx : 0;
    if (T.kind == GD_TAB_SPLINE1) return part == 0 ? T.nx : (part == 1 ? 4 * ((int64_t)T.nx - 1) : 0);
    return part == 0 ? T.nx : (part == 1 ? T.ny : ((int64_t)T.nx - 4) * ((int64_t)T.ny - 4));
}

inline bool tab_knots_ok(const double* t, int n) {
    for (int i = 0; i < n; ++i)
        if (!(t[i] - t[i] == 0.0) || (i > 0 && t[i] < t[i - 1])) return false;  // (inf - inf and NaN - NaN are NaN)
    return true;
}

// What gd_expr_eval_tab checks of one table before any launch: nullptr, or what is wrong with it.
inline const char* tab_check(const gd_expr_table& T) {
    if (!is_table_op(T.kind)) return "unknown table kind";
    const int64_t nx = T.nx, ny = T.ny;
    if (T.kind == GD_TAB_INTERP) {
        if (nx < 1) return "an interpolation table needs at least 1 knot";
        if (2 * nx > GD_TAB_MAX_DOUBLES) return "a table holds more than GD_TAB_MAX_DOUBLES doubles";
        if (!T.p0 || !T.p1) return "null table pointer";
    } else if (T.kind == GD_TAB_SPLINE1) {
        if (nx < 4) return "a cubic spline table needs at least 4 knots";
        if (nx + 4 * (nx - 1) > GD_TAB_MAX_DOUBLES) return "a table holds more than GD_TAB_MAX_DOUBLES doubles";
        if (T.deriv < 0 || T.deriv > 3) return "derivative order of a spline table out of range";
        if (!T.p0 || !T.p1) return "null table pointer";
    } else {
        if (nx < 8 || ny < 8) return "a bicubic spline table needs at least 8 knots per axis";
        if (nx > GD_TAB_MAX_DOUBLES || ny > GD_TAB_MAX_DOUBLES || nx + ny + (nx - 4) * (ny - 4) > GD_TAB_MAX_DOUBLES)
            return "a table holds more than GD_TAB_MAX_DOUBLES doubles";
        if (!T.p0 || !T.p1 || !T.p2) return "null table pointer";
        if (!tab_knots_ok(T.p1, T.ny)) return "table knots must be finite and non-decreasing";
    }
    if (!tab_knots_ok(T.p0, T.nx)) return "table knots must be finite and non-decreasing";
    return nullptr;
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
// included).  Returns nullptr when the program is valid, else what is wrong with it.  With `ntab` tables (gd_expr_eval_tab) the
// table ops are accepted and the tables checked; without, they are unknown ops.
inline const char* ex_pack(const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int64_t ncols, Program* P,
                           const gd_expr_table* tables = nullptr, int32_t ntab = 0) {
    if (ntab < 0 || ntab > GD_TAB_MAX_TABLES || (ntab > 0 && !tables)) return "number of tables out of range";
    for (int k = 0; k < ntab; ++k)
        if (const char* bad = tab_check(tables[k])) return bad;
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
        } else if (ntab > 0 && is_table_op(op)) {
            if (arg < 0 || arg >= ntab) return "table slot out of range";
            if (tables[arg].kind != op) return "the table's kind does not match the op";
            a = arg;
            if (depth < (op == GD_TAB_SPLINE2 ? 2 : 1)) return "stack underflow";
            if (op == GD_TAB_SPLINE2) --depth;
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
inline double ex_run_row(const Program& P, const double* vals, const gd_expr_table* tables = nullptr) {
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
        else if (op == GD_TAB_SPLINE2)
            st[d - 2] = tab_spline2(tables[P.arg(pc)], tables[P.arg(pc)].p0, tables[P.arg(pc)].p1, st[d - 2], st[d - 1]), --d;
        else if (is_table_op(op))
            st[d - 1] = tab_apply(op, tables[P.arg(pc)], tables[P.arg(pc)].p0, tables[P.arg(pc)].p1, 0.0, st[d - 1]);
        else
            st[d - 3] = op_where(st[d - 3], st[d - 2], st[d - 1]), d -= 2;
    }
    return st[0];
}

}  // namespace gdex
