// fast_arith.h -- the sweep's device arithmetic helpers: Julia's max(x, 0.0), the correctly rounded division and square
// root without the range scaffolding, fast_exp, the window test and pinned().  Included by every kernel header AND by
// tests/native/fastmath_check.hip, which checks these very functions against the compiler's sequences; it needs no other
// project header than sweep.h (kFastExp).
#pragma once

#include "sweep.h"

namespace cfmm {

// Julia's max(x, 0.0): NaN propagates, max(-0.0, 0.0) == +0.0.
__device__ __forceinline__ double max0(double x)
{
    double r = x > 0.0 ? x : 0.0;
    return (x != x) ? x : r;
}

// ---------------------------------------------------------------------------------------------
// Correctly rounded binary64 division and square root without the range scaffolding
// ---------------------------------------------------------------------------------------------
// For a / b the compiler emits   d = v_div_scale(b, b, a);  y = v_rcp(d);  two Newton steps on y (4 fma);
// n = v_div_scale(a, b, a);  q = n·y;  r = fma(−d, q, n);  v_div_fmas(r, y, q);  v_div_fixup     (11 instructions),
// and for sqrt(x) a compare / select / ldexp pair around   y = v_rsq(x);  s = x·y;  h = y/2;  two coupled Newton steps
// (7 fma)   plus a class test                                                                        (16 instructions).
// The scaffolding only acts outside a huge exponent range: for finite, normal operands with |exponent| <= 300 or so
// v_div_scale returns its input, v_div_fmas is a plain fma, v_div_fixup returns its first operand and the ldexp pair
// scales by 2^0.  The SAME core sequences without it therefore return the SAME correctly rounded bits whenever every
// operand is inside [2^-kFastExp, 2^kFastExp] -- pool constants are checked at upload, the prices by every block while
// it stages them (`FAST` below); anything else takes the compiler's sequences.  What this buys beyond the 3 + 7
// instructions: the refined reciprocal y depends on the DIVISOR only, so it is computed once per token (prices) and
// once per fee tier while they are staged in LDS, and a division by a price or by a fee costs three instructions.
// (tests/test_gpu_parity.py: every ProductTwoCoin / UniV3 trade bit-equal to the CPU restatement with fast_math on and
// off; tests/native/fastmath_check.hip: 2^30 random operands against the compiler's / and sqrt.)
__device__ __forceinline__ double rcp_refined(double b)
{
    double y = __builtin_amdgcn_rcp(b);
    double e = __builtin_fma(-b, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-b, y, 1.0);
    return __builtin_fma(y, e, y);
}
// a / b given yb = rcp_refined(b);  a finite (any sign, zero included: a = ±0 returns a·yb = ±0 like IEEE for b > 0 --
// the residual fma then adds +0 to −0, so the sign of a zero quotient is restored explicitly)
__device__ __forceinline__ double div_by(double a, double b, double yb)
{
    const double q = a * yb;
    const double r = __builtin_fma(-b, q, a);
    return __builtin_fma(r, yb, q);
}
__device__ __forceinline__ double div_by_signed_zero(double a, double b, double yb)
{
    const double q = div_by(a, b, yb);
    return a == 0.0 ? a : q;      // b > 0 everywhere this is used: ±0 / b = ±0
}
__device__ __forceinline__ double fast_div(double a, double b) { return div_by(a, b, rcp_refined(b)); }
__device__ __forceinline__ double fast_sqrt(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double s = x * y;
    double h = y * 0.5;
    const double r = __builtin_fma(-h, s, 0.5);
    s = __builtin_fma(s, r, s);
    double d = __builtin_fma(-s, s, x);
    h = __builtin_fma(h, r, h);
    s = __builtin_fma(d, h, s);
    d = __builtin_fma(-s, s, x);
    return __builtin_fma(d, h, s);
}
// exp(x) for |x| < 700 (no overflow / underflow handling: inside the window of the fast arithmetic the argument is the
// logarithm of a reserve, |x| <= ~312), < 1 ulp like the device library's: x = k ln2 + r, |r| <= ln2/2,
// exp(r) = 1 + r + r^2 g(r) with g the degree-9 Chebyshev interpolant of (e^r - 1 - r)/r^2 (approximation error 1.6e-17,
// scripts/fit_exp.py), result ldexp(., k).  19 instructions against the library's 38: that one handles the whole
// double range (two compares, four selects) and the compiler expands its Horner steps into v_mov + v_fmac pairs; here
// each step is ONE v_fma with the coefficient in scalar registers.  NaN in, NaN out.
__device__ __forceinline__ double fma_sc(double x, double acc, double c)   // x * acc + c, c from SGPRs
{
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(acc), "s"(c));
    return r;
}
__device__ __forceinline__ double fast_exp(double x)
{
    const double k = __builtin_rint(x * 0x1.71547652b82fep+0);
    double r = __builtin_fma(-k, 0x1.62e42fefa39efp-1, x);
    r = __builtin_fma(-k, 0x1.abc9e3b39803fp-56, r);
    double p = 0x1.af39091a8441ap-26;
    p = fma_sc(r, p, 0x1.2891d2ecb3ed9p-22);
    p = fma_sc(r, p, 0x1.71de0d863c737p-19);
    p = fma_sc(r, p, 0x1.a019b8cbe6585p-16);
    p = fma_sc(r, p, 0x1.a01a01a7ce75dp-13);
    p = fma_sc(r, p, 0x1.6c16c1789caa1p-10);
    p = fma_sc(r, p, 0x1.11111111109a6p-7);
    p = fma_sc(r, p, 0x1.5555555553d38p-5);
    p = fma_sc(r, p, 0x1.5555555555556p-3);
    p = fma_sc(r, p, 0x1.0000000000001p-1);
    p = __builtin_fma(r, p, 1.0);
    p = __builtin_fma(r, p, 1.0);
    return __builtin_ldexp(p, (int)k);
}

// |x| in [2^-kFastExp, 2^kFastExp] (false for NaN, infinities, zero, denormals)
__device__ __forceinline__ bool in_fast_window(double x)
{
    const int e = (__double2hiint(x) >> 20) & 0x7ff;
    return e >= 1023 - kFastExp && e <= 1023 + kFastExp;
}

// Keeps a freshly loaded value in registers at this point of the program.  (Without it the compiler defers the second
// half of a {γ, rcp(γ)} table read into the branch that uses it by SELECTING BETWEEN POINTERS -- the LDS entry or a
// stack slot holding the 0.0 of the unpacked path -- and reads it back with a flat load: scratch traffic per tile.)
__device__ __forceinline__ double pinned(double x)
{
    asm volatile("" : "+v"(x));
    return x;
}

} // namespace cfmm
