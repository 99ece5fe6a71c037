// The element rules of Arith and Math on sparse operands (src/SparseVec_Arith.c, src/SparseVec_Math.c of the
// reference; R's arithmetic.c for the operators), each stated once for the device kernels (kernels_arith.hip) and for
// a host program (tests/arith_rules_main.cpp): plain C++, no HIP header needed.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/svt_hip.h"

#ifdef __HIPCC__
#define SVT_HD __host__ __device__
#else
#define SVT_HD
#endif

#define SVT_NA_INT (-2147483647 - 1)

SVT_HD inline double svt_rule_bits(unsigned long long u)
{
	union { unsigned long long u; double d; } x;
	x.u = u;
	return x.d;
}
SVT_HD inline double svt_rule_na_real() { return svt_rule_bits(0x7FF00000000007A2ULL); }   // NA_real_
SVT_HD inline double svt_rule_nan() { return svt_rule_bits(0x7FF8000000000000ULL); }       // R_NaN
SVT_HD inline double svt_rule_inf() { return svt_rule_bits(0x7FF0000000000000ULL); }

// as.double() of an integer
SVT_HD inline double svt_rule_as_double(int32_t x) { return x == SVT_NA_INT ? svt_rule_na_real() : (double) x; }
SVT_HD inline double svt_rule_as_double(double x) { return x; }

// integer op integer for + - * %% %/%: NA propagates; + - * are done in double, a result <= INT_MIN or > INT_MAX is NA
// and raises *ovflow; %% takes the sign of the divisor, %/% floors, a zero divisor gives NA
SVT_HD inline int32_t svt_rule_arith_int(int op, int32_t x, int32_t y, int *ovflow)
{
	if (x == SVT_NA_INT || y == SVT_NA_INT)
		return SVT_NA_INT;
	double vv;
	switch (op) {
	case SVT_ARITH_ADD: vv = (double) x + (double) y; break;
	case SVT_ARITH_SUB: vv = (double) x - (double) y; break;
	case SVT_ARITH_MULT: vv = (double) x * (double) y; break;
	case SVT_ARITH_MOD: {
		if (y == 0) return SVT_NA_INT;
		if (y == -1) return 0;                      // (INT_MIN is NA: no other x overflows, but the C % may trap)
		int32_t zz = x % y;
		if ((y > 0 && zz < 0) || (y < 0 && zz > 0)) zz += y;
		return zz;
	}
	case SVT_ARITH_IDIV: {
		if (y == 0) return SVT_NA_INT;
		if (y == -1) return -x;
		int32_t zz = x / y;
		if (((y > 0 && x < 0) || (y < 0 && x > 0)) && zz * y != x) zz--;
		return zz;
	}
	default:
		return SVT_NA_INT;
	}
	if (vv <= -2147483648.0 || vv > 2147483647.0) {
		*ovflow = 1;
		return SVT_NA_INT;
	}
	return (int32_t) vv;
}

// x ^ y: 1 for x == 1 or y == 0; NaN for a NaN y, for x < 0 with an infinite y, for x == -Inf with a non-integer y; a
// NaN x comes back as x + y, as R_pow does it (arithmetic.c), so that an NA stays an NA whatever pow() makes of one
SVT_HD inline double svt_rule_pow(double x, double y)
{
	if (x == 1.0 || y == 0.0)
		return 1.0;
	if (x != x && y == y)
		return x + y;
	if (y != y || (x < 0.0 && (y == svt_rule_inf() || y == -svt_rule_inf())) || (x == -svt_rule_inf() && y != trunc(y)))
		return svt_rule_nan();
	return pow(x, y);
}

// x %% y = x - y * floor(x / y), with the zero and the infinite cases
SVT_HD inline double svt_rule_mod(double x, double y)
{
	const double inf = svt_rule_inf();
	if (y == 0.0 || x == inf || x == -inf)
		return svt_rule_nan();
	if (x == 0.0)
		return y != y ? y : 0.0;
	if (y == inf)
		return (x != x || x > 0) ? x : inf;
	if (y == -inf)
		return (x != x || x < 0) ? x : -inf;
	return x - y * floor(x / y);
}

// x %/% y = floor(x / y), with the infinite cases
SVT_HD inline double svt_rule_idiv(double x, double y)
{
	const double inf = svt_rule_inf();
	if (y == inf) {
		if (x == -inf) return svt_rule_nan();
		if (x < 0) return -1.0;
	} else if (y == -inf) {
		if (x == inf) return svt_rule_nan();
		if (x > 0) return -1.0;
	}
	return floor(x / y);
}

SVT_HD inline double svt_rule_arith_double(int op, double x, double y)
{
	switch (op) {
	case SVT_ARITH_ADD: return x + y;
	case SVT_ARITH_SUB: return x - y;
	case SVT_ARITH_MULT: return x * y;
	case SVT_ARITH_DIV: return x / y;
	case SVT_ARITH_POW: return svt_rule_pow(x, y);
	case SVT_ARITH_MOD: return svt_rule_mod(x, y);
	case SVT_ARITH_IDIV: return svt_rule_idiv(x, y);
	}
	return svt_rule_nan();
}

// the members of the Math group offered here, on a double
SVT_HD inline double svt_rule_math(int op, double x)
{
	switch (op) {
	case SVT_MATH_ABS: return fabs(x);
	case SVT_MATH_SIGN: return x != x ? x : (x > 0.0 ? 1.0 : (x == 0.0 ? 0.0 : -1.0));
	case SVT_MATH_SQRT: return sqrt(x);
	case SVT_MATH_FLOOR: return floor(x);
	case SVT_MATH_CEILING: return ceil(x);
	case SVT_MATH_TRUNC: return trunc(x);
	// below 2^-54 both series round to x itself (|x^2 / 2| < ulp(x) / 4); said here because the device library
	// answers 0 for the smallest denormals, and a zero result is an entry dropped
	case SVT_MATH_LOG1P: return fabs(x) < 0x1p-54 ? x : log1p(x);
	case SVT_MATH_EXPM1: return fabs(x) < 0x1p-54 ? x : expm1(x);
	}
	return svt_rule_nan();
}

// the type of the result (SVT_INTSXP / SVT_REALSXP), or 0 for a combination that is not offered
SVT_HD inline int svt_rule_out_Rtype(int kind, int op, int x_Rtype, int y_Rtype)
{
	const bool xi = x_Rtype == SVT_INTSXP, xd = x_Rtype == SVT_REALSXP;
	const bool yi = y_Rtype == SVT_INTSXP, yd = y_Rtype == SVT_REALSXP;
	switch (kind) {
	case SVT_ARITH_MERGE:
		if (!(xi || xd) || !(yi || yd) || op < SVT_ARITH_ADD || op > SVT_ARITH_MULT) return 0;
		return xi && yi ? SVT_INTSXP : SVT_REALSXP;
	case SVT_ARITH_SCALAR:
		if (!(xi || xd) || !(yi || yd) || op < SVT_ARITH_MULT || op > SVT_ARITH_IDIV) return 0;
		return xi && yi && op != SVT_ARITH_DIV && op != SVT_ARITH_POW ? SVT_INTSXP : SVT_REALSXP;
	case SVT_ARITH_NEG:
		return xi || xd ? x_Rtype : 0;
	case SVT_ARITH_MATH:
		return xd && op >= SVT_MATH_ABS && op <= SVT_MATH_EXPM1 ? SVT_REALSXP : 0;
	}
	return 0;
}
