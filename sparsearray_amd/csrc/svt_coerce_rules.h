// The element rules of the coercions dense array <-> sparse operand (C_build_SVT_from_Rarray and
// C_from_SVT_SparseArray_to_Rarray, src/SVT_SparseArray_class.c of the reference; collect_offsets_of_nonzero_* and
// collect_offsets_of_nonNA_*, src/Rvector_utils.c), each stated once for the device kernels (kernels_coerce.hip) and for
// a host program (tests/coerce_rules_main.cpp): plain C++, no HIP header needed.
#pragma once

#include <stdint.h>

#include "../../include/svt_hip.h"

#ifdef __HIPCC__
#define SVT_COERCE_HD __host__ __device__
#else
#define SVT_COERCE_HD
#endif

#define SVT_COERCE_NA_INT (-2147483647 - 1)

SVT_COERCE_HD inline unsigned long long svt_coerce_bits(double v)
{
	union { double d; unsigned long long u; } x;
	x.d = v;
	return x.u;
}
SVT_COERCE_HD inline double svt_coerce_na_real()                // NA_real_: the NaN whose low word is 1954
{
	union { unsigned long long u; double d; } x;
	x.u = 0x7FF00000000007A2ULL;
	return x.d;
}
SVT_COERCE_HD inline bool svt_coerce_is_na(double v)            // R_IsNA()
{
	return v != v && (unsigned int) (svt_coerce_bits(v) & 0xFFFFFFFFu) == 1954u;
}
SVT_COERCE_HD inline bool svt_coerce_is_na(int32_t v) { return v == SVT_COERCE_NA_INT; }

// Is a cell of the dense array stored?  Ordinary background: when it is != 0 -- so -0.0 and integer 0 are dropped and a
// NaN, NA_real_, +-Inf, a subnormal and NA_integer_ are stored.  na_background: when it is not NA -- R_IsNA for a
// double, so a plain NaN is stored; NA_integer_ for an integer or a logical; zeros are stored.
template <typename T>
SVT_COERCE_HD inline bool svt_rule_keep(T v, bool na_background)
{
	return na_background ? !svt_coerce_is_na(v) : v != (T) 0;
}

// A value in the result's type: the same element size moves as bits (logical -> integer too), integer or logical ->
// double converts the value and NA_integer_ becomes NA_real_.  The rule abind and subassignment state for their copies.
SVT_COERCE_HD inline void svt_rule_coerce(int32_t v, int32_t *out) { *out = v; }
SVT_COERCE_HD inline void svt_rule_coerce(double v, double *out) { *out = v; }
SVT_COERCE_HD inline void svt_rule_coerce(int32_t v, double *out) { *out = v == SVT_COERCE_NA_INT ? svt_coerce_na_real() : (double) v; }

// the implicit value of the dense form: zero, or NA of the type under na_background
SVT_COERCE_HD inline void svt_rule_background(bool na_background, int32_t *out) { *out = na_background ? SVT_COERCE_NA_INT : 0; }
SVT_COERCE_HD inline void svt_rule_background(bool na_background, double *out) { *out = na_background ? svt_coerce_na_real() : 0.0; }

// logical < integer < double; -1 for any other type
SVT_COERCE_HD inline int svt_rule_type_rank(int Rtype)
{
	return Rtype == SVT_LGLSXP ? 0 : Rtype == SVT_INTSXP ? 1 : Rtype == SVT_REALSXP ? 2 : -1;
}
// 0: `to` is `from` or a wider type; 1: narrower (not offered); -1: either is none of the three
SVT_COERCE_HD inline int svt_rule_coerce_status(int from_Rtype, int to_Rtype)
{
	const int f = svt_rule_type_rank(from_Rtype), t = svt_rule_type_rank(to_Rtype);
	if (f < 0 || t < 0) return -1;
	return t < f ? 1 : 0;
}
