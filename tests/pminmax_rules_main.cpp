// The three rules of pmin / pmax and is.na / is.nan / is.infinite (sparsearray_amd/csrc/svt_arith_rules.h) on the host,
// printed over the value table of tests/pminmax_cases.py (tests/test_zzzzzzz_pminmax_cpu.py builds this with the host
// compiler and its sanitizers and compares the text with numpy's statement of the formulas, on bits):
//   P <x type> <y type> <op> <na_rm> <i> <j> <bits of svt_rule_pminmax(op, na_rm, widen(X[i]), widen(Y[j]))>
//   F <type> <op> <i> <svt_rule_isfun(op, X[i])>
//   K <type> <op with or without SVT_PMINMAX_NA_RM> <i> <svt_rule_pminmax_keeps_sparse(op, X[i], type)>
// Types: d = double, i = integer.  A result prints as the hexadecimal of its bits (an int32 as 8 digits).
#include <float.h>
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include "../sparsearray_amd/csrc/svt_arith_rules.h"

static void put(double v)
{
	unsigned long long u;
	memcpy(&u, &v, 8);
	printf("%016llx\n", u);
}
static void put(int32_t v) { printf("%08x\n", (unsigned) v); }

template <typename TX, typename TY, typename TO>
static void pairs(char cx, char cy, const TX *X, int n, const TY *Y, int m)
{
	for (int op = SVT_PMINMAX_MIN; op <= SVT_PMINMAX_MAX; op++)
		for (int na_rm = 0; na_rm <= 1; na_rm++)
			for (int i = 0; i < n; i++)
				for (int j = 0; j < m; j++) {
					TO x, y;
					svt_rule_widen(X[i], &x);
					svt_rule_widen(Y[j], &y);
					printf("P %c %c %d %d %d %d ", cx, cy, op, na_rm, i, j);
					put(svt_rule_pminmax(op, na_rm, x, y));
				}
}

int main(void)
{
	const double D[9] = { 0.0, -0.0, 1.5, -2.0, DBL_MAX, svt_rule_inf(), -svt_rule_inf(), svt_rule_bits(0x7FF8000000ABCDEFULL),
			      svt_rule_na_real() };
	const int32_t I[5] = { 0, 1, -7, INT_MAX, SVT_NA_INT };
	pairs<double, double, double>('d', 'd', D, 9, D, 9);
	pairs<int32_t, int32_t, int32_t>('i', 'i', I, 5, I, 5);
	pairs<int32_t, double, double>('i', 'd', I, 5, D, 9);
	pairs<double, int32_t, double>('d', 'i', D, 9, I, 5);
	for (int op = SVT_IS_NA; op <= SVT_IS_INFINITE; op++) {
		for (int i = 0; i < 9; i++) printf("F d %d %d %d\n", op, i, (int) svt_rule_isfun(op, D[i]));
		for (int i = 0; i < 5; i++) printf("F i %d %d %d\n", op, i, (int) svt_rule_isfun(op, I[i]));
	}
	for (int op = SVT_PMINMAX_MIN; op <= SVT_PMINMAX_MAX; op++)
		for (int na_rm = 0; na_rm <= SVT_PMINMAX_NA_RM; na_rm += SVT_PMINMAX_NA_RM) {
			for (int i = 0; i < 9; i++)
				printf("K d %d %d %d\n", op | na_rm, i, (int) svt_rule_pminmax_keeps_sparse(op | na_rm, D[i], SVT_REALSXP));
			for (int i = 0; i < 5; i++)     // (handed over as the kernels hand it over: as a double, INT_MIN standing for NA)
				printf("K i %d %d %d\n", op | na_rm, i, (int) svt_rule_pminmax_keeps_sparse(op | na_rm, (double) I[i], SVT_INTSXP));
		}
	return 0;
}
