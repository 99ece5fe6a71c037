// The two predicates of sweep() (sparsearray_amd/csrc/svt_arith_rules.h) on the host: "this element of STATS keeps
// x op STATS[k] sparse".  One request per line of standard input, one answer (0 / 1) per line of standard output
// (tests/test_zzzzzz_sweep_cpu.py builds it with the host compiler and compares the answers with the issue's table).
// A double travels as the hexadecimal of its bits; an integer or logical element as its value, which is handed over as
// the kernels hand it over: converted to double, INT_MIN standing for NA.
//   A <op> <Rtype> <bits or value>   ->  <svt_rule_arith_keeps_sparse(op, s, Rtype)>
//   C <op> <Rtype> <bits or value>   ->  <svt_rule_compare_keeps_sparse(op, s, Rtype)>
#include <stdio.h>
#include <string.h>

#include "../sparsearray_amd/csrc/svt_arith_rules.h"

int main(void)
{
	char what;
	while (scanf(" %c", &what) == 1) {
		int op, Rtype;
		double s;
		if (scanf("%d %d", &op, &Rtype) != 2)
			return 2;
		if (Rtype == SVT_REALSXP) {
			unsigned long long u;
			if (scanf("%llx", &u) != 1) return 2;
			memcpy(&s, &u, 8);
		} else {
			int v;
			if (scanf("%d", &v) != 1) return 2;
			s = (double) v;
		}
		if (what == 'A')
			printf("%d\n", (int) svt_rule_arith_keeps_sparse(op, s, Rtype));
		else if (what == 'C')
			printf("%d\n", (int) svt_rule_compare_keeps_sparse(op, s, Rtype));
		else
			return 2;
	}
	return 0;
}
