// The element rules of sparsearray_amd/csrc/svt_arith_rules.h on the host: one request per line of standard input,
// one answer per line of standard output (tests/test_arith_cpu.py builds it with the host compiler and compares the
// answers with tests/arith_cases.py).  Doubles travel as the hexadecimal of their bits.
//   D <op> <x bits> <y bits>   ->  <bits of svt_rule_arith_double(op, x, y)>
//   I <op> <x> <y>             ->  <svt_rule_arith_int(op, x, y)> <overflow flag>
//   M <op> <x bits>            ->  <bits of svt_rule_math(op, x)>
//   T <kind> <op> <x Rtype> <y Rtype>  ->  <svt_rule_out_Rtype(...)>
#include <stdio.h>
#include <string.h>

#include "../sparsearray_amd/csrc/svt_arith_rules.h"

static double from_bits(unsigned long long u)
{
	double d;
	memcpy(&d, &u, 8);
	return d;
}
static unsigned long long to_bits(double d)
{
	unsigned long long u;
	memcpy(&u, &d, 8);
	return u;
}

int main(void)
{
	char what;
	while (scanf(" %c", &what) == 1) {
		int op, a, b, c;
		unsigned long long x, y;
		if (what == 'D' && scanf("%d %llx %llx", &op, &x, &y) == 3) {
			printf("%016llx\n", to_bits(svt_rule_arith_double(op, from_bits(x), from_bits(y))));
		} else if (what == 'I' && scanf("%d %d %d", &op, &a, &b) == 3) {
			int ov = 0;
			const int r = svt_rule_arith_int(op, a, b, &ov);
			printf("%d %d\n", r, ov);
		} else if (what == 'M' && scanf("%d %llx", &op, &x) == 2) {
			printf("%016llx\n", to_bits(svt_rule_math(op, from_bits(x))));
		} else if (what == 'T' && scanf("%d %d %d %d", &a, &op, &b, &c) == 4) {
			printf("%d\n", svt_rule_out_Rtype(a, op, b, c));
		} else {
			return 2;
		}
	}
	return 0;
}
