// The element rules of Compare and Logic (sparsearray_amd/csrc/svt_arith_rules.h) on the host: one request per line of
// standard input, one answer per line of standard output (tests/test_z_compare_cpu.py builds it with the host compiler
// and compares the answers with tests/compare_cases.py).  Doubles travel as the hexadecimal of their bits.
//   C <op> <x bits> <y bits>   ->  <svt_rule_compare(op, x, y)>
//   J <op> <x> <y>             ->  <svt_rule_compare(op, as.double(x), as.double(y))> for two integers
//   L <op> <x> <y>             ->  <svt_rule_logic(op, x, y)>
#include <stdio.h>
#include <string.h>

#include "../sparsearray_amd/csrc/svt_arith_rules.h"

static double from_bits(unsigned long long u)
{
	double d;
	memcpy(&d, &u, 8);
	return d;
}

int main(void)
{
	char what;
	while (scanf(" %c", &what) == 1) {
		int op, a, b;
		unsigned long long x, y;
		if (what == 'C' && scanf("%d %llx %llx", &op, &x, &y) == 3)
			printf("%d\n", svt_rule_compare(op, from_bits(x), from_bits(y)));
		else if (what == 'J' && scanf("%d %d %d", &op, &a, &b) == 3)
			printf("%d\n", svt_rule_compare(op, svt_rule_as_double((int32_t) a), svt_rule_as_double((int32_t) b)));
		else if (what == 'L' && scanf("%d %d %d", &op, &a, &b) == 3)
			printf("%d\n", svt_rule_logic(op, a, b));
		else
			return 2;
	}
	return 0;
}
