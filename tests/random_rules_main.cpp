// The host side of sparsearray_amd/csrc/svt_random_rules.h: one request per line on stdin, one answer per line on stdout
// (tests/test_zzzzzzzzzzzz_poisson_cpu.py).  Words, seeds, cells and doubles travel as hex digits.
//   philox <c0> <c1> <c2> <c3> <k0> <k1>  -> the four output words
//   cell <seed> <cell> <lambda>           -> <hex of u> <value>    (value -1: the lambda has no table)
//   ticks <lambda>                        -> <n> <hex of tick 0> ... <hex of tick n-1>
#include <stdio.h>
#include <string.h>

#include "../sparsearray_amd/csrc/svt_random_rules.h"

static double from_hex(unsigned long long u)
{
	union { unsigned long long u; double d; } x;
	x.u = u;
	return x.d;
}
static unsigned long long to_hex(double d)
{
	union { double d; unsigned long long u; } x;
	x.d = d;
	return x.u;
}

int main()
{
	char op[32];
	char line[512];
	while (fgets(line, sizeof(line), stdin)) {
		unsigned long long a[6] = { 0, 0, 0, 0, 0, 0 };
		if (sscanf(line, "%31s %llx %llx %llx %llx %llx %llx", op, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) < 1)
			continue;
		if (!strcmp(op, "philox")) {
			const svt_philox_words w = svt_philox4x32_10((uint32_t) a[0], (uint32_t) a[1], (uint32_t) a[2], (uint32_t) a[3],
								     (uint32_t) a[4], (uint32_t) a[5]);
			printf("%08x %08x %08x %08x\n", w.w[0], w.w[1], w.w[2], w.w[3]);
		} else if (!strcmp(op, "cell")) {
			svt_poisson_table t;
			memset(&t, 0, sizeof(t));
			t.n = svt_rule_poisson_ticks(from_hex(a[2]), t.ticks);
			const double u = svt_rule_cell_uniform(a[0], a[1]);
			const int v = t.n < 0 ? -1 : svt_rule_poisson_cell(a[0], a[1], t);
			if (t.n >= 0 && (v != 0) != svt_rule_poisson_nonzero(u, t)) {
				printf("the nonzero rule disagrees with find_interval\n");
				continue;
			}
			printf("%016llx %d\n", to_hex(u), v);
		} else if (!strcmp(op, "ticks")) {
			double ticks[SVT_POISSON_MAX_TICKS];
			const int n = svt_rule_poisson_ticks(from_hex(a[0]), ticks);
			printf("%d", n);
			for (int k = 0; k < n; k++) printf(" %016llx", to_hex(ticks[k]));
			printf("\n");
		} else {
			printf("?\n");
		}
	}
	return 0;
}
