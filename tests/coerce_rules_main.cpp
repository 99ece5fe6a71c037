// The host side of sparsearray_amd/csrc/svt_coerce_rules.h: one request per line on stdin, one answer per line on stdout
// (tests/test_zzzz_coerce_cpu.py).  Doubles travel as 16 hex digits, so that payloads and signs arrive as they are.
//   keepd <hex> <na_background>     -> 0 | 1
//   keepi <int32> <na_background>   -> 0 | 1
//   widen <int32>                   -> <hex> of the double
//   moved <hex>                     -> <hex> of the double moved as a double
//   movei <int32>                   -> the int32 moved as an int32
//   bgd <na_background>             -> <hex> of the double background
//   bgi <na_background>             -> the int32 background
//   status <from_Rtype> <to_Rtype>  -> 0 | 1 | -1
#include <stdio.h>
#include <string.h>

#include "../sparsearray_amd/csrc/svt_coerce_rules.h"

static double from_hex(const char *s)
{
	union { unsigned long long u; double d; } x;
	sscanf(s, "%llx", &x.u);
	return x.d;
}

int main()
{
	char op[32], a[64], b[64];
	char line[256];
	while (fgets(line, sizeof(line), stdin)) {
		a[0] = b[0] = 0;
		if (sscanf(line, "%31s %63s %63s", op, a, b) < 1)
			continue;
		int ia = 0, ib = 0;
		sscanf(a, "%d", &ia);
		sscanf(b, "%d", &ib);
		if (!strcmp(op, "keepd")) {
			printf("%d\n", (int) svt_rule_keep(from_hex(a), ib != 0));
		} else if (!strcmp(op, "keepi")) {
			printf("%d\n", (int) svt_rule_keep((int32_t) ia, ib != 0));
		} else if (!strcmp(op, "widen")) {
			double out;
			svt_rule_coerce((int32_t) ia, &out);
			printf("%016llx\n", svt_coerce_bits(out));
		} else if (!strcmp(op, "moved")) {
			double out;
			svt_rule_coerce(from_hex(a), &out);
			printf("%016llx\n", svt_coerce_bits(out));
		} else if (!strcmp(op, "movei")) {
			int32_t out;
			svt_rule_coerce((int32_t) ia, &out);
			printf("%d\n", out);
		} else if (!strcmp(op, "bgd")) {
			double out;
			svt_rule_background(ia != 0, &out);
			printf("%016llx\n", svt_coerce_bits(out));
		} else if (!strcmp(op, "bgi")) {
			int32_t out;
			svt_rule_background(ia != 0, &out);
			printf("%d\n", out);
		} else if (!strcmp(op, "status")) {
			printf("%d\n", svt_rule_coerce_status(ia, ib));
		} else {
			printf("?\n");
		}
	}
	return 0;
}
