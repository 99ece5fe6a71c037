// The element rule of the subassignment by an L-index or M-index (svt_rule_assign_cells,
// sparsearray_amd/csrc/svt_arith_rules.h) on the host: one request per line of standard input, one answer per line of
// standard output (tests/test_zzzzz_lindex_cpu.py builds it with the host compiler and compares the answers with the
// rule as tests/lindex_cases.py states it).  Values travel as the hexadecimal of their bits, 8 digits for an int32 and
// 16 for a double.
//   C <tx> <ty> <in_y> <x bits> <y bits>   ->  <kept 0|1> <result bits>
//       tx, ty: 'i' (int32: integer or logical) or 'd' (double); the result is a double when either side is
#include <stdio.h>
#include <string.h>

#include "../sparsearray_amd/csrc/svt_arith_rules.h"

template <typename T> static T from_bits(unsigned long long u)
{
	T v;
	memcpy(&v, &u, sizeof(T));
	return v;
}
template <typename T> static unsigned long long to_bits(T v)
{
	unsigned long long u = 0;
	memcpy(&u, &v, sizeof(T));
	return u;
}

template <typename TX, typename TY, typename TO>
static void answer(int in_y, unsigned long long x, unsigned long long y)
{
	TO out = (TO) 0;
	const bool kept = svt_rule_assign_cells(in_y != 0, from_bits<TX>(x), from_bits<TY>(y), &out);
	printf("%d %0*llx\n", kept ? 1 : 0, (int) (2 * sizeof(TO)), kept ? to_bits(out) : 0ULL);
}

int main(void)
{
	char what;
	while (scanf(" %c", &what) == 1) {
		char tx, ty;
		int in_y;
		unsigned long long x, y;
		if (what != 'C' || scanf(" %c %c %d %llx %llx", &tx, &ty, &in_y, &x, &y) != 5)
			return 2;
		if (tx == 'i' && ty == 'i') answer<int32_t, int32_t, int32_t>(in_y, x, y);
		else if (tx == 'i' && ty == 'd') answer<int32_t, double, double>(in_y, x, y);
		else if (tx == 'd' && ty == 'i') answer<double, int32_t, double>(in_y, x, y);
		else if (tx == 'd' && ty == 'd') answer<double, double, double>(in_y, x, y);
		else return 2;
	}
	return 0;
}
