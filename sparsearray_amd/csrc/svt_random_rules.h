// The rules of the random count arrays (C_poissonSparseArray and C_simple_rpois, src/randomSparseArray.c of the
// reference), each stated once for the device kernels (kernels_coerce.hip) and for a host program
// (tests/random_rules_main.cpp): plain C++, no HIP header needed.
//
// The reference draws its uniforms from R's global stream, one after the other.  Here the value of a cell is a pure
// function of (seed, flat cell index): a counter-based generator turns the pair into a uniform, the reference's table of
// cumulated Poisson probabilities turns the uniform into the value.  So an array does not depend on how it is tiled, on
// the grid, or on the window of leaves a call asks for, and no state is carried from one cell to the next.
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define SVT_RANDOM_HD __host__ __device__
#else
#define SVT_RANDOM_HD
#endif

#define SVT_POISSON_MAX_TICKS 32        // CUMSUM_DPOIS_MAX_LENGTH: enough for 0 <= lambda <= 4

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011)
#define SVT_PHILOX_M0 0xD2511F53u
#define SVT_PHILOX_M1 0xCD9E8D57u
#define SVT_PHILOX_W0 0x9E3779B9u
#define SVT_PHILOX_W1 0xBB67AE85u

struct svt_philox_words {
	uint32_t w[4];
};

SVT_RANDOM_HD inline svt_philox_words svt_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
							 uint32_t k1)
{
#pragma unroll
	for (int r = 0; r < 10; r++) {
		const uint64_t p0 = (uint64_t) SVT_PHILOX_M0 * c0, p1 = (uint64_t) SVT_PHILOX_M1 * c2;
		const uint32_t n0 = (uint32_t) (p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t) (p0 >> 32) ^ c3 ^ k1;
		c1 = (uint32_t) p1;
		c3 = (uint32_t) p0;
		c0 = n0;
		c2 = n2;
		k0 += SVT_PHILOX_W0;
		k1 += SVT_PHILOX_W1;
	}
	svt_philox_words out = { { c0, c1, c2, c3 } };
	return out;
}

// The Philox block of a pair of cells: block = cell >> 1 is the counter's low two words, the seed is the key.  Counter
// words 2 and 3 stay zero (reserved for a later value stream).
SVT_RANDOM_HD inline svt_philox_words svt_rule_cell_block(uint64_t seed, uint64_t block)
{
	return svt_philox4x32_10((uint32_t) block, (uint32_t) (block >> 32), 0u, 0u, (uint32_t) seed, (uint32_t) (seed >> 32));
}
// two output words -> the uniform in [0, 1): the top 53 bits of hi:lo, exact in a double
SVT_RANDOM_HD inline double svt_rule_uniform(uint32_t w_lo, uint32_t w_hi)
{
	const uint64_t x = (uint64_t) w_hi << 32 | w_lo;
	return (double) (x >> 11) * 0x1p-53;
}
// the even cell of a block takes the words (w0, w1), the odd cell (w2, w3)
SVT_RANDOM_HD inline double svt_rule_block_uniform(const svt_philox_words &b, int odd)
{
	return odd ? svt_rule_uniform(b.w[2], b.w[3]) : svt_rule_uniform(b.w[0], b.w[1]);
}
SVT_RANDOM_HD inline double svt_rule_cell_uniform(uint64_t seed, uint64_t cell)
{
	return svt_rule_block_uniform(svt_rule_cell_block(seed, cell >> 1), (int) (cell & 1));
}

// The table a kernel gets by value: the cumulated probabilities P(X <= k), k < n, ascending.
struct svt_poisson_table {
	double ticks[SVT_POISSON_MAX_TICKS];
	int n;
};

// find_interval (src/randomSparseArray.c:81-89): the first k with u < ticks[k], or n when there is none
SVT_RANDOM_HD inline int svt_rule_find_interval(double u, const svt_poisson_table &t)
{
	int k;
	for (k = 0; k < t.n; k++)
		if (u < t.ticks[k])
			break;
	return k;
}
// find_interval(u) != 0, which is all the count pass asks: one comparison
SVT_RANDOM_HD inline bool svt_rule_poisson_nonzero(double u, const svt_poisson_table &t)
{
	return t.n > 0 && !(u < t.ticks[0]);
}
SVT_RANDOM_HD inline int32_t svt_rule_poisson_cell(uint64_t seed, uint64_t cell, const svt_poisson_table &t)
{
	return (int32_t) svt_rule_find_interval(svt_rule_cell_uniform(seed, cell), t);
}

// compute_cumsum_dpois (src/randomSparseArray.c:19-38), host only, in long double as the reference does.  Two sums run
// side by side.  `ref` is the reference's own arithmetic -- the first term its double exp(), lambda / n its double
// quotient -- and decides, by the reference's tests, when every cell is 0 and where the table ends: the number of ticks
// is the reference's for every lambda (18 at lambda = 1, where a sum without those two roundings goes on to 19).  But those
// roundings put the reference's ticks 0.7 ulp from the true CDF at lambda = 1, 2.1 at 3.3 and 1.6 at 4, so the tick that
// is stored comes from `acc`, the same sum with the first term and the quotients in long double: the true CDF rounded
// once, within 0.5 ulp.  The stored ticks ascend; two may be equal where `ref` runs one term past what a double resolves,
// and find_interval then never answers the first of them.  Returns the number of ticks: 0 when every cell is 0, -1 when
// SVT_POISSON_MAX_TICKS are not enough ("'lambda' too big?") or lambda is negative, NaN or infinite.
inline int svt_rule_poisson_ticks(double lambda, double *ticks)
{
	if (!(lambda >= 0.0) || lambda > 1.7976931348623157e308)
		return -1;
	long double ref, ref_dp, acc, acc_dp;
	ref = ref_dp = exp(-lambda);
	if (ref >= 1.0)
		return 0;
	acc = acc_dp = expl(-(long double) lambda);
	double ref_last = (double) ref;
	ticks[0] = (double) acc;
	for (int n = 1; n < SVT_POISSON_MAX_TICKS; n++) {
		ref_dp *= lambda / n;
		ref += ref_dp;
		if ((double) ref == ref_last)
			return n;
		ref_last = (double) ref;
		acc_dp *= (long double) lambda / n;
		acc += acc_dp;
		ticks[n] = (double) acc;
	}
	return -1;
}
