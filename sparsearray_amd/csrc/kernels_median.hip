// colMedians, colQuantiles and colMads of an SVT_SparseMatrix on the CSC device layout: one counting kernel, one select
// kernel, and a rule per statistic (MedianRule, QuantileRule, MadRule) that says which value a stored element stands for,
// which ranks of a column are wanted and how the two values found there become the result.
//
// colMedians.  Reference: pure R, one leaf at a time (.colMedians_SVT_SparseMatrix /
// .padded_median / .positive_padded_median, R/SparseArray-matrixStats.R:690-784;
// its own TODO asks for a C version behind C_colStats_SVT).  .padded_median(x,
// padding) is "median(c(x, integer(padding)))" without realising the zeros: the
// n = length(x) + padding values are order statistics of [negatives | zeros |
// positives], the median is the middle one or the mean of the two middle ones.
// NA rule (:714-719): na.rm drops NA/NaN from the nonzeros (the padding keeps its
// size); otherwise any NA/NaN gives NA_real_.  n == 0 gives NA_real_ (:721-722).
//
// colQuantiles(x, probs, na.rm, type = 7): base R's quantile.default type 7 of each column's nrow values, the
// implicit zeros included.  The reference has no method (R/SparseArray-matrixStats.R:5-12 lists it among the
// ones to add).  With the n values left after the NA rule sorted ascending as x[1..n], in IEEE double exactly as written:
//     index = 1 + (n - 1) * p;  lo = floor(index);  hi = ceiling(index);  q = x[lo]
//     if (index > lo && x[hi] != x[lo]) { h = index - lo;  q = (1 - h) * x[lo] + h * x[hi] }
// NA rule as colMedians.  Result: out[j + q * ncol], ncol x nprobs column-major.
// The median is NOT the quantile at 0.5: (x[lo] + x[hi]) * 0.5 and 0.5 * x[lo] + 0.5 * x[hi] differ near overflow and
// on subnormals, so the finishing arithmetic belongs to the rule.
//
// Device (no library sort): a column asks for one or several REQUESTS, each a pair of ranks in the virtual sorted column
// and a weight.  ONE counting pass whatever the number of requests (one wavefront per column) finds the negatives,
// positives and NA/NaN among the stored values and, for a rule that asks for them, the smallest and largest nonzero
// stored value.  Most requests on a sparse matrix are decided there: the median is 0 when the middle ranks fall among
// the zeros (fewer than half of the column's values positive, fewer than half negative), a quantile is known when its
// ranks fall among the zeros or on the recorded extremes.  For the rest ONE select launch, a workgroup per undecided
// column, walks the column's requests (the column stays in the L2 between them) and SELECTS the one or two order
// statistics of each from the column where it lies -- a most-significant-digit-first radix select over the
// order-preserving 64-bit image of the doubles (digits of 11, 11, 11, 11, 10, 10 bits:
// counting passes over the column with a histogram in LDS until the bin of the wanted rank
// holds at most 1024 keys, which are then collected into LDS and ranked there; the second
// value of a pair comes from the same candidates or is the smallest key above
// their bin).  Nothing is copied and nothing is sorted (rounds 2-4: a key copy + rocprim's
// segmented radix sort of 64-bit keys, eight read + write passes over the values).
// Roofline: HBM; algorithmic bytes = 8 per nonzero for the count pass and typically 3 x 8
// (at most 8 x 8) per nonzero and request of an undecided column (short columns stay in the L2).
// colMads(x, center, constant, na.rm): stats::mad without low / high, stated at MadRule below -- the same two kernels
// over the deviations fabs(x - c), whose block of equal values is fabs(0.0 - c) instead of 0.0.
// Not built: colOrderStats (colRanks is kernels_ranks.hip: a sort per column, not a select), quantile types other than 7, the low / high medians of mad, N-d operands,
// NaArray operands.
#include "svt_common.h"

#include <string.h>

#define MSEL_NT 256
#define MSEL_BINS 2048
#define MSEL_CAND 1024        // candidates finished in LDS

// val[beg, end) walked by W threads, of which the caller is number t, four loads per thread in flight (one wavefront per
// column with a single load each kept 16 KB per CU on the way, 3.1 TB/s; and a long column is selected by ONE
// workgroup): f(d) for every element, decoded to double -- an integer NA is NaN.  The last round also hands over its
// slots past `end`, as 0.0: a stored zero, which counts among the zeros and is skipped by every caller (a guard here
// instead costs order_select_kernel<MedianRule> 5 SGPRs and with them one wavefront per SIMD).
template <int W, typename T, class F>
__device__ __forceinline__ void walk_column(const T *__restrict__ val, int64_t beg, int64_t end, int t, F &&f)
{
	for (int64_t k0 = beg; k0 < end; k0 += 4 * W) {
		T raw[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int64_t k = k0 + u * W + t;
			raw[u] = k < end ? val[k] : (T) 0;
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			double d;
			if (sizeof(T) == 8) d = (double) raw[u];
			else { const int v = (int) raw[u]; d = v == NA_INT ? NAN : (double) v; }
			f(d);
		}
	}
}

// ---- radix select -----------------------------------------------------------------------------------
// What a rule's kernels take beyond the operand, and its view of one column: the value a stored d stands for in the
// order statistics and the value of the BLOCK, the run of equal values in the sorted column that holds the implicit
// zeros.  The median and the quantiles take d itself and a block of zeros; nothing is passed and nothing is kept.
struct NoParams {};
struct IdentityKey {
	__device__ IdentityKey(const NoParams &, int64_t) {}
	__device__ double operator()(double d) const { return d; }
	__device__ static constexpr double block() { return 0.0; }
};

template <class X>
__device__ __forceinline__ bool msel_key(const X &xf, double d, unsigned long long *key)
{
	const double t = xf(d);
	if (t != t || t == xf.block())
		return false;                            // NA / NaN, and a value of the block (a stored zero is one)
	*key = f64_to_ordered(t);
	return true;
}

// Block-wide exclusive prefix of one count per thread (MSEL_NT threads); returns the thread's prefix, *total
// = the sum.  wsum: 4 words of LDS.
__device__ inline unsigned msel_block_scan(unsigned x, unsigned *wsum, unsigned *total)
{
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	unsigned incl = x;
	for (int o = 1; o < 64; o <<= 1) {
		const unsigned t = __shfl_up(incl, o, 64);
		if (lane >= o) incl += t;
	}
	if (lane == 63) wsum[w] = incl;
	__syncthreads();
	unsigned before = 0, all = 0;
	for (int i = 0; i < MSEL_NT / 64; i++) {
		const unsigned t = wsum[i];
		if (i < w) before += t;
		all += t;
	}
	__syncthreads();
	*total = all;
	return before + incl - x;
}

// Block-wide minimum of one 64-bit key per thread (MSEL_NT threads).  slot: MSEL_NT / 64 words of LDS.
__device__ inline unsigned long long msel_block_min(unsigned long long x, unsigned long long *slot)
{
	for (int o = 32; o > 0; o >>= 1) {
		const unsigned long long t = __shfl_down(x, o, 64);
		x = t < x ? t : x;
	}
	if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = x;
	__syncthreads();
	x = ~0ull;
	for (int i = 0; i < MSEL_NT / 64; i++)
		x = slot[i] < x ? slot[i] : x;
	__syncthreads();
	return x;
}

// Rank r of the virtual column [neg values below the block | zeros values of the block | values above] -> rank among
// the stored non-NA values outside the block, or -1 for "a value of the block".
__device__ inline int64_t msel_rank(int64_t r, int64_t neg, int64_t zeros)
{
	return r < neg ? r : r < neg + zeros ? -1 : r - zeros;
}

// The keys of ranks k and k + 1 (0-based, ascending) among the NONZERO, non-NA values of val[beg, end) -- *key1 only when
// want_next (the caller knows that rank k + 1 exists).  Counting passes, most significant digit first (11, 11, 11, 11,
// 10, 10 bits), until the bin that holds rank k has at most MSEL_CAND keys; those are then collected into LDS in one more
// pass over the column (which also finds the smallest key ABOVE the bin, for rank k + 1 when k is the bin's last) and
// ranked there.  Doubles of one sign and exponent differ in their mantissa: two counting passes (22 bits) leave
// n / 1024 candidates of a column of n values -- three passes over the column instead of seven.
// Called by all MSEL_NT threads of the workgroup with the same arguments.  Returns false when the keys never got few
// enough (more than MSEL_CAND equal keys): *key0 is exact after the six passes, *key1 is then left to the caller.
template <typename T, class X>
__device__ bool msel_select(const X &xf, const T *__restrict__ val, int64_t beg, int64_t end, unsigned k, bool want_next,
			    unsigned *hist, unsigned *wsum, unsigned *found, unsigned long long *red,
			    unsigned long long *cand, unsigned long long *key0, unsigned long long *key1)
{
	unsigned long long prefix = 0;
	int shift = 64;
	for (int pass = 0; pass < 6; pass++) {
		const int w = pass < 4 ? 11 : 10;
		const int hi_shift = shift;              // bits [hi_shift, 64) of the key are fixed by `prefix`
		shift -= w;
		const unsigned nb = 1u << w, mask = nb - 1;
		for (unsigned i = threadIdx.x; i < nb; i += MSEL_NT) hist[i] = 0;
		__syncthreads();
		walk_column<MSEL_NT>(val, beg, end, threadIdx.x, [&](double d) {
			unsigned long long key;
			if (msel_key(xf, d, &key) && (pass == 0 || (key >> hi_shift) == (prefix >> hi_shift)))
				atomicAdd(&hist[(unsigned) (key >> shift) & mask], 1u);
		});
		__syncthreads();
		// the digit whose bin holds rank k: a thread owns nb / MSEL_NT consecutive bins
		const unsigned per = nb / MSEL_NT, b0 = threadIdx.x * per;
		unsigned mine = 0;
		for (unsigned i = 0; i < per; i++) mine += hist[b0 + i];
		unsigned total;
		const unsigned before = msel_block_scan(mine, wsum, &total);
		if (k >= before && k < before + mine) {
			unsigned run = before;
			for (unsigned i = 0; i < per; i++) {
				const unsigned c = hist[b0 + i];
				if (k < run + c) { found[0] = b0 + i; found[1] = run; found[2] = c; break; }
				run += c;
			}
		}
		__syncthreads();
		prefix |= (unsigned long long) found[0] << shift;
		k -= found[1];
		const unsigned ncand = found[2];
		__syncthreads();
		if (ncand <= MSEL_CAND && shift > 0) {
			// collect the bin's keys (bits [shift, 64) equal to the prefix) and the smallest key above the bin
			if (threadIdx.x == 0) found[3] = 0;
			__syncthreads();
			unsigned long long above = ~0ull;
			walk_column<MSEL_NT>(val, beg, end, threadIdx.x, [&](double d) {
				unsigned long long key;
				if (!msel_key(xf, d, &key))
					return;
				const unsigned long long hi = key >> shift, want = prefix >> shift;
				if (hi == want) cand[atomicAdd(&found[3], 1u)] = key;
				else if (hi > want && key < above) above = key;
			});
			if (want_next)
				above = msel_block_min(above, red);
			// rank the candidates: cand[i] is the key of local rank k iff (keys below it) <= k < (keys below or equal)
			if (threadIdx.x == 0) { found[0] = 0; found[1] = 0; }
			__syncthreads();
			unsigned long long *res = (unsigned long long *) (hist + 64);       // [0] key of rank k, [1] of rank k + 1
			for (unsigned i = threadIdx.x; i < ncand; i += MSEL_NT) {
				const unsigned long long mk = cand[i];
				unsigned lt = 0, le = 0;
				for (unsigned jx = 0; jx < ncand; jx++) {
					const unsigned long long o = cand[jx];
					lt += o < mk; le += o <= mk;
				}
				if (lt <= k && k < le) res[0] = mk;                     // (equal keys write the same value)
				if (lt <= k + 1 && k + 1 < le) { res[1] = mk; found[1] = 1; }
			}
			__syncthreads();
			*key0 = res[0];
			*key1 = found[1] ? res[1] : above;      // rank k + 1 past the bin's last key: the smallest key above the bin
			__syncthreads();
			return true;
		}
	}
	*key0 = prefix;
	*key1 = 0;
	return false;
}

// The values of ranks klo and khi (0-based, ascending) among the non-NA values of val[beg, end) outside the block, as
// xf sees them; a rank of -1 stands for "a value of the block" (xf.block()).  khi is klo, klo + 1, or -1; at least one of the two is >= 0.  Called by all
// MSEL_NT threads of the workgroup with the same arguments.  red: MSEL_NT / 64 words of LDS.
template <typename T, class X>
__device__ inline void msel_two(const X &xf, const T *__restrict__ val, int64_t beg, int64_t end, int64_t klo, int64_t khi,
				unsigned *hist, unsigned *wsum, unsigned *found, unsigned long long *red,
				unsigned long long *cand, double *out_lo, double *out_hi)
{
	double vlo = xf.block(), vhi = xf.block();
	unsigned long long key_lo = 0, key_next = 0;
	bool have_next = false;
	if (klo >= 0) {
		have_next = msel_select<T>(xf, val, beg, end, (unsigned) klo, khi == klo + 1, hist, wsum, found, red, cand, &key_lo,
					   &key_next);
		vlo = ordered_to_f64(key_lo);
	}
	if (khi < 0) {
		vhi = xf.block();
	} else if (khi == klo) {
		vhi = vlo;
	} else if (klo >= 0 && have_next) {
		vhi = ordered_to_f64(key_next);          // (both ranks from the same candidates)
	} else if (klo >= 0) {
		// khi == klo + 1: the same key again if ranks <= klo + 1 are all covered by keys <= key_lo, else the
		// smallest key above it.  One pass: count of keys <= key_lo (a column has fewer than 2^31), minimum of the keys > key_lo.
		unsigned mine = 0, cnt;
		unsigned long long nxt = ~0ull;
		walk_column<MSEL_NT>(val, beg, end, threadIdx.x, [&](double d) {
			unsigned long long key;
			if (!msel_key(xf, d, &key))
				return;
			if (key <= key_lo) mine++;
			else if (key < nxt) nxt = key;
		});
		(void) msel_block_scan(mine, wsum, &cnt);
		nxt = msel_block_min(nxt, red);
		vhi = (int64_t) cnt > khi ? vlo : ordered_to_f64(nxt);
	} else {
		unsigned long long key_hi = 0, unused = 0;
		(void) msel_select<T>(xf, val, beg, end, (unsigned) khi, false, hist, wsum, found, red, cand, &key_hi, &unused);
		vhi = ordered_to_f64(key_hi);
	}
	*out_lo = vlo; *out_hi = vhi;
}

// ---- the two statistics -------------------------------------------------------------------------------
// One request of a column: its two 0-based ranks, mapped by msel_rank(), and the weight its rule's finish() reads.
struct RankPair { int64_t klo, khi; double h; };

// The pair of prob p in a column of n values; h = index - lo (0: no interpolation).
__device__ inline RankPair quant_pair(int64_t n, int64_t neg, int64_t zeros, double p)
{
#pragma clang fp contract(off)       // index is a product and a sum, each rounded on its own (the library builds with
	                             // -ffp-contract=off as well; hipcc's default would fuse them)
	const double prod = (double) (n - 1) * p;
	const double index = 1.0 + prod;
	const double fl = floor(index), ce = ceil(index);
	RankPair r;
	r.klo = msel_rank((int64_t) fl - 1, neg, zeros);
	r.khi = msel_rank((int64_t) ce - 1, neg, zeros);
	r.h = index - fl;
	return r;
}

// The value of rank k (msel_rank) when no select is needed: a zero (blk), or the smallest / largest of the nz nonzero
// values.
__device__ inline bool quant_known(int64_t k, int64_t nz, double vmin, double vmax, double blk, double *v)
{
	if (k < 0) { *v = blk; return true; }
	if (k == 0) { *v = vmin; return true; }
	if (k == nz - 1) { *v = vmax; return true; }
	return false;
}

__device__ inline double quant_value(double vlo, double vhi, double h)
{
#pragma clang fp contract(off)       // two products and one sum, each rounded on its own: no FMA
	if (!(h > 0.0) || vhi == vlo)
		return vlo;                      // (two equal neighbours give that value, infinities included)
	const double a = (1.0 - h) * vlo;
	const double b = h * vhi;
	return a + b;                            // (-Inf and +Inf as neighbours: NaN)
}

// A rule: what its kernels take beyond the operand (Params) and its view of a column (Key: the value a stored d stands
// for, and the block's value); whether the counting pass records the extremes of the nonzero values; whether the key is
// a transform of d, so that a deviation can be NaN where d is not and a column can be answered before it is walked;
// the requests of a column of n values (neg below the block, then `zeros` in it); which rank needs no select, and its
// value; the result from the two values of a pair; where the result of column j, request q goes.
struct MedianRule {
	using Params = NoParams;
	using Key = IdentityKey;
	static constexpr bool extremes = false;
	static constexpr bool transformed = false;
	static constexpr const char *name = "colMedians";
	__host__ __device__ static int nreq(int) { return 1; }
	// the middle value, or the two middle ones (h = 0.5) when n is even
	__device__ static RankPair request(int64_t n, int64_t neg, int64_t zeros, const double *, int)
	{
		return { msel_rank((n - 1) >> 1, neg, zeros), msel_rank(n >> 1, neg, zeros), (n & 1) ? 0.0 : 0.5 };
	}
	__device__ static bool known(int64_t k, int64_t, double, double, double blk, double *v) { *v = blk; return k < 0; }
	__device__ static double finish(const Params &, double vlo, double vhi, double h)
	{
		return h == 0.0 ? vlo : (vlo + vhi) * 0.5;       // (:707 mean of the two, :757)
	}
	__device__ static int64_t index(int64_t j, int, int64_t) { return j; }
};
struct QuantileRule {
	using Params = NoParams;
	using Key = IdentityKey;
	static constexpr bool extremes = true;          // ranks 1 and n need no select
	static constexpr bool transformed = false;
	static constexpr const char *name = "colQuantiles";
	__host__ __device__ static int nreq(int nprobs) { return nprobs; }
	__device__ static RankPair request(int64_t n, int64_t neg, int64_t zeros, const double *probs, int q)
	{
		return quant_pair(n, neg, zeros, probs[q]);
	}
	__device__ static bool known(int64_t k, int64_t nz, double vmin, double vmax, double blk, double *v)
	{
		return quant_known(k, nz, vmin, vmax, blk, v);
	}
	__device__ static double finish(const Params &, double vlo, double vhi, double h) { return quant_value(vlo, vhi, h); }
	__device__ static int64_t index(int64_t j, int q, int64_t ncol) { return j + (int64_t) q * ncol; }
};

// colMads(x, center, constant, na.rm): stats::mad without low / high on each column's nrow values.  With c the column's
// center (given, or its median by MedianRule) every value x becomes the deviation t = fabs(x - c), one subtraction; the
// stored and the implicit zeros all become b = fabs(0.0 - c), the block.  With below = #{t < b} and above = #{t > b}
// over the stored non-missing values the sorted deviations are [below | n - below - above values equal to b | above]:
// the median's request on (n, below, block), the select's keys are the t of stored values with t != b (a stored zero, a
// stored 2c and the walk's slots past the end fall into the block by themselves).  Result: constant * M, one product.
// NA_real_: the median's NA rule; c NA or NaN; any deviation NaN where x is not missing (x and c the same infinity),
// also under na.rm -- stats::mad takes the median of the deviations without na.rm.
struct MadParams {
	const double *center;                   // one per column
	double constant;
	const int64_t *mneg, *mpos, *mnan;      // the median's counts when `center` holds its medians, else NULL
};
struct MadKey {
	double c, b;
	__device__ MadKey(const MadParams &p, int64_t j) : c(p.center[j]) { b = fabs(0.0 - c); }
	__device__ double operator()(double d) const { return fabs(d - c); }
	__device__ double block() const { return b; }
};
struct MadRule {
	using Params = MadParams;
	using Key = MadKey;
	static constexpr bool extremes = false;
	static constexpr bool transformed = true;
	static constexpr const char *name = "colMads";
	__host__ __device__ static int nreq(int) { return 1; }
	__device__ static RankPair request(int64_t n, int64_t below, int64_t block, const double *, int)
	{
		return MedianRule::request(n, below, block, NULL, 0);
	}
	__device__ static bool known(int64_t k, int64_t, double, double, double blk, double *v) { *v = blk; return k < 0; }
	__device__ static double finish(const Params &p, double vlo, double vhi, double h)
	{
#pragma clang fp contract(off)       // the median's sum and product, then one product, each rounded on its own
		const double m = MedianRule::finish(NoParams(), vlo, vhi, h);
		return p.constant * m;
	}
	__device__ static int64_t index(int64_t j, int, int64_t) { return j; }
	// What is known of column j before its values are read.  A center that is NA / NaN gives NA_real_ (the median's
	// own NA rule arrives this way when the centers are its medians).  When they are, its counts are at hand: a median
	// of 0 with more zeros than n >> 1 means that the sorted |x| has zeros at both middle ranks, M = 0 -- the sparse
	// case, which is then one walk of the values (the median's), not two.
	__device__ static bool before_walk(const Params &p, const Key &xf, int64_t j, int64_t nrow, double *res)
	{
		if (xf.c != xf.c) { *res = svt_na_real(); return true; }
		if (p.mneg == NULL || xf.c != 0.0)
			return false;
		const int64_t n = nrow - p.mnan[j], zeros = n - p.mneg[j] - p.mpos[j];  // (a column with NA and no na.rm: c is NA)
		if ((n >> 1) >= zeros)
			return false;
		*res = finish(p, 0.0, 0.0, 0.0);
		return true;
	}
};

// What the counting pass leaves per column to the select pass: [below the block][above it][NA / NaN], with `extremes`
// [smallest nonzero][largest nonzero], then [undecided flag]; 256-byte aligned inside ws.
struct OrderWs {
	int64_t *neg, *pos, *nan;
	double *vmin, *vmax;        // NULL without extremes
	int *todo;
	uintptr_t end;
	static OrderWs carve(void *ws, int64_t ncol, bool extremes)
	{
		uintptr_t p = ((uintptr_t) ws + 255) & ~(uintptr_t) 255;
		auto take = [&](size_t elt) { const uintptr_t q = p; p += elt * (size_t) ncol; return q; };
		OrderWs w;
		w.neg = (int64_t *) take(8); w.pos = (int64_t *) take(8); w.nan = (int64_t *) take(8);
		w.vmin = extremes ? (double *) take(8) : NULL; w.vmax = extremes ? (double *) take(8) : NULL;
		w.todo = (int *) take(4);
		w.end = p;
		return w;
	}
	static size_t bytes(int64_t ncol, bool extremes)        // (carved at 0, plus room for the alignment)
	{
		return (size_t) carve(NULL, ncol > 0 ? ncol : 1, extremes).end + 1024;
	}
};

// One wavefront per column: the stored values below the block, above it and NA/NaN, and (R::extremes) the extremes among
// the nonzero non-NA stored values.  Writes every request that needs no select (NA rule, empty column, ranks that
// R::known() answers); todo[j] = 1 when a request of the column is left to order_select_kernel.  colMedians at BASELINE
// config 2 is this pass alone -- every median is a zero; colMads there is the median's pass and R::before_walk().
template <class R, typename T>
__global__ void __launch_bounds__(256)
order_count_kernel(const int64_t *__restrict__ col_ptr, const T *__restrict__ val, int64_t nrow, int64_t ncol, int na_rm,
		   const double *__restrict__ probs, int nprobs, double *__restrict__ out, OrderWs w,
		   const typename R::Params prm)
{
	const int lane = threadIdx.x & 63;
	const int64_t j = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
	if (j >= ncol) return;
	const typename R::Key xf(prm, j);
	if constexpr (R::transformed) {
		double res;
		if (R::before_walk(prm, xf, j, nrow, &res)) {    // (the same answer in every lane)
			if (lane == 0) { out[R::index(j, 0, ncol)] = res; w.todo[j] = 0; }
			return;
		}
	}
	const int64_t beg = col_ptr[j], end = col_ptr[j + 1];
	long long neg = 0, pos = 0, nan = 0, bad = 0;
	double mn = INFINITY, mx = -INFINITY;
	walk_column<64>(val, beg, end, lane, [&](double d) {
		const double t = xf(d);
		nan += d != d; neg += t < xf.block(); pos += t > xf.block();    // (a stored zero counts among the block)
		if constexpr (R::transformed)
			bad += t != t;                           // (every missing d, and a d that is the center's infinity)
		if constexpr (R::extremes)
			if (d != 0.0) { mn = d < mn ? d : mn; mx = d > mx ? d : mx; }   // (NaN fails both comparisons)
	});
	neg = wave_sum_ll(neg); pos = wave_sum_ll(pos); nan = wave_sum_ll(nan);
	neg = __shfl(neg, 0, 64); pos = __shfl(pos, 0, 64); nan = __shfl(nan, 0, 64);
	if constexpr (R::transformed) { bad = wave_sum_ll(bad); bad = __shfl(bad, 0, 64); }
	if constexpr (R::extremes) {
		mn = __shfl(wave_min(mn), 0, 64); mx = __shfl(wave_max(mx), 0, 64);
	}
	const int64_t len = end - beg, v = len - nan, padding = nrow - len, n = v + padding;
	const int64_t nz = neg + pos, zeros = n - nz;            // the block: stored + implicit zeros (and their equals)
	const bool all_na = (!na_rm && nan > 0) || n == 0 || (R::transformed && bad > nan);
	int undecided = 0;
	for (int q = lane; q < R::nreq(nprobs); q += 64) {       // (the requests of a column are dealt over the lanes)
		double res;
		if (all_na) {
			res = svt_na_real();
		} else {
			const RankPair pr = R::request(n, neg, zeros, probs, q);
			double vlo, vhi;
			const bool klo_known = R::known(pr.klo, nz, mn, mx, xf.block(), &vlo);
			const bool khi_known = R::known(pr.khi, nz, mn, mx, xf.block(), &vhi);
			if (!klo_known || !khi_known) { undecided = 1; continue; }
			res = R::finish(prm, vlo, vhi, pr.h);
		}
		out[R::index(j, q, ncol)] = res;
	}
	undecided = wave_or(undecided);
	if (lane != 0) return;
	w.neg[j] = neg; w.pos[j] = pos; w.nan[j] = nan; w.todo[j] = undecided;
	if constexpr (R::extremes) { w.vmin[j] = mn; w.vmax[j] = mx; }
}

// One workgroup per undecided column (grid-stride over the columns): the requests order_count_kernel left, one after
// the other.  The virtual sorted column is [below | z values of the block | above]; rank r < neg is the r-th smallest
// stored value, rank r >= neg + z the (r - z)-th smallest stored value OUTSIDE the block.
template <class R, typename T>
__global__ void __launch_bounds__(MSEL_NT)
order_select_kernel(const int64_t *__restrict__ col_ptr, const T *__restrict__ val, int64_t nrow, int64_t ncol,
		    const double *__restrict__ probs, int nprobs, OrderWs w, double *__restrict__ out,
		    const typename R::Params prm)
{
	__shared__ __attribute__((aligned(16))) unsigned hist[MSEL_BINS];      // (also read as 64-bit words by msel_select)
	__shared__ unsigned wsum[MSEL_NT / 64];
	__shared__ unsigned found[4];
	__shared__ unsigned long long red[MSEL_NT / 64];
	__shared__ unsigned long long cand[MSEL_CAND];
	for (int64_t j = blockIdx.x; j < ncol; j += gridDim.x) {
		if (!w.todo[j])
			continue;                                // (the same answer in every thread)
		const typename R::Key xf(prm, j);
		const int64_t beg = col_ptr[j], end = col_ptr[j + 1];
		const int64_t neg = w.neg[j], nz = neg + w.pos[j];       // non-NA stored values outside the block
		// (columns holding NA / NaN come here only under na.rm: those entries are dropped, the padding keeps its size)
		const int64_t n = nrow - w.nan[j], zeros = n - nz;       // the block: implicit zeros + stored ones
		double mn = 0.0, mx = 0.0;
		if constexpr (R::extremes) { mn = w.vmin[j]; mx = w.vmax[j]; }
		for (int q = 0; q < R::nreq(nprobs); q++) {
			const RankPair pr = R::request(n, neg, zeros, probs, q);
			double vlo, vhi;
			const bool klo_known = R::known(pr.klo, nz, mn, mx, xf.block(), &vlo);
			const bool khi_known = R::known(pr.khi, nz, mn, mx, xf.block(), &vhi);
			if (klo_known && khi_known)
				continue;                        // written by order_count_kernel
			double a, b;
			msel_two<T>(xf, val, beg, end, klo_known ? -1 : pr.klo, khi_known ? -1 : pr.khi, hist, wsum, found, red,
				    cand, &a, &b);
			if (!klo_known) vlo = a;
			if (!khi_known) vhi = b;
			if (threadIdx.x == 0)
				out[R::index(j, q, ncol)] = R::finish(prm, vlo, vhi, pr.h);
		}
	}
}

template <class R>
static int launch_order_rule(const int64_t *col_ptr, const void *val, int Rtype, int64_t nrow, int64_t ncol, int64_t nnz,
			     const double *probs, int nprobs, const typename R::Params &prm, int na_rm, double *out,
			     void *ws, hipStream_t s)
{
	if (ncol <= 0 || R::nreq(nprobs) <= 0)
		return 0;
	// (positions and counts are 64-bit throughout; ranks inside a column are < nrow < 2^31, so msel_select's 32-bit
	// ranks and LDS counters hold any column -- the operand's total count is not limited)
	if (ncol > 0x7FFFFFFFLL)
		return svt_set_unsupported("%s: more than 2^31-1 columns", R::name);
	const OrderWs w = OrderWs::carve(ws, ncol, R::extremes);
	const unsigned nbc = (unsigned) ((ncol + 3) / 4);
	// the undecided columns, one workgroup each, a few rounds of them in flight
	const unsigned nbs = (unsigned) (ncol < 4096 ? ncol : 4096);
	svt_by_rtype(Rtype, val, NULL, [&](auto *v, auto *) {          // (the kernels deduce T from v)
		hipLaunchKernelGGL(order_count_kernel<R>, dim3(nbc), dim3(256), 0, s, col_ptr, v, nrow, ncol, na_rm, probs,
				   nprobs, out, w, prm);
		if (nnz > 0)
			hipLaunchKernelGGL(order_select_kernel<R>, dim3(nbs), dim3(MSEL_NT), 0, s, col_ptr, v, nrow, ncol,
					   probs, nprobs, w, out, prm);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

// colMads in its workspace: [the median's OrderWs][the deviations' OrderWs][ncol centers], each 256-byte aligned.
// Without a given center the median's two kernels write the centers, and their counts serve MadRule::before_walk().
static int launch_mads(const int64_t *col_ptr, const void *val, int Rtype, int64_t nrow, int64_t ncol, int64_t nnz,
		       const double *center, double constant, int na_rm, double *out, void *ws, hipStream_t s)
{
	if (ncol <= 0)
		return 0;
	const OrderWs wm = OrderWs::carve(ws, ncol, MedianRule::extremes);
	const OrderWs wd = OrderWs::carve((void *) wm.end, ncol, MadRule::extremes);
	MadParams prm = { center, constant, NULL, NULL, NULL };
	if (center == NULL) {
		double *med = (double *) ((wd.end + 255) & ~(uintptr_t) 255);
		if (launch_order_rule<MedianRule>(col_ptr, val, Rtype, nrow, ncol, nnz, NULL, 0, NoParams(), na_rm, med, ws, s))
			return -1;
		prm.center = med; prm.mneg = wm.neg; prm.mpos = wm.pos; prm.mnan = wm.nan;
	}
	return launch_order_rule<MadRule>(col_ptr, val, Rtype, nrow, ncol, nnz, NULL, 0, prm, na_rm, out, (void *) wm.end, s);
}

size_t order_stat_ws_bytes(int what, int64_t ncol)
{
	if (what == ORDER_MADS)         // two carves without extremes (28 bytes a column each), the centers, three alignments
		return (size_t) (ncol > 0 ? ncol : 1) * 64 + 1024;
	return OrderWs::bytes(ncol, what == ORDER_QUANTILES ? QuantileRule::extremes : MedianRule::extremes);
}

int launch_order_stat(int what, const int64_t *col_ptr, const void *val, int Rtype, int64_t nrow, int64_t ncol,
		      int64_t nnz, const double *vec, int nprobs, double constant, int na_rm, double *out, void *ws,
		      hipStream_t s)
{
	if (what == ORDER_MADS)
		return launch_mads(col_ptr, val, Rtype, nrow, ncol, nnz, vec, constant, na_rm, out, ws, s);
	return what == ORDER_QUANTILES
		? launch_order_rule<QuantileRule>(col_ptr, val, Rtype, nrow, ncol, nnz, vec, nprobs, NoParams(), na_rm, out, ws, s)
		: launch_order_rule<MedianRule>(col_ptr, val, Rtype, nrow, ncol, nnz, vec, nprobs, NoParams(), na_rm, out, ws, s);
}
