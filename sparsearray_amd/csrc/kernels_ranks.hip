// colRanks of an SVT_SparseMatrix on the CSC device layout, in the compact form a sparse matrix allows: one rank per
// stored value and one rank per column for its zeros, which all tie.
//
// The rule: matrixStats::colRanks(x, ties.method) = rank(na.last = "keep", ties.method) of each column's nrow values,
// the implicit zeros included (the reference has no method).  With n the non-missing values of a column (missing: NaN
// or NA for doubles, NA_integer_ for integers and logicals), and for a non-missing value v
//     L = the non-missing values < v (the implicit zeros count when 0 < v),
//     E = the values == v under IEEE == (-0.0, a stored 0.0 and the implicit zeros are one tie group; v counts),
//     "max" L + E, "min" L + 1, "average" (double) (2L + E + 1) * 0.5 (exact), "dense" 1 + the distinct values < v
//     (the zeros are one distinct value if the column holds any);
// +-Inf are ordinary values; a missing value gets NA and is counted in nobody's L or E; there is no na.rm.
// int32 results (NA_integer_) for max / min / dense, doubles (NA_real_, for NaN and NA alike) for average.
//
// Device.  A stored value becomes the key f64_to_ordered(d) of its decoded double, -0.0 folded onto 0.0; a missing one
// the key RK_NA above every value.  Everything a rank needs is then a count over the column's SORTED stored keys:
// Ls = keys below, Es = keys equal (the bounds of the key's tie run), Ds = tie runs below; the z = nrow - length implicit
// zeros are added afterwards (rank_value()), and the rank of the zeros themselves comes from the run of the key of 0.0
// (rank_zero()).  One classification launch deals the columns by stored length over three forms:
//   form 0  length <= RK_F0_MAX: one wavefront per column, several columns per workgroup.  Nothing is sorted: the keys
//           sit in LDS and every element counts Ls, Es (and for "dense" Ds over the first occurrences) by comparing
//           with all of them, length^2 / 64 broadcast LDS reads per lane.  Empty columns are answered by the
//           classification launch itself.
//   form 1  length <= RK_F1_MAX: one workgroup of 1024 threads per column; (key, position) pairs are sorted in LDS by
//           rocprim's block-level radix sort (2, 6 or 12 items per thread by the column's length), the sorted keys stay
//           in LDS (96 KB) next to the running count of tie-run starts (48 KB) and every element finds its run by its
//           neighbours, or by binary search when a neighbour ties.
//   form 2  any length: the long columns' keys are gathered, with a compact column number above them, into one array
//           of 128-bit keys, sorted with the library's own stable LSD sort (svt_sort.h; 8 passes for the key and 1 to 3
//           for the column number), and every element finds its run by lower_bound / upper_bound in its column's
//           segment of the sorted array; "dense" reads an exclusive scan (svt_scan.h) of the run-start flags.
//           Cost: 68 bytes of workspace per long nonzero and about (8 + passes * 56 + 60) bytes of traffic per long
//           nonzero -- a sort, not a select; see DESIGN.md for what else was weighed.
// Launches: memsets of the flag and the list counters, the classification, the scan of the long columns' lengths, one
// launch each for forms 0 and 1, and for form 2 the gather, the sort's launches, (dense) the flags and their scan, and
// the finishing launch.  Nothing is allocated, read back or synchronised: which lists are empty is known on the device
// only, so a launch over an empty list ends at once.  The host sizes the sort by the long nonzeros the workspace was
// made for (and never more than nnz); if the long columns hold more, *flag is set and nothing is written for them.
// Not built: ties.method "first" / "last" / "random" (every implicit zero would need a rank of its own: no compact
// form), colOrderStats, N-d operands, NaArray operands.  Ranks of operands of 2^31 nonzeros or more run through the
// same 64-bit positions but are not tested.
#include "svt_common.h"
#include "svt_scan.h"
#include "svt_sort.h"

#include <type_traits>

#define RK_F0_MAX 256                   // stored values of a form-0 column
#define RK_F0_PER ((RK_F0_MAX + 63) / 64)
#define RK_NT1 1024
#define RK_F1_MAX (RK_NT1 * 12)         // 12 288 stored values: every column of BASELINE config 2 (mean 1e4, sd 100)
#define RK_F1_KEYS_BYTES (RK_F1_MAX * 8)
#define RK_F1_LDS (RK_F1_MAX * 12)      // sorted keys (or the sort's storage) + run-start counts: 147 456 bytes

#define RK_ZERO 0x8000000000000000ULL   // f64_to_ordered(0.0)
#define RK_NA 0xFFFFFFFFFFFFFFFEULL     // above f64_to_ordered(+Inf) = 0xFFF0000000000000
#define RK_PAD 0xFFFFFFFFFFFFFFFFULL    // slots past a column's end: after the missing values
#define RK_LEN_BITS 44                  // packed scan word: [long columns before | their stored values before]
#define RK_LEN_MASK ((1LL << RK_LEN_BITS) - 1)

typedef unsigned long long rk_key;
typedef unsigned __int128 rk_wide;      // [compact long-column number : 64][key : 64]

int ranks_form(int64_t col_nnz)
{
	return col_nnz <= RK_F0_MAX ? 0 : col_nnz <= RK_F1_MAX ? 1 : 2;
}

template <typename T>
__device__ __forceinline__ rk_key rank_key(T raw)
{
	double d;
	if (sizeof(T) == 8) d = (double) raw;
	else { const int v = (int) raw; d = v == NA_INT ? NAN : (double) v; }      // (as walk_column, kernels_median.hip)
	if (d != d)
		return RK_NA;
	unsigned long long u = (unsigned long long) __double_as_longlong(d);
	if ((u << 1) == 0) u = 0;                                                 // -0.0 is 0.0
	return f64_to_ordered(__longlong_as_double((long long) u));
}

// What a column's stored keys say about its zeros: z implicit zeros, neg stored non-missing values below 0, nzs stored
// zeros, dneg distinct values below 0 (read by "dense" only).
struct RankCol { int64_t z, neg, nzs, dneg; };

__device__ __forceinline__ void rank_store(void *out, int64_t idx, int ties, bool na, int64_t L, int64_t E, int64_t D)
{
	if (ties == SVT_TIES_AVERAGE) {
		((double *) out)[idx] = na ? svt_na_real() : (double) (2 * L + E + 1) * 0.5;
	} else {
		const int64_t r = ties == SVT_TIES_MAX ? L + E : ties == SVT_TIES_MIN ? L + 1 : D + 1;
		((int *) out)[idx] = na ? NA_INT : (int) r;                       // (r <= nrow < 2^31)
	}
}

// The rank of a stored value of key k with Ls stored keys below it, Es equal to it and Ds tie runs below it.
__device__ __forceinline__ void rank_value(void *rank_nz, int64_t idx, int ties, rk_key k, int64_t Ls, int64_t Es, int64_t Ds,
					   const RankCol &c)
{
	int64_t L = Ls, E = Es, D = Ds;
	if (k == RK_ZERO) E += c.z;
	else if (k > RK_ZERO) { L += c.z; D += c.z > 0 && c.nzs == 0; }   // (stored zeros are a run among the keys already)
	rank_store(rank_nz, idx, ties, k == RK_NA, L, E, D);
}

// The rank of the column's zeros: NA when it holds none, stored or implicit.
__device__ __forceinline__ void rank_zero(void *zero_rank, int64_t j, int ties, const RankCol &c)
{
	rank_store(zero_rank, j, ties, c.z + c.nzs == 0, c.neg, c.z + c.nzs, c.dneg);
}

// What the classification leaves: the lists of the form-0 and form-1 columns and their lengths cnt[0], cnt[1]; packed[j]
// = (1 << RK_LEN_BITS | length) for a long column and 0 for the others, scanned in place afterwards, so that
// packed[j] = [long columns before j | their stored values], packed[ncol] = the totals.  For L long nonzeros: the
// three (wide key, payload) arrays of the sort, the start and the column of every compact long-column number, the
// run-start flags / their scan, and the scratch of scan and sort.  Every array 256-byte aligned inside ws.
struct RanksWs {
	unsigned *cnt;
	int *list0, *list1;
	int64_t *packed;
	void *scan_ws;
	rk_wide *wa, *wb, *wt;
	uint32_t *pa, *pb, *pt;
	int64_t *loff;
	int *lcol;
	int64_t *runs;
	void *runs_scan_ws, *sort_ws;
	uintptr_t end;
	static RanksWs carve(void *ws, int64_t ncol, int64_t L)
	{
		uintptr_t p = (uintptr_t) ws;
		auto take = [&](size_t bytes) { p = (p + 255) & ~(uintptr_t) 255; const uintptr_t q = p; p += bytes; return q; };
		const size_t nc = (size_t) (ncol > 0 ? ncol : 1), nl = (size_t) L, ncomp = nl / (RK_F1_MAX + 1) + 1;
		RanksWs w = {};
		w.cnt = (unsigned *) take(64);
		w.list0 = (int *) take(4 * nc); w.list1 = (int *) take(4 * nc);
		w.packed = (int64_t *) take(8 * (nc + 1));
		w.scan_ws = (void *) take(exclusive_scan_ws_bytes((int64_t) nc + 1));
		if (L > 0) {
			w.wa = (rk_wide *) take(16 * nl); w.wb = (rk_wide *) take(16 * nl); w.wt = (rk_wide *) take(16 * nl);
			w.pa = (uint32_t *) take(4 * nl); w.pb = (uint32_t *) take(4 * nl); w.pt = (uint32_t *) take(4 * nl);
			w.loff = (int64_t *) take(8 * ncomp); w.lcol = (int *) take(4 * ncomp);
			w.runs = (int64_t *) take(8 * nl);
			w.runs_scan_ws = (void *) take(exclusive_scan_ws_bytes(L));
			w.sort_ws = (void *) take(svt_sort_ws_bytes(L));
		}
		w.end = p;
		return w;
	}
	static size_t bytes(int64_t ncol, int64_t L)            // (carved at 0, plus room for the alignment of ws itself)
	{
		return (size_t) carve(NULL, ncol, L).end + 256;
	}
};

size_t ranks_ws_bytes(int64_t ncol, int64_t long_nnz)
{
	if (long_nnz < 0) long_nnz = 0;
	if (long_nnz > 0xFFFFFFFFLL)
		return 0;                                       // not offered: the sort's payload is 32 bits
	return RanksWs::bytes(ncol, long_nnz);
}

// ---- classification ---------------------------------------------------------------------------------------
// One thread per column (and one for packed[ncol]).  An empty column is answered here.
__global__ void __launch_bounds__(256)
ranks_classify_kernel(const int64_t *__restrict__ col_ptr, int64_t nrow, int64_t ncol, int ties, void *__restrict__ zero_rank,
		      RanksWs w)
{
	const int64_t j = (int64_t) blockIdx.x * 256 + threadIdx.x;
	const int lane = threadIdx.x & 63;
	int form = -1;
	if (j < ncol) {
		const int64_t len = col_ptr[j + 1] - col_ptr[j];
		form = len <= 0 ? -1 : len <= RK_F0_MAX ? 0 : len <= RK_F1_MAX ? 1 : 2;
		w.packed[j] = form == 2 ? ((1LL << RK_LEN_BITS) | len) : 0;
		if (form < 0) {
			const RankCol c = { nrow, 0, 0, 0 };
			rank_zero(zero_rank, j, ties, c);
		}
	} else if (j == ncol) {
		w.packed[j] = 0;
	}
	// the lists: one atomic per wavefront and form
	for (int f = 0; f < 2; f++) {
		const unsigned long long m = __ballot(form == f);
		if (m == 0)
			continue;
		const int leader = __ffsll((long long) m) - 1;
		unsigned base = 0;
		if (lane == leader) base = atomicAdd(&w.cnt[f], (unsigned) __popcll(m));
		base = __shfl(base, leader, 64);
		if (form == f)
			(f == 0 ? w.list0 : w.list1)[base + __popcll(m & ((1ULL << lane) - 1))] = (int) j;
	}
}

// ---- form 0 -------------------------------------------------------------------------------------------------
// Orders this wavefront's LDS writes before its LDS reads (the lanes run in lockstep; this keeps the compiler from
// moving the accesses across the point).
__device__ __forceinline__ void rank_wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__global__ void __launch_bounds__(256)
ranks_short_kernel(const int64_t *__restrict__ col_ptr, const T *__restrict__ val, int64_t nrow, int ties,
		   void *__restrict__ rank_nz, void *__restrict__ zero_rank, RanksWs w)
{
	__shared__ rk_key keys[4][RK_F0_MAX];
	__shared__ unsigned char first[4][RK_F0_MAX];           // 1: no element before it in the column has its key
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const unsigned n0 = w.cnt[0];
	for (unsigned q = blockIdx.x * 4 + wv; q < n0; q += gridDim.x * 4) {
		const int64_t j = w.list0[q];
		const int64_t beg = col_ptr[j];
		const int len = (int) (col_ptr[j + 1] - beg);   // 1 .. RK_F0_MAX
		rk_key k[RK_F0_PER];
#pragma unroll
		for (int u = 0; u < RK_F0_PER; u++) {
			const int e = u * 64 + lane;
			k[u] = e < len ? rank_key(val[beg + e]) : RK_PAD;
			if (e < len) keys[wv][e] = k[u];
		}
		rank_wave_sync();
		int lt[RK_F0_PER], eq[RK_F0_PER], eb[RK_F0_PER];
#pragma unroll
		for (int u = 0; u < RK_F0_PER; u++) lt[u] = eq[u] = eb[u] = 0;
		for (int i = 0; i < len; i++) {
			const rk_key o = keys[wv][i];           // (one address for the wavefront: a broadcast)
#pragma unroll
			for (int u = 0; u < RK_F0_PER; u++) {
				lt[u] += o < k[u];
				eq[u] += o == k[u];
				eb[u] += o == k[u] && i < u * 64 + lane;
			}
		}
		long long neg = 0, nzs = 0, dneg = 0;
#pragma unroll
		for (int u = 0; u < RK_F0_PER; u++) {
			neg += k[u] < RK_ZERO; nzs += k[u] == RK_ZERO; dneg += k[u] < RK_ZERO && eb[u] == 0;
		}
		RankCol c;
		c.z = nrow - len;
		c.neg = __shfl(wave_sum_ll(neg), 0, 64);
		c.nzs = __shfl(wave_sum_ll(nzs), 0, 64);
		c.dneg = __shfl(wave_sum_ll(dneg), 0, 64);
		int dl[RK_F0_PER];
#pragma unroll
		for (int u = 0; u < RK_F0_PER; u++) dl[u] = 0;
		if (ties == SVT_TIES_DENSE) {                   // the first occurrences below: one more round of comparisons
#pragma unroll
			for (int u = 0; u < RK_F0_PER; u++)
				if (u * 64 + lane < len) first[wv][u * 64 + lane] = eb[u] == 0;
			rank_wave_sync();
			for (int i = 0; i < len; i++) {
				const rk_key o = keys[wv][i];
				const int f = first[wv][i];
#pragma unroll
				for (int u = 0; u < RK_F0_PER; u++) dl[u] += f && o < k[u];
			}
		}
#pragma unroll
		for (int u = 0; u < RK_F0_PER; u++)
			if (u * 64 + lane < len)
				rank_value(rank_nz, beg + u * 64 + lane, ties, k[u], lt[u], eq[u], dl[u], c);
		if (lane == 0)
			rank_zero(zero_rank, j, ties, c);
		rank_wave_sync();                               // (the next column writes keys[] and first[])
	}
}

// ---- form 1 -------------------------------------------------------------------------------------------------
// First index of a[0, n) whose element is >= k (upper = false) or > k (upper = true).
template <typename K>
__device__ __forceinline__ int64_t rank_bound(const K *a, int64_t n, K k, bool upper)
{
	int64_t lo = 0, hi = n;
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1;
		const K o = a[mid];
		if (upper ? o <= k : o < k) lo = mid + 1; else hi = mid;
	}
	return lo;
}

// Block-wide exclusive prefix of one count per thread (RK_NT1 threads).  wsum: RK_NT1 / 64 words of LDS.
__device__ inline unsigned rank_block_scan(unsigned x, unsigned *wsum)
{
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	unsigned incl = x;
	for (int o = 1; o < 64; o <<= 1) {
		const unsigned t = __shfl_up(incl, o, 64);
		if (lane >= o) incl += t;
	}
	if (lane == 63) wsum[wv] = incl;
	__syncthreads();
	unsigned before = 0;
	for (int i = 0; i < wv; i++) before += wsum[i];
	__syncthreads();
	return before + incl - x;
}

// One column of len <= RK_NT1 * IT stored values, by all RK_NT1 threads of the workgroup.
template <typename T, int IT>
__device__ void ranks_lds_column(const T *__restrict__ val, int64_t beg, int len, int64_t j, int64_t nrow, int ties,
				 void *__restrict__ rank_nz, void *__restrict__ zero_rank, unsigned char *lds, unsigned *wsum)
{
	typedef rocprim::block_radix_sort<rk_key, RK_NT1, IT, unsigned> Sort;
	static_assert(sizeof(typename Sort::storage_type) <= RK_F1_KEYS_BYTES, "the sort's storage shares the keys' LDS");
	rk_key *sk = (rk_key *) lds;                            // sorted keys [RK_NT1 * IT]
	unsigned *runs = (unsigned *) (lds + RK_F1_KEYS_BYTES);  // run starts in [0, p], "dense" only
	const int t = threadIdx.x;
	rk_key key[IT];
	unsigned pos[IT];
#pragma unroll
	for (int u = 0; u < IT; u++) {                          // (striped: any order will do, equal keys get equal ranks)
		const int e = u * RK_NT1 + t;
		pos[u] = (unsigned) e;
		key[u] = e < len ? rank_key(val[beg + e]) : RK_PAD;
	}
	Sort().sort(key, pos, *(typename Sort::storage_type *) lds);       // blocked: thread t holds ranks t * IT ...
	__syncthreads();
#pragma unroll
	for (int u = 0; u < IT; u++) sk[t * IT + u] = key[u];
	__syncthreads();
	if (ties == SVT_TIES_DENSE) {
		unsigned inc[IT], mine = 0;
#pragma unroll
		for (int u = 0; u < IT; u++) {
			const int p = t * IT + u;
			mine += p < len && (p == 0 || sk[p] != sk[p - 1]);
			inc[u] = mine;
		}
		const unsigned before = rank_block_scan(mine, wsum);
#pragma unroll
		for (int u = 0; u < IT; u++) runs[t * IT + u] = before + inc[u];
		__syncthreads();
	}
	RankCol c;
	const int64_t lb0 = rank_bound<rk_key>(sk, len, RK_ZERO, false), ub0 = rank_bound<rk_key>(sk, len, RK_ZERO, true);
	c.z = nrow - len; c.neg = lb0; c.nzs = ub0 - lb0;
	c.dneg = ties == SVT_TIES_DENSE && lb0 > 0 ? runs[lb0 - 1] : 0;
#pragma unroll
	for (int u = 0; u < IT; u++) {
		const int p = t * IT + u;
		if (p >= len)
			continue;
		const rk_key k = key[u];
		int64_t lo = p, hi = p + 1;
		if (p > 0 && sk[p - 1] == k) lo = rank_bound<rk_key>(sk, p, k, false);
		if (p + 1 < len && sk[p + 1] == k) hi = rank_bound<rk_key>(sk, len, k, true);
		const int64_t ds = ties == SVT_TIES_DENSE ? (int64_t) runs[p] - 1 : 0;
		rank_value(rank_nz, beg + pos[u], ties, k, lo, hi - lo, ds, c);
	}
	if (t == 0)
		rank_zero(zero_rank, j, ties, c);
	__syncthreads();                                        // (the next column sorts in the same LDS)
}

template <typename T>
__global__ void __launch_bounds__(RK_NT1)
ranks_lds_kernel(const int64_t *__restrict__ col_ptr, const T *__restrict__ val, int64_t nrow, int ties,
		 void *__restrict__ rank_nz, void *__restrict__ zero_rank, RanksWs w)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char rk_lds[];   // RK_F1_LDS bytes
	__shared__ unsigned wsum[RK_NT1 / 64];
	const unsigned n1 = w.cnt[1];
	for (unsigned q = blockIdx.x; q < n1; q += gridDim.x) {
		const int64_t j = w.list1[q];
		const int64_t beg = col_ptr[j];
		const int len = (int) (col_ptr[j + 1] - beg);   // RK_F0_MAX + 1 .. RK_F1_MAX, the same in every thread
		if (len <= RK_NT1 * 2)
			ranks_lds_column<T, 2>(val, beg, len, j, nrow, ties, rank_nz, zero_rank, rk_lds, wsum);
		else if (len <= RK_NT1 * 6)
			ranks_lds_column<T, 6>(val, beg, len, j, nrow, ties, rank_nz, zero_rank, rk_lds, wsum);
		else
			ranks_lds_column<T, 12>(val, beg, len, j, nrow, ties, rank_nz, zero_rank, rk_lds, wsum);
	}
}

// ---- form 2 -------------------------------------------------------------------------------------------------
#define RK_GATHER_SLICES 16
// The long columns' keys into wa[0, total), column c's at its offset, the column number above the key; payload = the
// position in wa; the slots [total, n_sort) sort to the end.  blockIdx.x strides over the columns, blockIdx.y over the
// slices of a column.  More long nonzeros than the sort was sized for: *flag = 1 and nothing is gathered.
template <typename T>
__global__ void __launch_bounds__(256)
ranks_gather_kernel(const int64_t *__restrict__ col_ptr, const T *__restrict__ val, int64_t ncol, int64_t n_sort,
		    int *__restrict__ flag, RanksWs w)
{
	const int64_t total = w.packed[ncol] & RK_LEN_MASK;
	if (total > n_sort) {
		if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *flag = 1;
		return;
	}
	for (int64_t j = blockIdx.x; j < ncol; j += gridDim.x) {
		const int64_t s0 = w.packed[j], s1 = w.packed[j + 1];
		if ((s0 >> RK_LEN_BITS) == (s1 >> RK_LEN_BITS))
			continue;                               // not a long column (the same answer in every thread)
		const int64_t c = s0 >> RK_LEN_BITS, off = s0 & RK_LEN_MASK;
		const int64_t beg = col_ptr[j], len = col_ptr[j + 1] - beg;
		if (blockIdx.y == 0 && threadIdx.x == 0) { w.loff[c] = off; w.lcol[c] = (int) j; }
		for (int64_t i = (int64_t) blockIdx.y * 256 + threadIdx.x; i < len; i += 256 * RK_GATHER_SLICES) {
			w.wa[off + i] = ((rk_wide) (unsigned long long) c << 64) | rank_key(val[beg + i]);
			w.pa[off + i] = (uint32_t) (off + i);
		}
	}
	const int64_t nthr = (int64_t) gridDim.x * RK_GATHER_SLICES * 256;
	for (int64_t r = total + ((int64_t) blockIdx.x * RK_GATHER_SLICES + blockIdx.y) * 256 + threadIdx.x; r < n_sort; r += nthr) {
		w.wa[r] = ~(rk_wide) 0;
		w.pa[r] = 0;
	}
}

// A workspace without room for any long column: *flag = 1 if there is one.
__global__ void ranks_no_room_kernel(int64_t ncol, int *__restrict__ flag, RanksWs w)
{
	if (threadIdx.x == 0 && (w.packed[ncol] & RK_LEN_MASK) > 0) *flag = 1;
}

// runs[r] = 1 where a tie run starts in the sorted array (a new column starts one by its number), 0 elsewhere.
__global__ void __launch_bounds__(256)
ranks_runs_kernel(int64_t ncol, int64_t n_sort, RanksWs w)
{
	const int64_t total = w.packed[ncol] & RK_LEN_MASK;
	const int64_t nthr = (int64_t) gridDim.x * 256;
	for (int64_t r = (int64_t) blockIdx.x * 256 + threadIdx.x; r < n_sort; r += nthr)
		w.runs[r] = total <= n_sort && r < total && (r == 0 || w.wb[r] != w.wb[r - 1]);
}

// One thread per element of the sorted array wb / pb (runs: scanned, "dense" only).
__global__ void __launch_bounds__(256)
ranks_long_kernel(const int64_t *__restrict__ col_ptr, int64_t nrow, int64_t ncol, int64_t n_sort, int ties,
		  void *__restrict__ rank_nz, void *__restrict__ zero_rank, RanksWs w)
{
	const int64_t total = w.packed[ncol] & RK_LEN_MASK;
	if (total > n_sort)
		return;
	const bool dense = ties == SVT_TIES_DENSE;
	const int64_t nthr = (int64_t) gridDim.x * 256;
	for (int64_t r = (int64_t) blockIdx.x * 256 + threadIdx.x; r < total; r += nthr) {
		const rk_wide me = w.wb[r];
		const int64_t cn = (int64_t) (unsigned long long) (me >> 64);
		const rk_key k = (rk_key) me;
		const rk_wide hi_part = me ^ (rk_wide) k;       // the column number alone
		const int64_t j = w.lcol[cn], off = w.loff[cn];
		const int64_t beg = col_ptr[j], len = col_ptr[j + 1] - beg;
		const rk_wide *seg = w.wb + off;
		const int64_t p = r - off;
		// runs started in seg[0, q): q > 0
		auto runs_before = [&](int64_t q) {
			const int64_t at = off + q - 1;
			return w.runs[at] + (at == off || w.wb[at] != w.wb[at - 1]) - w.runs[off];
		};
		RankCol c;
		const int64_t lb0 = rank_bound<rk_wide>(seg, len, hi_part | RK_ZERO, false);
		const int64_t ub0 = rank_bound<rk_wide>(seg, len, hi_part | RK_ZERO, true);
		c.z = nrow - len; c.neg = lb0; c.nzs = ub0 - lb0;
		c.dneg = dense && lb0 > 0 ? runs_before(lb0) : 0;
		int64_t lo = p, hi = p + 1;
		if (p > 0 && seg[p - 1] == me) lo = rank_bound<rk_wide>(seg, p, me, false);
		if (p + 1 < len && seg[p + 1] == me) hi = rank_bound<rk_wide>(seg, len, me, true);
		const int64_t ds = dense ? runs_before(p + 1) - 1 : 0;
		rank_value(rank_nz, beg + ((int64_t) w.pb[r] - off), ties, k, lo, hi - lo, ds, c);
		if (p == 0)
			rank_zero(zero_rank, j, ties, c);
	}
}

// ---- host ---------------------------------------------------------------------------------------------------
// The long nonzeros a workspace of ws_bytes has room for, at most `most`.
static int64_t ranks_ws_capacity(int64_t ncol, size_t ws_bytes, int64_t most)
{
	int64_t lo = 0, hi = most;                              // (bytes() grows with L)
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo + 1) / 2;
		if (RanksWs::bytes(ncol, mid) <= ws_bytes) lo = mid; else hi = mid - 1;
	}
	return lo;
}

static int ranks_bits(int64_t v)
{
	int b = 0;
	while (v > 0) { b++; v >>= 1; }
	return b;
}

int launch_ranks(const int64_t *col_ptr, const void *val, int Rtype, int64_t nrow, int64_t ncol, int64_t nnz, int ties,
		 void *rank_nz, void *zero_rank, int *flag, void *ws, size_t ws_bytes, hipStream_t s)
{
	HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), s));
	if (ws_bytes < RanksWs::bytes(ncol, 0))
		return svt_set_error("svt_dev_colranks: workspace too small");
	if (ncol <= 0)
		return 0;
	if (ncol > 0x7FFFFFFFLL)
		return svt_set_unsupported("colRanks: more than 2^31-1 columns");
	// the long nonzeros the sort is sized for: what the workspace holds, and never more than there are
	const int64_t most = nnz <= RK_F1_MAX ? 0 : nnz < 0xFFFFFFFFLL ? nnz : 0xFFFFFFFFLL;
	const int64_t n_sort = ranks_ws_capacity(ncol, ws_bytes, most);
	const uintptr_t base = ((uintptr_t) ws + 255) & ~(uintptr_t) 255;
	const RanksWs w = RanksWs::carve((void *) base, ncol, n_sort);
	HIP_TRY(hipMemsetAsync(w.cnt, 0, 64, s));
	hipLaunchKernelGGL(ranks_classify_kernel, dim3((unsigned) ((ncol + 256) / 256)), dim3(256), 0, s, col_ptr, nrow, ncol,
			   ties, zero_rank, w);
	if (nnz <= 0) {
		HIP_TRY(hipGetLastError());
		return 0;
	}
	int rc = 0;
	svt_by_rtype(Rtype, val, NULL, [&](auto *v, auto *) {
		typedef typename std::remove_cv<typename std::remove_pointer<decltype(v)>::type>::type T;
		const int64_t nb0 = (ncol + 3) / 4;
		hipLaunchKernelGGL(ranks_short_kernel<T>, dim3((unsigned) (nb0 < 16384 ? nb0 : 16384)), dim3(256), 0, s, col_ptr,
				   v, nrow, ties, rank_nz, zero_rank, w);
		int64_t nb1 = nnz / (RK_F0_MAX + 1);            // no more form-1 columns than that
		if (nb1 > ncol) nb1 = ncol;
		if (nb1 > 2048) nb1 = 2048;
		if (nb1 > 0) {
			if (hipFuncSetAttribute((const void *) ranks_lds_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
						RK_F1_LDS) != hipSuccess) {
				(void) hipGetLastError();
				rc = svt_set_unsupported("colRanks: the device refuses %d bytes of LDS per workgroup", RK_F1_LDS);
				return;
			}
			hipLaunchKernelGGL(ranks_lds_kernel<T>, dim3((unsigned) nb1), dim3(RK_NT1), RK_F1_LDS, s, col_ptr, v, nrow,
					   ties, rank_nz, zero_rank, w);
		}
	});
	if (rc)
		return rc;
	if (nnz <= RK_F1_MAX) {                                 // no column can be long
		HIP_TRY(hipGetLastError());
		return 0;
	}
	// the long columns: their offsets by one scan, then gather, sort, (dense: run starts and their scan,) ranks
	if (launch_exclusive_scan_i64(w.packed, ncol + 1, w.scan_ws, s))
		return -1;
	if (n_sort <= 0) {
		// no room for a long column: the check alone, which sets the flag if there is one
		hipLaunchKernelGGL(ranks_no_room_kernel, dim3(1), dim3(64), 0, s, ncol, flag, w);
		HIP_TRY(hipGetLastError());
		return 0;
	}
	const int64_t ncomp = n_sort / (RK_F1_MAX + 1) + 1;
	const unsigned nbg = (unsigned) (ncol < 2048 ? ncol : 2048);
	const int64_t nbe = (n_sort + 255) / 256;
	const unsigned nbl = (unsigned) (nbe < 65536 ? nbe : 65536);
	svt_by_rtype(Rtype, val, NULL, [&](auto *v, auto *) {
		typedef typename std::remove_cv<typename std::remove_pointer<decltype(v)>::type>::type T;
		hipLaunchKernelGGL(ranks_gather_kernel<T>, dim3(nbg, RK_GATHER_SLICES), dim3(256), 0, s, col_ptr, v, ncol, n_sort,
				   flag, w);
	});
	if (svt_sort_pairs<rk_wide>(w.wa, w.wb, w.wt, w.pa, w.pb, w.pt, n_sort, 64 + ranks_bits(ncomp), w.sort_ws, s))
		return -1;
	if (ties == SVT_TIES_DENSE) {
		hipLaunchKernelGGL(ranks_runs_kernel, dim3(nbl), dim3(256), 0, s, ncol, n_sort, w);
		if (launch_exclusive_scan_i64(w.runs, n_sort, w.runs_scan_ws, s))
			return -1;
	}
	hipLaunchKernelGGL(ranks_long_kernel, dim3(nbl), dim3(256), 0, s, col_ptr, nrow, ncol, n_sort, ties, rank_nz, zero_rank, w);
	HIP_TRY(hipGetLastError());
	return 0;
}
