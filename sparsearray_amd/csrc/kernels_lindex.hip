// Subsetting and subassignment by a linear index (L-index) or a matrix subscript (M-index) on resident sparse operands
// (C_subset_SVT_by_Lindex / _by_Mindex, src/SparseArray_subsetting.c; C_subassign_SVT_by_Lindex / _by_Mindex and
// subassign_leaf_by_OPBuf, src/SparseArray_subassignment.c of the reference).  A cell of the N-d array is a cell of the
// (nrow x nleaves) device layout: cell L is row L % nrow of leaf L / nrow, and the M-index row (m_0 .. m_{N-1}) is the
// cell sum(m_a * prod(dim[0 .. a-1])).  lx_cell() turns either form into a checked cell number; every kernel here goes
// through it, and nothing is used as an address before it was checked.
//
//   gather     one thread per index: the two col_ptr of the cell's leaf, a binary search of row_idx between them, the
//              stored value moved as bits, or the background (0, or NA under na_background); an NA index gives NA.  A
//              first kernel checks every index and raises the device word *bad; the gather reads it and writes nothing
//              once it is up.
//   placement  the placed operand Y of x[index] <- vals: one entry per DISTINCT assigned cell holding the cell's last
//              value, zeros included (a zero in Y is the deletion mark of the merge under ARI_RULE_ASSIGN_CELLS,
//              kernels_arith.hip).  The check pass writes the cells as keys, raises the flag for a bad index (an NA
//              is one here) and notes whether the cells are strictly increasing -- the output of nzwhich() / which()
//              always is.  SORTED ROUTE: position p is entry p of Y, no sort and no de-duplication.  UNSORTED ROUTE:
//              (cell, p) through the stable radix sort of svt_sort.h on the bits of ncells - 1, so the last key of a run
//              of equal cells is the cell's last occurrence; a flag per run end, scanned in 64 bits (svt_scan.h),
//              compacts them.  Y.col_ptr[c] = the scanned count at the first key >= c * nrow: one binary search per leaf.
//              Y.row_idx = cell % nrow, Y.val = vals[p % nvals].  No atomic decides a position (the two atomics raise
//              flags), and two runs give the same bits.
#include "svt_common.h"
#include "svt_scan.h"
#include "svt_sort.h"

#include <type_traits>

#define LX_NT 256

enum { LX_NA = -1, LX_BAD = -2 };
enum { LX_BAD_INDEX = 1, LX_BAD_OPERAND = 2 };

struct LxIndex {
	const int64_t *L;       // ndim == 0
	const int32_t *M;       // ndim >= 1: M[p + a * K]
	int64_t K;
	int ndim;
	int64_t dim[8];
	int64_t ncells;
};

// the cell of index p: >= 0 and < ncells, or LX_NA (an L-index of INT64_MIN), or LX_BAD (outside the array; an
// NA_integer_ coordinate, which is negative, included)
__device__ inline int64_t lx_cell(const LxIndex &I, int64_t p)
{
	if (I.ndim == 0) {
		const int64_t v = I.L[p];
		if (v == INT64_MIN) return LX_NA;
		return v < 0 || v >= I.ncells ? (int64_t) LX_BAD : v;
	}
	int64_t cell = 0, stride = 1;
	for (int a = 0; a < I.ndim; a++) {
		const int64_t m = I.M[p + a * I.K];
		if (m < 0 || m >= I.dim[a]) return LX_BAD;
		cell += m * stride;
		stride *= I.dim[a];
	}
	return cell;
}

template <typename T> __device__ inline T lx_na();
template <> __device__ inline int32_t lx_na<int32_t>() { return NA_INT; }
template <> __device__ inline double lx_na<double>() { return svt_na_real(); }

// raises `bits` in *word once per wavefront that has a lane with `mine`: a shuffled index has half its positions out of
// order, and one atomic per such position on the one word would take longer than the sort (every lane comes here)
__device__ inline void lx_raise(int *word, bool mine, int bits)
{
	const unsigned long long who = __ballot(mine);
	if (who != 0ULL && (int) (threadIdx.x & 63) == __ffsll((long long) who) - 1) atomicOr(word, bits);
}

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(LX_NT) void lindex_gather_check_kernel(LxIndex I, int *bad)
{
	const int64_t p = (int64_t) blockIdx.x * LX_NT + threadIdx.x;
	lx_raise(bad, p < I.K && lx_cell(I, p) == LX_BAD, LX_BAD_INDEX);
}

template <typename T>
__global__ __launch_bounds__(LX_NT) void lindex_gather_kernel(LxIndex I, const int64_t *__restrict__ col_ptr,
							       const int32_t *__restrict__ row_idx, const T *__restrict__ val, int64_t nrow,
							       int64_t nnz, int na_bg, T *__restrict__ out, int *bad)
{
	const int64_t p = (int64_t) blockIdx.x * LX_NT + threadIdx.x;
	if (p >= I.K || (*bad & LX_BAD_INDEX)) return;
	const int64_t cell = lx_cell(I, p);
	if (cell == LX_BAD) return;                         // (the check kernel raised the word)
	if (cell == LX_NA) {
		out[p] = lx_na<T>();
		return;
	}
	const int64_t c = cell / nrow;
	const int32_t r = (int32_t) (cell - c * nrow);
	T v = na_bg ? lx_na<T>() : (T) 0;
	int64_t lo = col_ptr[c];
	const int64_t end = col_ptr[c + 1];
	if (lo < 0 || end > nnz || lo > end) {
		atomicOr(bad, LX_BAD_OPERAND);
	} else {
		int64_t hi = end;
		while (lo < hi) {
			const int64_t mid = lo + (hi - lo) / 2;
			if (row_idx[mid] < r) lo = mid + 1; else hi = mid;
		}
		if (lo < end && row_idx[lo] == r) v = val[lo];
	}
	out[p] = v;
}

// ---------------------------------------------------------------------------
// placement
// ---------------------------------------------------------------------------
struct LxHead {                 // the head of the workspace
	int flag;               // LX_BAD_INDEX
	int pad;
	int64_t total;          // the entries of Y
	int unsorted;           // the cells are not strictly increasing
	int route;              // what the placement took: 0 sorted, 1 unsorted
};

__global__ __launch_bounds__(LX_NT) void lindex_check_kernel(LxIndex I, LxHead *head, int64_t *keys, uint32_t *pay)
{
	const int64_t p = (int64_t) blockIdx.x * LX_NT + threadIdx.x;
	bool bad = false, unsorted = false;
	if (p < I.K) {
		const int64_t cell = lx_cell(I, p);
		bad = cell < 0;                                     // an NA is a bad index of a subassignment
		pay[p] = (uint32_t) p;
		keys[p] = bad ? 0 : cell;
		unsorted = !bad && p > 0 && lx_cell(I, p - 1) >= cell;
	}
	lx_raise(&head->flag, bad, LX_BAD_INDEX);
	lx_raise(&head->unsorted, unsorted, 1);
}

// pos[i] = 1 when sorted key i ends a run of equal cells, i < K; pos[K] = 0 (the scan's total)
__global__ __launch_bounds__(LX_NT) void lindex_runend_kernel(const int64_t *skeys, int64_t K, int64_t *pos)
{
	const int64_t i = (int64_t) blockIdx.x * LX_NT + threadIdx.x;
	if (i > K) return;
	pos[i] = i < K && (i == K - 1 || skeys[i + 1] != skeys[i]);
}

// y_col_ptr[c] = the entries of Y before leaf c: the scanned count (pos; NULL on the sorted route: the position itself)
// at the first key >= c * nrow.  head <- the total and the route.
__global__ __launch_bounds__(LX_NT) void lindex_colptr_kernel(const int64_t *k, int64_t K, const int64_t *pos, int64_t nrow, int64_t ncol,
							       int64_t *y_col_ptr, LxHead *head)
{
	const int64_t c = (int64_t) blockIdx.x * LX_NT + threadIdx.x;
	if (c == 0) {
		head->total = pos != NULL ? pos[K] : K;
		head->route = pos != NULL;
	}
	if (c > ncol) return;
	const int64_t target = c * nrow;
	int64_t lo = 0, hi = K;
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (k[mid] < target) lo = mid + 1; else hi = mid;
	}
	y_col_ptr[c] = pos != NULL ? pos[lo] : lo;
}

// entry o of Y: sorted route, o = p = i; unsorted route, the run end i goes to o = pos[i] with p = spay[i]
template <typename T>
__global__ __launch_bounds__(LX_NT) void lindex_fill_kernel(const LxHead *head, const int64_t *keys, const int64_t *skeys,
							     const uint32_t *spay, const int64_t *pos, int64_t K, int64_t nrow,
							     const T *__restrict__ vals, int64_t nvals, int64_t y_nnz, int32_t *y_row_idx, T *y_val)
{
	const int64_t i = (int64_t) blockIdx.x * LX_NT + threadIdx.x;
	if (i >= K) return;
	int64_t cell, o, p;
	if (head->route == 0) {
		cell = keys[i]; o = i; p = i;
	} else {
		cell = skeys[i];
		if (i < K - 1 && skeys[i + 1] == cell) return;
		o = pos[i]; p = spay[i];
	}
	if (o < 0 || o >= y_nnz || p < 0 || p >= K) return;
	y_row_idx[o] = (int32_t) (cell % nrow);
	y_val[o] = vals[p % nvals];
}

// ---------------------------------------------------------------------------
// launchers.  Workspace of the placement: [head 256][keys int64[K]][skeys int64[K]][ktmp int64[K + 1], after the sort
// the run-end flags and their scan][pay uint32[K]][spay uint32[K]][ptmp uint32[K]][the sort's workspace][scratch of the
// scan]; the parts at multiples of 256
// ---------------------------------------------------------------------------
static inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
static inline unsigned blocks_for(int64_t n) { return (unsigned) ((n + LX_NT - 1) / LX_NT); }

struct LindexWs {
	size_t keys, skeys, ktmp, pay, spay, ptmp, sort, scan, total;
};
static LindexWs lindex_ws(int64_t K)
{
	LindexWs L;
	if (K < 0) K = 0;
	L.keys = 256;
	L.skeys = L.keys + up256((size_t) K * 8);
	L.ktmp = L.skeys + up256((size_t) K * 8);
	L.pay = L.ktmp + up256(((size_t) K + 1) * 8);
	L.spay = L.pay + up256((size_t) K * 4);
	L.ptmp = L.spay + up256((size_t) K * 4);
	L.sort = L.ptmp + up256((size_t) K * 4);
	L.scan = L.sort + up256(svt_sort_ws_bytes(K));
	L.total = L.scan + exclusive_scan_ws_bytes(K + 1);
	return L;
}

size_t lindex_place_ws_bytes(int64_t K, int64_t ncol)
{
	(void) ncol;                                        // (Y.col_ptr is the caller's; nothing here is sized by the leaves)
	return lindex_ws(K).total;
}

// the digits of the sort: 8 bits each over the bit length of ncells - 1
static int lindex_key_bits(int64_t nrow, int64_t ncol)
{
	uint64_t top = nrow > 0 && ncol > 0 ? (uint64_t) nrow * (uint64_t) ncol - 1 : 0;
	int bits = 0;
	while (top) { bits++; top >>= 1; }
	return bits > 0 ? bits : 1;
}
int lindex_sort_passes(int64_t nrow, int64_t ncol)
{
	return (lindex_key_bits(nrow, ncol) + 7) / 8;
}

static LxIndex lx_index(const LindexArgs &a)
{
	LxIndex I;
	I.L = a.ndim == 0 ? (const int64_t *) a.index : NULL;
	I.M = a.ndim == 0 ? NULL : (const int32_t *) a.index;
	I.K = a.K; I.ndim = a.ndim;
	for (int k = 0; k < 8; k++) I.dim[k] = k < a.ndim ? a.dim[k] : 1;
	I.ncells = a.nrow * a.ncol;
	return I;
}

int launch_lindex_gather(const LindexArgs &a, const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype, int64_t nnz,
			 int na_background, void *out, int *bad, hipStream_t s)
{
	if (a.K <= 0)
		return 0;
	const LxIndex I = lx_index(a);
	hipLaunchKernelGGL(lindex_gather_check_kernel, dim3(blocks_for(a.K)), dim3(LX_NT), 0, s, I, bad);
	svt_by_rtype(Rtype, val, out, [&](auto *v, auto *o) {
		typedef std::remove_pointer_t<decltype(o)> T;
		hipLaunchKernelGGL(lindex_gather_kernel<T>, dim3(blocks_for(a.K)), dim3(LX_NT), 0, s, I, col_ptr, row_idx, v, a.nrow, nnz,
				   na_background, o, bad);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_lindex_check(const LindexArgs &a, void *ws, hipStream_t s)
{
	const LindexWs L = lindex_ws(a.K);
	char *w = (char *) ws;
	HIP_TRY(hipMemsetAsync(w, 0, 256, s));
	if (a.K > 0)
		hipLaunchKernelGGL(lindex_check_kernel, dim3(blocks_for(a.K)), dim3(LX_NT), 0, s, lx_index(a), (LxHead *) w,
				   (int64_t *) (w + L.keys), (uint32_t *) (w + L.pay));
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_lindex_place(const LindexArgs &a, int unsorted, int64_t *y_col_ptr, void *ws, hipStream_t s)
{
	const LindexWs L = lindex_ws(a.K);
	const int64_t K = a.K;
	char *w = (char *) ws;
	int64_t *keys = (int64_t *) (w + L.keys), *skeys = (int64_t *) (w + L.skeys), *ktmp = (int64_t *) (w + L.ktmp);
	const int64_t *k = keys, *pos = NULL;
	if (unsorted) {
		if (svt_sort_pairs<int64_t>(keys, skeys, ktmp, (const uint32_t *) (w + L.pay), (uint32_t *) (w + L.spay),
					    (uint32_t *) (w + L.ptmp), K, lindex_key_bits(a.nrow, a.ncol), w + L.sort, s))
			return -1;
		hipLaunchKernelGGL(lindex_runend_kernel, dim3(blocks_for(K + 1)), dim3(LX_NT), 0, s, (const int64_t *) skeys, K, ktmp);
		if (launch_exclusive_scan_i64(ktmp, K + 1, w + L.scan, s))
			return -1;
		k = skeys; pos = ktmp;
	}
	hipLaunchKernelGGL(lindex_colptr_kernel, dim3(blocks_for(a.ncol + 1)), dim3(LX_NT), 0, s, k, K, pos, a.nrow, a.ncol, y_col_ptr,
			   (LxHead *) w);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_lindex_fill(const LindexArgs &a, const void *vals, int64_t nvals, int v_Rtype, int64_t y_nnz, int32_t *y_row_idx, void *y_val,
		       const void *ws, hipStream_t s)
{
	if (a.K <= 0 || y_nnz <= 0)
		return 0;
	const LindexWs L = lindex_ws(a.K);
	const char *w = (const char *) ws;
	svt_by_rtype(v_Rtype, vals, y_val, [&](auto *v, auto *o) {
		typedef std::remove_pointer_t<decltype(o)> T;
		hipLaunchKernelGGL(lindex_fill_kernel<T>, dim3(blocks_for(a.K)), dim3(LX_NT), 0, s, (const LxHead *) w,
				   (const int64_t *) (w + L.keys), (const int64_t *) (w + L.skeys), (const uint32_t *) (w + L.spay),
				   (const int64_t *) (w + L.ktmp), a.K, a.nrow, v, nvals, y_nnz, y_row_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}
