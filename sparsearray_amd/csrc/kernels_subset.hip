// x[i, j] of a resident 2-D operand by an N-index (C_subset_SVT_by_Nindex, src/SparseArray_subsetting.c:223-297,
// 759-843, on the device layout col_ptr / row_idx / val).  Two primitives, both plain copies (values move as bits):
//
//   column gather   out column q = column cols[q] of A, any order, repeats allowed
//   row filter      the rows of a strictly increasing subscript kept, renumbered by their place in it
//
// Both cut their work into TILES of SUB_TILE = 4096 consecutive nonzeros -- of the RESULT for the gather, of the OPERAND
// for the filter -- one tile per trip of a 256-thread workgroup, 16 entries per thread, entry it * 256 + tid of the tile
// in trip `it` (every access to the nonzero arrays is coalesced).  A tile does the same work whatever the columns look
// like: the columns it touches are a contiguous range found by two binary searches over the column pointers (two
// threads, in parallel), and what has to happen per column boundary inside the tile is done by one lane per boundary.
// A column that spans many tiles has no boundary in most of them; a run of empty columns is a run of lanes that find
// nothing to do.  No atomic decides a position: every position is a prefix sum (row filter) or the entry's own index
// (gather), all 64-bit.
//
// The tile: 4096 = 64 chunks of 64 consecutive entries, one chunk per wavefront and trip, so that the table over the
// chunks of a tile is scanned by ONE wavefront with shuffles (rank of a kept entry = tile prefix + chunk prefix +
// popcount of the wavefront's ballot below the lane).  16 independent loads per lane are in flight; the gather's
// 16 KB of LDS (one int per entry) leave room for 8 workgroups per CU.
#include "svt_common.h"
#include "svt_scan.h"
#include "svt_tile.h"

#include <type_traits>

#define SUB_NT SVT_TILE_NT
#define SUB_ITEMS SVT_TILE_ITEMS
#define SUB_TILE SVT_TILE
#define SUB_CHUNKS SVT_TILE_CHUNKS
#define SUB_SHIFT SVT_TILE_SHIFT
#define SUB_GATHER_GRID 2048            // the gather's grid: its tile count is known on the device only (out_col_ptr)

enum { SUB_BAD_INDEX = 1, SUB_NOT_INCREASING = 2 };

// ---------------------------------------------------------------------------
// column gather
// ---------------------------------------------------------------------------
// len[q] = length of column cols[q], 0 and the flag for an index outside [0, ncol); len[ncols_sel] = 0 (the scan's total)
__global__ __launch_bounds__(SUB_NT) void subset_cols_len_kernel(const int64_t *col_ptr, int64_t ncol, const int32_t *cols,
								  int64_t ncols_sel, int64_t *len, int *flag)
{
	const int64_t q = (int64_t) blockIdx.x * SUB_NT + threadIdx.x;
	if (q > ncols_sel) return;
	int64_t l = 0;
	if (q < ncols_sel) {
		const int64_t c = cols[q];
		if (c < 0 || c >= ncol) atomicOr(flag, SUB_BAD_INDEX);
		else l = col_ptr[c + 1] - col_ptr[c];
	}
	len[q] = l;
}

// the scanned lengths become out_col_ptr unless an index was bad; head[1] <- the total either way
__global__ __launch_bounds__(SUB_NT) void subset_cols_publish_kernel(const int64_t *len, int64_t ncols_sel, const int *flag,
								      int64_t *out_col_ptr, int64_t *head)
{
	const int64_t q = (int64_t) blockIdx.x * SUB_NT + threadIdx.x;
	if (q == 0) head[1] = len[ncols_sel];
	if (q > ncols_sel || *flag) return;
	out_col_ptr[q] = len[q];
}

// One tile of SUB_TILE output entries per trip.  seg[i]: for the first entry of every column that starts inside the
// tile, the column (relative to q0, the column of the tile's first entry); an inclusive max-scan spreads it over the
// column's entries (svt_tile_max_scan, svt_tile.h).
template <typename T>
__global__ __launch_bounds__(SUB_NT) void subset_cols_copy_kernel(const int64_t *col_ptr, const int32_t *row_idx, const T *val,
								   int64_t ncol, int64_t nnz, const int32_t *cols, int64_t ncols_sel,
								   const int64_t *ocp, int32_t *out_row_idx, T *out_val)
{
	__shared__ int seg[SUB_TILE];
	__shared__ int cmax[SUB_CHUNKS];
	__shared__ int64_t qq[2];
	const int tid = threadIdx.x, w = tid >> 6;
	const int64_t total = ocp[ncols_sel];
	for (int64_t ts = (int64_t) blockIdx.x << SUB_SHIFT; ts < total; ts += (int64_t) gridDim.x << SUB_SHIFT) {
		const int n = (int) (total - ts < SUB_TILE ? total - ts : SUB_TILE);
		if (tid == 0) qq[0] = sub_last_le(ocp, ncols_sel, ts);
		if (tid == SVT_WAVE) qq[1] = sub_last_le(ocp, ncols_sel, ts + n - 1);
#pragma unroll
		for (int it = 0; it < SUB_ITEMS; it++) seg[it * SUB_NT + tid] = 0;
		__syncthreads();
		const int64_t q0 = qq[0], q1 = qq[1];
		// q0 < q <= q1: ts < ocp[q] <= ts + n - 1; one lane per boundary, the non-empty column of a position marks it
		for (int64_t q = q0 + 1 + tid; q <= q1; q += SUB_NT) {
			const int64_t p = ocp[q];
			if (ocp[q + 1] > p) seg[p - ts] = (int) (q - q0);
		}
		__syncthreads();
		int v[SUB_ITEMS];
		svt_tile_max_scan(seg, cmax, v);
#pragma unroll
		for (int it = 0; it < SUB_ITEMS; it++) {
			const int i = it * SUB_NT + tid;
			if (i >= n) continue;
			const int before = cmax[it * (SUB_NT / SVT_WAVE) + w];
			const int64_t q = q0 + (v[it] > before ? v[it] : before);
			const int64_t c = cols[q];
			if (c < 0 || c >= ncol) continue;  // (svt_dev_subset_cols_count refused such a subscript)
			const int64_t src = col_ptr[c] + (ts + i - ocp[q]);
			if (src >= nnz) continue;
			out_row_idx[ts + i] = row_idx[src];
			out_val[ts + i] = val[src];
		}
		__syncthreads();                           // seg, cmax and qq are written again by the next trip
	}
}

// ---------------------------------------------------------------------------
// row filter
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SUB_NT) void subset_fill_i32_kernel(int32_t *a, int64_t n, int32_t x)
{
	const int64_t i = (int64_t) blockIdx.x * SUB_NT + threadIdx.x;
	if (i < n) a[i] = x;
}

// map[rows[p]] = p; the flag for an index outside [0, nrow) and for rows[p] <= rows[p - 1]
__global__ __launch_bounds__(SUB_NT) void subset_rows_map_kernel(const int32_t *rows, int64_t nrows_sel, int64_t nrow,
								  int32_t *map, int *flag)
{
	const int64_t p = (int64_t) blockIdx.x * SUB_NT + threadIdx.x;
	if (p >= nrows_sel) return;
	const int64_t r = rows[p];
	if (r < 0 || r >= nrow) {
		atomicOr(flag, SUB_BAD_INDEX);
		return;
	}
	if (p > 0 && rows[p - 1] >= r) {
		atomicOr(flag, SUB_NOT_INCREASING);
		return;
	}
	map[r] = (int32_t) p;
}

// m[it] = new row of entry it * 256 + tid of the tile (-1: not kept, or past the tile's n entries); ballots[c] = the
// kept entries of chunk c as a mask, cpre[c] = how many are kept in the chunks before c, cpre[64] = in the tile
__device__ inline void subset_rows_rank(const int32_t *row_idx, const int32_t *map, int64_t ts, int n, int (&m)[SUB_ITEMS],
					 unsigned long long *ballots, int *cpre)
{
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
	for (int it = 0; it < SUB_ITEMS; it++) {
		const int i = it * SUB_NT + tid;
		m[it] = i < n ? map[row_idx[ts + i]] : -1;
	}
#pragma unroll
	for (int it = 0; it < SUB_ITEMS; it++) {
		const unsigned long long b = __ballot(m[it] >= 0);
		if (lane == 0) ballots[it * (SUB_NT / SVT_WAVE) + w] = b;
	}
	__syncthreads();
	if (tid < SVT_WAVE) {
		const int c = __popcll(ballots[tid]);
		int incl = c;
		for (int o = 1; o < SVT_WAVE; o <<= 1) {
			const int t = __shfl_up(incl, o, SVT_WAVE);
			if (lane >= o) incl += t;
		}
		cpre[tid] = incl - c;
		if (tid == SVT_WAVE - 1) cpre[SUB_CHUNKS] = incl;
	}
	__syncthreads();
}

// count pass: tile_cnt[tile] = kept entries of the tile; local[q] = kept entries of the tile before col_ptr[q], for
// every column q that starts inside the tile
__global__ __launch_bounds__(SUB_NT) void subset_rows_count_kernel(const int64_t *col_ptr, const int32_t *row_idx, int64_t ncol,
								    int64_t nnz, const int32_t *map, int64_t *tile_cnt, int32_t *local)
{
	__shared__ unsigned long long ballots[SUB_CHUNKS];
	__shared__ int cpre[SUB_CHUNKS + 1];
	__shared__ int64_t qq[2];
	const int tid = threadIdx.x;
	const int64_t ts = (int64_t) blockIdx.x << SUB_SHIFT;
	const int n = (int) (nnz - ts < SUB_TILE ? nnz - ts : SUB_TILE);
	if (tid == 0) qq[0] = sub_first_ge(col_ptr, ncol, ts);
	if (tid == SVT_WAVE) qq[1] = sub_last_le(col_ptr, ncol, ts + n - 1);
	int m[SUB_ITEMS];
	subset_rows_rank(row_idx, map, ts, n, m, ballots, cpre);
	if (tid == 0) tile_cnt[blockIdx.x] = cpre[SUB_CHUNKS];
	const int64_t q1 = qq[1];
	for (int64_t q = qq[0] + tid; q <= q1; q += SUB_NT) {      // ts <= col_ptr[q] <= ts + n - 1
		const int p = (int) (col_ptr[q] - ts);
		local[q] = cpre[p >> 6] + __popcll(ballots[p >> 6] & ((1ULL << (p & 63)) - 1ULL));
	}
}

// out_col_ptr[j] = kept entries before col_ptr[j]: those of the tiles before + those of its tile before it; nothing
// is written when the subscript was refused.  head[1] <- the kept entries in all.
__global__ __launch_bounds__(SUB_NT) void subset_rows_ptr_kernel(const int64_t *col_ptr, int64_t ncol, int64_t nnz,
								  const int64_t *tile_pre, int64_t ntiles, const int32_t *local,
								  const int *flag, int64_t *out_col_ptr, int64_t *head)
{
	const int64_t j = (int64_t) blockIdx.x * SUB_NT + threadIdx.x;
	if (j == 0) head[1] = tile_pre[ntiles];
	if (j > ncol || *flag) return;
	const int64_t p = col_ptr[j];
	out_col_ptr[j] = p >= nnz ? tile_pre[ntiles] : tile_pre[p >> SUB_SHIFT] + local[j];
}

// fill pass: the same tiles, the ranks recomputed; (new row, value) of a kept entry at tile prefix + rank in the tile
template <typename T>
__global__ __launch_bounds__(SUB_NT) void subset_rows_fill_kernel(const int32_t *row_idx, const T *val, int64_t nnz,
								   const int32_t *map, const int64_t *tile_pre, const int *flag,
								   int32_t *out_row_idx, T *out_val)
{
	__shared__ unsigned long long ballots[SUB_CHUNKS];
	__shared__ int cpre[SUB_CHUNKS + 1];
	if (*flag) return;
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const int64_t ts = (int64_t) blockIdx.x << SUB_SHIFT;
	const int n = (int) (nnz - ts < SUB_TILE ? nnz - ts : SUB_TILE);
	int m[SUB_ITEMS];
	subset_rows_rank(row_idx, map, ts, n, m, ballots, cpre);
	const int64_t base = tile_pre[blockIdx.x];
#pragma unroll
	for (int it = 0; it < SUB_ITEMS; it++) {
		if (m[it] < 0) continue;
		const int c = it * (SUB_NT / SVT_WAVE) + w;
		const int64_t pos = base + cpre[c] + __popcll(ballots[c] & ((1ULL << lane) - 1ULL));
		out_row_idx[pos] = m[it];
		out_val[pos] = val[ts + it * SUB_NT + tid];
	}
}

// ---------------------------------------------------------------------------
// launchers.  Workspaces: [head: int flag, int64 total at byte 8][...]; the parts at multiples of 256 bytes
// ---------------------------------------------------------------------------
static inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
static inline unsigned blocks_for(int64_t n) { return (unsigned) ((n + SUB_NT - 1) / SUB_NT); }

int subset_tile(void) { return SUB_TILE; }

// [head 256][len int64[ncols_sel + 1]][scratch of its scan]
size_t subset_cols_ws_bytes(int64_t ncols_sel)
{
	if (ncols_sel < 0) ncols_sel = 0;
	return 256 + up256(((size_t) ncols_sel + 1) * 8) + exclusive_scan_ws_bytes(ncols_sel + 1);
}

int launch_subset_cols_count(const int64_t *col_ptr, int64_t ncol, const int32_t *cols, int64_t ncols_sel,
			     int64_t *out_col_ptr, void *ws, hipStream_t s)
{
	char *w = (char *) ws;
	int64_t *len = (int64_t *) (w + 256);
	void *scan_ws = w + 256 + up256(((size_t) ncols_sel + 1) * 8);
	HIP_TRY(hipMemsetAsync(w, 0, 256, s));
	hipLaunchKernelGGL(subset_cols_len_kernel, dim3(blocks_for(ncols_sel + 1)), dim3(SUB_NT), 0, s, col_ptr, ncol, cols,
			   ncols_sel, len, (int *) w);
	if (launch_exclusive_scan_i64(len, ncols_sel + 1, scan_ws, s))
		return -1;
	hipLaunchKernelGGL(subset_cols_publish_kernel, dim3(blocks_for(ncols_sel + 1)), dim3(SUB_NT), 0, s, len, ncols_sel,
			   (const int *) w, out_col_ptr, (int64_t *) w);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_subset_cols_fill(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype, int64_t ncol,
			    int64_t nnz, const int32_t *cols, int64_t ncols_sel, const int64_t *out_col_ptr,
			    int32_t *out_row_idx, void *out_val, hipStream_t s)
{
	svt_by_rtype(Rtype, val, out_val, [&](auto *v, auto *o) {
		typedef std::remove_pointer_t<decltype(o)> T;
		hipLaunchKernelGGL(subset_cols_copy_kernel<T>, dim3(SUB_GATHER_GRID), dim3(SUB_NT), 0, s, col_ptr, row_idx, v, ncol,
				   nnz, cols, ncols_sel, out_col_ptr, out_row_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

struct SubsetRowsWs {
	size_t map, tile, local, scan, total;
	int64_t ntiles;
};
// [head 256][map int32[nrow]][tile counts -> prefixes int64[ntiles + 1]][local int32[ncol + 1]][scratch of the scan]
static SubsetRowsWs subset_rows_ws(int64_t nrow, int64_t ncol, int64_t nnz)
{
	SubsetRowsWs L;
	if (nrow < 0) nrow = 0;
	if (ncol < 0) ncol = 0;
	if (nnz < 0) nnz = 0;
	L.ntiles = (nnz + SUB_TILE - 1) >> SUB_SHIFT;
	L.map = 256;
	L.tile = L.map + up256((size_t) nrow * 4);
	L.local = L.tile + up256(((size_t) L.ntiles + 1) * 8);
	L.scan = L.local + up256(((size_t) ncol + 1) * 4);
	L.total = L.scan + exclusive_scan_ws_bytes(L.ntiles + 1);
	return L;
}

size_t subset_rows_ws_bytes(int64_t nrow, int64_t ncol, int64_t nnz)
{
	return subset_rows_ws(nrow, ncol, nnz).total;
}

int launch_subset_rows_count(const int64_t *col_ptr, const int32_t *row_idx, int64_t nrow, int64_t ncol, int64_t nnz,
			     const int32_t *rows, int64_t nrows_sel, int64_t *out_col_ptr, void *ws, hipStream_t s)
{
	const SubsetRowsWs L = subset_rows_ws(nrow, ncol, nnz);
	if (L.ntiles > 0x7FFFFFFFLL)
		return svt_set_error("svt_dev_subset_rows_count: too many nonzeros");
	char *w = (char *) ws;
	int *flag = (int *) w;
	int32_t *map = (int32_t *) (w + L.map), *local = (int32_t *) (w + L.local);
	int64_t *tile = (int64_t *) (w + L.tile);
	HIP_TRY(hipMemsetAsync(w, 0, 256, s));
	if (nrow > 0)
		hipLaunchKernelGGL(subset_fill_i32_kernel, dim3(blocks_for(nrow)), dim3(SUB_NT), 0, s, map, nrow, (int32_t) -1);
	if (nrows_sel > 0)
		hipLaunchKernelGGL(subset_rows_map_kernel, dim3(blocks_for(nrows_sel)), dim3(SUB_NT), 0, s, rows, nrows_sel, nrow,
				   map, flag);
	HIP_TRY(hipMemsetAsync(tile + L.ntiles, 0, 8, s));
	if (L.ntiles > 0)
		hipLaunchKernelGGL(subset_rows_count_kernel, dim3((unsigned) L.ntiles), dim3(SUB_NT), 0, s, col_ptr, row_idx, ncol,
				   nnz, map, tile, local);
	if (launch_exclusive_scan_i64(tile, L.ntiles + 1, w + L.scan, s))
		return -1;
	hipLaunchKernelGGL(subset_rows_ptr_kernel, dim3(blocks_for(ncol + 1)), dim3(SUB_NT), 0, s, col_ptr, ncol, nnz, tile,
			   L.ntiles, local, (const int *) flag, out_col_ptr, (int64_t *) w);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_subset_rows_fill(const int32_t *row_idx, const void *val, int Rtype, int64_t nrow, int64_t ncol, int64_t nnz,
			    int32_t *out_row_idx, void *out_val, const void *ws, hipStream_t s)
{
	const SubsetRowsWs L = subset_rows_ws(nrow, ncol, nnz);
	if (L.ntiles == 0)
		return 0;
	const char *w = (const char *) ws;
	svt_by_rtype(Rtype, val, out_val, [&](auto *v, auto *o) {
		typedef std::remove_pointer_t<decltype(o)> T;
		hipLaunchKernelGGL(subset_rows_fill_kernel<T>, dim3((unsigned) L.ntiles), dim3(SUB_NT), 0, s, row_idx, v, nnz,
				   (const int32_t *) (w + L.map), (const int64_t *) (w + L.tile), (const int *) w, out_row_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}
