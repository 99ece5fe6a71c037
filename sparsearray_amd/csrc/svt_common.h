// Shared device/host helpers for the SVT HIP backend (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svt_hip.h"
#include "svt_random_rules.h"

#define SVT_WAVE 64
#define NA_INT (-2147483647 - 1)

// R's NA_real_: the NaN whose low word is 1954 (R arithmetic.c).  Device code
// builds it from bits so that the payload survives constant folding.
__host__ __device__ inline double svt_na_real()
{
	union { unsigned long long u; double d; } x;
	x.u = 0x7FF00000000007A2ULL;
	return x.d;
}
__host__ __device__ inline bool svt_is_na(double v)   // R_IsNA()
{
	union { double d; unsigned long long u; } x;
	x.d = v;
	return v != v && (unsigned int) (x.u & 0xFFFFFFFFu) == 1954u;
}
__host__ __device__ inline bool svt_is_finite(double v)   // R_FINITE()
{
	union { double d; unsigned long long u; } x;
	x.d = v;
	return ((x.u >> 52) & 0x7FF) != 0x7FF;
}

// ---- 64-lane wavefront reductions -----------------------------------------
__device__ inline double wave_sum(double v)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_down(v, o, SVT_WAVE);
	return v;   // valid in lane 0
}
__device__ inline double wave_prod(double v)
{
	for (int o = 32; o > 0; o >>= 1)
		v *= __shfl_down(v, o, SVT_WAVE);
	return v;
}
__device__ inline long long wave_sum_ll(long long v)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_down(v, o, SVT_WAVE);
	return v;
}
__device__ inline int wave_or(int v)
{
	for (int o = 32; o > 0; o >>= 1)
		v |= __shfl_down(v, o, SVT_WAVE);
	return v;
}
__device__ inline double wave_min(double v)
{
	for (int o = 32; o > 0; o >>= 1) {
		double t = __shfl_down(v, o, SVT_WAVE);
		v = t < v ? t : v;
	}
	return v;
}
__device__ inline double wave_max(double v)
{
	for (int o = 32; o > 0; o >>= 1) {
		double t = __shfl_down(v, o, SVT_WAVE);
		v = t > v ? t : v;
	}
	return v;
}
__device__ inline int wave_min_i(int v)
{
	for (int o = 32; o > 0; o >>= 1) {
		int t = __shfl_down(v, o, SVT_WAVE);
		v = t < v ? t : v;
	}
	return v;
}
__device__ inline int wave_max_i(int v)
{
	for (int o = 32; o > 0; o >>= 1) {
		int t = __shfl_down(v, o, SVT_WAVE);
		v = t > v ? t : v;
	}
	return v;
}

// Order-preserving map double <-> uint64 so that integer atomicMin/Max order
// doubles (no NaNs go through it).
__device__ inline unsigned long long f64_to_ordered(double v)
{
	unsigned long long u = (unsigned long long) __double_as_longlong(v);
	return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ inline double ordered_to_f64(unsigned long long u)
{
	u = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFULL) : ~u;
	return __longlong_as_double((long long) u);
}

// ---- host-side plumbing (svt_hip.cpp) ----------------------------------------
int svt_set_error(const char *fmt, ...);
int svt_set_unsupported(const char *fmt, ...);     // status > 0 at the ABI: the caller runs its CPU body
void svt_clear_unsupported(void);
#define HIP_TRY(expr)                                                         \
	do {                                                                  \
		hipError_t e__ = (expr);                                      \
		if (e__ != hipSuccess)                                        \
			return svt_set_error("%s failed: %s (%s:%d)", #expr, \
					     hipGetErrorString(e__),         \
					     __FILE__, __LINE__);             \
	} while (0)

// f(in, out) with two value arrays typed by the R type of the values, double or int32_t (host side; a templated
// kernel deduces its type from them):
//   svt_by_rtype(Rtype, val, out_val, [&](auto *v, auto *o) { hipLaunchKernelGGL(kernel, ..., v, ..., o); });
template <class F>
static inline void svt_by_rtype(int Rtype, const void *in, void *out, F &&f)
{
	if (Rtype == SVT_REALSXP) f((const double *) in, (double *) out);
	else f((const int32_t *) in, (int32_t *) out);
}

// kernel launchers implemented in the .hip files ---------------------------------
struct StatsArgs {
	const int64_t *col_ptr;
	const void *val;
	int Rtype;
	int64_t nseg;       // number of results
	int64_t inner;      // leaves per segment
	int64_t seg_len;    // inner * dim0: length of the virtual vector
	int opcode;
	int na_rm;
	double center;
	void *out;
	int *warn_flag;
	int na_bg;          // NaArray: implicit values are NAs (Rvector_summarization.c:1078-1106)
	int dgc;            // dgCMatrix flavour of var1 (src/sparseMatrix_utils.c:173-223): plain IEEE, no NA rule
};
// launch forms of the column statistics (values of svt_dev_colstats_form, include/svt_hip.h)
enum {
	COLSTATS_THREAD = 0,        // colstats_thread_kernel: one thread per segment
	COLSTATS_LANES16 = 1,       // colstats_kernel<T, 16, 16>
	COLSTATS_WAVE = 2,          // colstats_kernel<T, 64, 16>
	COLSTATS_GROUP_CACHED = 3,  // colstats_kernel<T, 256, 48>
	COLSTATS_GROUP_STREAM = 4,  // colstats_kernel<T, 256, 0>
	COLSTATS_SPLIT = 5          // launch_colstats_split: nchunk workgroups per segment
};
struct ColStatsRoute {
	int form;
	int nchunk;         // COLSTATS_SPLIT: chunks per segment, else 1
};
ColStatsRoute colstats_route(int64_t nseg, int64_t nnz);
int launch_colstats(const StatsArgs &a, int64_t nnz, hipStream_t s);
// colMedians / colQuantiles / colMads (kernels_median.hip): out on the device.  ORDER_QUANTILES (type 7): vec = the probs,
// on the device too, out[j + q * ncol].  ORDER_MADS: vec = one center per column on the device, or NULL for the column's
// median; the result is constant * (median of the deviations).  ORDER_MEDIANS: vec, nprobs and constant are not read
enum { ORDER_MEDIANS = 0, ORDER_QUANTILES = 1, ORDER_MADS = 2 };
size_t order_stat_ws_bytes(int what, int64_t ncol);
int launch_order_stat(int what, const int64_t *col_ptr, const void *val, int Rtype, int64_t nrow, int64_t ncol,
		      int64_t nnz, const double *vec, int nprobs, double constant, int na_rm, double *out, void *ws,
		      hipStream_t s);
// colRanks in the compact form (kernels_ranks.hip): rank_nz one rank per stored value, zero_rank one per column, int32
// or (SVT_TIES_AVERAGE) double; flag: a device word, cleared first, set when the workspace was made for fewer long
// nonzeros than the operand holds.  ranks_form(): 0, 1 or 2 by a column's stored length (svt_dev_colranks_form).
int ranks_form(int64_t col_nnz);
size_t ranks_ws_bytes(int64_t ncol, int64_t long_nnz);
int launch_ranks(const int64_t *col_ptr, const void *val, int Rtype, int64_t nrow, int64_t ncol, int64_t nnz, int ties,
		 void *rank_nz, void *zero_rank, int *flag, void *ws, size_t ws_bytes, hipStream_t s);

struct RowStatsArgs {
	const int64_t *col_ptr;
	const int32_t *row_idx;
	const void *val;
	int Rtype;
	int64_t ncol;       // leaves
	int64_t nrow;       // dim0
	int64_t inner;      // prod(dim[1..dims-1])
	int64_t nstrata;
	int64_t out_len;    // inner * nrow
	int opcode;
	int na_rm;
	const double *center;   // device, or NULL
	void *out;              // device, out_len elements
	void *scratch;          // device scratch (see rowstats_scratch_bytes)
	int *warn_flag;
	int64_t nnz_hint;       // nonzeros of the operand (launch tuning only), 0 = unknown
	int na_bg;              // NaArray: implicit entries are NAs (SparseArray_matrixStats.c:756-1019)
	int table_mode;         // launch_rowstats_panel, ROWSTATS_TABLE_*
};
enum {
	ROWSTATS_TABLE_BUILD = 0,   // build the table of run bounds and use it
	ROWSTATS_TABLE_ONLY = 1,    // build it only
	ROWSTATS_TABLE_READY = 2    // it is in `ws` already (same operand, same operation class)
};
size_t rowstats_scratch_bytes(int opcode, int64_t out_len);
int launch_rowstats(const RowStatsArgs &a, hipStream_t s);      // memory atomics
size_t rowstats_panel_ws_bytes(int64_t nrow, int64_t ncol);
int launch_rowstats_panel(const RowStatsArgs &a, void *ws, hipStream_t s);      // LDS row panels
// the form launch_rowstats_panel() takes for `a` (values of svt_dev_rowstats_form, include/svt_hip.h); *ps, *nsplit:
// panel shift and strata ranges of the panel form, 0 and 1 otherwise
int rowstats_panel_form(const RowStatsArgs &a, int *ps, int64_t *nsplit);
size_t rowstats_fused_ws_bytes(int64_t out_len);
int launch_rowstats_fused(const RowStatsArgs &a, void *ws, void *fws, hipStream_t s);   // mean / var1 / sd1
void launch_rowpanel_table(const int64_t *col_ptr, const int32_t *row_idx, int64_t ncol, int64_t nnz_hint,
			   int64_t npan, int ps, int32_t *pt, hipStream_t s);
bool launch_rowpanel_table_scan(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
				int64_t ncol, int64_t nnz_hint, int64_t npan, int ps, int32_t *pt,
				const uint8_t *skip, int *flag, hipStream_t s);

// sparse x sparse product by row panels (kernels_spmm.hip)
struct SpmmArgs {
	const int64_t *a_ptr; const int32_t *a_idx; const void *a_val; int a_type; int64_t nrow, ninner;
	const int64_t *b_ptr; const int32_t *b_idx; const void *b_val; int b_type; int64_t K;
	double *out; int64_t ldo;           // out[r + k * ldo]
	const int32_t *pt; int64_t npan; int ps;
	int *flag;                          // set when a non-finite value / an NA took part: the result is not the reference's
};
size_t spmm_ws_bytes(int64_t nrow, int64_t ninner);
int launch_spmm_prepare(const SpmmArgs &a, int64_t a_nnz, void *ws, hipStream_t s);
int launch_spmm_prepare_for(const SpmmArgs &a, int64_t a_nnz, int64_t b_nnz, void *ws, hipStream_t s, int *zero2);
int launch_spmm_product(SpmmArgs a, int64_t a_nnz, int64_t b_nnz, const void *ws, hipStream_t s);

// sparse x sparse product with a sparse result (kernels_spgemm.hip): a count launcher that leaves out_col_ptr
// int64[K + 1], the caller's flag word (device, may be NULL) and, in the head of `ws`, [int: a value of A or of B is not
// finite or an NA][int64 at byte 8: the nonzeros of the result], and a fill launcher that reads `ws` as the count
// launcher left it.  Both asynchronous.  spgemm_check(): the refusals that depend on the launch (operand types, grid,
// LDS), for the caller to ask before anything is written.
struct SpgemmArgs {
	const int64_t *a_ptr; const int32_t *a_idx; const void *a_val; int a_type; int64_t nrow, ninner;
	const int64_t *b_ptr; const int32_t *b_idx; const void *b_val; int b_type; int64_t K;
};
int spgemm_panel(void);
size_t spgemm_ws_bytes(int64_t nrow, int64_t ninner, int64_t K);
int spgemm_check(const SpgemmArgs &a);
int launch_spgemm_count(const SpgemmArgs &a, int64_t a_nnz, int64_t b_nnz, int64_t *out_col_ptr, int *not_finite, void *ws,
			hipStream_t s);
int launch_spgemm_fill(const SpgemmArgs &a, int32_t *out_row_idx, double *out_val, const void *ws, hipStream_t s);

// sparse x sparse crossprod without a dense operand (kernels_gram.hip)
struct GramArgs {
	const int64_t *a_ptr; const int32_t *a_idx; const void *a_val; int a_type;   // t(X): nrow leaves of (column of X, value)
	int64_t nx, nrow;
	const int64_t *b_ptr; const int32_t *b_idx; const void *b_val; int b_type; int64_t ny;   // Y: ny leaves of (row, value)
	double *out; int64_t ldo;           // out[c + j * ldo]
	int sym;                            // Y is X: cells c <= j, then mirrored
	const int32_t *pt; int64_t npan; int ps;
	int *flag;
};
void gram_set_panel(int one_block_max, int log2_panel);
size_t gram_ws_bytes(int64_t nx, int64_t nrow, int64_t a_nnz);
int launch_gram(GramArgs a, int64_t a_nnz, int64_t b_nnz, void *ws, hipStream_t s);
int launch_gram_mirror(double *out, int64_t n, int64_t ld, hipStream_t s);
int launch_gram_pairs(const int64_t *a_ptr, int64_t nrow, double *out, hipStream_t s);

size_t transpose_ws_bytes(int64_t nrow, int64_t nnz);
// the same with the boxed driver past the box limit (box_nnz_get(), read once per call and passed down)
size_t transpose_ws_bytes_box(int64_t nrow, int64_t nnz, int64_t box_limit);
int launch_transpose_box(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
			 int64_t nrow, int64_t ncol, int64_t nnz, int64_t *out_ptr, int32_t *out_idx,
			 void *out_val, void *ws, int64_t box_limit, hipStream_t s);
void box_nnz_set(int64_t n);
int64_t box_nnz_get(void);
int64_t boxed_calls(int reset);
int launch_transpose(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
		     int64_t nrow, int64_t ncol, int64_t nnz, int64_t *out_ptr, int32_t *out_idx,
		     void *out_val, void *ws, hipStream_t s);

// x[i, j] by an N-index (kernels_subset.hip): the column gather and the row filter, each a count call that leaves
// out_col_ptr and a fill call.  The count launchers are asynchronous and leave in the head of `ws` [int: 1 an index out
// of range, 2 (rows) the subscript not strictly increasing][int64 at byte 8: the nonzeros of the result]; with the flag
// up nothing is written outside `ws`.
int subset_tile(void);
size_t subset_cols_ws_bytes(int64_t ncols_sel);
int launch_subset_cols_count(const int64_t *col_ptr, int64_t ncol, const int32_t *cols, int64_t ncols_sel,
			     int64_t *out_col_ptr, void *ws, hipStream_t s);
int launch_subset_cols_fill(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype, int64_t ncol,
			    int64_t nnz, const int32_t *cols, int64_t ncols_sel, const int64_t *out_col_ptr,
			    int32_t *out_row_idx, void *out_val, hipStream_t s);
size_t subset_rows_ws_bytes(int64_t nrow, int64_t ncol, int64_t nnz);
int launch_subset_rows_count(const int64_t *col_ptr, const int32_t *row_idx, int64_t nrow, int64_t ncol, int64_t nnz,
			     const int32_t *rows, int64_t nrows_sel, int64_t *out_col_ptr, void *ws, hipStream_t s);
int launch_subset_rows_fill(const int32_t *row_idx, const void *val, int Rtype, int64_t nrow, int64_t ncol, int64_t nnz,
			    int32_t *out_row_idx, void *out_val, const void *ws, hipStream_t s);

// Arith and Math (kernels_arith.hip): the map f(x) and the merge x op y, each a count launcher that leaves out_col_ptr
// and, in the head of `ws`, [int64 at byte 8: the nonzeros of the result], and a fill launcher that reads `ws` as the
// count launcher left it.  All asynchronous.  `entries`: nnz for the map, nnz(x) + nnz(y) for the merge.  `rule`: the
// element rule the tiles evaluate -- Arith and Math as `kind` and `op` say, or Compare / Logic (`op` a SVT_COMPARE_* /
// SVT_LOGIC_* opcode, `kind` not read), whose result is int32 whatever the operands and has no overflow word, or the
// subassignment rule (merge only; y the placed operand of kernels_subassign.hip, `op` not read, `cover_row` /
// `cover_leaf` one byte per row / per leaf, NULL: the whole axis; the result double when either side is, else int32),
// or the rule of the subassignment by cells (merge only; y the placed operand of kernels_lindex.hip, a zero in it the
// deletion mark; no tables, `op` not read; the result typed like ARI_RULE_ASSIGN's), or pmin / pmax (map with the
// scalar in `sd` / `si`, merge and sweep; `op` SVT_PMINMAX_MIN / _MAX, ORed with SVT_PMINMAX_NA_RM; the result int32
// unless a side is double; no overflow word), or is.na / is.nan / is.infinite (map only; `op` a SVT_IS_* opcode; the
// result int32).
enum { ARI_RULE_ARITH = 0, ARI_RULE_COMPARE = 1, ARI_RULE_LOGIC = 2, ARI_RULE_ASSIGN = 3, ARI_RULE_ASSIGN_CELLS = 4,
       ARI_RULE_PMINMAX = 5, ARI_RULE_ISFUN = 6 };
struct ArithMapArgs {
	const int64_t *col_ptr;
	const int32_t *row_idx;
	const void *val;
	int Rtype;
	int64_t ncol, nnz;
	int kind, op;           // SVT_ARITH_SCALAR / _NEG / _MATH and its opcode
	double sd;              // the scalar, as a double and as an integer
	int32_t si;
	int out_Rtype;
	int rule = ARI_RULE_ARITH;
};
struct ArithMergeArgs {
	const int64_t *x_col_ptr; const int32_t *x_row_idx; const void *x_val; int x_Rtype; int64_t x_nnz;
	const int64_t *y_col_ptr; const int32_t *y_row_idx; const void *y_val; int y_Rtype; int64_t y_nnz;
	int64_t nrow, ncol;
	int op;
	int rule = ARI_RULE_ARITH;
	const unsigned char *cover_row = NULL, *cover_leaf = NULL;     // ARI_RULE_ASSIGN
};
int arith_tile(void);
size_t arith_ws_bytes(int64_t ncol, int64_t entries, int merge);
int launch_arith_map_count(const ArithMapArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s);
int launch_arith_map_fill(const ArithMapArgs &a, int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, hipStream_t s);
int launch_arith_merge_count(const ArithMergeArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s);
int launch_arith_merge_fill(const ArithMergeArgs &a, int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, hipStream_t s);
// The sweep, a third family: f(v, stats[k]) on the stored values of one operand, k = (with_rows ? row : 0) +
// (with_rows ? nrow : 1) * ((leaf / stride) % len) -- one element of `stats` per row, per leaf, or per row of a group of
// leaves.  `rule`: ARI_RULE_ARITH (op one of * / ^ %% %/%), ARI_RULE_COMPARE or ARI_RULE_PMINMAX.  The workspace is the map's
// (arith_ws_bytes(ncol, nnz, 0)); the count launcher first checks every element of `stats` and leaves, in the head of
// `ws`, [int64 at byte 8: the nonzeros of the result][uint64 at byte 16: the smallest index of an element that does not
// keep the result sparse, or all ones]; with such an element out_col_ptr is not written.  All asynchronous.
struct ArithSweepArgs {
	const int64_t *col_ptr;
	const int32_t *row_idx;
	const void *val;
	int Rtype;
	int64_t nrow, ncol, nnz;
	int rule, op;
	const void *stats;
	int stats_Rtype;
	int with_rows;
	int64_t stride, len;
	int out_Rtype;
};
int launch_arith_sweep_count(const ArithSweepArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s);
int launch_arith_sweep_fill(const ArithSweepArgs &a, int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, hipStream_t s);

// Subassignment (kernels_subassign.hip): the placed operand Y of x[rows, leaves] <- value and the two cover tables,
// for the merge under ARI_RULE_ASSIGN.  `rows` / `leaves`: device int32, 0-based; nrows_sel / nleaves_sel < 0: the whole
// axis (the pointer is not read).  The vector form recycles `vals` (nvals >= 1 values of v_Rtype) over the row subscript,
// the last occurrence of a row winning, and keeps the non-zero values only; the SVT form renames the rows of `v`'s
// leaves (v_* : its arrays; rows strictly increasing, leaves without repeats).  The count launcher leaves y_col_ptr
// int64[ncol + 1], the tables (a NULL table is not written) and, in the head of `ws`, [int: 1 a bad index, 2 rows not
// strictly increasing or a repeated leaf (SVT form)][int64 at byte 8: the entries of Y]; with the flag up nothing is
// written outside `ws`.  The fill launcher reads `ws` as the count launcher left it.  All asynchronous.
struct SubassignArgs {
	int64_t nrow, ncol;
	const int32_t *rows; int64_t nrows_sel;
	const int32_t *leaves; int64_t nleaves_sel;
	const void *vals; int64_t nvals;        // the vector form
	const int64_t *v_col_ptr; const int32_t *v_row_idx; const void *v_val; int64_t v_nnz;   // the SVT form (v_col_ptr != NULL)
	int v_Rtype;
};
int subassign_tile(void);
size_t subassign_ws_bytes(int64_t nrow, int64_t ncol);
int launch_subassign_count(const SubassignArgs &a, int64_t *y_col_ptr, unsigned char *cover_row, unsigned char *cover_leaf, void *ws,
			   hipStream_t s);
int launch_subassign_fill(const SubassignArgs &a, const int64_t *y_col_ptr, int64_t y_nnz, int32_t *y_row_idx, void *y_val,
			  const void *ws, hipStream_t s);

// Subsetting and subassignment by an L-index or an M-index (kernels_lindex.hip).  `index`: device int64[K] 0-based cell
// numbers with INT64_MIN for NA (ndim == 0), or device int32[K * ndim] 0-based coordinates, column-major (ndim >= 1,
// `dim` the extents with dim[0] == nrow and prod(dim[1:]) == ncol; an NA_integer_ coordinate is a bad index).
// launch_lindex_gather writes out[K] (A's type): the stored value, the background, or NA for an NA index; a first
// kernel checks every index and raises *bad (1: an index outside the array, 2: a col_ptr pair that cannot be followed),
// the gather reads *bad and writes nothing once it is up.  The placement builds the placed operand Y of
// x[index] <- vals: one entry per distinct cell with the cell's last value, zeros included.  launch_lindex_check leaves
// in the head of `ws` [int: 1 a bad index (NA included)][int at byte 16: 1 the cells are not strictly increasing] and
// the cells as keys; launch_lindex_place (after the head was read: `unsorted` says which route) sorts and compacts
// them when it must, writes y_col_ptr and leaves [int64 at byte 8: the entries of Y]; launch_lindex_fill reads `ws` as
// they left it.  All asynchronous; none launches over an empty range.
struct LindexArgs {
	const void *index;
	int64_t K;
	int ndim;               // 0: an L-index
	int64_t dim[8];
	int64_t nrow, ncol;
};
size_t lindex_place_ws_bytes(int64_t K, int64_t ncol);
int lindex_sort_passes(int64_t nrow, int64_t ncol);
int launch_lindex_gather(const LindexArgs &a, const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype, int64_t nnz,
			 int na_background, void *out, int *bad, hipStream_t s);
int launch_lindex_check(const LindexArgs &a, void *ws, hipStream_t s);
int launch_lindex_place(const LindexArgs &a, int unsorted, int64_t *y_col_ptr, void *ws, hipStream_t s);
int launch_lindex_fill(const LindexArgs &a, const void *vals, int64_t nvals, int v_Rtype, int64_t y_nnz, int32_t *y_row_idx, void *y_val,
		       const void *ws, hipStream_t s);

// abind (kernels_abind.hip): the result as a sequence of pieces, each a whole leaf of one object.  The count launcher
// copies the table of objects into `ws` (one asynchronous copy: the table must live until the stream has passed it) and
// leaves out_col_ptr and, in the head of `ws`, [int: 1 an object's pointers do not ascend inside its nnz][int64 at byte
// 8: the nonzeros of the result]; with the flag up nothing is written outside `ws`.  The fill launcher reads `ws` as
// the count launcher left it.  Both asynchronous.
struct AbindObj {               // one object, in the layout the count kernels read
	const int64_t *col_ptr;
	const int32_t *row_idx;
	const void *val;
	int64_t nnz;
	int64_t nleaves;
	int64_t shift;          // along the rows: off[n], the rows of the objects before; along a leaf dim: start[n]
	int64_t ext;            // along a leaf dim: the extent along the binding dimension
	int32_t Rtype;
	int32_t pad;
};
struct AbindArgs {
	const AbindObj *objs;   // host
	int nobj;
	int rows_form;
	int64_t inner, D;       // along a leaf dim: prod of the dims between the rows and the binding one, sum of ext[]
	int64_t npieces;        // rows: out_nleaves * nobj; leaf dim: out_nleaves
	int64_t out_nleaves;
	int64_t max_nnz;        // sum of the objects' nnz: the result's nonzeros (the copy's grid is sized from it)
	int ans_Rtype;
	int uniform;            // every object has the result's element size and needs no conversion
};
int abind_tile(void);
size_t abind_ws_bytes(int nobj, int64_t npieces);
int launch_abind_count(const AbindArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s);
int launch_abind_fill(const AbindArgs &a, int32_t *out_row_idx, void *out_val, const void *ws, hipStream_t s);

// Coercions dense array <-> operand and nzwhich (kernels_coerce.hip).  Dense -> sparse over tiles of coerce_tile() cells
// of the column-major array x[nrow, nleaves], ncells = nrow * nleaves > 0: the count launcher leaves out_col_ptr and, in
// `ws`, [head: int 0, int64 at byte 8: the kept cells][the tile bases][one bit per cell]; the fill launcher reads `ws` as
// the count launcher left it.  launch_to_dense writes every cell of out[nrow * ncol] (out aligned to 16 bytes) and
// raises *bad (may be NULL) for pointers or rows it refuses to follow; launch_nzwhich writes int64[nnz] linear indices or
// (arr_ind) int32[nnz * ndim] coordinates, column-major.  All asynchronous; none launches over an empty range.
struct FromDenseArgs {
	const void *x;
	int x_Rtype;
	int64_t nrow, nleaves, ncells;
	int ans_Rtype;
	int na_background;
};
int coerce_tile(void);
size_t from_dense_ws_bytes(int64_t ncells);
int launch_from_dense_count(const FromDenseArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s);
int launch_from_dense_fill(const FromDenseArgs &a, int32_t *out_row_idx, void *out_val, const void *ws, hipStream_t s);
// The same two launchers over generated cells (poissonSparseArray(); svt_random_rules.h): the leaves [first_leaf,
// first_leaf + nleaves) of an integer array of nrow rows, ncells = nrow * nleaves > 0, the workspace that of
// from_dense_ws_bytes(ncells).  launch_rpois: out[i] = the value of cell first + i, n > 0.
struct PoissonArgs {
	svt_poisson_table table;
	uint64_t seed;
	int64_t nrow, first_leaf, nleaves, ncells;
};
int launch_poisson_count(const PoissonArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s);
int launch_poisson_fill(const PoissonArgs &a, int32_t *out_row_idx, int32_t *out_val, const void *ws, hipStream_t s);
int launch_rpois(const svt_poisson_table &table, uint64_t seed, int64_t first, int64_t n, int32_t *out, hipStream_t s);
int launch_to_dense(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype, int64_t nrow, int64_t ncol,
		    int64_t nnz, int na_background, int out_Rtype, void *out, int *bad, hipStream_t s);
int launch_nzwhich(const int64_t *col_ptr, const int32_t *row_idx, int64_t nrow, int64_t ncol, int64_t nnz, int ndim,
		   const int64_t *dim, int arr_ind, void *out, hipStream_t s);

void aperm_route_counts(int64_t *out, int reset);
size_t aperm_ws_bytes(int64_t nnz, const int64_t *dim, int ndim);
// aperm, with the boxed driver for the permutations that move the rows past the box limit (read once per call and
// passed down); perm is 0-based.  aperm_ws_bytes_box(): at least the need of every permutation, and aperm_ws_bytes()
// itself whenever the driver is not taken; aperm_perm_ws_bytes_box(): the need of one permutation.
size_t aperm_ws_bytes_box(int64_t nnz, const int64_t *dim, int ndim, int64_t box_limit);
size_t aperm_perm_ws_bytes_box(int64_t nnz, const int64_t *dim, int ndim, const int *perm, int64_t box_limit);
int launch_aperm_box(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
		     int64_t ncol, int64_t nnz, const int64_t *dim, int ndim, const int *perm,
		     int64_t *out_ptr, int32_t *out_idx, void *out_val, void *ws, int64_t box_limit, hipStream_t s);

struct GroupSumArgs {
	const int64_t *col_ptr64;   // one of the two col_ptr flavours is set
	const int32_t *col_ptr32;
	const int32_t *row_idx;
	const void *val;
	int Rtype;
	int64_t nrow, ncol;
	int64_t nnz;                // nonzeros of the operand (launch_rowsum: route choice; launch_rowsum_gid: ids to write)
	const int *group;           // device
	int ngroup;
	int na_rm;
	void *out;                  // device, zeroed by the launcher
	void *scratch;              // int path: int64 sums + NA flags
	int *ovflow_flag;
};
size_t groupsum_scratch_bytes(int Rtype, int64_t out_len);
// launch forms of rowsum() (values of svt_dev_rowsum_form, include/svt_hip.h) and of the prepared ids
// (svt_dev_rowsum_prepare_form)
enum {
	ROWSUM_ATOMIC = 0,          // groupsum_atomic_kernel: a wavefront per column, memory atomics
	ROWSUM_LDS_TABLE = 1,       // rowsum_f64_lds_kernel<int>: a workgroup per column, the int group table
	ROWSUM_LDS_G16 = 2,         // rowsum_f64_lds_kernel<uint16_t>: the same behind the 16-bit copy of the table
	ROWSUM_WINDOWED = 3         // rowsum_f64_cols_kernel: cols_per_wg columns per workgroup, window by window
};
enum {
	ROWSUM_IDS_FLAT = 0,        // rowsum_gid_kernel: two ids per thread
	ROWSUM_IDS_WINDOWED = 1     // rowsum_gid_cols_kernel: the walk of the windowed kernel
};
struct RowsumRoute {
	int form;
	int cols_per_wg;    // ROWSUM_WINDOWED / ROWSUM_IDS_WINDOWED: columns (a wavefront each) per workgroup, else 0
};
RowsumRoute rowsum_route(int64_t nrow, int64_t ncol, int64_t nnz, int ngroup, int Rtype, bool col_ptr32);
RowsumRoute rowsum_gid_route(int64_t nrow, int64_t ncol, int64_t nnz, int ngroup, bool col_ptr32);
int rowsum_prepared_route(int64_t ncol, int ngroup, bool col_ptr32, int *cols_per_wg);
int64_t rowsum_window_rows(void);   // rows per window of the windowed forms
int launch_rowsum(const GroupSumArgs &a, hipStream_t s);       // doubles: LDS or atomic kernels by shape
int launch_rowsum_gid(const GroupSumArgs &a, uint16_t *gid, hipStream_t s);
int launch_rowsum_prepared(const GroupSumArgs &a, const uint16_t *gid, hipStream_t s);   // f64, ngroup * 8 <= LDS
int launch_colsum(const GroupSumArgs &a, hipStream_t s);

struct CrossprodArgs {
	const int64_t *col_ptr;
	const int32_t *row_idx;
	const void *val;
	int Rtype;               // REALSXP or INTSXP (A and Y agree)
	int64_t nrow, ncol;
	const void *Y;           // dense operand (device)
	int64_t ldY;
	int K;
	int tr_y;
	double *out;
	int64_t out_stride_c, out_stride_k;
	void *ws;
	size_t ws_bytes;
};
size_t crossprod_ws_bytes(int64_t nrow, int64_t ncol, int K);
int launch_dense_prepare(const CrossprodArgs &a, hipStream_t s);
int launch_crossprod_prepared(const CrossprodArgs &a, hipStream_t s);
int launch_crossprod_csc_dense(const CrossprodArgs &a, hipStream_t s);
// Scatter leaves [c0, c0+nc) of a CSC into a dense column-major nrow x nc
// matrix (the "preprocessing" of src/SparseMatrix_mult.c:632-724).
int launch_densify(const int64_t *col_ptr, const int32_t *row_idx,
		   const void *val, int Rtype, int64_t nrow, int64_t c0,
		   int64_t nc, void *dense, hipStream_t s);
// out[j, i] = out[i, j] for i > j (n x n, column-major)
int launch_mirror_lower(double *out, int64_t n, hipStream_t s);
void pbc_auto_layout(int64_t nrow, int64_t ncol, int64_t nnz, int *CBW, int *WPB, int *logR);
// Which product kernel reads the panel-blocked layout (CBW, WPB, logR) of an operand of nrow rows
// (kernels_mult_pbc.hip): PBC_KIND_BAD = none is built; PBC_KIND_NONE = built without records, the
// general kernels answer the product.
enum { PBC_KIND_BAD = -1, PBC_KIND_NONE = 0, PBC_KIND_DMA = 1, PBC_KIND_GATHER = 2 };
int pbc_kind(int64_t nrow, int CBW, int WPB, int logR);
int launch_int_to_f64(const int *in, int64_t n, double *out, hipStream_t s);
// kernels_shard.hip: the sharded host entry points (svt_set_devices).  out = ((p_0 + p_1) + ...) + p_{nparts-1}
// elementwise, part t at parts + t * stride (stride even, >= n); and idx[k] -= base for k < n.
int launch_shard_sum(const double *parts, int nparts, int64_t stride, int64_t n, double *out, hipStream_t s);
int launch_rebase_rows(int32_t *idx, int64_t n, int32_t base, hipStream_t s);
