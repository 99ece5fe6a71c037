// Subassignment x[i, j] <- value on resident sparse operands (.subassign_SVT_by_Nindex, R/SparseArray-subassignment.R;
// C_subassign_SVT_with_short_Rvector, src/SparseArray_subassignment.c of the reference).  On the device layout it is a
// merge: these kernels PLACE the new values as a sparse operand Y with x's extents and mark what the subscripts cover,
// one byte per row and one per leaf; the merge of kernels_arith.hip under ARI_RULE_ASSIGN (svt_rule_assign) then takes
// Y's value where Y stores one, drops an x entry whose row and leaf are both covered, and keeps the rest.
//
//   vector form  `vals` recycled over the row subscript: last[r] = the largest p with rows[p] == r (atomicMax on an
//                int32: the result does not depend on the order), the row's new value vals[last[r] % nvals]; a scan
//                over the rows whose new value is not zero compacts them into the PATCH LEAF of P entries, rows
//                ascending; Y is the patch leaf in every covered leaf: Y.col_ptr = scan of P * cover_leaf[c].
//                x[i, j] <- 0 has P == 0 and an empty Y: its cost is the merge's, by nnz(x), whatever the selection.
//   SVT form     leaf leaves[q] of Y = leaf q of v with row r renamed rows[r] (rows strictly increasing, so the order
//                inside the leaf stays; leaves without repeats, in any order); every other leaf of Y is empty; values
//                move as bits, stored zeros of v travel (the merge drops them).
//
// A count pass and a fill pass.  The count pass checks every index before it is used as an address and raises the flag
// in the head of the workspace (1: an index outside its axis; 2, SVT form: rows not strictly increasing, a repeated
// leaf -- atomicCAS on the leaf's source word, any repeat raises it whatever the order); everything it computes before
// the flag is complete stays inside the workspace, and the kernels that write outside it (the cover tables, Y.col_ptr)
// read the flag first.  The fill pass copies in tiles of SVT_TILE entries of Y: the leaf of an entry by the boundary
// marks and the max-scan of svt_tile.h, so a tile may cross any number of leaf edges.  Positions are 64-bit prefix sums
// (svt_scan.h), no atomic decides one, and two runs give the same bits.  Nothing is launched over an empty range.
#include "svt_common.h"
#include "svt_scan.h"
#include "svt_tile.h"

#include <type_traits>

#define SBA_NT SVT_TILE_NT
#define SBA_ITEMS SVT_TILE_ITEMS

enum { SBA_BAD_INDEX = 1, SBA_BAD_ORDER = 2 };

// last[r] = r (the whole axis) or -1; lsrc[c] = c (the whole axis) or -1
__global__ __launch_bounds__(SBA_NT) void subassign_init_kernel(int32_t *last, int64_t nrow, int whole_rows, int32_t *lsrc, int64_t ncol,
								 int whole_leaves)
{
	const int64_t i = (int64_t) blockIdx.x * SBA_NT + threadIdx.x;
	if (i < nrow) last[i] = whole_rows ? (int32_t) i : -1;
	if (i < ncol) lsrc[i] = whole_leaves ? (int32_t) i : -1;
}

// vector form: last[rows[p]] = max p.  SVT form: last[rows[p]] = p, the flag for rows[p] <= rows[p - 1].
template <bool SVT_FORM>
__global__ __launch_bounds__(SBA_NT) void subassign_rows_kernel(const int32_t *rows, int64_t nrows_sel, int64_t nrow, int32_t *last,
								 int *flag)
{
	const int64_t p = (int64_t) blockIdx.x * SBA_NT + threadIdx.x;
	if (p >= nrows_sel) return;
	const int64_t r = rows[p];
	if (r < 0 || r >= nrow) {
		atomicOr(flag, SBA_BAD_INDEX);
		return;
	}
	if constexpr (SVT_FORM) {
		if (p > 0 && rows[p - 1] >= r) {
			atomicOr(flag, SBA_BAD_ORDER);
			return;
		}
		last[r] = (int32_t) p;
	} else {
		atomicMax(&last[r], (int32_t) p);
	}
}

// lsrc[leaves[q]] = q: which leaf of v goes there (SVT form; a second claim of a leaf raises the flag), or 0 (vector
// form: covered, whoever wrote it)
template <bool SVT_FORM>
__global__ __launch_bounds__(SBA_NT) void subassign_leaves_kernel(const int32_t *leaves, int64_t nleaves_sel, int64_t ncol, int32_t *lsrc,
								   int *flag)
{
	const int64_t q = (int64_t) blockIdx.x * SBA_NT + threadIdx.x;
	if (q >= nleaves_sel) return;
	const int64_t c = leaves[q];
	if (c < 0 || c >= ncol) {
		atomicOr(flag, SBA_BAD_INDEX);
		return;
	}
	if constexpr (SVT_FORM) {
		if (atomicCAS(&lsrc[c], (int32_t) -1, (int32_t) q) != -1) atomicOr(flag, SBA_BAD_ORDER);
	} else {
		lsrc[c] = 0;
	}
}

template <typename T> __device__ inline bool sba_is_zero(T v) { return v == (T) 0; }      // -0.0 too; a NaN or NA is not

// rpos[r] = 1 for a covered row whose new value is not zero, else 0; rpos[nrow] = 0 (the scan's total: P)
template <typename T>
__global__ __launch_bounds__(SBA_NT) void subassign_rowflag_kernel(const int32_t *last, int64_t nrow, const T *vals, int64_t nvals,
								    int64_t *rpos)
{
	const int64_t r = (int64_t) blockIdx.x * SBA_NT + threadIdx.x;
	if (r > nrow) return;
	int64_t f = 0;
	if (r < nrow && last[r] >= 0) f = !sba_is_zero(vals[(int64_t) last[r] % nvals]);
	rpos[r] = f;
}

// the patch leaf: entry rpos[r] = (r, the row's new value) for every row flagged above
template <typename T>
__global__ __launch_bounds__(SBA_NT) void subassign_patch_kernel(const int32_t *last, int64_t nrow, const T *vals, int64_t nvals,
								  const int64_t *rpos, int32_t *prow, T *pval)
{
	const int64_t r = (int64_t) blockIdx.x * SBA_NT + threadIdx.x;
	if (r >= nrow || last[r] < 0) return;
	const T v = vals[(int64_t) last[r] % nvals];
	if (sba_is_zero(v)) return;
	prow[rpos[r]] = (int32_t) r;
	pval[rpos[r]] = v;
}

__global__ __launch_bounds__(SBA_NT) void subassign_cover_row_kernel(const int32_t *last, int64_t nrow, const int *flag,
								      unsigned char *cover_row)
{
	const int64_t r = (int64_t) blockIdx.x * SBA_NT + threadIdx.x;
	if (r >= nrow || *flag) return;
	cover_row[r] = last[r] >= 0;
}

// lp[c] = the entries of leaf c of Y: the patch leaf's *P (vector form) or those of leaf lsrc[c] of v, for a covered
// leaf; lp[ncol] = 0 (the scan's total)
__global__ __launch_bounds__(SBA_NT) void subassign_leaflen_kernel(const int32_t *lsrc, int64_t ncol, const int64_t *v_col_ptr,
								    const int64_t *P, int64_t *lp)
{
	const int64_t c = (int64_t) blockIdx.x * SBA_NT + threadIdx.x;
	if (c > ncol) return;
	int64_t l = 0;
	if (c < ncol && lsrc[c] >= 0) l = v_col_ptr != NULL ? v_col_ptr[lsrc[c] + 1] - v_col_ptr[lsrc[c]] : *P;
	lp[c] = l;
}

// the scanned lengths become Y.col_ptr and the leaf table is written unless the flag is up; head[1] <- the total
__global__ __launch_bounds__(SBA_NT) void subassign_publish_kernel(const int64_t *lp, const int32_t *lsrc, int64_t ncol, const int *flag,
								    int64_t *y_col_ptr, unsigned char *cover_leaf, int64_t *head)
{
	const int64_t c = (int64_t) blockIdx.x * SBA_NT + threadIdx.x;
	if (c == 0) head[1] = lp[ncol];
	if (c > ncol || *flag) return;
	y_col_ptr[c] = lp[c];
	if (c < ncol && cover_leaf != NULL) cover_leaf[c] = lsrc[c] >= 0;
}

// One tile of SVT_TILE entries of Y per workgroup: entry e of leaf c at offset k = e - ycp[c] is entry k of the patch
// leaf (vector form) or entry v_col_ptr[lsrc[c]] + k of v with its row renamed (SVT form).
template <typename T, bool SVT_FORM>
__global__ __launch_bounds__(SBA_NT) void subassign_fill_kernel(const int64_t *ycp, int64_t ncol, int64_t total, const int32_t *prow,
								 const T *pval, const int32_t *lsrc, const int64_t *v_col_ptr,
								 const int32_t *v_row_idx, const T *v_val, int64_t v_nnz, const int32_t *rows,
								 int64_t nrows_sel, int32_t *y_row_idx, T *y_val)
{
	__shared__ int seg[SVT_TILE];
	__shared__ int cmax[SVT_TILE_CHUNKS];
	__shared__ int64_t qq[2];
	const int tid = threadIdx.x, w = tid >> 6;
	const int64_t ts = (int64_t) blockIdx.x << SVT_TILE_SHIFT;
	if (ts >= total) return;
	const int n = (int) (total - ts < SVT_TILE ? total - ts : SVT_TILE);
	if (tid == 0) qq[0] = sub_last_le(ycp, ncol, ts);
	if (tid == SVT_WAVE) qq[1] = sub_last_le(ycp, ncol, ts + n - 1);
#pragma unroll
	for (int it = 0; it < SBA_ITEMS; it++) seg[it * SBA_NT + tid] = 0;
	__syncthreads();
	const int64_t q0 = qq[0], q1 = qq[1];
	// q0 < q <= q1: ts < ycp[q] <= ts + n - 1; one lane per boundary, the non-empty leaf of a position marks it
	for (int64_t q = q0 + 1 + tid; q <= q1; q += SBA_NT) {
		const int64_t p = ycp[q];
		if (ycp[q + 1] > p) seg[p - ts] = (int) (q - q0);
	}
	__syncthreads();
	int v[SBA_ITEMS];
	svt_tile_max_scan(seg, cmax, v);
#pragma unroll
	for (int it = 0; it < SBA_ITEMS; it++) {
		const int i = it * SBA_NT + tid;
		if (i >= n) continue;
		const int before = cmax[it * (SBA_NT / SVT_WAVE) + w];
		const int64_t c = q0 + (v[it] > before ? v[it] : before);
		const int64_t k = ts + i - ycp[c];
		if constexpr (SVT_FORM) {
			const int32_t sl = lsrc[c];
			if (sl < 0) continue;                       // (the count pass gave such a leaf no entries)
			const int64_t src = v_col_ptr[sl] + k;
			if (src < 0 || src >= v_nnz) continue;
			int32_t r = v_row_idx[src];
			if (rows != NULL) {
				if (r < 0 || r >= nrows_sel) continue;
				r = rows[r];
			}
			y_row_idx[ts + i] = r;
			y_val[ts + i] = v_val[src];
		} else {
			y_row_idx[ts + i] = prow[k];
			y_val[ts + i] = pval[k];
		}
	}
}

// ---------------------------------------------------------------------------
// launchers.  Workspace: [head 256: int flag, int64 entries of Y at byte 8][last int32[nrow]][rpos int64[nrow + 1]]
// [prow int32[nrow]][pval 8 * nrow][lsrc int32[ncol]][lp int64[ncol + 1]][scratch of the two scans, one after the other];
// the parts at multiples of 256
// ---------------------------------------------------------------------------
static inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
static inline unsigned blocks_for(int64_t n) { return (unsigned) ((n + SBA_NT - 1) / SBA_NT); }

int subassign_tile(void) { return SVT_TILE; }

struct SubassignWs {
	size_t last, rpos, prow, pval, lsrc, lp, scan, total;
};
static SubassignWs subassign_ws(int64_t nrow, int64_t ncol)
{
	SubassignWs L;
	if (nrow < 0) nrow = 0;
	if (ncol < 0) ncol = 0;
	L.last = 256;
	L.rpos = L.last + up256((size_t) nrow * 4);
	L.prow = L.rpos + up256(((size_t) nrow + 1) * 8);
	L.pval = L.prow + up256((size_t) nrow * 4);
	L.lsrc = L.pval + up256((size_t) nrow * 8);
	L.lp = L.lsrc + up256((size_t) ncol * 4);
	L.scan = L.lp + up256(((size_t) ncol + 1) * 8);
	const size_t s1 = exclusive_scan_ws_bytes(nrow + 1), s2 = exclusive_scan_ws_bytes(ncol + 1);
	L.total = L.scan + (s1 > s2 ? s1 : s2);
	return L;
}

size_t subassign_ws_bytes(int64_t nrow, int64_t ncol)
{
	return subassign_ws(nrow, ncol).total;
}

// f(typed vals / v_val) by the type of the new values (a logical value is an int32 value)
template <class F>
static inline void subassign_by_type(int v_Rtype, const void *p, F &&f)
{
	if (v_Rtype == SVT_REALSXP) f((const double *) p);
	else f((const int32_t *) p);
}

int launch_subassign_count(const SubassignArgs &a, int64_t *y_col_ptr, unsigned char *cover_row, unsigned char *cover_leaf, void *ws,
			   hipStream_t s)
{
	const SubassignWs L = subassign_ws(a.nrow, a.ncol);
	const bool svt_form = a.v_col_ptr != NULL;
	const int64_t nrow = a.nrow, ncol = a.ncol, big = nrow > ncol ? nrow : ncol;
	char *w = (char *) ws;
	int *flag = (int *) w;
	int32_t *last = (int32_t *) (w + L.last), *lsrc = (int32_t *) (w + L.lsrc);
	int64_t *rpos = (int64_t *) (w + L.rpos), *lp = (int64_t *) (w + L.lp);
	HIP_TRY(hipMemsetAsync(w, 0, 256, s));
	if (big > 0)
		hipLaunchKernelGGL(subassign_init_kernel, dim3(blocks_for(big)), dim3(SBA_NT), 0, s, last, nrow, (int) (a.nrows_sel < 0), lsrc,
				   ncol, (int) (a.nleaves_sel < 0));
	if (a.nrows_sel > 0) {
		if (svt_form)
			hipLaunchKernelGGL(subassign_rows_kernel<true>, dim3(blocks_for(a.nrows_sel)), dim3(SBA_NT), 0, s, a.rows, a.nrows_sel,
					   nrow, last, flag);
		else
			hipLaunchKernelGGL(subassign_rows_kernel<false>, dim3(blocks_for(a.nrows_sel)), dim3(SBA_NT), 0, s, a.rows, a.nrows_sel,
					   nrow, last, flag);
	}
	if (a.nleaves_sel > 0) {
		if (svt_form)
			hipLaunchKernelGGL(subassign_leaves_kernel<true>, dim3(blocks_for(a.nleaves_sel)), dim3(SBA_NT), 0, s, a.leaves,
					   a.nleaves_sel, ncol, lsrc, flag);
		else
			hipLaunchKernelGGL(subassign_leaves_kernel<false>, dim3(blocks_for(a.nleaves_sel)), dim3(SBA_NT), 0, s, a.leaves,
					   a.nleaves_sel, ncol, lsrc, flag);
	}
	if (!svt_form) {
		subassign_by_type(a.v_Rtype, a.vals, [&](auto *vals) {
			typedef std::remove_const_t<std::remove_pointer_t<decltype(vals)>> T;
			hipLaunchKernelGGL(subassign_rowflag_kernel<T>, dim3(blocks_for(nrow + 1)), dim3(SBA_NT), 0, s, (const int32_t *) last, nrow,
					   vals, a.nvals, rpos);
		});
		if (launch_exclusive_scan_i64(rpos, nrow + 1, w + L.scan, s))
			return -1;
		if (nrow > 0)
			subassign_by_type(a.v_Rtype, a.vals, [&](auto *vals) {
				typedef std::remove_const_t<std::remove_pointer_t<decltype(vals)>> T;
				hipLaunchKernelGGL(subassign_patch_kernel<T>, dim3(blocks_for(nrow)), dim3(SBA_NT), 0, s, (const int32_t *) last, nrow,
						   vals, a.nvals, (const int64_t *) rpos, (int32_t *) (w + L.prow), (T *) (w + L.pval));
			});
	}
	if (cover_row != NULL && nrow > 0)
		hipLaunchKernelGGL(subassign_cover_row_kernel, dim3(blocks_for(nrow)), dim3(SBA_NT), 0, s, (const int32_t *) last, nrow,
				   (const int *) flag, cover_row);
	hipLaunchKernelGGL(subassign_leaflen_kernel, dim3(blocks_for(ncol + 1)), dim3(SBA_NT), 0, s, (const int32_t *) lsrc, ncol, a.v_col_ptr,
			   (const int64_t *) (rpos + nrow), lp);
	if (launch_exclusive_scan_i64(lp, ncol + 1, w + L.scan, s))
		return -1;
	hipLaunchKernelGGL(subassign_publish_kernel, dim3(blocks_for(ncol + 1)), dim3(SBA_NT), 0, s, (const int64_t *) lp,
			   (const int32_t *) lsrc, ncol, (const int *) flag, y_col_ptr, cover_leaf, (int64_t *) w);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_subassign_fill(const SubassignArgs &a, const int64_t *y_col_ptr, int64_t y_nnz, int32_t *y_row_idx, void *y_val,
			  const void *ws, hipStream_t s)
{
	if (y_nnz <= 0)
		return 0;
	const SubassignWs L = subassign_ws(a.nrow, a.ncol);
	const int64_t ntiles = (y_nnz + SVT_TILE - 1) >> SVT_TILE_SHIFT;
	if (ntiles > 0x7FFFFFFFLL)
		return svt_set_error("svt_dev_subassign_place_fill: too many entries");
	const char *w = (const char *) ws;
	const int32_t *prow = (const int32_t *) (w + L.prow), *lsrc = (const int32_t *) (w + L.lsrc);
	subassign_by_type(a.v_Rtype, a.v_col_ptr != NULL ? a.v_val : (const void *) (w + L.pval), [&](auto *vv) {
		typedef std::remove_const_t<std::remove_pointer_t<decltype(vv)>> T;
		if (a.v_col_ptr != NULL)
			hipLaunchKernelGGL((subassign_fill_kernel<T, true>), dim3((unsigned) ntiles), dim3(SBA_NT), 0, s, y_col_ptr, a.ncol, y_nnz,
					   prow, (const T *) NULL, lsrc, a.v_col_ptr, a.v_row_idx, vv, a.v_nnz,
					   a.nrows_sel < 0 ? (const int32_t *) NULL : a.rows, a.nrows_sel, y_row_idx, (T *) y_val);
		else
			hipLaunchKernelGGL((subassign_fill_kernel<T, false>), dim3((unsigned) ntiles), dim3(SBA_NT), 0, s, y_col_ptr, a.ncol, y_nnz,
					   prow, vv, lsrc, (const int64_t *) NULL, (const int32_t *) NULL, (const T *) NULL, (int64_t) 0,
					   (const int32_t *) NULL, (int64_t) 0, y_row_idx, (T *) y_val);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}
