// abind() / cbind() / rbind() of resident operands (C_abind_SVT_SparseArray_objects, src/SparseArray_abind.c, on the
// device layout col_ptr / row_idx / val; the rules are stated once in include/svt_hip.h).  A pure copy: the result is a
// sequence of PIECES, each a whole leaf of one object,
//
//   along the rows       piece p = L * nobj + n      leaf L of object n, its rows shifted by off[n]
//   along a leaf dim     piece p = q = a + inner * (j + D * c)   leaf a + inner * ((j - start[n]) + ext[n] * c) of the
//                                                    object n whose [start[n], start[n] + ext[n]) holds j
//
// and a result entry is entry `e - start of its piece` of that leaf.
//
// Count pass: one thread per piece finds its object and leaf (the only divisions, and the only search over the
// objects -- a binary search over start[]) and writes the leaf's length; one 64-bit exclusive scan (svt_scan.h) turns
// the lengths into the piece starts ps[0 .. npieces]; one more thread per piece writes the piece's descriptor and the
// result's col_ptr at the leaf boundaries.  The descriptor is the source folded into two addresses,
//
//   row_addr = &row_idx_n[leaf start] - 4 * ps[p]      val_addr = &val_n[leaf start] - elt size * ps[p]
//
// so that the copy pass reads entry e of the result at row_addr + 4 * e: no division, no search, no object table per
// entry.  (Kept as integers: the address of entry 0 of the result may lie before the object's array.)
//
// Copy pass: the tiles of svt_tile.h over the RESULT's entries, like the column gather of kernels_subset.hip -- the
// pieces a tile touches by two binary searches over ps (two threads), one lane per piece boundary inside the tile, the
// max-scan.  Every load and store of the nonzero arrays is coalesced; no atomic decides a position; every position is
// 64-bit.  Templated on the result type and on whether every object has its element size: the uniform kernels load the
// value as it is, only the mixed double kernel looks at the piece's element size (without a branch).
#include "svt_common.h"
#include "svt_scan.h"
#include "svt_tile.h"

#define ABIND_GRID 2048                 // the copy's grid at most: 8 workgroups of 16 KB LDS on each of 256 CUs

static_assert(sizeof(AbindObj) == 64, "the workspace is carved by this size");

struct AbindPiece {
	int64_t row_addr, val_addr;
	int32_t off;            // added to every row
	int32_t vshift;         // log2 of the source's element size: 3 a double, 2 an integer or a logical
};
static_assert(sizeof(AbindPiece) == 24, "the workspace is carved by this size");

struct AbindShape {
	int64_t npieces;
	int nobj;
	int rows_form;
	int64_t inner, D;       // leaf dim only
};

// object and leaf of piece p < npieces
__device__ inline void abind_source(const AbindShape &S, const AbindObj *objs, int64_t p, int *n_out, int64_t *leaf_out)
{
	if (S.rows_form) {
		*n_out = (int) (p % S.nobj);
		*leaf_out = p / S.nobj;
		return;
	}
	const int64_t a = p % S.inner, t = p / S.inner, j = t % S.D, c = t / S.D;
	int lo = 0, hi = S.nobj;            // the last n with start[n] <= j: an object of extent > 0 (the others share
	while (hi - lo > 1) {               // their start with the next one)
		const int mid = lo + (hi - lo) / 2;
		if (objs[mid].shift <= j) lo = mid; else hi = mid;
	}
	*n_out = lo;
	*leaf_out = a + S.inner * ((j - objs[lo].shift) + objs[lo].ext * c);
}

// len[p] = length of piece p, len[npieces] = 0 (the scan's total); the flag for a leaf outside the object, pointers that
// descend or that pass the object's nnz -- nothing is read through such a pointer, the piece counts as empty
__global__ __launch_bounds__(SVT_TILE_NT) void abind_len_kernel(AbindShape S, const AbindObj *objs, int64_t *len, int *flag)
{
	const int64_t p = (int64_t) blockIdx.x * SVT_TILE_NT + threadIdx.x;
	if (p > S.npieces) return;
	int64_t l = 0;
	if (p < S.npieces) {
		int n;
		int64_t leaf;
		abind_source(S, objs, p, &n, &leaf);
		const AbindObj &O = objs[n];
		if (leaf < 0 || leaf >= O.nleaves) {
			atomicOr(flag, 1);
		} else {
			const int64_t s = O.col_ptr[leaf], e = O.col_ptr[leaf + 1];
			if (s < 0 || e < s || e > O.nnz) atomicOr(flag, 1);
			else l = e - s;
		}
	}
	len[p] = l;
}

// after the scan: the descriptors, out_col_ptr at the leaf boundaries (unless the flag is up), head[1] <- the total
__global__ __launch_bounds__(SVT_TILE_NT) void abind_publish_kernel(AbindShape S, const AbindObj *objs, const int64_t *ps,
								    AbindPiece *desc, const int *flag, int64_t *out_col_ptr,
								    int64_t *head)
{
	const int64_t p = (int64_t) blockIdx.x * SVT_TILE_NT + threadIdx.x;
	if (p == 0) head[1] = ps[S.npieces];
	if (p > S.npieces || *flag) return;
	if (S.rows_form) {
		if (p % S.nobj == 0) out_col_ptr[p / S.nobj] = ps[p];
	} else {
		out_col_ptr[p] = ps[p];
	}
	if (p == S.npieces) return;
	int n;
	int64_t leaf;
	abind_source(S, objs, p, &n, &leaf);
	const AbindObj &O = objs[n];
	const int64_t delta = O.col_ptr[leaf] - ps[p];
	AbindPiece d;
	d.row_addr = (int64_t) (uintptr_t) O.row_idx + 4 * delta;
	d.vshift = O.Rtype == SVT_REALSXP ? 3 : 2;
	d.val_addr = (int64_t) (uintptr_t) O.val + (delta << d.vshift);
	d.off = S.rows_form ? (int32_t) O.shift : 0;
	desc[p] = d;
}

// One tile of SVT_TILE result entries per trip.  seg[i]: for the first entry of every piece that starts inside the tile,
// the piece (relative to p0, the piece of the tile's first entry); svt_tile_max_scan spreads it over the piece's entries.
template <typename OutT, bool UNIFORM>
__global__ __launch_bounds__(SVT_TILE_NT) void abind_copy_kernel(const int64_t *ps, int64_t npieces, const AbindPiece *desc,
								 int32_t *out_row_idx, OutT *out_val)
{
	__shared__ int seg[SVT_TILE];
	__shared__ int cmax[SVT_TILE_CHUNKS];
	__shared__ int64_t pp[2];
	const int tid = threadIdx.x, w = tid >> 6;
	const int64_t total = ps[npieces];
	for (int64_t ts = (int64_t) blockIdx.x << SVT_TILE_SHIFT; ts < total; ts += (int64_t) gridDim.x << SVT_TILE_SHIFT) {
		const int n = (int) (total - ts < SVT_TILE ? total - ts : SVT_TILE);
		if (tid == 0) pp[0] = sub_last_le(ps, npieces, ts);
		if (tid == SVT_WAVE) pp[1] = sub_last_le(ps, npieces, ts + n - 1);
#pragma unroll
		for (int it = 0; it < SVT_TILE_ITEMS; it++) seg[it * SVT_TILE_NT + tid] = 0;
		__syncthreads();
		const int64_t p0 = pp[0], p1 = pp[1];
		// p0 < p <= p1 < npieces: ts < ps[p] <= ts + n - 1; one lane per boundary, the non-empty piece of a position marks it
		for (int64_t p = p0 + 1 + tid; p <= p1; p += SVT_TILE_NT) {
			const int64_t s = ps[p];
			if (ps[p + 1] > s) seg[s - ts] = (int) (p - p0);
		}
		__syncthreads();
		int v[SVT_TILE_ITEMS];
		svt_tile_max_scan(seg, cmax, v);
#pragma unroll
		for (int it = 0; it < SVT_TILE_ITEMS; it++) {
			const int i = it * SVT_TILE_NT + tid;
			if (i >= n) continue;
			const int before = cmax[it * (SVT_TILE_NT / SVT_WAVE) + w];
			const AbindPiece d = desc[p0 + (v[it] > before ? v[it] : before)];
			const int64_t e = ts + i;
			out_row_idx[e] = *(const int32_t *) (uintptr_t) (d.row_addr + 4 * e) + d.off;
			if constexpr (UNIFORM) {
				out_val[e] = *(const OutT *) (uintptr_t) (d.val_addr + (int64_t) sizeof(OutT) * e);
			} else {
				// No branch on the piece's type (it would keep the 16 entries of a thread from being in flight
				// together): the low word of either element, and the high word of a double -- for an integer the
				// same word again, never the word after the array.  integer or logical -> double: NA_integer_
				// becomes NA_real_.
				const int64_t a = d.val_addr + (e << d.vshift);
				const int32_t lo = *(const int32_t *) (uintptr_t) a;
				const int32_t hi = *(const int32_t *) (uintptr_t) (a + ((d.vshift & 1) << 2));
				const double asis = __hiloint2double(hi, lo);
				const double conv = lo == NA_INT ? svt_na_real() : (double) lo;
				out_val[e] = (OutT) (d.vshift == 3 ? asis : conv);
			}
		}
		__syncthreads();                           // seg, cmax and pp are written again by the next trip
	}
}

// ---------------------------------------------------------------------------
// launchers.  Workspace: [head 256: int flag, int64 total at byte 8][objects AbindObj[nobj]][ps int64[npieces + 1]]
// [descriptors AbindPiece[npieces]][scratch of the scan]; the parts at multiples of 256 bytes
// ---------------------------------------------------------------------------
static inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
static inline unsigned blocks_for(int64_t n) { return (unsigned) ((n + SVT_TILE_NT - 1) / SVT_TILE_NT); }

struct AbindWs {
	size_t objs, ps, desc, scan, total;
};
static AbindWs abind_ws(int nobj, int64_t npieces)
{
	AbindWs L;
	if (nobj < 0) nobj = 0;
	if (npieces < 0) npieces = 0;
	L.objs = 256;
	L.ps = L.objs + up256((size_t) nobj * sizeof(AbindObj));
	L.desc = L.ps + up256(((size_t) npieces + 1) * 8);
	L.scan = L.desc + up256((size_t) npieces * sizeof(AbindPiece));
	L.total = L.scan + exclusive_scan_ws_bytes(npieces + 1);
	return L;
}

int abind_tile(void) { return SVT_TILE; }

size_t abind_ws_bytes(int nobj, int64_t npieces)
{
	return abind_ws(nobj, npieces).total;
}

int launch_abind_count(const AbindArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s)
{
	const AbindWs L = abind_ws(a.nobj, a.npieces);
	char *w = (char *) ws;
	AbindObj *objs = (AbindObj *) (w + L.objs);
	int64_t *ps = (int64_t *) (w + L.ps);
	const AbindShape S = { a.npieces, a.nobj, a.rows_form, a.inner, a.D };
	HIP_TRY(hipMemsetAsync(w, 0, 256, s));
	HIP_TRY(hipMemcpyAsync(objs, a.objs, (size_t) a.nobj * sizeof(AbindObj), hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(abind_len_kernel, dim3(blocks_for(a.npieces + 1)), dim3(SVT_TILE_NT), 0, s, S, (const AbindObj *) objs, ps,
			   (int *) w);
	if (launch_exclusive_scan_i64(ps, a.npieces + 1, w + L.scan, s))
		return -1;
	hipLaunchKernelGGL(abind_publish_kernel, dim3(blocks_for(a.npieces + 1)), dim3(SVT_TILE_NT), 0, s, S, (const AbindObj *) objs,
			   (const int64_t *) ps, (AbindPiece *) (w + L.desc), (const int *) w, out_col_ptr, (int64_t *) w);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_abind_fill(const AbindArgs &a, int32_t *out_row_idx, void *out_val, const void *ws, hipStream_t s)
{
	if (a.npieces <= 0 || a.max_nnz <= 0)
		return 0;
	const AbindWs L = abind_ws(a.nobj, a.npieces);
	const char *w = (const char *) ws;
	const int64_t *ps = (const int64_t *) (w + L.ps);
	const AbindPiece *desc = (const AbindPiece *) (w + L.desc);
	const int64_t ntiles = (a.max_nnz + SVT_TILE - 1) >> SVT_TILE_SHIFT;
	const dim3 grid((unsigned) (ntiles < ABIND_GRID ? ntiles : ABIND_GRID)), block(SVT_TILE_NT);
	if (a.ans_Rtype != SVT_REALSXP)
		hipLaunchKernelGGL((abind_copy_kernel<int32_t, true>), grid, block, 0, s, ps, a.npieces, desc, out_row_idx,
				   (int32_t *) out_val);
	else if (a.uniform)
		hipLaunchKernelGGL((abind_copy_kernel<double, true>), grid, block, 0, s, ps, a.npieces, desc, out_row_idx,
				   (double *) out_val);
	else
		hipLaunchKernelGGL((abind_copy_kernel<double, false>), grid, block, 0, s, ps, a.npieces, desc, out_row_idx,
				   (double *) out_val);
	HIP_TRY(hipGetLastError());
	return 0;
}
