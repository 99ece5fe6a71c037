// Arith and Math on resident sparse operands (C_Arith_SVT1_SVT2, C_Arith_SVT1_v2, C_unary_minus_SVT, C_Math_SVT of the
// reference; the element rules are in svt_arith_rules.h).  Three families, each a count pass and a fill pass over the
// same tiles:
//
//   map     f(v) on the stored values of one operand; an entry is kept when its result is not zero
//   sweep   f(v, stats[k]) on the stored values of one operand, k the entry's row, its leaf or both (sweep() and R's
//           recycling of a vector of length nrow); kept when not zero; the vector is checked on the device first
//   merge   x op y, op in + - *: the two entry sequences, each ascending by (column, row), merged; a position stored
//           on one side meets an implicit zero, a position stored on both is ONE result entry
//
// The rules are those of kernels_subset.hip.  A TILE is ARI_TILE = 2048 consecutive entries -- of the operand for the
// map, of the merged sequence (length nnz(x) + nnz(y): a matching pair takes two places, x's entry first) for the merge
// -- one tile per 256-thread workgroup, entry it * 256 + tid of the tile in trip `it`.  The columns a tile touches are
// found by two binary searches over the column pointers (of the merged sequence: col_ptr_x[q] + col_ptr_y[q]); the kept
// entries before a column boundary inside the tile are counted by one lane per boundary from the wavefront ballots;
// every output position is tile prefix + chunk prefix + popcount below the lane, in 64 bits.  No atomic decides a
// position (the one atomic raises the overflow flag), rows ascend inside every result column, and two runs give the
// same bits.
//
// The merge cuts the merged sequence by a merge-path search per tile boundary (arith_merge_cut_kernel: cut[t] = how
// many of the first t * ARI_TILE merged entries are x's; equal keys: x's entry first).  A tile then loads the keys
// column * nrow + row of its x part and its y part into LDS -- the column of an entry by binary search over the column
// pointers, inside the tile's column range -- every thread finds its own 8 consecutive merged places by a merge-path
// search in LDS and walks them, leaving per place the source (side, index, pair flag), and the values are then read
// and combined in the striped order.  A matching pair is owned by its x entry: that entry looks at the next y key
// (the first key of the next thread's or the next tile's y part: one key past the part is loaded), the y entry looks
// at the x key before it (one key before the part is loaded) and emits nothing.
//
// Compare and Logic (C_Compare_SVT1_v2, C_Compare_SVT1_SVT2, C_Logic_SVT1_SVT2; the rules svt_rule_compare and
// svt_rule_logic) are further rules on the same two families: the tile evaluators and the four tile kernels take the
// rule as a template parameter (ARI_RULE_ARITH / _COMPARE / _LOGIC), the result of the two new rules is int32 whatever
// the operands, and no overflow is raised.  Everything else -- tiles, column search, ranking, placement, the cut, the
// ownership of a pair, the workspace -- is shared as it is.
//
// Subassignment x[i, j] <- value is a fourth rule on the merge (ARI_RULE_ASSIGN, svt_rule_assign): y is the placed
// operand kernels_subassign.hip builds, the rule reads two cover tables in place of an opcode, the result is double when
// either side is and int32 else, and no overflow is raised.  It adds nothing to the LDS: the leaf of an x entry is found
// again from the x part's column range (sh.rng), not kept next to its key.
//
// Subassignment by an L-index or M-index is a fifth (ARI_RULE_ASSIGN_CELLS, svt_rule_assign_cells): y is the placed
// operand kernels_lindex.hip builds, a zero in it deletes, an x entry alone always stays; it reads no table and no opcode.
//
// pmin / pmax (ARI_RULE_PMINMAX, svt_rule_pminmax: .pminmax2 of the reference cell by cell) is a sixth rule, on all three
// families: both sides widened to the result's type, the opcode carrying min / max and na.rm, the scalar or vector element
// checked as the Arith and Compare ones are.  is.na / is.nan / is.infinite (ARI_RULE_ISFUN, svt_rule_isfun) is a seventh,
// on the map alone, with an int32 result.  Neither raises an overflow; neither adds a kernel body, a byte of LDS or a
// workspace part.
//
// LDS: keys 8 * (2048 + 2), sources 4 * 2048, ballots and chunk prefixes 0.4 KB: 24.5 KB for the merge (6 workgroups
// of a CU's 160 KB), 0.4 KB for the map.
#include "svt_common.h"
#include "svt_scan.h"
#include "svt_arith_rules.h"

#include <type_traits>

#define ARI_NT 256
#define ARI_ITEMS 8
#define ARI_TILE (ARI_NT * ARI_ITEMS)
#define ARI_SHIFT 11
#define ARI_CHUNKS (ARI_TILE / SVT_WAVE)
#define ARI_WAVES (ARI_NT / SVT_WAVE)
static_assert(ARI_TILE == 1 << ARI_SHIFT && ARI_CHUNKS <= SVT_WAVE, "one wavefront scans the chunk table of a tile");

#define ARI_FROM_Y 0x80000000u          // source word of a merged place: side, pair / duplicate flag, index in the part
#define ARI_PAIRED 0x40000000u
#define ARI_INDEX 0x00000FFFu

// the column pointers of the sequence the tiles cut: one operand's, or the sum of two (the merged sequence)
struct AriPtr {
	const int64_t *a, *b;
	__device__ int64_t operator()(int64_t q) const { return b ? a[q] + b[q] : a[q]; }
};
// the last q in [lo, hi] with P(q) <= x (P ascending, P(lo) <= x)
template <class P>
__device__ inline int64_t ari_last_le(const P &ptr, int64_t lo, int64_t hi, int64_t x)
{
	hi++;
	while (hi - lo > 1) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (ptr(mid) <= x) lo = mid; else hi = mid;
	}
	return lo;
}
// the first q in [0, n] with P(q) >= x (x <= P(n))
template <class P>
__device__ inline int64_t ari_first_ge(const P &ptr, int64_t n, int64_t x)
{
	int64_t lo = -1, hi = n;
	while (hi - lo > 1) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (ptr(mid) >= x) hi = mid; else lo = mid;
	}
	return hi;
}

struct AriShared {
	unsigned long long ballots[ARI_CHUNKS];
	int cpre[ARI_CHUNKS + 1];
	int64_t qq[2];
};

// ballots[c] = the kept entries of chunk c as a mask, cpre[c] = how many are kept in the chunks before c,
// cpre[ARI_CHUNKS] = in the tile
__device__ inline void ari_rank(const bool (&keep)[ARI_ITEMS], AriShared &sh)
{
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
	for (int it = 0; it < ARI_ITEMS; it++) {
		const unsigned long long b = __ballot(keep[it]);
		if (lane == 0) sh.ballots[it * ARI_WAVES + w] = b;
	}
	__syncthreads();
	if (tid < SVT_WAVE) {
		const int c = tid < ARI_CHUNKS ? __popcll(sh.ballots[tid]) : 0;
		int incl = c;
		for (int o = 1; o < SVT_WAVE; o <<= 1) {
			const int t = __shfl_up(incl, o, SVT_WAVE);
			if (lane >= o) incl += t;
		}
		if (tid < ARI_CHUNKS) sh.cpre[tid] = incl - c;
		if (tid == ARI_CHUNKS - 1) sh.cpre[ARI_CHUNKS] = incl;
	}
	__syncthreads();
}

// the count pass's end: tile_cnt[tile] = kept entries of the tile; local[q] = kept entries of the tile before P(q), for
// every column q that starts inside the tile (sh.qq: the first and the last such column, found before the last barrier)
__device__ inline void ari_count_tail(const AriPtr &P, int64_t ts, const AriShared &sh, int64_t *tile_cnt, int32_t *local)
{
	const int tid = threadIdx.x;
	if (tid == 0) tile_cnt[blockIdx.x] = sh.cpre[ARI_CHUNKS];
	const int64_t q1 = sh.qq[1];
	for (int64_t q = sh.qq[0] + tid; q <= q1; q += ARI_NT) {          // ts <= P(q) <= ts + n - 1
		const int p = (int) (P(q) - ts);
		local[q] = sh.cpre[p >> 6] + __popcll(sh.ballots[p >> 6] & ((1ULL << (p & 63)) - 1ULL));
	}
}
__device__ inline void ari_tile_columns(const AriPtr &P, int64_t ncol, int64_t ts, int n, AriShared &sh)
{
	if (threadIdx.x == 0) sh.qq[0] = ari_first_ge(P, ncol, ts);
	if (threadIdx.x == SVT_WAVE) sh.qq[1] = ari_last_le(P, 0, ncol, ts + n - 1);
}
// where kept entry `it` of this thread goes
__device__ inline int64_t ari_position(int64_t base, int it, const AriShared &sh)
{
	const int lane = threadIdx.x & 63, c = it * ARI_WAVES + (threadIdx.x >> 6);
	return base + sh.cpre[c] + __popcll(sh.ballots[c] & ((1ULL << lane) - 1ULL));
}

// out_col_ptr[j] = kept entries before P(j): those of the tiles before + those of its tile before it.  head[1] <- the
// kept entries in all.
__global__ __launch_bounds__(ARI_NT) void arith_ptr_kernel(AriPtr P, int64_t ncol, int64_t total, const int64_t *tile_pre,
							   int64_t ntiles, const int32_t *local, int64_t *out_col_ptr, int64_t *head)
{
	const int64_t j = (int64_t) blockIdx.x * ARI_NT + threadIdx.x;
	if (j == 0) head[1] = tile_pre[ntiles];
	if (j > ncol) return;
	const int64_t p = P(j);
	out_col_ptr[j] = p >= total ? tile_pre[ntiles] : tile_pre[p >> ARI_SHIFT] + local[j];
}

template <typename T> __device__ inline bool ari_is_zero(T v) { return v == (T) 0; }      // -0.0 too; a NaN is kept

// ---------------------------------------------------------------------------
// map
// ---------------------------------------------------------------------------
struct AriMapOp {
	int kind, op;
	double sd;          // the scalar as a double
	int32_t si;         // and as an integer (integer results)
};

template <typename TX, typename TO, int RULE>
__device__ inline TO ari_map_eval(const AriMapOp &m, TX v, int *ovf)
{
	if constexpr (RULE == ARI_RULE_COMPARE) {
		return svt_rule_compare(m.op, svt_rule_as_double(v), m.sd);
	} else if constexpr (RULE == ARI_RULE_ISFUN) {
		return svt_rule_isfun(m.op, v);
	} else if constexpr (RULE == ARI_RULE_PMINMAX) {
		TO x;
		svt_rule_widen(v, &x);
		if constexpr (std::is_same<TO, int32_t>::value) return svt_rule_pminmax(m.op & ~SVT_PMINMAX_NA_RM, m.op & SVT_PMINMAX_NA_RM, x, m.si);
		else return svt_rule_pminmax(m.op & ~SVT_PMINMAX_NA_RM, m.op & SVT_PMINMAX_NA_RM, x, m.sd);
	} else if constexpr (std::is_same<TO, int32_t>::value) {
		if (m.kind == SVT_ARITH_NEG) return v == NA_INT ? NA_INT : -v;
		return svt_rule_arith_int(m.op, v, m.si, ovf);
	} else {
		const double x = svt_rule_as_double(v);
		if (m.kind == SVT_ARITH_NEG) return -x;
		if (m.kind == SVT_ARITH_MATH) return svt_rule_math(m.op, x);
		return svt_rule_arith_double(m.op, x, m.sd);
	}
}

// the results of this thread's entries of the tile (striped) and whether they are kept
template <typename TX, typename TO, int RULE>
__device__ inline void ari_map_tile(const TX *val, int64_t ts, int n, const AriMapOp &m, TO (&r)[ARI_ITEMS],
				    bool (&keep)[ARI_ITEMS], int *ovf)
{
#pragma unroll
	for (int it = 0; it < ARI_ITEMS; it++) {
		const int i = it * ARI_NT + threadIdx.x;
		keep[it] = false;
		if (i < n) {
			r[it] = ari_map_eval<TX, TO, RULE>(m, val[ts + i], ovf);
			keep[it] = !ari_is_zero(r[it]);
		}
	}
}

template <typename TX, typename TO, int RULE>
__global__ __launch_bounds__(ARI_NT) void arith_map_count_kernel(const int64_t *col_ptr, const TX *val, int64_t ncol, int64_t nnz,
								 AriMapOp m, int64_t *tile_cnt, int32_t *local)
{
	__shared__ AriShared sh;
	const int64_t ts = (int64_t) blockIdx.x << ARI_SHIFT;
	const int n = (int) (nnz - ts < ARI_TILE ? nnz - ts : ARI_TILE);
	const AriPtr P = { col_ptr, NULL };
	ari_tile_columns(P, ncol, ts, n, sh);
	TO r[ARI_ITEMS];
	bool keep[ARI_ITEMS];
	int ovf = 0;
	ari_map_tile<TX, TO, RULE>(val, ts, n, m, r, keep, &ovf);
	ari_rank(keep, sh);
	ari_count_tail(P, ts, sh, tile_cnt, local);
}

template <typename TX, typename TO, int RULE>
__global__ __launch_bounds__(ARI_NT) void arith_map_fill_kernel(const int32_t *row_idx, const TX *val, int64_t nnz, AriMapOp m,
								const int64_t *tile_pre, int32_t *out_row_idx, TO *out_val,
								int *ovflow)
{
	__shared__ AriShared sh;
	const int64_t ts = (int64_t) blockIdx.x << ARI_SHIFT;
	const int n = (int) (nnz - ts < ARI_TILE ? nnz - ts : ARI_TILE);
	TO r[ARI_ITEMS];
	bool keep[ARI_ITEMS];
	int ovf = 0;
	ari_map_tile<TX, TO, RULE>(val, ts, n, m, r, keep, &ovf);
	ari_rank(keep, sh);
	const int64_t base = tile_pre[blockIdx.x];
#pragma unroll
	for (int it = 0; it < ARI_ITEMS; it++) {
		if (!keep[it]) continue;
		const int64_t pos = ari_position(base, it, sh);
		out_row_idx[pos] = row_idx[ts + it * ARI_NT + threadIdx.x];
		out_val[pos] = r[it];
	}
	if (ovf && ovflow != NULL) atomicOr(ovflow, 1);
}

// ---------------------------------------------------------------------------
// merge
// ---------------------------------------------------------------------------
struct AriSide {
	const int64_t *col_ptr;
	const int32_t *row_idx;
	int64_t nnz;
};
struct AriColPtr {
	const int64_t *p;
	__device__ int64_t operator()(int64_t q) const { return p[q]; }
};
// key of entry g of a side whose column lies in [qlo, qhi]
__device__ inline int64_t ari_key(const AriSide &S, int64_t qlo, int64_t qhi, int64_t nrow, int64_t g)
{
	const AriColPtr cp = { S.col_ptr };
	return ari_last_le(cp, qlo, qhi, g) * nrow + S.row_idx[g];
}

// cut[t] = how many of the first min(t * ARI_TILE, total) merged entries are x's, t in [0, ntiles]
__global__ __launch_bounds__(ARI_NT) void arith_merge_cut_kernel(AriSide X, AriSide Y, int64_t ncol, int64_t nrow, int64_t ntiles,
								 int64_t *cut)
{
	const int64_t t = (int64_t) blockIdx.x * ARI_NT + threadIdx.x;
	if (t > ntiles) return;
	const int64_t total = X.nnz + Y.nnz;
	const int64_t d = t << ARI_SHIFT < total ? t << ARI_SHIFT : total;
	int64_t lo = d - Y.nnz > 0 ? d - Y.nnz : 0, hi = d < X.nnz ? d : X.nnz;
	while (lo < hi) {                                   // x[mid] before y[d - 1 - mid]: more than mid of x's among the first d
		const int64_t mid = lo + (hi - lo) / 2;
		if (ari_key(X, 0, ncol, nrow, mid) <= ari_key(Y, 0, ncol, nrow, d - 1 - mid)) lo = mid + 1; else hi = mid;
	}
	cut[t] = lo;
}

struct AriMergeShared {
	AriShared r;
	int64_t keys[ARI_TILE + 2];     // [x key before the part][x part: na keys][y part: nb keys][y key after the part]
	uint32_t src[ARI_TILE];
	int64_t rng[4];                 // column ranges of the two parts
};

template <typename TX, typename TY, int RULE> struct AriMergeOut {
	typedef typename std::conditional<RULE == ARI_RULE_COMPARE || RULE == ARI_RULE_LOGIC ||
					  (std::is_same<TX, int32_t>::value && std::is_same<TY, int32_t>::value),
					  int32_t, double>::type type;
};
// what a rule reads besides the two values: the opcode, or, for the subassignment rule, the cover tables (one byte per
// row, one per leaf; NULL: the whole axis).  The kernels of the other rules keep their `int op` argument as it was.
struct AriCover {
	const unsigned char *row, *leaf;
};
template <int RULE> struct AriOp { typedef int type; };
template <> struct AriOp<ARI_RULE_ASSIGN> { typedef AriCover type; };
template <int RULE> static inline typename AriOp<RULE>::type ari_op(const ArithMergeArgs &a)
{
	if constexpr (RULE == ARI_RULE_ASSIGN) return AriCover{ a.cover_row, a.cover_leaf };
	else return a.op;
}

// One tile of the merged sequence: merged places [ts, ts + n), x entries [a0, a0 + na), y entries [b0, b0 + nb).  Leaves
// per striped place of this thread the result, its row and whether it is kept.
template <typename TX, typename TY, int RULE>
__device__ inline void ari_merge_tile(const AriSide &X, const TX *xval, const AriSide &Y, const TY *yval, int64_t ncol, int64_t nrow,
				      const typename AriOp<RULE>::type &op, int64_t a0, int na, int64_t b0, int nb, AriMergeShared &sh,
				      typename AriMergeOut<TX, TY, RULE>::type (&r)[ARI_ITEMS], int32_t (&row)[ARI_ITEMS],
				      bool (&keep)[ARI_ITEMS], int *ovf)
{
	typedef typename AriMergeOut<TX, TY, RULE>::type TO;
	const int tid = threadIdx.x, n = na + nb;
	const AriColPtr xcp = { X.col_ptr }, ycp = { Y.col_ptr };
	// the keys that are read: x entries [a0 - 1, a0 + na), y entries [b0, b0 + nb] (those that exist)
	if (tid == 0 && X.nnz > 0) sh.rng[0] = ari_last_le(xcp, 0, ncol, a0 > 0 ? a0 - 1 : 0);
	if (tid == SVT_WAVE && X.nnz > 0) sh.rng[1] = ari_last_le(xcp, 0, ncol, a0 + na > 0 ? a0 + na - 1 : 0);
	if (tid == 2 * SVT_WAVE && Y.nnz > 0) sh.rng[2] = ari_last_le(ycp, 0, ncol, b0 < Y.nnz ? b0 : Y.nnz - 1);
	if (tid == 3 * SVT_WAVE && Y.nnz > 0) sh.rng[3] = ari_last_le(ycp, 0, ncol, b0 + nb < Y.nnz ? b0 + nb : Y.nnz - 1);
	__syncthreads();
	int64_t *ka = sh.keys, *kb = sh.keys + na + 1;      // ka[1 + i]: x entry a0 + i; kb[j]: y entry b0 + j
	for (int s = tid; s < na + 1; s += ARI_NT) {
		const int64_t g = a0 - 1 + s;
		ka[s] = g < 0 ? (int64_t) -1 : ari_key(X, sh.rng[0], sh.rng[1], nrow, g);
	}
	for (int s = tid; s < nb + 1; s += ARI_NT) {
		const int64_t g = b0 + s;
		kb[s] = g >= Y.nnz ? (int64_t) 0x7FFFFFFFFFFFFFFFLL : ari_key(Y, sh.rng[2], sh.rng[3], nrow, g);
	}
	__syncthreads();
	// this thread's ARI_ITEMS consecutive merged places: its start by a merge-path search in LDS, then a walk
	{
		const int d = tid * ARI_ITEMS < n ? tid * ARI_ITEMS : n;
		int lo = d - nb > 0 ? d - nb : 0, hi = d < na ? d : na;
		while (lo < hi) {
			const int mid = (lo + hi) >> 1;
			if (ka[1 + mid] <= kb[d - 1 - mid]) lo = mid + 1; else hi = mid;
		}
		int ia = lo, ib = d - lo;
		for (int k = 0; k < ARI_ITEMS && d + k < n; k++) {
			if (ia < na && (ib >= nb || ka[1 + ia] <= kb[ib])) {
				sh.src[d + k] = (uint32_t) ia | (kb[ib] == ka[1 + ia] ? ARI_PAIRED : 0u);    // kb[nb]: the key after the part
				ia++;
			} else {
				sh.src[d + k] = ARI_FROM_Y | (uint32_t) ib | (ka[ia] == kb[ib] ? ARI_PAIRED : 0u);  // ka[0]: the key before
				ib++;
			}
		}
	}
	__syncthreads();
#pragma unroll
	for (int it = 0; it < ARI_ITEMS; it++) {
		const int p = it * ARI_NT + tid;
		keep[it] = false;
		if (p >= n) continue;
		const uint32_t s = sh.src[p];
		const int idx = (int) (s & ARI_INDEX);
		TX xv = (TX) 0;
		TY yv = (TY) 0;
		if (s & ARI_FROM_Y) {
			if (s & ARI_PAIRED) continue;                // the x entry before it owns the pair
			yv = yval[b0 + idx];
			row[it] = Y.row_idx[b0 + idx];
		} else {
			xv = xval[a0 + idx];
			row[it] = X.row_idx[a0 + idx];
			if (s & ARI_PAIRED) yv = yval[b0 + (p - idx)];  // idx of x's and p - idx of y's come before place p
		}
		if constexpr (RULE == ARI_RULE_ASSIGN) {
			// the tables are read where the rule reads them: an entry of Y lies in a covered leaf; an x entry alone
			// needs its row's byte, and its leaf's -- the column by a search inside the x part's column range, as the
			// keys found it -- only when the row is covered or the value is a zero (else it is kept either way)
			const bool in_y = (s & (ARI_FROM_Y | ARI_PAIRED)) != 0u;
			bool rc = false, lc = true;
			if (!in_y) {
				rc = op.row == NULL || op.row[row[it]] != 0;
				lc = (rc || ari_is_zero(xv)) &&
				     (op.leaf == NULL || op.leaf[ari_last_le(xcp, sh.rng[0], sh.rng[1], a0 + idx)] != 0);
			}
			keep[it] = svt_rule_assign(in_y, xv, yv, rc, lc, &r[it]);
			continue;
		} else if constexpr (RULE == ARI_RULE_ASSIGN_CELLS) {
			keep[it] = svt_rule_assign_cells((s & (ARI_FROM_Y | ARI_PAIRED)) != 0u, xv, yv, &r[it]);
			continue;
		} else if constexpr (RULE == ARI_RULE_COMPARE)
			r[it] = svt_rule_compare(op, svt_rule_as_double(xv), svt_rule_as_double(yv));
		else if constexpr (RULE == ARI_RULE_LOGIC)
			r[it] = svt_rule_logic(op, xv, yv);
		else if constexpr (RULE == ARI_RULE_PMINMAX) {
			TO xw, yw;
			svt_rule_widen(xv, &xw);
			svt_rule_widen(yv, &yw);
			r[it] = svt_rule_pminmax(op & ~SVT_PMINMAX_NA_RM, op & SVT_PMINMAX_NA_RM, xw, yw);
		} else if constexpr (std::is_same<TO, int32_t>::value)
			r[it] = svt_rule_arith_int(op, xv, yv, ovf);
		else
			r[it] = svt_rule_arith_double(op, svt_rule_as_double(xv), svt_rule_as_double(yv));
		keep[it] = !ari_is_zero(r[it]);
	}
}

template <typename TX, typename TY, int RULE>
__global__ __launch_bounds__(ARI_NT) void arith_merge_count_kernel(AriSide X, const TX *xval, AriSide Y, const TY *yval, int64_t ncol,
								   int64_t nrow, typename AriOp<RULE>::type op, const int64_t *cut,
								   int64_t *tile_cnt, int32_t *local)
{
	typedef typename AriMergeOut<TX, TY, RULE>::type TO;
	__shared__ AriMergeShared sh;
	const int64_t ts = (int64_t) blockIdx.x << ARI_SHIFT, total = X.nnz + Y.nnz;
	const int n = (int) (total - ts < ARI_TILE ? total - ts : ARI_TILE);
	const int64_t a0 = cut[blockIdx.x], a1 = cut[blockIdx.x + 1];
	const AriPtr P = { X.col_ptr, Y.col_ptr };
	ari_tile_columns(P, ncol, ts, n, sh.r);
	TO r[ARI_ITEMS];
	int32_t row[ARI_ITEMS];
	bool keep[ARI_ITEMS];
	int ovf = 0;
	ari_merge_tile<TX, TY, RULE>(X, xval, Y, yval, ncol, nrow, op, a0, (int) (a1 - a0), ts - a0, n - (int) (a1 - a0), sh, r, row, keep,
			       &ovf);
	ari_rank(keep, sh.r);
	ari_count_tail(P, ts, sh.r, tile_cnt, local);
}

template <typename TX, typename TY, int RULE>
__global__ __launch_bounds__(ARI_NT) void arith_merge_fill_kernel(AriSide X, const TX *xval, AriSide Y, const TY *yval, int64_t ncol,
								  int64_t nrow, typename AriOp<RULE>::type op, const int64_t *cut,
								  const int64_t *tile_pre, int32_t *out_row_idx,
								  typename AriMergeOut<TX, TY, RULE>::type *out_val, int *ovflow)
{
	typedef typename AriMergeOut<TX, TY, RULE>::type TO;
	__shared__ AriMergeShared sh;
	const int64_t ts = (int64_t) blockIdx.x << ARI_SHIFT, total = X.nnz + Y.nnz;
	const int n = (int) (total - ts < ARI_TILE ? total - ts : ARI_TILE);
	const int64_t a0 = cut[blockIdx.x], a1 = cut[blockIdx.x + 1];
	TO r[ARI_ITEMS];
	int32_t row[ARI_ITEMS];
	bool keep[ARI_ITEMS];
	int ovf = 0;
	ari_merge_tile<TX, TY, RULE>(X, xval, Y, yval, ncol, nrow, op, a0, (int) (a1 - a0), ts - a0, n - (int) (a1 - a0), sh, r, row, keep,
			       &ovf);
	ari_rank(keep, sh.r);
	const int64_t base = tile_pre[blockIdx.x];
#pragma unroll
	for (int it = 0; it < ARI_ITEMS; it++) {
		if (!keep[it]) continue;
		const int64_t pos = ari_position(base, it, sh.r);
		out_row_idx[pos] = row[it];
		out_val[pos] = r[it];
	}
	if (ovf && ovflow != NULL) atomicOr(ovflow, 1);
}

// ---------------------------------------------------------------------------
// sweep: f(v, stats[k]) on the stored values of one operand, k = (with_rows ? row : 0) + mult * ((leaf / stride) % len)
// ---------------------------------------------------------------------------
// The map's tile with two additions: the entry's row (the count pass reads row_idx only when stats has a row part) and
// its leaf, found inside the tile's own column range [the leaf that holds entry ts, sh.qq[1]] as the merge finds the
// column of a key.  A tile that lies inside one leaf (the common case of the leaf forms: q0 == q1) does no search and
// one division per thread, and its gather is one address per wavefront; a tile that spans many leaves does one search of
// log2(leaves in the tile) steps per entry, whatever the leaves' lengths.  The row form's gather is a plain global load
// per entry: rows ascend inside a leaf, so a wavefront's 64 entries of one trip read ascending, often neighbouring,
// elements.
struct AriSweepOp {
	int op, with_rows, narrow;      // narrow: ncol < 2^32, so a leaf number, stride and len fit 32 bits
	int64_t mult;                   // with_rows ? nrow : 1
	int64_t stride, len;
};
__device__ inline int64_t ari_sweep_leaf(const AriSweepOp &w, int64_t q)
{
	if (w.narrow)
		return w.mult * (int64_t) ((uint32_t) q / (uint32_t) w.stride % (uint32_t) w.len);
	return w.mult * (q / w.stride % w.len);
}

template <typename TX, typename TS, typename TO, int RULE>
__device__ inline TO ari_sweep_eval(int op, TX v, TS s, int *ovf)
{
	if constexpr (RULE == ARI_RULE_COMPARE)
		return svt_rule_compare(op, svt_rule_as_double(v), svt_rule_as_double(s));
	else if constexpr (RULE == ARI_RULE_PMINMAX) {
		TO x, y;
		svt_rule_widen(v, &x);
		svt_rule_widen(s, &y);
		return svt_rule_pminmax(op & ~SVT_PMINMAX_NA_RM, op & SVT_PMINMAX_NA_RM, x, y);
	} else if constexpr (std::is_same<TO, int32_t>::value)
		return svt_rule_arith_int(op, v, s, ovf);
	else
		return svt_rule_arith_double(op, svt_rule_as_double(v), svt_rule_as_double(s));
}

// the results of this thread's entries of the tile (striped), their rows (`rows`: read them even without a row part)
// and whether they are kept; sh.qq as ari_tile_columns leaves it
template <typename TX, typename TS, typename TO, int RULE>
__device__ inline void ari_sweep_tile(const int64_t *col_ptr, const int32_t *row_idx, const TX *val, const TS *stats,
				      const AriSweepOp &w, int64_t ts, int n, bool rows, AriShared &sh, int32_t (&row)[ARI_ITEMS],
				      TO (&r)[ARI_ITEMS], bool (&keep)[ARI_ITEMS], int *ovf)
{
	TX v[ARI_ITEMS];
#pragma unroll
	for (int it = 0; it < ARI_ITEMS; it++) {
		const int i = it * ARI_NT + threadIdx.x;
		row[it] = 0;
		if (i < n) {
			v[it] = val[ts + i];
			if (rows) row[it] = row_idx[ts + i];
		}
	}
	__syncthreads();                                    // sh.qq
	const AriColPtr cp = { col_ptr };
	const int64_t q0 = sh.qq[0] > 0 ? sh.qq[0] - 1 : 0, q1 = sh.qq[1];        // col_ptr[q0] <= ts, the last entry is in leaf q1
	const int64_t k0 = ari_sweep_leaf(w, q0);
#pragma unroll
	for (int it = 0; it < ARI_ITEMS; it++) {
		const int i = it * ARI_NT + threadIdx.x;
		keep[it] = false;
		if (i < n) {
			const int64_t kl = q0 >= q1 ? k0 : ari_sweep_leaf(w, ari_last_le(cp, q0, q1, ts + i));
			r[it] = ari_sweep_eval<TX, TS, TO, RULE>(w.op, v[it], stats[(w.with_rows ? (int64_t) row[it] : 0) + kl], ovf);
			keep[it] = !ari_is_zero(r[it]);
		}
	}
}

template <typename TX, typename TS, typename TO, int RULE>
__global__ __launch_bounds__(ARI_NT) void arith_sweep_count_kernel(const int64_t *col_ptr, const int32_t *row_idx, const TX *val,
								   const TS *stats, int64_t ncol, int64_t nnz, AriSweepOp w,
								   int64_t *tile_cnt, int32_t *local)
{
	__shared__ AriShared sh;
	const int64_t ts = (int64_t) blockIdx.x << ARI_SHIFT;
	const int n = (int) (nnz - ts < ARI_TILE ? nnz - ts : ARI_TILE);
	const AriPtr P = { col_ptr, NULL };
	ari_tile_columns(P, ncol, ts, n, sh);
	TO r[ARI_ITEMS];
	int32_t row[ARI_ITEMS];
	bool keep[ARI_ITEMS];
	int ovf = 0;
	ari_sweep_tile<TX, TS, TO, RULE>(col_ptr, row_idx, val, stats, w, ts, n, w.with_rows != 0, sh, row, r, keep, &ovf);
	ari_rank(keep, sh);
	ari_count_tail(P, ts, sh, tile_cnt, local);
}

// (the second launch bound, for pmin / pmax alone: with no long-latency arithmetic behind the eight gathers of the vector
// the compiler hoists them all and takes 82 VGPRs, 5 waves per SIMD against the Arith instantiations' 6; asked for 6 it
// takes 50 and spills nothing.  The other rules' instantiations compile as before.)
template <typename TX, typename TS, typename TO, int RULE>
__global__ __launch_bounds__(ARI_NT, RULE == ARI_RULE_PMINMAX ? 6 : 1) void arith_sweep_fill_kernel(const int64_t *col_ptr, const int32_t *row_idx, const TX *val,
								  const TS *stats, int64_t ncol, int64_t nnz, AriSweepOp w,
								  const int64_t *tile_pre, int32_t *out_row_idx, TO *out_val, int *ovflow)
{
	__shared__ AriShared sh;
	const int64_t ts = (int64_t) blockIdx.x << ARI_SHIFT;
	const int n = (int) (nnz - ts < ARI_TILE ? nnz - ts : ARI_TILE);
	const AriPtr P = { col_ptr, NULL };
	ari_tile_columns(P, ncol, ts, n, sh);
	TO r[ARI_ITEMS];
	int32_t row[ARI_ITEMS];
	bool keep[ARI_ITEMS];
	int ovf = 0;
	ari_sweep_tile<TX, TS, TO, RULE>(col_ptr, row_idx, val, stats, w, ts, n, true, sh, row, r, keep, &ovf);
	ari_rank(keep, sh);
	const int64_t base = tile_pre[blockIdx.x];
#pragma unroll
	for (int it = 0; it < ARI_ITEMS; it++) {
		if (!keep[it]) continue;
		const int64_t pos = ari_position(base, it, sh);
		out_row_idx[pos] = row[it];
		out_val[pos] = r[it];
	}
	if (ovf && ovflow != NULL) atomicOr(ovflow, 1);
}

// *bad <- the smallest index of an element of stats[0, n) that does not keep the result sparse (the word starts as all
// ones).  The word is an error flag, not a position: the atomic decides no placement.
template <typename TS, int RULE>
__global__ __launch_bounds__(ARI_NT) void arith_sweep_valid_kernel(const TS *stats, int64_t n, int op, int s_Rtype,
								   unsigned long long *bad)
{
	const int64_t step = (int64_t) gridDim.x * ARI_NT;
	for (int64_t i = (int64_t) blockIdx.x * ARI_NT + threadIdx.x; i < n; i += step) {
		const double s = (double) stats[i];
		const bool ok = RULE == ARI_RULE_COMPARE ? svt_rule_compare_keeps_sparse(op, s, s_Rtype)
				: RULE == ARI_RULE_PMINMAX ? svt_rule_pminmax_keeps_sparse(op, s, s_Rtype)
							   : svt_rule_arith_keeps_sparse(op, s, s_Rtype);
		if (!ok) {
			atomicMin(bad, (unsigned long long) i);     // (this thread's later indices are larger)
			break;
		}
	}
}

// arith_ptr_kernel for the sweep: nothing outside the workspace is written once an element was refused
__global__ __launch_bounds__(ARI_NT) void arith_sweep_ptr_kernel(AriPtr P, int64_t ncol, int64_t total, const int64_t *tile_pre,
								 int64_t ntiles, const int32_t *local, int64_t *out_col_ptr, int64_t *head)
{
	if ((unsigned long long) head[2] != ~0ULL) return;
	const int64_t j = (int64_t) blockIdx.x * ARI_NT + threadIdx.x;
	if (j == 0) head[1] = tile_pre[ntiles];
	if (j > ncol) return;
	const int64_t p = P(j);
	out_col_ptr[j] = p >= total ? tile_pre[ntiles] : tile_pre[p >> ARI_SHIFT] + local[j];
}

// ---------------------------------------------------------------------------
// launchers.  Workspace: [head 256: int64 total at byte 8][tile counts -> prefixes int64[ntiles + 1]]
// [local int32[ncol + 1]][cut int64[ntiles + 1], the merge only][scratch of the scan]; the parts at multiples of 256
// ---------------------------------------------------------------------------
static inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
static inline unsigned blocks_for(int64_t n) { return (unsigned) ((n + ARI_NT - 1) / ARI_NT); }

int arith_tile(void) { return ARI_TILE; }

struct ArithWs {
	size_t tile, local, cut, scan, total;
	int64_t ntiles;
};
static ArithWs arith_ws(int64_t ncol, int64_t entries, bool merge)
{
	ArithWs L;
	if (ncol < 0) ncol = 0;
	if (entries < 0) entries = 0;
	L.ntiles = (entries + ARI_TILE - 1) >> ARI_SHIFT;
	L.tile = 256;
	L.local = L.tile + up256(((size_t) L.ntiles + 1) * 8);
	L.cut = L.local + up256(((size_t) ncol + 1) * 4);
	L.scan = L.cut + (merge ? up256(((size_t) L.ntiles + 1) * 8) : 0);
	L.total = L.scan + exclusive_scan_ws_bytes(L.ntiles + 1);
	return L;
}

size_t arith_ws_bytes(int64_t ncol, int64_t entries, int merge)
{
	return arith_ws(ncol, entries, merge != 0).total;
}

// what both count launchers do after their tile kernel: the tile prefixes, then out_col_ptr and the total
static int arith_count_finish(const ArithWs &L, AriPtr P, int64_t ncol, int64_t entries, int64_t *out_col_ptr, char *w, hipStream_t s)
{
	int64_t *tile = (int64_t *) (w + L.tile);
	if (launch_exclusive_scan_i64(tile, L.ntiles + 1, w + L.scan, s))
		return -1;
	hipLaunchKernelGGL(arith_ptr_kernel, dim3(blocks_for(ncol + 1)), dim3(ARI_NT), 0, s, P, ncol, entries, tile, L.ntiles,
			   (const int32_t *) (w + L.local), out_col_ptr, (int64_t *) w);
	HIP_TRY(hipGetLastError());
	return 0;
}

template <int RULE> using AriRule = std::integral_constant<int, RULE>;

// f(x values, AriMapOp, result type tag, rule tag) by the rule and the operand's and the result's type; only the
// combinations that are offered are instantiated (Compare: an int32 -- logical or integer -- or a double operand)
template <class F>
static inline int arith_map_by_types(const ArithMapArgs &a, F &&f)
{
	const AriMapOp m = { a.kind, a.op, a.sd, a.si };
	if (a.rule == ARI_RULE_COMPARE) {
		if (a.Rtype == SVT_REALSXP) f((const double *) a.val, m, (int32_t *) NULL, AriRule<ARI_RULE_COMPARE>());
		else if (a.Rtype == SVT_INTSXP || a.Rtype == SVT_LGLSXP)
			f((const int32_t *) a.val, m, (int32_t *) NULL, AriRule<ARI_RULE_COMPARE>());
		else return svt_set_error("compare map: no kernel for this type");
		return 0;
	}
	if (a.rule == ARI_RULE_ISFUN) {
		if (a.Rtype == SVT_REALSXP) f((const double *) a.val, m, (int32_t *) NULL, AriRule<ARI_RULE_ISFUN>());
		else if (a.Rtype == SVT_INTSXP || a.Rtype == SVT_LGLSXP)
			f((const int32_t *) a.val, m, (int32_t *) NULL, AriRule<ARI_RULE_ISFUN>());
		else return svt_set_error("isfun map: no kernel for this type");
		return 0;
	}
	if (a.rule == ARI_RULE_PMINMAX) {                   // (a logical operand or result is an int32 one)
		const bool xi = a.Rtype == SVT_INTSXP || a.Rtype == SVT_LGLSXP, oi = a.out_Rtype == SVT_INTSXP || a.out_Rtype == SVT_LGLSXP;
		if (a.Rtype == SVT_REALSXP && a.out_Rtype == SVT_REALSXP) f((const double *) a.val, m, (double *) NULL, AriRule<ARI_RULE_PMINMAX>());
		else if (xi && a.out_Rtype == SVT_REALSXP) f((const int32_t *) a.val, m, (double *) NULL, AriRule<ARI_RULE_PMINMAX>());
		else if (xi && oi) f((const int32_t *) a.val, m, (int32_t *) NULL, AriRule<ARI_RULE_PMINMAX>());
		else return svt_set_error("pminmax map: no kernel for these types");
		return 0;
	}
	if (a.rule != ARI_RULE_ARITH) return svt_set_error("arith map: no kernel for this rule");
	if (a.Rtype == SVT_REALSXP && a.out_Rtype == SVT_REALSXP) f((const double *) a.val, m, (double *) NULL, AriRule<ARI_RULE_ARITH>());
	else if (a.Rtype == SVT_INTSXP && a.out_Rtype == SVT_REALSXP) f((const int32_t *) a.val, m, (double *) NULL, AriRule<ARI_RULE_ARITH>());
	else if (a.Rtype == SVT_INTSXP && a.out_Rtype == SVT_INTSXP) f((const int32_t *) a.val, m, (int32_t *) NULL, AriRule<ARI_RULE_ARITH>());
	else return svt_set_error("arith map: no kernel for these types");
	return 0;
}

int launch_arith_map_count(const ArithMapArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s)
{
	const ArithWs L = arith_ws(a.ncol, a.nnz, false);
	if (L.ntiles > 0x7FFFFFFFLL)
		return svt_set_error("svt_dev_arith_map_count: too many nonzeros");
	char *w = (char *) ws;
	int64_t *tile = (int64_t *) (w + L.tile);
	HIP_TRY(hipMemsetAsync(w, 0, 256, s));
	HIP_TRY(hipMemsetAsync(tile + L.ntiles, 0, 8, s));
	if (L.ntiles > 0) {
		const int rc = arith_map_by_types(a, [&](auto *v, const AriMapOp &m, auto *o, auto rule) {
			typedef std::remove_const_t<std::remove_pointer_t<decltype(v)>> TX;
			typedef std::remove_pointer_t<decltype(o)> TO;
			hipLaunchKernelGGL((arith_map_count_kernel<TX, TO, decltype(rule)::value>), dim3((unsigned) L.ntiles), dim3(ARI_NT), 0, s, a.col_ptr, v,
					   a.ncol, a.nnz, m, tile, (int32_t *) (w + L.local));
		});
		if (rc) return rc;
	}
	const AriPtr P = { a.col_ptr, NULL };
	return arith_count_finish(L, P, a.ncol, a.nnz, out_col_ptr, w, s);
}

int launch_arith_map_fill(const ArithMapArgs &a, int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, hipStream_t s)
{
	const ArithWs L = arith_ws(a.ncol, a.nnz, false);
	if (L.ntiles == 0)
		return 0;
	const int64_t *tile = (const int64_t *) ((const char *) ws + L.tile);
	const int rc = arith_map_by_types(a, [&](auto *v, const AriMapOp &m, auto *o, auto rule) {
		typedef std::remove_const_t<std::remove_pointer_t<decltype(v)>> TX;
		typedef std::remove_pointer_t<decltype(o)> TO;
		hipLaunchKernelGGL((arith_map_fill_kernel<TX, TO, decltype(rule)::value>), dim3((unsigned) L.ntiles), dim3(ARI_NT), 0, s, a.row_idx, v, a.nnz, m,
				   tile, out_row_idx, (TO *) out_val, ovflow);
	});
	if (rc) return rc;
	HIP_TRY(hipGetLastError());
	return 0;
}

// f(x values, y values, rule tag) by the two operands' types (a logical operand is an int32 operand)
template <class F, class R>
static inline void arith_merge_by_operands(const ArithMergeArgs &a, F &&f, R rule)
{
	if (a.x_Rtype == SVT_REALSXP && a.y_Rtype == SVT_REALSXP) f((const double *) a.x_val, (const double *) a.y_val, rule);
	else if (a.x_Rtype == SVT_REALSXP) f((const double *) a.x_val, (const int32_t *) a.y_val, rule);
	else if (a.y_Rtype == SVT_REALSXP) f((const int32_t *) a.x_val, (const double *) a.y_val, rule);
	else f((const int32_t *) a.x_val, (const int32_t *) a.y_val, rule);
}
// and by the rule: Arith, Compare, the two subassignment rules and pmin / pmax for the four type pairs, Logic for
// int32 x int32 alone
template <class F>
static inline int arith_merge_by_types(const ArithMergeArgs &a, F &&f)
{
	if (a.rule == ARI_RULE_ARITH) arith_merge_by_operands(a, f, AriRule<ARI_RULE_ARITH>());
	else if (a.rule == ARI_RULE_COMPARE) arith_merge_by_operands(a, f, AriRule<ARI_RULE_COMPARE>());
	else if (a.rule == ARI_RULE_ASSIGN) arith_merge_by_operands(a, f, AriRule<ARI_RULE_ASSIGN>());
	else if (a.rule == ARI_RULE_ASSIGN_CELLS) arith_merge_by_operands(a, f, AriRule<ARI_RULE_ASSIGN_CELLS>());
	else if (a.rule == ARI_RULE_PMINMAX) arith_merge_by_operands(a, f, AriRule<ARI_RULE_PMINMAX>());
	else if (a.rule == ARI_RULE_LOGIC && a.x_Rtype != SVT_REALSXP && a.y_Rtype != SVT_REALSXP)
		f((const int32_t *) a.x_val, (const int32_t *) a.y_val, AriRule<ARI_RULE_LOGIC>());
	else return svt_set_error("arith merge: no kernel for this rule and these types");
	return 0;
}

int launch_arith_merge_count(const ArithMergeArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s)
{
	const int64_t entries = a.x_nnz + a.y_nnz;
	const ArithWs L = arith_ws(a.ncol, entries, true);
	if (L.ntiles > 0x7FFFFFFFLL)
		return svt_set_error("svt_dev_arith_merge_count: too many nonzeros");
	char *w = (char *) ws;
	int64_t *tile = (int64_t *) (w + L.tile), *cut = (int64_t *) (w + L.cut);
	const AriSide X = { a.x_col_ptr, a.x_row_idx, a.x_nnz }, Y = { a.y_col_ptr, a.y_row_idx, a.y_nnz };
	HIP_TRY(hipMemsetAsync(w, 0, 256, s));
	HIP_TRY(hipMemsetAsync(tile + L.ntiles, 0, 8, s));
	if (L.ntiles > 0) {
		hipLaunchKernelGGL(arith_merge_cut_kernel, dim3(blocks_for(L.ntiles + 1)), dim3(ARI_NT), 0, s, X, Y, a.ncol, a.nrow,
				   L.ntiles, cut);
		const int rc = arith_merge_by_types(a, [&](auto *xv, auto *yv, auto rule) {
			typedef std::remove_const_t<std::remove_pointer_t<decltype(xv)>> TX;
			typedef std::remove_const_t<std::remove_pointer_t<decltype(yv)>> TY;
			hipLaunchKernelGGL((arith_merge_count_kernel<TX, TY, decltype(rule)::value>), dim3((unsigned) L.ntiles), dim3(ARI_NT), 0,
					   s, X, xv, Y, yv, a.ncol, a.nrow, ari_op<decltype(rule)::value>(a), (const int64_t *) cut, tile,
					   (int32_t *) (w + L.local));
		});
		if (rc) return rc;
	}
	const AriPtr P = { a.x_col_ptr, a.y_col_ptr };
	return arith_count_finish(L, P, a.ncol, entries, out_col_ptr, w, s);
}

int launch_arith_merge_fill(const ArithMergeArgs &a, int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, hipStream_t s)
{
	const ArithWs L = arith_ws(a.ncol, a.x_nnz + a.y_nnz, true);
	if (L.ntiles == 0)
		return 0;
	const char *w = (const char *) ws;
	const AriSide X = { a.x_col_ptr, a.x_row_idx, a.x_nnz }, Y = { a.y_col_ptr, a.y_row_idx, a.y_nnz };
	const int rc = arith_merge_by_types(a, [&](auto *xv, auto *yv, auto rule) {
		typedef std::remove_const_t<std::remove_pointer_t<decltype(xv)>> TX;
		typedef std::remove_const_t<std::remove_pointer_t<decltype(yv)>> TY;
		typedef typename AriMergeOut<TX, TY, decltype(rule)::value>::type TO;
		hipLaunchKernelGGL((arith_merge_fill_kernel<TX, TY, decltype(rule)::value>), dim3((unsigned) L.ntiles), dim3(ARI_NT), 0, s, X,
				   xv, Y, yv, a.ncol, a.nrow, ari_op<decltype(rule)::value>(a), (const int64_t *) (w + L.cut),
				   (const int64_t *) (w + L.tile), out_row_idx, (TO *) out_val, ovflow);
	});
	if (rc) return rc;
	HIP_TRY(hipGetLastError());
	return 0;
}

// f(x values, stats values, result type tag, rule tag) by the rule and the three types: Compare for an int32 (logical or
// integer) or double operand and vector; Arith with an int32 result for int32 x int32 alone
template <class F>
static inline int arith_sweep_by_types(const ArithSweepArgs &a, F &&f)
{
	const bool xd = a.Rtype == SVT_REALSXP, sd = a.stats_Rtype == SVT_REALSXP;
	if (a.rule == ARI_RULE_COMPARE) {
		if (xd && sd) f((const double *) a.val, (const double *) a.stats, (int32_t *) NULL, AriRule<ARI_RULE_COMPARE>());
		else if (xd) f((const double *) a.val, (const int32_t *) a.stats, (int32_t *) NULL, AriRule<ARI_RULE_COMPARE>());
		else if (sd) f((const int32_t *) a.val, (const double *) a.stats, (int32_t *) NULL, AriRule<ARI_RULE_COMPARE>());
		else f((const int32_t *) a.val, (const int32_t *) a.stats, (int32_t *) NULL, AriRule<ARI_RULE_COMPARE>());
		return 0;
	}
	if (a.rule == ARI_RULE_PMINMAX) {                   // int32 for two int32 sides, double with a double side
		if (xd && sd) f((const double *) a.val, (const double *) a.stats, (double *) NULL, AriRule<ARI_RULE_PMINMAX>());
		else if (xd) f((const double *) a.val, (const int32_t *) a.stats, (double *) NULL, AriRule<ARI_RULE_PMINMAX>());
		else if (sd) f((const int32_t *) a.val, (const double *) a.stats, (double *) NULL, AriRule<ARI_RULE_PMINMAX>());
		else f((const int32_t *) a.val, (const int32_t *) a.stats, (int32_t *) NULL, AriRule<ARI_RULE_PMINMAX>());
		return 0;
	}
	if (a.rule != ARI_RULE_ARITH) return svt_set_error("arith sweep: no kernel for this rule");
	if (a.out_Rtype == SVT_INTSXP) {
		if (xd || sd) return svt_set_error("arith sweep: no kernel for these types");
		f((const int32_t *) a.val, (const int32_t *) a.stats, (int32_t *) NULL, AriRule<ARI_RULE_ARITH>());
	} else if (xd && sd) f((const double *) a.val, (const double *) a.stats, (double *) NULL, AriRule<ARI_RULE_ARITH>());
	else if (xd) f((const double *) a.val, (const int32_t *) a.stats, (double *) NULL, AriRule<ARI_RULE_ARITH>());
	else if (sd) f((const int32_t *) a.val, (const double *) a.stats, (double *) NULL, AriRule<ARI_RULE_ARITH>());
	else f((const int32_t *) a.val, (const int32_t *) a.stats, (double *) NULL, AriRule<ARI_RULE_ARITH>());
	return 0;
}
static inline AriSweepOp arith_sweep_op(const ArithSweepArgs &a)
{
	return AriSweepOp{ a.op, a.with_rows, a.ncol <= 0xFFFFFFFFLL, a.with_rows ? a.nrow : 1, a.stride, a.len };
}

int launch_arith_sweep_count(const ArithSweepArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s)
{
	const ArithWs L = arith_ws(a.ncol, a.nnz, false);
	if (L.ntiles > 0x7FFFFFFFLL)
		return svt_set_error("svt_dev_arith_sweep_count: too many nonzeros");
	char *w = (char *) ws;
	int64_t *tile = (int64_t *) (w + L.tile);
	unsigned long long *bad = (unsigned long long *) (w + 16);
	HIP_TRY(hipMemsetAsync(w, 0, 256, s));
	HIP_TRY(hipMemsetAsync(bad, 0xFF, 8, s));
	HIP_TRY(hipMemsetAsync(tile + L.ntiles, 0, 8, s));
	const int64_t nstats = (a.with_rows ? a.nrow : 1) * a.len;
	if (nstats > 0) {
		const unsigned nb = blocks_for(nstats < 1024 * ARI_NT ? nstats : 1024 * ARI_NT);
		const bool cmp = a.rule == ARI_RULE_COMPARE, pmm = a.rule == ARI_RULE_PMINMAX;
		if (a.stats_Rtype == SVT_REALSXP) {
			if (cmp) hipLaunchKernelGGL((arith_sweep_valid_kernel<double, ARI_RULE_COMPARE>), dim3(nb), dim3(ARI_NT), 0, s,
						    (const double *) a.stats, nstats, a.op, a.stats_Rtype, bad);
			else if (pmm) hipLaunchKernelGGL((arith_sweep_valid_kernel<double, ARI_RULE_PMINMAX>), dim3(nb), dim3(ARI_NT), 0, s,
							 (const double *) a.stats, nstats, a.op, a.stats_Rtype, bad);
			else hipLaunchKernelGGL((arith_sweep_valid_kernel<double, ARI_RULE_ARITH>), dim3(nb), dim3(ARI_NT), 0, s,
						(const double *) a.stats, nstats, a.op, a.stats_Rtype, bad);
		} else {
			if (cmp) hipLaunchKernelGGL((arith_sweep_valid_kernel<int32_t, ARI_RULE_COMPARE>), dim3(nb), dim3(ARI_NT), 0, s,
						    (const int32_t *) a.stats, nstats, a.op, a.stats_Rtype, bad);
			else if (pmm) hipLaunchKernelGGL((arith_sweep_valid_kernel<int32_t, ARI_RULE_PMINMAX>), dim3(nb), dim3(ARI_NT), 0, s,
							 (const int32_t *) a.stats, nstats, a.op, a.stats_Rtype, bad);
			else hipLaunchKernelGGL((arith_sweep_valid_kernel<int32_t, ARI_RULE_ARITH>), dim3(nb), dim3(ARI_NT), 0, s,
						(const int32_t *) a.stats, nstats, a.op, a.stats_Rtype, bad);
		}
		HIP_TRY(hipGetLastError());
	}
	if (L.ntiles > 0) {
		const AriSweepOp op = arith_sweep_op(a);
		const int rc = arith_sweep_by_types(a, [&](auto *v, auto *st, auto *o, auto rule) {
			typedef std::remove_const_t<std::remove_pointer_t<decltype(v)>> TX;
			typedef std::remove_const_t<std::remove_pointer_t<decltype(st)>> TS;
			typedef std::remove_pointer_t<decltype(o)> TO;
			hipLaunchKernelGGL((arith_sweep_count_kernel<TX, TS, TO, decltype(rule)::value>), dim3((unsigned) L.ntiles), dim3(ARI_NT),
					   0, s, a.col_ptr, a.row_idx, v, st, a.ncol, a.nnz, op, tile, (int32_t *) (w + L.local));
		});
		if (rc) return rc;
	}
	if (launch_exclusive_scan_i64(tile, L.ntiles + 1, w + L.scan, s))
		return -1;
	const AriPtr P = { a.col_ptr, NULL };
	hipLaunchKernelGGL(arith_sweep_ptr_kernel, dim3(blocks_for(a.ncol + 1)), dim3(ARI_NT), 0, s, P, a.ncol, a.nnz, tile, L.ntiles,
			   (const int32_t *) (w + L.local), out_col_ptr, (int64_t *) w);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_arith_sweep_fill(const ArithSweepArgs &a, int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, hipStream_t s)
{
	const ArithWs L = arith_ws(a.ncol, a.nnz, false);
	if (L.ntiles == 0)
		return 0;
	const int64_t *tile = (const int64_t *) ((const char *) ws + L.tile);
	const AriSweepOp op = arith_sweep_op(a);
	const int rc = arith_sweep_by_types(a, [&](auto *v, auto *st, auto *o, auto rule) {
		typedef std::remove_const_t<std::remove_pointer_t<decltype(v)>> TX;
		typedef std::remove_const_t<std::remove_pointer_t<decltype(st)>> TS;
		typedef std::remove_pointer_t<decltype(o)> TO;
		hipLaunchKernelGGL((arith_sweep_fill_kernel<TX, TS, TO, decltype(rule)::value>), dim3((unsigned) L.ntiles), dim3(ARI_NT), 0,
				   s, a.col_ptr, a.row_idx, v, st, a.ncol, a.nnz, op, tile, out_row_idx, (TO *) out_val, ovflow);
	});
	if (rc) return rc;
	HIP_TRY(hipGetLastError());
	return 0;
}
