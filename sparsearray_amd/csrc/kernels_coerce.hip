// The coercions dense array <-> resident sparse operand and nzwhich() (C_build_SVT_from_Rarray,
// C_from_SVT_SparseArray_to_Rarray and C_nzwhich_SVT, src/SVT_SparseArray_class.c of the reference, on the device layout
// col_ptr / row_idx / val; the rules are stated once in include/svt_hip.h and svt_coerce_rules.h).  The dense array is in
// R's layout, column-major with the rows fastest, so CSC order IS flat cell order: the three passes are streams over the
// flat cell index (dense -> sparse, sparse -> dense) or over the entries (nzwhich), cut into tiles of SVT_TILE, and what
// a workgroup does for a tile does not depend on how the cells are cut into leaves.
//
// Dense -> sparse is a stream compaction.  Count pass: a tile's 256 threads test 16 cells each, cell it * 256 + tid in
// trip `it`, so that a wavefront's ballot is the keep mask of 64 consecutive cells -- one bit per cell, 64 words per
// tile, left in the workspace next to the tile's count; one 64-bit exclusive scan (svt_scan.h) turns the counts into the
// tile bases; a second pass over the MASKS (1/64 of the array) writes col_ptr: the rank of cell q * nrow, for the leaf
// boundaries a tile holds, from the base, the prefix of the words before it and the bits below it.  Fill pass: the rank
// of a kept cell the same way, its row from the tile's first row (one 64-bit division per tile), its value loaded only
// where the bit is set -- the array is not tested again and, at low densities, mostly not read again.  No atomic decides
// a position; every position is 64-bit.
//
// Sparse -> dense: a workgroup owns a run of consecutive tiles of OUTPUT cells.  It builds a tile in LDS, the background
// first, then the entries that fall into it, and writes it out in 16-byte pieces: every cell is written once.  The
// entries of a tile are consecutive (they are sorted by flat cell), so the workgroup walks them in batches of 256 from
// where the tile before stopped; only the first tile of a run finds its first entry by a binary search over the rows of
// its first leaf.  The leaf of an entry: sub_last_le over the col_ptr of the leaves the tile touches, which are checked
// first (ascending, inside [0, nnz]); a row outside [0, nrow) or a cell outside the tile is never used as an address.
//
// The compaction takes its cells from a SOURCE: value(c), the cell c of the call, and keep(v), whether it is stored.
// DenseSource loads the cell from the array.  PoissonSource generates it (poissonSparseArray(), svt_random_rules.h): the
// value of cell `first + c` of the whole array under the seed, so the count pass marks what the generator makes and the
// fill pass makes the value again only where the bit is set -- no array of the cells ever exists.  A Philox block serves
// the two cells 2b and 2b + 1.  poisson_mark_pairs_kernel, taken when `first` is even, computes every block once: a lane
// makes the block of two neighbouring cells and the two ballots (even cells, odd cells) are dealt back into the mask words
// of 64 consecutive cells by two more ballots.  With `first` odd the pairs straddle the tiles and the mark kernel of the
// source computes a block per cell (profiles/poisson_timing.txt has both times).
//
// nzwhich: the tiles of svt_tile.h over the entries, like the copy of abind -- the leaves a tile touches by two binary
// searches, one lane per leaf boundary inside the tile, the max-scan.
#include <string.h>

#include "svt_common.h"
#include "svt_coerce_rules.h"
#include "svt_random_rules.h"
#include "svt_scan.h"
#include "svt_tile.h"

#define COERCE_GRID 2048                // count / fill / nzwhich: 8 workgroups on each of 256 CUs
#define COERCE_DENSE_GRID 1024          // sparse -> dense: 4 workgroups of 32 KB LDS on each CU

typedef unsigned long long coerce_word;

static_assert(SVT_TILE_CHUNKS == 64, "a tile's keep mask is 64 words, scanned by one wavefront");

// The 64 mask words of tile t into LDS with the exclusive prefix of their bit counts (the first wavefront); ends with a
// barrier, the caller puts one before wb and cpre are written again
__device__ inline void coerce_stage_mask(const coerce_word *bits, int64_t t, coerce_word *wb, int *cpre)
{
	const int tid = threadIdx.x;
	if (tid < SVT_WAVE) {
		const coerce_word m = bits[(t << 6) + tid];
		const int pc = __popcll(m);
		int x = pc;
		for (int o = 1; o < SVT_WAVE; o <<= 1) {
			const int u = __shfl_up(x, o, SVT_WAVE);
			if (tid >= o) x += u;
		}
		wb[tid] = m;
		cpre[tid] = x - pc;
	}
	__syncthreads();
}
// kept cells of the tile before cell o of it
__device__ inline int coerce_rank(const coerce_word *wb, const int *cpre, int o)
{
	return cpre[o >> 6] + __popcll(wb[o >> 6] & ((1ULL << (o & 63)) - 1ULL));
}

// ---------------------------------------------------------------------------
// dense -> sparse
// ---------------------------------------------------------------------------
template <typename T>
struct DenseSource {
	typedef T value_type;
	const T *__restrict__ x;
	int na_bg;
	__device__ T value(int64_t c) const { return x[c]; }
	__device__ bool keep(T v) const { return svt_rule_keep(v, na_bg != 0); }
};
struct PoissonSource {
	typedef int32_t value_type;
	svt_poisson_table table;
	uint64_t seed, first;                   // cell c of the call is cell first + c of the array
	__device__ int32_t value(int64_t c) const { return svt_rule_poisson_cell(seed, first + (uint64_t) c, table); }
	__device__ bool keep(int32_t v) const { return v != 0; }
};

// a tile's count from those of its four wavefronts; ends with a barrier (wsum is written again by the next tile)
__device__ inline void coerce_tile_count(int mine, int *wsum, int64_t *cnt, int64_t t)
{
	const int tid = threadIdx.x;
	if ((tid & 63) == 0) wsum[tid >> 6] = mine;
	__syncthreads();
	if (tid == 0) cnt[t] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
	__syncthreads();
}

template <typename Source>
__global__ __launch_bounds__(SVT_TILE_NT) void from_dense_mark_kernel(const Source src, int64_t ncells, int64_t ntiles,
									  coerce_word *__restrict__ bits, int64_t *__restrict__ cnt)
{
	typedef typename Source::value_type T;
	__shared__ int wsum[SVT_TILE_NT / SVT_WAVE];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const int64_t ts = t << SVT_TILE_SHIFT;
		T v[SVT_TILE_ITEMS];
#pragma unroll
		for (int it = 0; it < SVT_TILE_ITEMS; it++) {
			const int64_t c = ts + it * SVT_TILE_NT + tid;
			v[it] = c < ncells ? src.value(c) : (T) 0;
		}
		int mine = 0;
#pragma unroll
		for (int it = 0; it < SVT_TILE_ITEMS; it++) {
			const int64_t c = ts + it * SVT_TILE_NT + tid;
			const coerce_word m = __ballot(c < ncells && src.keep(v[it]));
			if (lane == 0) bits[(t << 6) + it * (SVT_TILE_NT / SVT_WAVE) + w] = m;
			mine += __popcll(m);
		}
		coerce_tile_count(mine, wsum, cnt, t);
	}
	if (blockIdx.x == 0 && tid == 0) cnt[ntiles] = 0;       // the scan's total
}

// The mark pass of the Poisson source for an even `first`: trip j of wavefront w takes the 128 cells of the chunks 2k and
// 2k + 1, k = j * 4 + w; lane l makes the block of the cells 128 k + 2 l and + 1.  The count pass asks value != 0 alone.
__global__ __launch_bounds__(SVT_TILE_NT) void poisson_mark_pairs_kernel(const PoissonSource src, int64_t ncells, int64_t ntiles,
									 coerce_word *__restrict__ bits, int64_t *__restrict__ cnt)
{
	__shared__ int wsum[SVT_TILE_NT / SVT_WAVE];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const int half = lane >> 1, odd = lane & 1;
	for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const int64_t ts = t << SVT_TILE_SHIFT;
		int mine = 0;
#pragma unroll 2
		for (int j = 0; j < SVT_TILE_ITEMS / 2; j++) {
			const int k = j * (SVT_TILE_NT / SVT_WAVE) + w;
			const int64_t c = ts + k * (2 * SVT_WAVE) + 2 * lane;           // even, like src.first
			bool k0 = false, k1 = false;
			if (c < ncells) {
				const svt_philox_words b = svt_rule_cell_block(src.seed, (src.first + (uint64_t) c) >> 1);
				k0 = svt_rule_poisson_nonzero(svt_rule_block_uniform(b, 0), src.table);
				k1 = c + 1 < ncells && svt_rule_poisson_nonzero(svt_rule_block_uniform(b, 1), src.table);
			}
			const coerce_word be = __ballot(k0), bo = __ballot(k1);
			const coerce_word mix = odd ? bo : be;                          // cell 2 h + odd of the 128 is bit h of it
			const coerce_word m0 = __ballot((mix >> half) & 1ULL), m1 = __ballot((mix >> (32 + half)) & 1ULL);
			if (lane == 0) {
				bits[(t << 6) + 2 * k] = m0;
				bits[(t << 6) + 2 * k + 1] = m1;
			}
			mine += __popcll(m0) + __popcll(m1);
		}
		coerce_tile_count(mine, wsum, cnt, t);
	}
	if (blockIdx.x == 0 && tid == 0) cnt[ntiles] = 0;       // the scan's total
}

// after the scan: out_col_ptr[q] for the leaves that start inside a tile, out_col_ptr[nleaves] and head[1] <- the total
__global__ __launch_bounds__(SVT_TILE_NT) void from_dense_publish_kernel(int64_t nrow, int64_t nleaves, int64_t ncells,
									 int64_t ntiles, const coerce_word *__restrict__ bits,
									 const int64_t *__restrict__ base,
									 int64_t *__restrict__ out_col_ptr, int64_t *__restrict__ head)
{
	__shared__ coerce_word wb[SVT_TILE_CHUNKS];
	__shared__ int cpre[SVT_TILE_CHUNKS];
	const int tid = threadIdx.x;
	for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const int64_t ts = t << SVT_TILE_SHIFT;
		const int64_t n = ncells - ts < SVT_TILE ? ncells - ts : SVT_TILE;
		const int64_t qa = ts / nrow;
		const int64_t q0 = qa * nrow == ts ? qa : qa + 1;       // the first leaf that starts at or after ts
		const int64_t q1 = (ts + n - 1) / nrow;                 // the leaf of the tile's last cell, < nleaves
		if (q0 > q1) continue;                                  // (uniform: no boundary inside the tile)
		coerce_stage_mask(bits, t, wb, cpre);
		const int64_t b = base[t];
		for (int64_t q = q0 + tid; q <= q1; q += SVT_TILE_NT)
			out_col_ptr[q] = b + coerce_rank(wb, cpre, (int) (q * nrow - ts));
		__syncthreads();
	}
	if (blockIdx.x == 0 && tid == 0) {
		out_col_ptr[nleaves] = base[ntiles];
		head[0] = 0;
		head[1] = base[ntiles];
	}
}

template <typename Source, typename TO>
__global__ __launch_bounds__(SVT_TILE_NT) void from_dense_fill_kernel(const Source src, int64_t nrow, int64_t ntiles,
									  const coerce_word *__restrict__ bits,
									  const int64_t *__restrict__ base,
									  int32_t *__restrict__ out_row_idx, TO *__restrict__ out_val)
{
	__shared__ coerce_word wb[SVT_TILE_CHUNKS];
	__shared__ int cpre[SVT_TILE_CHUNKS];
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const uint32_t nr = (uint32_t) nrow;
	const bool one_wrap = nrow >= SVT_TILE;         // a tile then passes the end of a leaf once at most
	for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
		const int64_t b = base[t];
		if (base[t + 1] == b) continue;                 // (uniform: nothing kept in this tile)
		const int64_t ts = t << SVT_TILE_SHIFT;
		const uint32_t r0 = (uint32_t) (ts - ts / nrow * nrow);    // the row of the tile's first cell
		coerce_stage_mask(bits, t, wb, cpre);
#pragma unroll
		for (int it = 0; it < SVT_TILE_ITEMS; it++) {
			const int c = it * (SVT_TILE_NT / SVT_WAVE) + w;
			const coerce_word m = wb[c];
			if (!((m >> lane) & 1ULL)) continue;
			const int o = c * SVT_WAVE + lane;
			const int64_t rank = b + cpre[c] + __popcll(m & ((1ULL << lane) - 1ULL));
			const uint32_t v = r0 + (uint32_t) o;       // < nrow + SVT_TILE <= 2^31 + 4095
			out_row_idx[rank] = (int32_t) (one_wrap ? (v >= nr ? v - nr : v) : v % nr);
			TO ov;
			svt_rule_coerce(src.value(ts + o), &ov);
			out_val[rank] = ov;
		}
		__syncthreads();
	}
}

// ---------------------------------------------------------------------------
// sparse -> dense
// ---------------------------------------------------------------------------
// the first e in [lo, hi) with row_idx[e] >= r, hi when there is none (rows ascending; on rows out of order some e in
// [lo, hi] all the same)
__device__ inline int64_t coerce_first_row_ge(const int32_t *row_idx, int64_t lo, int64_t hi, int64_t r)
{
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (row_idx[mid] >= r) hi = mid; else lo = mid + 1;
	}
	return lo;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(SVT_TILE_NT) void to_dense_kernel(const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ row_idx,
								 const TI *__restrict__ val, int64_t nrow, int64_t nnz, int64_t ncells,
								 int64_t ntiles, int64_t per, int na_bg, TO *__restrict__ out, int *bad)
{
	constexpr int VEC = 16 / (int) sizeof(TO);
	struct alignas(16) Piece { TO v[VEC]; };
	__shared__ Piece piece[SVT_TILE / VEC];
	__shared__ int64_t first;
	TO *cell = &piece[0].v[0];
	const int tid = threadIdx.x;
	TO bg;
	svt_rule_background(na_bg != 0, &bg);
	int flag = 0;
	int64_t cur = -1;                               // the tile's first entry; < 0: not known, search
	const int64_t t_end = ((int64_t) blockIdx.x + 1) * per < ntiles ? ((int64_t) blockIdx.x + 1) * per : ntiles;
	for (int64_t t = (int64_t) blockIdx.x * per; t < t_end; t++) {
		const int64_t ts = t << SVT_TILE_SHIFT;
		const int n = (int) (ncells - ts < SVT_TILE ? ncells - ts : SVT_TILE);
		const int64_t q0 = ts / nrow, q1 = (ts + n - 1) / nrow;         // the leaves of the first and the last cell
		const int64_t r0 = ts - q0 * nrow;
		int viol = 0;
		for (int64_t q = q0 + tid; q <= q1; q += SVT_TILE_NT) {
			const int64_t s = col_ptr[q], e = col_ptr[q + 1];
			if (s < 0 || e < s || e > nnz) viol = 1;
		}
#pragma unroll
		for (int it = 0; it < SVT_TILE_ITEMS; it++) cell[it * SVT_TILE_NT + tid] = bg;
		viol = __syncthreads_or(viol);
		if (viol) {                                 // (uniform) nothing is read through these pointers: the background alone
			flag = 1;
			cur = -1;
		} else {
			if (cur < 0) {
				if (tid == 0)
					first = r0 == 0 ? col_ptr[q0] : coerce_first_row_ge(row_idx, col_ptr[q0], col_ptr[q0 + 1], r0);
				__syncthreads();
				cur = first;
			}
			const int64_t e_end = col_ptr[q1 + 1];
			for (;;) {                              // batches of 256 entries until one lies past the tile
				const int64_t e = cur + tid;
				// Row and value are loaded together, the value before the row says whether it is wanted: a batch is
				// one round of loads, not two (profiles/coerce_timing.txt, section 3).  Two blocks on purpose: stated
				// as one, the compiler moves the value's load behind the tests of the row.
				int32_t r = 0;
				TI v = (TI) 0;
				int64_t l = 0;
				if (e < e_end) {
					r = row_idx[e];
					v = val[e];
					// the leaf of e among those of the tile, relative to q0: col_ptr[q1 + 1] = e_end > e
					l = sub_last_le(col_ptr + q0, q1 - q0 + 1, e);
				}
				bool used = false;
				if (e < e_end) {
					const int64_t o = l * nrow + r - r0;
					if (r < 0 || r >= nrow || o < 0) {      // (o < 0: rows out of order)
						used = true;
						flag = 1;
					} else if (o < n) {
						used = true;
						TO ov;
						svt_rule_coerce(v, &ov);
						cell[o] = ov;
					}
				}
				const int nb = __syncthreads_count(used);
				cur += nb;
				if (nb < SVT_TILE_NT) break;
			}
		}
		// (the scatter is behind a barrier: __syncthreads_or, or the last __syncthreads_count)
		for (int p = tid; p * VEC < n; p += SVT_TILE_NT) {
			if (p * VEC + VEC <= n) {
				*(Piece *) (out + ts + p * VEC) = piece[p];
			} else {
				for (int k = 0; p * VEC + k < n; k++) out[ts + p * VEC + k] = piece[p].v[k];
			}
		}
		__syncthreads();                            // cell and first are written again by the next tile
	}
	if (flag && bad != NULL) atomicOr(bad, 1);
}

// ---------------------------------------------------------------------------
// nzwhich
// ---------------------------------------------------------------------------
struct NzwhichDims {
	int ndim;
	int64_t d[8];
};

// One tile of SVT_TILE entries per trip; seg[i]: at the first entry of every leaf that starts inside the tile the leaf
// (relative to p0, the leaf of the tile's first entry); svt_tile_max_scan spreads it over the leaf's entries.  The
// relative leaf is a 32-bit int in LDS: ncol <= 2^31 - 1, which the host checks.
template <bool ARR_IND>
__global__ __launch_bounds__(SVT_TILE_NT) void nzwhich_kernel(const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ row_idx,
								int64_t nrow, int64_t ncol, int64_t nnz, NzwhichDims D,
								void *__restrict__ out)
{
	__shared__ int seg[SVT_TILE];
	__shared__ int cmax[SVT_TILE_CHUNKS];
	__shared__ int64_t pp[2];
	const int tid = threadIdx.x, w = tid >> 6;
	for (int64_t ts = (int64_t) blockIdx.x << SVT_TILE_SHIFT; ts < nnz; ts += (int64_t) gridDim.x << SVT_TILE_SHIFT) {
		const int n = (int) (nnz - ts < SVT_TILE ? nnz - ts : SVT_TILE);
		if (tid == 0) pp[0] = sub_last_le(col_ptr, ncol, ts);
		if (tid == SVT_WAVE) pp[1] = sub_last_le(col_ptr, ncol, ts + n - 1);
#pragma unroll
		for (int it = 0; it < SVT_TILE_ITEMS; it++) seg[it * SVT_TILE_NT + tid] = 0;
		__syncthreads();
		const int64_t p0 = pp[0], p1 = pp[1];
		// p0 < p <= p1: ts < col_ptr[p] <= ts + n - 1 (checked: the pointers of the operand are not); one lane per
		// boundary, the non-empty leaf of a position marks it
		for (int64_t p = p0 + 1 + tid; p <= p1 && p < ncol; p += SVT_TILE_NT) {
			const int64_t s = col_ptr[p];
			if (col_ptr[p + 1] > s && s > ts && s < ts + n) seg[s - ts] = (int) (p - p0);
		}
		__syncthreads();
		int v[SVT_TILE_ITEMS];
		svt_tile_max_scan(seg, cmax, v);
#pragma unroll
		for (int it = 0; it < SVT_TILE_ITEMS; it++) {
			const int i = it * SVT_TILE_NT + tid;
			if (i >= n) continue;
			const int before = cmax[it * (SVT_TILE_NT / SVT_WAVE) + w];
			const int64_t leaf = p0 + (v[it] > before ? v[it] : before);
			const int64_t e = ts + i;
			const int32_t r = row_idx[e];
			if constexpr (!ARR_IND) {
				((int64_t *) out)[e] = leaf * nrow + r;
			} else {
				int32_t *o = (int32_t *) out;
				o[e] = r;
				uint32_t rem = (uint32_t) leaf;     // (the host refuses 2^31 leaves or more)
				for (int k = 1; k < D.ndim; k++) {
					const uint32_t dk = (uint32_t) D.d[k];
					const uint32_t c = k == D.ndim - 1 ? rem : rem % dk;
					if (k < D.ndim - 1) rem /= dk;
					o[(int64_t) k * nnz + e] = (int32_t) c;
				}
			}
		}
		__syncthreads();                           // seg, cmax and pp are written again by the next trip
	}
}

// ---------------------------------------------------------------------------
// launchers.  Workspace of dense -> sparse: [head 256: int flag (0), int64 total at byte 8][tile bases int64[ntiles + 1]]
// [keep masks, 64 words per tile][scratch of the scan]; the parts at multiples of 256 bytes
// ---------------------------------------------------------------------------
static inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
static inline int64_t coerce_ntiles(int64_t n) { return n <= 0 ? 0 : ((n - 1) >> SVT_TILE_SHIFT) + 1; }
static inline unsigned coerce_grid(int64_t ntiles, int cap) { return (unsigned) (ntiles < cap ? ntiles : cap); }

struct CoerceWs {
	size_t base, bits, scan, total;
	int64_t ntiles;
};
static CoerceWs coerce_ws(int64_t ncells)
{
	CoerceWs L;
	L.ntiles = coerce_ntiles(ncells);
	L.base = 256;
	L.bits = L.base + up256(((size_t) L.ntiles + 1) * 8);
	L.scan = L.bits + (size_t) L.ntiles * SVT_TILE_CHUNKS * sizeof(coerce_word);
	L.total = L.scan + exclusive_scan_ws_bytes(L.ntiles + 1);
	return L;
}

int coerce_tile(void) { return SVT_TILE; }

size_t from_dense_ws_bytes(int64_t ncells)
{
	return coerce_ws(ncells).total;
}

// The count pass of either source behind `mark(grid, block, bits, cnt)`, which launches the source's mark kernel: the
// masks and the tile counts, the scan of the counts into the tile bases, out_col_ptr and the head from the masks.
template <class Mark>
static int coerce_count(int64_t nrow, int64_t nleaves, int64_t ncells, int64_t *out_col_ptr, void *ws, hipStream_t s, Mark mark)
{
	const CoerceWs L = coerce_ws(ncells);
	char *w = (char *) ws;
	int64_t *base = (int64_t *) (w + L.base);
	coerce_word *bits = (coerce_word *) (w + L.bits);
	const dim3 grid(coerce_grid(L.ntiles, COERCE_GRID)), block(SVT_TILE_NT);
	mark(grid, block, L.ntiles, bits, base);
	if (launch_exclusive_scan_i64(base, L.ntiles + 1, w + L.scan, s))
		return -1;
	hipLaunchKernelGGL(from_dense_publish_kernel, grid, block, 0, s, nrow, nleaves, ncells, L.ntiles,
			   (const coerce_word *) bits, (const int64_t *) base, out_col_ptr, (int64_t *) w);
	HIP_TRY(hipGetLastError());
	return 0;
}
template <typename Source, typename TO>
static int coerce_fill(const Source &src, int64_t nrow, int64_t ncells, int32_t *out_row_idx, TO *out_val, const void *ws,
		       hipStream_t s)
{
	if (ncells <= 0)
		return 0;
	const CoerceWs L = coerce_ws(ncells);
	const char *w = (const char *) ws;
	const dim3 grid(coerce_grid(L.ntiles, COERCE_GRID)), block(SVT_TILE_NT);
	hipLaunchKernelGGL((from_dense_fill_kernel<Source, TO>), grid, block, 0, s, src, nrow, L.ntiles,
			   (const coerce_word *) (w + L.bits), (const int64_t *) (w + L.base), out_row_idx, out_val);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_from_dense_count(const FromDenseArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s)
{
	return coerce_count(a.nrow, a.nleaves, a.ncells, out_col_ptr, ws, s,
		[&](dim3 grid, dim3 block, int64_t ntiles, coerce_word *bits, int64_t *cnt) {
			if (a.x_Rtype == SVT_REALSXP)
				hipLaunchKernelGGL(from_dense_mark_kernel<DenseSource<double>>, grid, block, 0, s,
						   DenseSource<double>{ (const double *) a.x, a.na_background }, a.ncells, ntiles, bits, cnt);
			else
				hipLaunchKernelGGL(from_dense_mark_kernel<DenseSource<int32_t>>, grid, block, 0, s,
						   DenseSource<int32_t>{ (const int32_t *) a.x, a.na_background }, a.ncells, ntiles, bits, cnt);
		});
}

int launch_from_dense_fill(const FromDenseArgs &a, int32_t *out_row_idx, void *out_val, const void *ws, hipStream_t s)
{
	if (a.x_Rtype == SVT_REALSXP)
		return coerce_fill(DenseSource<double>{ (const double *) a.x, a.na_background }, a.nrow, a.ncells, out_row_idx,
				   (double *) out_val, ws, s);
	const DenseSource<int32_t> src = { (const int32_t *) a.x, a.na_background };
	if (a.ans_Rtype == SVT_REALSXP)
		return coerce_fill(src, a.nrow, a.ncells, out_row_idx, (double *) out_val, ws, s);
	return coerce_fill(src, a.nrow, a.ncells, out_row_idx, (int32_t *) out_val, ws, s);
}

// ---------------------------------------------------------------------------
// generated cells: poissonSparseArray() through the same passes, simple_rpois() by a plain kernel
// ---------------------------------------------------------------------------
#define RPOIS_GRID 2048

__global__ __launch_bounds__(SVT_TILE_NT) void rpois_kernel(const PoissonSource src, int64_t n, int32_t *__restrict__ out)
{
	for (int64_t i = (int64_t) blockIdx.x * SVT_TILE_NT + threadIdx.x; i < n; i += (int64_t) gridDim.x * SVT_TILE_NT)
		out[i] = src.value(i);
}

static PoissonSource poisson_source(const PoissonArgs &a)
{
	return PoissonSource{ a.table, a.seed, (uint64_t) a.first_leaf * (uint64_t) a.nrow };
}

int launch_poisson_count(const PoissonArgs &a, int64_t *out_col_ptr, void *ws, hipStream_t s)
{
	const PoissonSource src = poisson_source(a);
	return coerce_count(a.nrow, a.nleaves, a.ncells, out_col_ptr, ws, s,
		[&](dim3 grid, dim3 block, int64_t ntiles, coerce_word *bits, int64_t *cnt) {
			if ((src.first & 1) == 0)
				hipLaunchKernelGGL(poisson_mark_pairs_kernel, grid, block, 0, s, src, a.ncells, ntiles, bits, cnt);
			else
				hipLaunchKernelGGL(from_dense_mark_kernel<PoissonSource>, grid, block, 0, s, src, a.ncells, ntiles, bits, cnt);
		});
}

int launch_poisson_fill(const PoissonArgs &a, int32_t *out_row_idx, int32_t *out_val, const void *ws, hipStream_t s)
{
	return coerce_fill(poisson_source(a), a.nrow, a.ncells, out_row_idx, out_val, ws, s);
}

int launch_rpois(const svt_poisson_table &table, uint64_t seed, int64_t first, int64_t n, int32_t *out, hipStream_t s)
{
	if (n <= 0)
		return 0;
	const int64_t nb = (n + SVT_TILE_NT - 1) / SVT_TILE_NT;
	hipLaunchKernelGGL(rpois_kernel, dim3((unsigned) (nb < RPOIS_GRID ? nb : RPOIS_GRID)), dim3(SVT_TILE_NT), 0, s,
			   PoissonSource{ table, seed, (uint64_t) first }, n, out);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_to_dense(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype, int64_t nrow, int64_t ncol,
		    int64_t nnz, int na_background, int out_Rtype, void *out, int *bad, hipStream_t s)
{
	const int64_t ncells = nrow * ncol;
	if (ncells <= 0)
		return 0;
	const int64_t ntiles = coerce_ntiles(ncells);
	const dim3 grid(coerce_grid(ntiles, COERCE_DENSE_GRID)), block(SVT_TILE_NT);
	const int64_t per = (ntiles + grid.x - 1) / grid.x;             // consecutive tiles per workgroup
	if (Rtype == SVT_REALSXP)
		hipLaunchKernelGGL((to_dense_kernel<double, double>), grid, block, 0, s, col_ptr, row_idx, (const double *) val, nrow,
				   nnz, ncells, ntiles, per, na_background, (double *) out, bad);
	else if (out_Rtype == SVT_REALSXP)
		hipLaunchKernelGGL((to_dense_kernel<int32_t, double>), grid, block, 0, s, col_ptr, row_idx, (const int32_t *) val, nrow,
				   nnz, ncells, ntiles, per, na_background, (double *) out, bad);
	else
		hipLaunchKernelGGL((to_dense_kernel<int32_t, int32_t>), grid, block, 0, s, col_ptr, row_idx, (const int32_t *) val, nrow,
				   nnz, ncells, ntiles, per, na_background, (int32_t *) out, bad);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_nzwhich(const int64_t *col_ptr, const int32_t *row_idx, int64_t nrow, int64_t ncol, int64_t nnz, int ndim,
		   const int64_t *dim, int arr_ind, void *out, hipStream_t s)
{
	if (nnz <= 0)
		return 0;
	NzwhichDims D;
	memset(&D, 0, sizeof(D));
	D.ndim = ndim;
	for (int k = 0; k < ndim && k < 8; k++) D.d[k] = dim[k];
	const int64_t ntiles = coerce_ntiles(nnz);
	const dim3 grid(coerce_grid(ntiles, COERCE_GRID)), block(SVT_TILE_NT);
	if (arr_ind)
		hipLaunchKernelGGL(nzwhich_kernel<true>, grid, block, 0, s, col_ptr, row_idx, nrow, ncol, nnz, D, out);
	else
		hipLaunchKernelGGL(nzwhich_kernel<false>, grid, block, 0, s, col_ptr, row_idx, nrow, ncol, nnz, D, out);
	HIP_TRY(hipGetLastError());
	return 0;
}
