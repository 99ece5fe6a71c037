// Device transpose of a 2-d SVT in its CSC device layout (CSC -> CSC of t(A)),
// the device counterpart of transpose_2D_SVT (src/SparseArray_aperm.c:148-423):
// `%*%`, tcrossprod() and the non-native row* stats all start with t()
// (R/SparseMatrix-mult.R:165-206).  The reference makes 3 serial passes (count
// per row, allocate, scatter in column order); here: a stable LSD radix sort of
// (row index -> position) pairs, which keeps the entries of every output leaf in
// ascending column order as the SVT format requires (src/leaf_utils.h:12-15),
// then one gather pass.  Traffic ~ 3 sort passes x 16 B/nz + 28 B/nz.
// (Round 2 also built a two-pass form -- sort on row >> 4 with 16-bit keys, the low 4 bits riding in
// the payload, the order inside every 16-row bucket finished by one wavefront inside the gather
// (ballot ranks + running counters): correct, but 4.4 ms against 4.0: the two passes of 6-byte pairs
// take as long per pass as 8-byte ones (0.65 ms), and the finishing gather stores to 16 row segments
// at once instead of one coalesced run: 2.3 ms against 1.5 + 0.12.)
#include "svt_common.h"

#include <string.h>

#include <algorithm>
#include <atomic>
#include <utility>
#include <vector>

#include "svt_scan.h"

#include "svt_sort.h"

// ---------------------------------------------------------------------------
// Exclusive scan of an int64 array (svt_scan.h)
// ---------------------------------------------------------------------------
__device__ inline int64_t wave_incl_scan_i64(int64_t v)
{
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int64_t t = __shfl_up(v, o, SVT_WAVE);
		if (lane >= o) v += t;
	}
	return v;
}

// tile of SVT_SCAN_TILE elements per workgroup: exclusive scan in place, tile total to sums[block]
__global__ void __launch_bounds__(SVT_SCAN_NT)
scan_tile_kernel(int64_t *__restrict__ data, int64_t n, int64_t *__restrict__ sums)
{
	__shared__ int64_t wtot[SVT_SCAN_NT / SVT_WAVE];
	const int64_t base = (int64_t) blockIdx.x * SVT_SCAN_TILE + (int64_t) threadIdx.x * SVT_SCAN_ITEMS;
	int64_t v[SVT_SCAN_ITEMS], run = 0;
#pragma unroll
	for (int u = 0; u < SVT_SCAN_ITEMS; u++) {
		v[u] = base + u < n ? data[base + u] : 0;
		const int64_t t = v[u];
		v[u] = run;                                     // exclusive within the thread
		run += t;
	}
	const int64_t incl = wave_incl_scan_i64(run);
	const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	if (lane == 63) wtot[w] = incl;
	__syncthreads();
	int64_t off = incl - run;
	for (int i = 0; i < w; i++) off += wtot[i];
#pragma unroll
	for (int u = 0; u < SVT_SCAN_ITEMS; u++)
		if (base + u < n) data[base + u] = v[u] + off;
	if (threadIdx.x == SVT_SCAN_NT - 1 && sums != NULL) sums[blockIdx.x] = off + run;
}

__global__ void __launch_bounds__(SVT_SCAN_NT)
scan_add_kernel(int64_t *__restrict__ data, int64_t n, const int64_t *__restrict__ sums)
{
	const int64_t add = sums[blockIdx.x];
	const int64_t base = (int64_t) blockIdx.x * SVT_SCAN_TILE + (int64_t) threadIdx.x * SVT_SCAN_ITEMS;
#pragma unroll
	for (int u = 0; u < SVT_SCAN_ITEMS; u++)
		if (base + u < n) data[base + u] += add;
}

int launch_exclusive_scan_i64(int64_t *data, int64_t n, void *ws, hipStream_t s)
{
	if (n <= 0)
		return 0;
	const int64_t nb = (n + SVT_SCAN_TILE - 1) / SVT_SCAN_TILE;
	if (nb > 0x7FFFFFFFLL)
		return svt_set_error("exclusive scan: too many elements");
	int64_t *sums = (int64_t *) ws;
	hipLaunchKernelGGL(scan_tile_kernel, dim3((unsigned) nb), dim3(SVT_SCAN_NT), 0, s, data, n, nb > 1 ? sums : (int64_t *) NULL);
	if (nb > 1) {
		if (launch_exclusive_scan_i64(sums, nb, (char *) ws + ((size_t) nb * 8 + 255) / 256 * 256, s))
			return -1;
		hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned) nb), dim3(SVT_SCAN_NT), 0, s, data, n, sums);
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

// ---------------------------------------------------------------------------
// t(A): bucketed transposition (round 3; replaces the radix sort of (row, position) pairs of rounds 1-2).
//
// What the reference does serially -- count per row, allocate, scatter column by column
// (src/SparseArray_aperm.c:148-393) -- is stable because it visits the columns in order.  The parallel
// form below keeps that order without a general-purpose sort by using what a CSC operand gives for free:
// the rows inside a column ascend (src/leaf_utils.h:12-15), so the nonzeros of one column that fall into
// a given range of rows are one contiguous run.
//
//   fine bucket   = F consecutive rows (a power of two <= 64: ~3000 nonzeros), the unit of the last pass
//   coarse bucket = 16 fine buckets
//   group         = 256 consecutive columns
//
//   pass 1 (count)   a streaming pass over the offsets: a workgroup takes a stretch of one group's nonzeros,
//                    counts them by fine bucket in LDS and adds its counts to the table
//                    T[coarse bucket][group][fine bucket in the coarse one].
//   scan             exclusive scan of T in that order: where the piece (coarse i, group g, fine s) starts
//                    in an intermediate array ordered (coarse, group, fine, column, row).
//   pass 2 (scatter) workgroup (g, i), one thread per column: the column's run of rows in the coarse bucket
//                    (an interpolated guess, then a search over what is left), the position of each of its
//                    nonzeros among the workgroup's = a scan over the 128 threads per fine bucket; the
//                    workgroup's nonzeros are assembled in LDS in their final intermediate order and leave
//                    as ONE contiguous, coalesced copy (the 16 pieces of a workgroup follow one another).
//   pass 3 (finish)  one workgroup per fine bucket: its pieces (one per group, in group order = column
//                    order) are read in sequence; a stable counting sort on the F rows (ranks inside a
//                    wavefront from ballots of the row bits, across wavefronts from a small LDS table) puts
//                    them in (row, column) order -- in LDS, and from there in one coalesced copy to their
//                    final place -- and gives the row pointers.
//
// Traffic at 1e8 nonzeros (f64): pass 1 reads the offsets (0.4 GB), pass 2 reads 1.2 GB and writes 1.3 GB
// (column 4 B + row-in-bucket 1 B + value 8 B), pass 3 reads 1.3 GB and writes 1.2 GB: 5.4 GB, every
// store coalesced.  (The first version of this round wrote pass 2 straight to memory, fine-bucket-major:
// every lane of a store instruction in another line, 48 open write streams per workgroup -- 7.5 ms for that
// pass alone; and counted with one thread per column and two binary searches: 2.2 ms.)
// Shapes it does not fit (less than one nonzero per column and coarse bucket) take the key sort of
// launch_transpose_sorted() below.
// ---------------------------------------------------------------------------
// which route the transpositions / permutations of this process took (svt_dev_aperm_route_counts; the fuzzers print it:
// evidence for what is hot and what is a fallback), in the order device.aperm_route_counts() names them.  Atomic: the
// sharded host entry points transpose on one thread per device.
enum {
	R_T_BUCKETED, R_T_KEY_SORT, R_LEAF_PRESERVING, R_SWAP01 /* first two axes swapped (bucketed) */, R_SLAB,
	R_VIA_3D, R_GENERAL /* composed */, R_SORT32, R_SORT64, R_SLAB_REFUSED /* at run time */, R_NROUTES
};
static std::atomic<int64_t> g_route[R_NROUTES];
void aperm_route_counts(int64_t *out, int reset)
{
	for (int i = 0; i < R_NROUTES; i++) {
		const int64_t v = reset ? g_route[i].exchange(0) : g_route[i].load();
		if (out != NULL) out[i] = v;
	}
}

// bytes of n elements of esz bytes as a part of a workspace: rounded up to 256
static size_t t2_a(size_t n, size_t esz) { return (n * esz + 255) / 256 * 256; }

// product of the extents dim[from .. to) as a double, without axis `skip`; an extent below 1 counts as 1 unless !clamp
static double extent_prod(const int64_t *dim, int from, int to, int skip = -1, bool clamp = true)
{
	double p = 1.0;
	for (int a = from; a < to; a++)
		if (a != skip) p *= (double) (clamp && dim[a] < 1 ? 1 : dim[a]);
	return p;
}
#define LEAVES_MAX 2147483646.0   // leaf counts the 32-bit forms take lie below this

#define T2_NT 256                 // columns per group = threads per workgroup of pass 2
#define T2_NFINE_MAX 32           // fine buckets per coarse bucket: 16 or 32 (T2Shape::cbits = 4 or 5)
#define T2_CAP 2048               // nonzeros a pass-2 workgroup assembles in LDS (more: straight to memory)
#define T2_CPW 2                  // coarse buckets a pass-2 workgroup takes, one after the other (t(A) at config 2: 1 -> 2.06 ms, 2 -> 2.05, 4 -> 2.12, 8 -> 2.20, 16 -> 2.30)
#define T1_NT 1024
#define T1_HIST 65536             // fine buckets counted per sweep of pass 1 (LDS: two 16-bit counters per word --
                                  // a workgroup's 16 columns hold at most 16 * 64 nonzeros of one fine bucket)
#define T3_NT 512
#define T3_CAP 4096               // nonzeros a pass-3 workgroup ranks in one round (more: round by round, straight to memory)
#define T3_STAGE 2048             // of which the LDS image of the output holds this many at a time

// Batched form (round 4): `nslab` independent matrices of srow x scol that follow one another in the operand's
// columns (slab s = columns [s * scol, (s + 1) * scol)), each transposed on its own -- aperm(x, c(2, 1, 3, ...)) of an
// N-d array; nfb / ncoarse / ngroups count per slab, the table is ordered (slab, coarse, group, fine).  One matrix:
// nslab = 1, srow = nrow, scol = ncol.
struct T2Shape {
	int fbits;                // log2(F)
	int64_t nfb;              // fine buckets (per slab)
	int64_t ncoarse;
	int64_t ngroups;
	int64_t nslab, srow, scol;
	int cbits;                // log2(fine buckets per coarse bucket): 4, or 5 where that fills the pass-2 workgroups better
};

__device__ inline int64_t t2_slot(const T2Shape &sh, int64_t sl, int64_t fb, int64_t g)
{
	return ((((sl * sh.ncoarse + (fb >> sh.cbits)) * sh.ngroups + g) << sh.cbits)) + (fb & ((1 << sh.cbits) - 1));
}

// pass 1: workgroup = 16 columns (16 divides the group size), one per wavefront (coalesced along the column); counts by fine bucket in
// LDS, and cstart[c * (ncoarse + 1) + i] = first position of column c whose row lies in coarse bucket i or
// later (i = 0 .. ncoarse), which is where pass 2 finds its runs without a search (a wavefront writes the
// starts of its column next to one another; a pass-2 workgroup reads nine consecutive ones per column).
__global__ void __launch_bounds__(T1_NT)
transpose_count_kernel(const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ row_idx,
		       int64_t ncol, T2Shape sh, unsigned long long *__restrict__ table,
		       uint32_t *__restrict__ cstart)
{
	extern __shared__ uint32_t hist[];              // [T1_HIST / 2]
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const int64_t wps = (sh.scol + T1_NT / 64 - 1) / (T1_NT / 64);            // workgroups per slab
	const int64_t sl = (int64_t) blockIdx.x / wps, bl = (int64_t) blockIdx.x % wps;
	const int64_t cl = bl * (T1_NT / 64) + w;                                  // column inside the slab
	const bool have = cl < sh.scol;
	const int64_t c = sl * sh.scol + cl;
	const int64_t g = (bl * (T1_NT / 64)) / T2_NT;                            // (16 divides 256: one group per workgroup)
	const int cshift = sh.fbits + sh.cbits;         // log2(rows per coarse bucket)
	int64_t beg = 0, end = 0;
	if (have) { beg = col_ptr[c]; end = col_ptr[c + 1]; }
	for (int64_t w0 = 0; w0 < sh.nfb; w0 += T1_HIST) {          // (one sweep unless there are > T1_HIST = 65536 fine buckets)
		const int64_t w1 = w0 + T1_HIST < sh.nfb ? w0 + T1_HIST : sh.nfb;
		for (int x = threadIdx.x; x < (int) ((w1 - w0 + 1) >> 1); x += T1_NT) hist[x] = 0;
		__syncthreads();
		for (int64_t kb = beg; kb < end; kb += 256) {           // four batches of 64 in flight
			int32_t r4[4];
#pragma unroll
			for (int u = 0; u < 4; u++) r4[u] = kb + u * 64 + lane < end ? row_idx[kb + u * 64 + lane] : 0x7FFFFFFF;
			const int32_t r_before = kb > beg ? row_idx[kb - 1] : -1;
#pragma unroll
			for (int u = 0; u < 4; u++) {
				const int64_t k0 = kb + u * 64, k = k0 + lane;
				if (k0 >= end) break;
				const int32_t r = r4[u];
				if (k < end) {
					const int64_t fb = (int64_t) r >> sh.fbits;
					if (fb >= w0 && fb < w1) atomicAdd(&hist[(fb - w0) >> 1], 1u << (16 * (int) ((fb - w0) & 1)));
				}
				if (w0 == 0 && have) {
					// coarse buckets that start at position k: those after the previous entry's, up to this one's
					int32_t rp = __shfl_up(r, 1, SVT_WAVE);
					const int32_t last_prev = __shfl(r4[u > 0 ? u - 1 : 0], 63, SVT_WAVE);      // (all lanes take part)
					if (lane == 0) rp = u == 0 ? r_before : last_prev;
					const int64_t ip = rp < 0 ? -1 : ((int64_t) rp >> cshift);
					const int64_t ic = k < end ? ((int64_t) r >> cshift) : (k == end ? sh.ncoarse : ip);
					for (int64_t i = ip + 1; i <= ic; i++) cstart[c * (sh.ncoarse + 1) + i] = (uint32_t) k;
				}
			}
		}
		if (w0 == 0 && have && lane == 0) {
			// (a column whose length is a multiple of 64 -- or zero -- has not closed its last buckets)
			if (((end - beg) & 63) == 0) {
				const int64_t ip = end > beg ? ((int64_t) row_idx[end - 1] >> cshift) : -1;
				for (int64_t i = ip + 1; i <= sh.ncoarse; i++) cstart[c * (sh.ncoarse + 1) + i] = (uint32_t) end;
			}
		}
		__syncthreads();
		for (int x = threadIdx.x; x < (int) (w1 - w0); x += T1_NT) {
			const uint32_t n = (hist[x >> 1] >> (16 * (x & 1))) & 0xFFFFu;
			if (n) atomicAdd(table + t2_slot(sh, sl, w0 + x, g), (unsigned long long) n);
		}
		__syncthreads();
	}
}

// Passes 2 and 3 are the same operation: a workgroup holds a SEQUENCE of nonzeros made of pieces (pass 2:
// the runs of its 128 columns inside the coarse bucket; pass 3: the pieces of its fine bucket, one per
// group) and splits it by a small key (pass 2: the fine bucket, 4 bits; pass 3: the row inside the bucket,
// <= 6 bits) keeping the order inside every key.  Element x of the sequence is read by thread x mod NT
// (consecutive lanes = consecutive addresses inside a piece: coalesced), kept in registers, ranked --
// rank inside the wavefront from one ballot per key bit, the wavefronts' counts per key in an LDS table,
// prefixed in element order -- and written to its place in an LDS image of the output, which leaves in one
// linear copy.  Sequences longer than the image (NT * ITEMS elements) go round by round, straight to memory.
template <int NT, int ITEMS, int MAXKEYS>
struct SplitLds {
	int32_t binstart[MAXKEYS];              // first output slot of every key (histogram first, then its prefix)
	int32_t run[MAXKEYS];                   // slots used by earlier rounds
	int32_t rtot[MAXKEYS];                  // elements of the current round
	int32_t totu[ITEMS][MAXKEYS];           // per key: elements of the chunks before chunk u (this round)
	uint16_t wc[ITEMS][NT / 64][MAXKEYS];   // per key: elements of chunk u in the wavefronts before w (<= NT)
};

// lanes of the wavefront whose element is valid and has the same key: one ballot per key bit
__device__ inline uint64_t split_peers(bool valid, int key, int kbits)
{
	uint64_t peers = __ballot(valid);
	for (int bit = 0; bit < kbits; bit++) {
		const uint64_t m = __ballot((key >> bit) & 1);
		peers &= ((key >> bit) & 1) ? m : ~m;
	}
	return peers;
}

// binstart[0 .. nkeys) holds the histogram: turn it into its exclusive prefix (nkeys <= 256, wavefront 0;
// the other wavefronts wait at the caller's barrier).  f(k, start) is called for every key by the lane that
// owns it.
template <typename F>
__device__ inline void split_scan_bins(int32_t *binstart, int nkeys, F f)
{
	const int lane = threadIdx.x & 63;
	if ((threadIdx.x >> 6) != 0) return;
	int32_t v[4], tot = 0;
#pragma unroll
	for (int u = 0; u < 4; u++) { v[u] = lane * 4 + u < nkeys ? binstart[lane * 4 + u] : 0; tot += v[u]; }
	int32_t incl = tot;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int32_t x = __shfl_up(incl, o, SVT_WAVE);
		if (lane >= o) incl += x;
	}
	int32_t off = incl - tot;
#pragma unroll
	for (int u = 0; u < 4; u++) {
		const int k = lane * 4 + u;
		if (k < nkeys) { binstart[k] = off; f(k, off); }
		off += v[u];
	}
}

// Output slots of one round: key[u] (valid[u]) belongs to element u * NT + t of the round.  All threads of
// the workgroup call it; nkeys = 1 << kbits <= MAXKEYS.
template <int NT, int ITEMS, int MAXKEYS>
__device__ inline void split_round(SplitLds<NT, ITEMS, MAXKEYS> &L, const bool (&valid)[ITEMS],
				   const int (&key)[ITEMS], int kbits, int32_t (&at)[ITEMS])
{
	const int t = threadIdx.x, lane = t & 63, w = t >> 6, nkeys = 1 << kbits;
	const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
	for (int k = t; k < nkeys; k += NT) { L.run[k] += L.rtot[k]; L.rtot[k] = 0; }      // the previous round's elements
	for (int x = t; x < ITEMS * (NT / 64) * MAXKEYS / 2; x += NT) ((uint32_t *) &L.wc[0][0][0])[x] = 0;
	__syncthreads();
	int rank[ITEMS];
#pragma unroll
	for (int u = 0; u < ITEMS; u++) {
		const uint64_t peers = split_peers(valid[u], key[u], kbits);
		rank[u] = __popcll(peers & lt);
		if (valid[u] && rank[u] == 0) L.wc[u][w][key[u]] = (uint16_t) __popcll(peers);
	}
	__syncthreads();
	// exclusive prefix in element order (chunk u, then wavefront w), per key
	for (int x = t; x < ITEMS * nkeys; x += NT) {
		const int u = x / nkeys, k = x % nkeys;
		int32_t sum = 0;
		for (int ww = 0; ww < NT / 64; ww++) { const int32_t v = L.wc[u][ww][k]; L.wc[u][ww][k] = (uint16_t) sum; sum += v; }
		L.totu[u][k] = sum;
	}
	__syncthreads();
	for (int k = t; k < nkeys; k += NT) {
		int32_t sum = 0;
		for (int u = 0; u < ITEMS; u++) { const int32_t v = L.totu[u][k]; L.totu[u][k] = sum; sum += v; }
		L.rtot[k] = sum;
	}
	__syncthreads();
#pragma unroll
	for (int u = 0; u < ITEMS; u++)
		at[u] = valid[u] ? L.binstart[key[u]] + L.run[key[u]] + L.totu[u][key[u]] + L.wc[u][w][key[u]] + rank[u] : 0;
}

// last j in [0, np) with pre[j] <= x  (pre[0] = 0, pre[np] = length of the sequence > x)
__device__ inline int split_piece_of(const int32_t *pre, int np, int32_t x)
{
	int lo = 0, hi = np - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (pre[mid] <= x) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// pass 2
#define T2_ITEMS (T2_CAP / T2_NT)
template <typename T>
__global__ void __launch_bounds__(T2_NT)
transpose_scatter_kernel(const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ row_idx,
			 const T *__restrict__ val, int64_t nrow, int64_t ncol, T2Shape sh,
			 const int64_t *__restrict__ table, const uint32_t *__restrict__ cstart,
			 int32_t *__restrict__ col1, uint8_t *__restrict__ rlow1, T *__restrict__ val1)
{
	__shared__ SplitLds<T2_NT, T2_ITEMS, T2_NFINE_MAX> L;
	const int nfine = 1 << sh.cbits;
	__shared__ int64_t pa[T2_NT];                   // first position of every column's run
	__shared__ int32_t ppre[T2_NT + 1];             // lengths of the runs, then their prefix
	__shared__ uint8_t owner[T2_CAP];               // column (0 .. 255) of every element of the sequence
	__shared__ int32_t s_col[T2_CAP];
	__shared__ T s_val[T2_CAP];
	__shared__ uint8_t s_row[T2_CAP];
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	const int64_t wps = sh.ngroups * ((sh.ncoarse + T2_CPW - 1) / T2_CPW);     // workgroups per slab
	const int64_t sl = (int64_t) blockIdx.x / wps, bl = (int64_t) blockIdx.x % wps;
	const int64_t g = bl % sh.ngroups, i0 = (bl / sh.ngroups) * T2_CPW;
	const bool have = g * T2_NT + t < sh.scol;
	const int64_t c = sl * sh.scol + g * T2_NT + t;
	// where this column's runs of the workgroup's T2_CPW coarse buckets start (recorded by pass 1)
	uint32_t cs[T2_CPW + 1];
#pragma unroll
	for (int q = 0; q <= T2_CPW; q++)
		cs[q] = (have && i0 + q <= sh.ncoarse) ? cstart[c * (sh.ncoarse + 1) + i0 + q] : 0u;
#pragma unroll 1
	for (int q = 0; q < T2_CPW; q++) {
	const int64_t i = i0 + q;
	if (i >= sh.ncoarse) break;                     // (uniform)
	if (q > 0) __syncthreads();                     // the previous bucket's image has left
	const int64_t r_lo = (i << sh.cbits) << sh.fbits;
	int64_t a = 0, b = 0;
	if (have) {
#pragma unroll
		for (int qq = 0; qq < T2_CPW; qq++) if (qq == q) { a = cs[qq]; b = cs[qq + 1]; }
	}
	pa[t] = a;
	// prefix of the run lengths over the threads
	{
		__shared__ int32_t wsum[T2_NT / 64];
		const int32_t v = (int32_t) (b - a);
		int32_t incl = v;
#pragma unroll
		for (int o = 1; o < 64; o <<= 1) {
			const int32_t x = __shfl_up(incl, o, SVT_WAVE);
			if (lane >= o) incl += x;
		}
		if (lane == 63) wsum[w] = incl;
		if (t < nfine) { L.binstart[t] = 0; L.run[t] = 0; L.rtot[t] = 0; }
		__syncthreads();
		int32_t off = 0;
		for (int ww = 0; ww < w; ww++) off += wsum[ww];
		ppre[t + 1] = incl + off;
		if (t == 0) ppre[0] = 0;
		__syncthreads();
	}
	const int32_t n = ppre[T2_NT];
	const int64_t base = table[((sl * sh.ncoarse + i) * sh.ngroups + g) << sh.cbits];     // start of the workgroup's stretch
	if (n <= T2_CAP) {
		for (int32_t x = ppre[t]; x < ppre[t + 1]; x++) owner[x] = (uint8_t) t;
		__syncthreads();
	}
	const int fmask = (1 << sh.fbits) - 1;
	const bool staged = n <= T2_CAP;
	if (!staged) {
		// more than the image holds (rare): the histogram needs a pass of its own
		for (int32_t x = t; x < n; x += T2_NT) {
			const int j = split_piece_of(ppre, T2_NT, x);
			const int q = (int) ((int64_t) row_idx[pa[j] + (x - ppre[j])] - r_lo);
			atomicAdd(&L.binstart[q >> sh.fbits], 1);
		}
		__syncthreads();
		split_scan_bins(L.binstart, nfine, [](int, int32_t) {});
		__syncthreads();
	}
	for (int32_t x0 = 0; x0 < n; x0 += T2_CAP) {
		bool valid[T2_ITEMS];
		int key[T2_ITEMS], rl[T2_ITEMS], cj[T2_ITEMS];
		int32_t rw[T2_ITEMS];
		T vv[T2_ITEMS];
		int32_t at[T2_ITEMS];
		int64_t kk[T2_ITEMS];
#pragma unroll
		for (int u = 0; u < T2_ITEMS; u++) {
			const int32_t x = x0 + u * T2_NT + t;
			valid[u] = x < n;
			cj[u] = !valid[u] ? 0 : (n <= T2_CAP ? (int) owner[x] : split_piece_of(ppre, T2_NT, x));
			kk[u] = valid[u] ? pa[cj[u]] + (x - ppre[cj[u]]) : 0;
		}
		// (all loads of the round in flight together: one memory latency per round, not one per element)
#pragma unroll
		for (int u = 0; u < T2_ITEMS; u++) rw[u] = valid[u] ? row_idx[kk[u]] : 0;
#pragma unroll
		for (int u = 0; u < T2_ITEMS; u++) vv[u] = valid[u] ? val[kk[u]] : (T) 0;
#pragma unroll
		for (int u = 0; u < T2_ITEMS; u++) {
			const int q = valid[u] ? (int) ((int64_t) rw[u] - r_lo) : 0;
			key[u] = q >> sh.fbits; rl[u] = q & fmask;
		}
		if (staged) {                                   // the only round: histogram from the registers
#pragma unroll
			for (int u = 0; u < T2_ITEMS; u++) if (valid[u]) atomicAdd(&L.binstart[key[u]], 1);
			__syncthreads();
			split_scan_bins(L.binstart, nfine, [](int, int32_t) {});
			__syncthreads();
		}
		split_round<T2_NT, T2_ITEMS, T2_NFINE_MAX>(L, valid, key, sh.cbits, at);
#pragma unroll
		for (int u = 0; u < T2_ITEMS; u++) {
			if (!valid[u]) continue;
			const int32_t cc = (int32_t) (g * T2_NT + cj[u]);
			if (staged) { s_col[at[u]] = cc; s_row[at[u]] = (uint8_t) rl[u]; s_val[at[u]] = vv[u]; }
			else { col1[base + at[u]] = cc; rlow1[base + at[u]] = (uint8_t) rl[u]; val1[base + at[u]] = vv[u]; }
		}
	}
	if (!staged)
		continue;
	__syncthreads();
	for (int32_t e = t; e < n; e += T2_NT) {
		col1[base + e] = s_col[e];
		rlow1[base + e] = s_row[e];
		val1[base + e] = s_val[e];
	}
	}
}

// pass 3
#define T3_ITEMS (T3_CAP / T3_NT)
template <typename T>
__global__ void __launch_bounds__(T3_NT)
transpose_finish_kernel(const int64_t *__restrict__ table, T2Shape sh, int64_t nrow, int64_t nnz,
			const int32_t *__restrict__ col1, const uint8_t *__restrict__ rlow1,
			const T *__restrict__ val1, const int64_t *__restrict__ fb_base,
			int64_t *__restrict__ out_ptr, int32_t *__restrict__ out_idx, T *__restrict__ out_val)
{
	extern __shared__ unsigned char t3_lds[];
	// [split tables][piece starts ngroups * 8][piece prefix (ngroups + 1) * 4][sorted columns CAP][sorted values CAP]
	typedef SplitLds<T3_NT, T3_ITEMS, 64> Tables;
	Tables &L = *(Tables *) t3_lds;
	const int ng = (int) sh.ngroups;
	int64_t *pa = (int64_t *) (t3_lds + ((sizeof(Tables) + 15) & ~(size_t) 15));
	int32_t *ppre = (int32_t *) (pa + ng);
	int32_t *s_idx = ppre + ((ng + 1 + 3) & ~3);
	T *s_val = (T *) (s_idx + T3_STAGE);
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	const int F = 1 << sh.fbits;
	const int64_t sl = (int64_t) blockIdx.x / sh.nfb, fb = (int64_t) blockIdx.x % sh.nfb, ci = fb >> sh.cbits;
	const int sf = (int) (fb & ((1 << sh.cbits) - 1));
	// the pieces of this fine bucket, one per group: starts, sizes, then the prefix of the sizes
	for (int g = t; g < ng; g += T3_NT) {
		const int64_t slot = (((sl * sh.ncoarse + ci) * ng + g) << sh.cbits) + sf;
		const int64_t p0 = table[slot];
		pa[g] = p0;
		ppre[g + 1] = (int32_t) (table[slot + 1] - p0);
	}
	for (int k = t; k < 64; k += T3_NT) { L.binstart[k] = 0; L.run[k] = 0; L.rtot[k] = 0; }
	__syncthreads();
	if (w == 0) {                                   // inclusive scan of the piece sizes by one wavefront
		int32_t carry = 0;
		for (int g0 = 0; g0 < ng; g0 += 64) {
			const int g = g0 + lane;
			const int32_t v = g < ng ? ppre[g + 1] : 0;
			int32_t incl = v;
#pragma unroll
			for (int o = 1; o < 64; o <<= 1) {
				const int32_t u = __shfl_up(incl, o, SVT_WAVE);
				if (lane >= o) incl += u;
			}
			if (g < ng) ppre[g + 1] = carry + incl;
			carry += __shfl(incl, 63, SVT_WAVE);
		}
		if (lane == 0) ppre[0] = 0;
	}
	__syncthreads();
	const int32_t n = ppre[ng];
	const int64_t b0 = fb_base[sl * sh.nfb + fb];   // first output position of the bucket's rows
	const bool staged = n <= T3_CAP;
	auto bins_done = [&]() {
		__syncthreads();
		split_scan_bins(L.binstart, F, [&](int r, int32_t off) {
			const int64_t row = (fb << sh.fbits) + r;
			if (row < sh.srow) out_ptr[sl * sh.srow + row] = b0 + off;
		});
		if (sl == sh.nslab - 1 && fb == sh.nfb - 1 && t == 0) out_ptr[sh.nslab * sh.srow] = nnz;
		__syncthreads();
	};
	if (!staged || n == 0) {
		// more than the image holds (rare): the histogram needs a pass of its own
		for (int32_t x = t; x < n; x += T3_NT) {
			const int j = split_piece_of(ppre, ng, x);
			atomicAdd(&L.binstart[rlow1[pa[j] + (x - ppre[j])]], 1);
		}
		bins_done();
	}
	for (int32_t x0 = 0; x0 < n; x0 += T3_CAP) {
		bool valid[T3_ITEMS];
		int key[T3_ITEMS];
		int32_t cc[T3_ITEMS], at[T3_ITEMS];
		T vv[T3_ITEMS];
		int64_t kk[T3_ITEMS];
#pragma unroll
		for (int u = 0; u < T3_ITEMS; u++) {
			const int32_t x = x0 + u * T3_NT + t;
			valid[u] = x < n;
			const int j = valid[u] ? split_piece_of(ppre, ng, x) : 0;
			kk[u] = valid[u] ? pa[j] + (x - ppre[j]) : 0;
		}
		// (all loads of the round in flight together)
#pragma unroll
		for (int u = 0; u < T3_ITEMS; u++) key[u] = valid[u] ? (int) rlow1[kk[u]] : 0;
#pragma unroll
		for (int u = 0; u < T3_ITEMS; u++) cc[u] = valid[u] ? col1[kk[u]] : 0;
#pragma unroll
		for (int u = 0; u < T3_ITEMS; u++) vv[u] = valid[u] ? val1[kk[u]] : (T) 0;
		if (staged) {                                   // the only round: histogram from the registers
#pragma unroll
			for (int u = 0; u < T3_ITEMS; u++) if (valid[u]) atomicAdd(&L.binstart[key[u]], 1);
			bins_done();
		}
		split_round<T3_NT, T3_ITEMS, 64>(L, valid, key, sh.fbits, at);
		if (!staged) {
#pragma unroll
			for (int u = 0; u < T3_ITEMS; u++)
				if (valid[u]) { out_idx[b0 + at[u]] = cc[u]; out_val[b0 + at[u]] = vv[u]; }
			continue;
		}
		// the LDS image holds a quarter of the output at a time (the elements stay in registers): 24 KB
		// instead of 96, three workgroups per CU instead of one
		for (int32_t q0 = 0; q0 < n; q0 += T3_STAGE) {
			const int32_t q1 = q0 + T3_STAGE < n ? q0 + T3_STAGE : n;
			__syncthreads();
#pragma unroll
			for (int u = 0; u < T3_ITEMS; u++)
				if (valid[u] && at[u] >= q0 && at[u] < q1) { s_idx[at[u] - q0] = cc[u]; s_val[at[u] - q0] = vv[u]; }
			__syncthreads();
			for (int32_t e = q0 + t; e < q1; e += T3_NT) { out_idx[b0 + e] = s_idx[e - q0]; out_val[b0 + e] = s_val[e - q0]; }
		}
	}
}

// fb_base[fb] = nonzeros in the fine buckets before fb (= first output position of its rows): the sum of
// the table over (group, fine = fb) ... computed from the scanned table: the pieces of one COARSE bucket are
// contiguous, so base(coarse i) = T[(i * ngroups) * 16]; inside it the fine buckets are interleaved by group.
__global__ void transpose_fb_base_kernel(const int64_t *__restrict__ table, T2Shape sh, int64_t nnz,
					 int64_t *__restrict__ fb_base)
{
	// one wavefront per coarse bucket: sizes of its 16 fine buckets summed over the groups, then a prefix
	const int lane = threadIdx.x & 63;
	// (ci counts over all slabs: the pieces of one (slab, coarse bucket) pair are contiguous in the table)
	const int64_t ci = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (ci >= sh.nslab * sh.ncoarse) return;
	const int64_t sl = ci / sh.ncoarse, cil = ci % sh.ncoarse;
	const int64_t ng = sh.ngroups;
	const int nfine = 1 << sh.cbits;
	int64_t acc[T2_NFINE_MAX];
#pragma unroll
	for (int s = 0; s < T2_NFINE_MAX; s++) acc[s] = 0;
	const int64_t tot = ng * nfine;                   // slots of this coarse bucket
	const int64_t s0 = ci * tot;
	for (int64_t x = lane; x < tot; x += 64) {
		const int64_t sz = table[s0 + x + 1] - table[s0 + x];
		const int s = (int) (x & (nfine - 1));
#pragma unroll
		for (int q = 0; q < T2_NFINE_MAX; q++) if (q == s) acc[q] += sz;
	}
	int64_t run = table[s0];
#pragma unroll
	for (int s = 0; s < T2_NFINE_MAX; s++) {
		if (s >= nfine) break;
		int64_t v = acc[s];
		for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, SVT_WAVE);
		const int64_t fb = cil * nfine + s;
		if (lane == 0 && fb < sh.nfb) fb_base[sl * sh.nfb + fb] = run;
		run += v;
	}
	if (ci == sh.nslab * sh.ncoarse - 1 && lane == 0) fb_base[sh.nslab * sh.nfb] = nnz;
}

// the bucketed form applies to this operand: fills *sh
static bool t2_shape(int64_t nrow, int64_t ncol, int64_t nnz_all, T2Shape *sh, int64_t nslab = 1)
{
	if (nrow <= 0 || ncol <= 0 || nnz_all <= 0 || nslab <= 0)
		return false;
	const int64_t nnz = nnz_all / nslab;            // (per slab; nrow, ncol are a slab's)
	if (nnz <= 0)
		return false;
	const double per_row = (double) nnz / (double) nrow, per_col = (double) nnz / (double) ncol;
	// the largest F <= 64 with ~3000 nonzeros per fine bucket (pass 3 ranks 4096 per round) and ~1500 per
	// pass-2 workgroup (it assembles 2048 in LDS); 32 fine buckets per coarse one where that costs no F (short
	// columns: aperm(x, c(2, 1, 3)) at BASELINE config 5 fills a pass-2 workgroup with 1310 nonzeros instead of 655)
	int fbits = -1, cbits = 4;
	for (int cb = 5; cb >= 4; cb--) {
		int fb = 6;
		while (fb > 0 && (ldexp(per_row, fb) > 3520.0 ||
				  (double) T2_NT * per_col * ldexp((double) (1 << cb), fb) / (double) nrow > 1536.0))
			fb--;
		if (fb > fbits) { fbits = fb; cbits = cb; }
	}
	const int nfine = 1 << cbits;
	if (per_col * ldexp((double) nfine, fbits) / (double) nrow < 1.0)      // less than one nonzero per thread of pass 2
		return false;
	sh->cbits = cbits;
	sh->fbits = fbits;
	sh->nfb = (nrow + ((int64_t) 1 << fbits) - 1) >> fbits;
	sh->ncoarse = (sh->nfb + nfine - 1) / nfine;
	sh->ngroups = (ncol + T2_NT - 1) / T2_NT;
	sh->nslab = nslab; sh->srow = nrow; sh->scol = ncol;
	const double ntab = (double) nslab * (double) sh->ncoarse * (double) sh->ngroups * nfine;
	const double nwg = (double) nslab * (double) sh->ncoarse * (double) sh->ngroups;
	if ((double) nslab * (double) sh->nfb >= 2.0e9 || (double) nslab * (double) ncol >= 2.0e9)
		return false;
	// many small slabs: a pass-3 workgroup per fine bucket needs a few hundred nonzeros to be worth its launch
	// (slabs of 2e4 x 64 with 6400 nonzeros would make 6e6 workgroups of 20) -- the key sort takes those
	if (nslab > 1 && ldexp(per_row, fbits) < 512.0)
		return false;
	if ((double) (sh->ncoarse + 1) * (double) ncol > 2.0 * (double) nnz + 32.0)     // (the table of coarse-bucket starts)
		return false;
	return ntab < 1.0e8 && nwg < 2.0e9 && sh->ngroups <= 6000;      // (pass 3 keeps one int per group in LDS)
}

// Head of the bucketed form's workspace: [table ntab * 8][fine buckets' output positions (nslab * nfb + 1) * 8][scan scratch].
// launch_transpose() tests it against t2_reserve(), aperm_swap01_bytes() sizes its reserve from it, launch_transpose_bucketed() carves it.
struct T2Head { int64_t ntab; size_t table, fb_base, scan, total; };
static T2Head t2_head(const T2Shape &sh)
{
	const int64_t ntab = ((sh.nslab * sh.ncoarse * sh.ngroups) << sh.cbits) + 1;
	const size_t fb = t2_a((size_t) ntab, 8), scan = fb + t2_a((size_t) (sh.nslab * sh.nfb + 1), 8);
	return T2Head{ntab, 0, fb, scan, scan + exclusive_scan_ws_bytes(ntab)};
}

// ---- fallback: stable LSD radix sort of (row -> position) pairs, then a gather (rounds 1-2; any shape) ----
__global__ void iota_u32_kernel(uint32_t *__restrict__ p, int64_t n)
{
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) p[i] = (uint32_t) i;
}

// out_ptr[r] = first position of row r in the sorted order (lower bound)
__global__ void row_bounds_kernel(const int32_t *__restrict__ sorted_rows, int64_t nnz,
				  int64_t nrow, int64_t *__restrict__ out_ptr)
{
	const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (r > nrow) return;
	int64_t lo = 0, hi = nnz;
	while (lo < hi) {
		const int64_t mid = (lo + hi) >> 1;
		if ((int64_t) sorted_rows[mid] < r) lo = mid + 1; else hi = mid;
	}
	out_ptr[r] = lo;
}

// Which chunk of 256 outputs a workgroup takes.  Workgroups are dealt round-robin over the 8 XCDs
// (MI355X_MICROARCH.md, Workgroup dispatch): with chunk = blockIdx the 8 entries of one 64-byte
// sector of `val` -- 8 consecutive nonzeros of a column, i.e. 8 output rows ~100 rows apart -- are
// gathered by workgroups of 8 different XCDs and every XCD's L2 fetches the sector for itself.
// Here XCD x walks the x-th eighth of the output in order, so a sector is fetched by one L2 and
// its other entries hit it (2.9 -> ~1 ms for the gather of t(A) at 1e8 nonzeros).
__device__ inline int64_t xcd_chunk(int64_t nchunks)
{
	const int64_t b = blockIdx.x, per = (nchunks + 7) / 8;
	return (b & 7) * per + (b >> 3);
}

// Column of source position k without a search over all of col_ptr: hint[b] = the column that
// holds position b << HINT_SHIFT.  A full binary search per output costs ~8 L2 requests on the same
// few col_ptr lines from every CU (the gather ran at the L2's request rate: 5.6e8 requests in 3 ms,
// 97 % hits, profiles/r02_transpose_*); with the hint the search runs over the handful of columns
// that start inside one block of 256 positions.
#define HINT_SHIFT 8
__global__ void col_hint_kernel(const int64_t *__restrict__ col_ptr, int64_t ncol, int64_t nblk,
				uint32_t *__restrict__ hint)
{
	const int64_t b = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (b > nblk) return;
	const int64_t k = b << HINT_SHIFT;
	int64_t lo = 0, hi = ncol;                  // last c with col_ptr[c] <= k (ncol if k is past the end)
	while (lo < hi) {
		const int64_t mid = (lo + hi + 1) >> 1;
		if (col_ptr[mid] <= k) lo = mid; else hi = mid - 1;
	}
	hint[b] = (uint32_t) lo;
}

// (4 outputs per thread with streamed loads / stores: 2.0 ms against 1.5 ms for this form)
template <typename T>
__global__ void transpose_gather_kernel(const int64_t *__restrict__ col_ptr, int64_t ncol,
					const T *__restrict__ val, const uint32_t *__restrict__ perm,
					const uint32_t *__restrict__ hint,
					int64_t nnz, int32_t *__restrict__ out_idx, T *__restrict__ out_val)
{
	const int64_t i = xcd_chunk((nnz + blockDim.x - 1) / blockDim.x) * blockDim.x + threadIdx.x;
	if (i >= nnz) return;
	const int64_t k = perm[i];
	// column of position k: last c with col_ptr[c] <= k, between the hints of k's block and the next
	int64_t lo = hint[k >> HINT_SHIFT], hi = hint[(k >> HINT_SHIFT) + 1];
	if (hi > ncol - 1) hi = ncol - 1;
	while (lo < hi) {
		const int64_t mid = (lo + hi + 1) >> 1;
		if (col_ptr[mid] <= k) lo = mid; else hi = mid - 1;
	}
	out_idx[i] = (int32_t) lo;
	out_val[i] = val[k];
}

static unsigned blocks256(int64_t n) { return (unsigned) ((n + 255) / 256); }
static unsigned blocks256_xcd(int64_t n) { return (unsigned) (((n + 255) / 256 + 7) / 8 * 8); }      // whole rounds over the 8 XCDs (xcd_chunk)

static int key_bits(int64_t nrow)
{
	int b = 1;
	while (b < 31 && ((int64_t) 1 << b) < nrow) b++;
	return b;
}

static size_t hint_bytes(int64_t nnz)
{
	return ((size_t) ((nnz >> HINT_SHIFT) + 2) * 4 + 255) / 256 * 256;
}

// [sorted rows nnz*4][positions nnz*4][sorted positions nnz*4][second buffers of the sort's passes 2 * nnz*4][column hints]
// [the sort's histograms] + 256
struct TSortedLayout { size_t srows, pos, perm, ktmp, ptmp, hint, sort, total; };
static TSortedLayout t_sorted_layout(int64_t nnz)
{
	const size_t a = t2_a((size_t) (nnz > 0 ? nnz : 1), 4), sort = 5 * a + hint_bytes(nnz);
	return TSortedLayout{0, a, 2 * a, 3 * a, 4 * a, 5 * a, sort, sort + svt_sort_ws_bytes(nnz) + 256};
}
static size_t transpose_sorted_ws_bytes(int64_t nnz) { return t_sorted_layout(nnz).total; }

static int launch_transpose_sorted(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
		     int64_t nrow, int64_t ncol, int64_t nnz, int64_t *out_ptr, int32_t *out_idx,
		     void *out_val, void *ws, hipStream_t s)
{
	g_route[R_T_KEY_SORT]++;
	const TSortedLayout L = t_sorted_layout(nnz);
	char *w = (char *) ws;
	uint32_t *srows = (uint32_t *) (w + L.srows), *pos = (uint32_t *) (w + L.pos), *perm = (uint32_t *) (w + L.perm);
	uint32_t *ktmp = (uint32_t *) (w + L.ktmp), *ptmp = (uint32_t *) (w + L.ptmp), *hint = (uint32_t *) (w + L.hint);
	hipLaunchKernelGGL(iota_u32_kernel, dim3(blocks256(nnz)), dim3(256), 0, s, pos, nnz);
	const int64_t nblk = (nnz >> HINT_SHIFT) + 1;
	hipLaunchKernelGGL(col_hint_kernel, dim3(blocks256(nblk + 1)), dim3(256), 0, s, col_ptr, ncol, nblk, hint);
	// stable sort of (row, position) by row: positions ascend inside a row = (row, column) order
	if (svt_sort_pairs<uint32_t>((const uint32_t *) row_idx, srows, ktmp, pos, perm, ptmp, nnz, key_bits(nrow), w + L.sort, s))
		return -1;
	hipLaunchKernelGGL(row_bounds_kernel, dim3(blocks256(nrow + 1)), dim3(256), 0, s, (const int32_t *) srows, nnz, nrow, out_ptr);
	svt_by_rtype(Rtype, val, out_val, [&](auto *v, auto *o) {
		hipLaunchKernelGGL(transpose_gather_kernel, dim3(blocks256_xcd(nnz)), dim3(256), 0, s, col_ptr, ncol, v, perm, hint, nnz, out_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

// workspace of the bucketed form: [reserve, which starts with t2_head()][t2_body()].  What t() reserves:
// The caller sizes the workspace from (nrow, nnz) alone; the shapes the bucketed form accepts (at least one
// nonzero per column and coarse bucket) have at most ~nnz / 8 + 512 * nnz / nrow table entries and at most
// nrow fine buckets, and never more than 96 MiB are set aside: an operand that needs more takes the key sort.
static size_t t2_reserve(int64_t nrow, int64_t nnz)
{
	const double per_row = nrow > 0 ? (double) nnz / (double) nrow : 0.0;
	const double ntab = (double) nnz / 8.0 + 512.0 * per_row + (double) nrow + 4096.0;
	const double b = 8.25 * ntab + 65536.0;
	const size_t cap = (size_t) 96 << 20;
	return b >= (double) cap ? cap : ((size_t) b + 255) / 256 * 256;
}

// behind the reserve: [columns nnz*4][rows in bucket nnz][values nnz*8][coarse-bucket starts per column ncstart*4] + 512
struct T2Body { size_t col1, rlow1, val1, cstart, total; };
static T2Body t2_body(size_t reserve, size_t nnz, size_t ncstart)
{
	const size_t rlow1 = reserve + t2_a(nnz, 4), val1 = rlow1 + t2_a(nnz, 1), cstart = val1 + t2_a(nnz, 8);
	return T2Body{reserve, rlow1, val1, cstart, cstart + t2_a(ncstart, 4) + 512};
}

size_t transpose_ws_bytes(int64_t nrow, int64_t nnz)
{
	const size_t n = (size_t) (nnz > 0 ? nnz : 1);
	const size_t sorted = transpose_sorted_ws_bytes(nnz);
	// (the coarse-bucket starts per column: (ncoarse + 1) * ncol <= 2 * nnz entries for the shapes accepted)
	const size_t b2 = t2_body(t2_reserve(nrow, nnz), n, 2 * n + 64).total;
	return sorted > b2 ? sorted : b2;
}

// `reserve`: where the body starts (t2_reserve() for t(), the head's own size for the batched form)
static int launch_transpose_bucketed(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
				     int64_t nrow, int64_t ncol, int64_t nnz, const T2Shape &sh, int64_t *out_ptr,
				     int32_t *out_idx, void *out_val, void *ws, size_t reserve, hipStream_t s)
{
	const T2Head H = t2_head(sh);
	const T2Body B = t2_body(reserve, (size_t) nnz, 0);
	const int64_t ntab = H.ntab;
	char *w = (char *) ws;
	int64_t *table = (int64_t *) (w + H.table), *fb_base = (int64_t *) (w + H.fb_base);
	int32_t *col1 = (int32_t *) (w + B.col1);
	uint8_t *rlow1 = (uint8_t *) (w + B.rlow1);
	void *scan_ws = w + H.scan, *val1 = w + B.val1;
	uint32_t *cstart = (uint32_t *) (w + B.cstart);         // [(ncoarse + 1) * ncol]
	HIP_TRY(hipMemsetAsync(table, 0, (size_t) ntab * 8, s));
	const size_t hist_b = (size_t) ((sh.nfb < T1_HIST ? sh.nfb : T1_HIST) + 1) / 2 * 4;
	(void) hipFuncSetAttribute((const void *) transpose_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
				   T1_HIST * 2);
	hipLaunchKernelGGL(transpose_count_kernel, dim3((unsigned) (sh.nslab * ((sh.scol + T1_NT / 64 - 1) / (T1_NT / 64)))), dim3(T1_NT),
			   hist_b, s, col_ptr, row_idx, ncol, sh, (unsigned long long *) table, cstart);
	if (launch_exclusive_scan_i64(table, ntab, scan_ws, s))
		return -1;
	hipLaunchKernelGGL(transpose_fb_base_kernel, dim3((unsigned) ((sh.nslab * sh.ncoarse + 3) / 4)), dim3(256), 0, s,
			   table, sh, nnz, fb_base);
	svt_by_rtype(Rtype, val, out_val, [&](auto *v, auto *o) {
		typedef std::remove_pointer_t<decltype(o)> T;
		hipLaunchKernelGGL(transpose_scatter_kernel<T>, dim3((unsigned) (sh.nslab * sh.ngroups * ((sh.ncoarse + T2_CPW - 1) / T2_CPW))), dim3(T2_NT), 0, s,
				   col_ptr, row_idx, v, nrow, ncol, sh, table, cstart, col1, rlow1, (T *) val1);
		const size_t lds = ((sizeof(SplitLds<T3_NT, T3_ITEMS, 64>) + 15) & ~(size_t) 15) + (size_t) sh.ngroups * 8 +
				   (size_t) ((sh.ngroups + 1 + 3) & ~(int64_t) 3) * 4 + (size_t) T3_STAGE * 4 + (size_t) T3_STAGE * sizeof(T);
		(void) hipFuncSetAttribute((const void *) transpose_finish_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
		hipLaunchKernelGGL(transpose_finish_kernel<T>, dim3((unsigned) (sh.nslab * sh.nfb)), dim3(T3_NT), lds, s, table, sh, nrow, nnz,
				   col1, rlow1, (const T *) val1, fb_base, out_ptr, out_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

// The route of t() below 2^31 nonzeros: 0 the bucketed form (*sh, *reserve filled), 1 t2_shape() refuses the operand,
// 2 the head of its workspace does not fit what t2_reserve() sets aside; 1 and 2 take the key sort.
static int t_route(int64_t nrow, int64_t ncol, int64_t nnz, T2Shape *sh, size_t *reserve)
{
	*reserve = t2_reserve(nrow, nnz);
	// (one matrix: t2_shape() leaves nslab = 1, srow = nrow, scol = ncol)
	if (!t2_shape(nrow, ncol, nnz, sh))
		return 1;
	return t2_head(*sh).total > *reserve ? 2 : 0;
}

int launch_transpose(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
		     int64_t nrow, int64_t ncol, int64_t nnz, int64_t *out_ptr, int32_t *out_idx,
		     void *out_val, void *ws, hipStream_t s)
{
	if (nnz >= ((int64_t) 1 << 31))
		return svt_set_unsupported("svt_dev_transpose: more than 2^31-1 nonzeros");
	if (nnz == 0) {
		HIP_TRY(hipMemsetAsync(out_ptr, 0, (size_t) (nrow + 1) * 8, s));
		return 0;
	}
	T2Shape sh;
	size_t reserve = 0;
	if (t_route(nrow, ncol, nnz, &sh, &reserve) != 0)
		return launch_transpose_sorted(col_ptr, row_idx, val, Rtype, nrow, ncol, nnz, out_ptr, out_idx, out_val, ws, s);
	g_route[R_T_BUCKETED]++;
	return launch_transpose_bucketed(col_ptr, row_idx, val, Rtype, nrow, ncol, nnz, sh, out_ptr, out_idx, out_val, ws, reserve, s);
}

// ---------------------------------------------------------------------------
// t(A) past 2^31 nonzeros: the boxed driver.  The routes above count positions in 32 bits; an SVT's nonzero count is
// unbounded (src/SVT_SparseArray_class.c:200-218).  The operand is cut into BOXES -- runs of consecutive columns, each
// holding at most `box` nonzeros, or a single column (<= nrow < 2^31 entries) -- and every box is transposed by the
// unchanged routes above as an operand of its own, into a box-sized temporary, from which a placement pass copies it to
// its final place:
//   count   one pass over row_idx: the length of every output leaf (a row histogram, privatised in LDS when nrow
//           allows), scanned in place into out_ptr (launch_exclusive_scan_i64); fill[L] = 0 (placed so far).
//   cuts    one search per multiple p of `box` over col_ptr: the column holding position p; boxes end on both sides
//           of it, so every other box lies strictly between two such columns and holds fewer than `box` nonzeros.
//           Columns W = 2^20 apart are cut the same way (a run of empty columns cannot make the box's rebased
//           col_ptr larger than the workspace; t(A) has ncol < 2^31 rows, so at most 2048 such cuts).  The cuts and col_ptr there are read back: one stream sync per call.
//   per box rebase its slice of col_ptr (-col_ptr[c0]); the route (bucketed or key sort) on (nrow x width, nnz_b);
//           placement: one wavefront per output leaf L copies the box's run of L to out_ptr[L] + fill[L], adding c0
//           to every row index (the box-local column), and advances fill[L].
// Why the result is exact: the entries of output leaf L are ordered by their old column.  Boxes are consecutive column
// ranges, processed in order, so every box contributes ONE contiguous run to every output leaf, and the runs come in
// box order = column order; inside a run the route orders them.  Only copies happen: the result is bit for bit the
// unboxed route's (and out_ptr is the same scan of the same counts).
// Workspace: box_layout() -- the route's at max(box, nrow) nonzeros, a box-sized temporary, O(nrow) and O(nnz / box), not O(nnz).
// ---------------------------------------------------------------------------
static std::atomic<int64_t> g_box_nnz{0};
static std::atomic<int64_t> g_boxed_calls{0};

void box_nnz_set(int64_t n) { g_box_nnz.store(n > 0 ? n : 0); }
int64_t box_nnz_get(void) { return g_box_nnz.load(); }
int64_t boxed_calls(int reset) { return reset ? g_boxed_calls.exchange(0) : g_boxed_calls.load(); }

#define BOX_DEFAULT ((int64_t) 1 << 30)
#define BOX_W ((int64_t) 1 << 20)
#define BOX_HIST_NT 1024
#define BOX_HIST_LDS 32768            // rows counted in LDS (128 KB of 32-bit counters); more: memory atomics

static bool box_taken(int64_t nnz, int64_t box_limit)
{
	return box_limit > 0 ? nnz > box_limit : nnz >= ((int64_t) 1 << 31);
}

static int64_t box_size(int64_t box_limit, int64_t dflt)
{
	return box_limit > 0 ? (box_limit < 0x7FFFFFFFLL ? box_limit : 0x7FFFFFFFLL) : dflt;
}

struct BoxLayout {
	int64_t bsz, bmax, W, npts_max;
	size_t pts, fill, scan, bcp, bptr, bidx, bval, route, total;
};

static BoxLayout box_layout(int64_t nrow, int64_t nnz, int64_t box_limit)
{
	BoxLayout L;
	L.bsz = box_size(box_limit, BOX_DEFAULT);
	L.bmax = L.bsz > nrow ? L.bsz : nrow;                   // a box: <= bsz nonzeros, or one column
	if (L.bmax > nnz) L.bmax = nnz > 0 ? nnz : 1;
	L.W = BOX_W;
	// (ncol = nrow of t(A) < 2^31: at most 2^31 / W cuts by width)
	L.npts_max = (nnz + L.bsz - 1) / L.bsz + (((int64_t) 1 << 31) + L.W - 1) / L.W + 1;
	size_t o = 0;
	L.pts = o;   o += t2_a((size_t) L.npts_max * 3, 8);
	L.fill = o;  o += t2_a((size_t) nrow + 1, 8);
	L.scan = o;  o += t2_a(exclusive_scan_ws_bytes(nrow + 1), 1);
	L.bcp = o;   o += t2_a((size_t) L.W + 1, 8);
	L.bptr = o;  o += t2_a((size_t) nrow + 1, 8);
	L.bidx = o;  o += t2_a((size_t) L.bmax, 4);
	L.bval = o;  o += t2_a((size_t) L.bmax, 8);
	L.route = o; o += transpose_ws_bytes(nrow, L.bmax);
	L.total = o + 256;
	return L;
}

// out[r] += entries of row r (out zeroed by the caller); grid-stride over all positions
__global__ void __launch_bounds__(BOX_HIST_NT)
box_row_hist_kernel(const int32_t *__restrict__ row_idx, int64_t nnz, int64_t nrow, int use_lds,
		    unsigned long long *__restrict__ cnt)
{
	extern __shared__ uint32_t h[];
	const bool lds = use_lds != 0;                  // (nrow <= BOX_HIST_LDS counters of dynamic LDS)
	if (lds) {
		for (int64_t r = threadIdx.x; r < nrow; r += BOX_HIST_NT) h[r] = 0;
		__syncthreads();
	}
	const int64_t stride = (int64_t) gridDim.x * BOX_HIST_NT * 4;
	for (int64_t k0 = (int64_t) blockIdx.x * BOX_HIST_NT * 4 + threadIdx.x; k0 < nnz; k0 += stride) {
		int32_t r[4];
#pragma unroll
		for (int u = 0; u < 4; u++) r[u] = k0 + u * BOX_HIST_NT < nnz ? row_idx[k0 + u * BOX_HIST_NT] : -1;
#pragma unroll
		for (int u = 0; u < 4; u++) {
			if (r[u] < 0) continue;
			if (lds) atomicAdd(&h[r[u]], 1u);
			else atomicAdd(&cnt[r[u]], 1ull);
		}
	}
	if (lds) {
		__syncthreads();
		for (int64_t r = threadIdx.x; r < nrow; r += BOX_HIST_NT)
			if (h[r]) atomicAdd(&cnt[r], (unsigned long long) h[r]);
	}
}

// Cut point i: i < nk -- the column holding position (i + 1) * box (last c with col_ptr[c] <= p); else the column
// (i - nk + 1) * W.  pts[3 i ..] = (c, col_ptr[c], col_ptr[c + 1]).
__global__ void box_cut_kernel(const int64_t *__restrict__ col_ptr, int64_t ncol, int64_t nk, int64_t box,
			       int64_t W, int64_t npts, int64_t *__restrict__ pts)
{
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= npts) return;
	int64_t c;
	if (i < nk) {
		const int64_t p = (i + 1) * box;
		int64_t lo = 0, hi = ncol - 1;
		while (lo < hi) {
			const int64_t mid = (lo + hi + 1) >> 1;
			if (col_ptr[mid] <= p) lo = mid; else hi = mid - 1;
		}
		c = lo;
	} else {
		c = (i - nk + 1) * W;
	}
	pts[3 * i] = c;
	pts[3 * i + 1] = col_ptr[c];
	pts[3 * i + 2] = col_ptr[c + 1];
}

__global__ void box_rebase_kernel(const int64_t *__restrict__ col_ptr, int64_t c0, int64_t w, int64_t base,
				  int64_t *__restrict__ bcp)
{
	const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i <= w) bcp[i] = col_ptr[c0 + i] - base;
}

// One wavefront per output leaf: the box's run of leaf L goes to out_ptr[L] + fill[L], its row indices (box-local
// columns) shifted by the box's first column.  Coalesced: consecutive lanes on consecutive entries of one run.
template <typename T>
__global__ void __launch_bounds__(256)
box_place_kernel(const int64_t *__restrict__ bptr, const int32_t *__restrict__ bidx, const T *__restrict__ bval,
		 int64_t nleaf, int32_t add, const int64_t *__restrict__ out_ptr, int64_t *__restrict__ fill,
		 int32_t *__restrict__ out_idx, T *__restrict__ out_val)
{
	const int lane = threadIdx.x & 63;
	const int64_t L = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
	if (L >= nleaf) return;
	const int64_t b = bptr[L], n = bptr[L + 1] - b;
	if (n == 0) return;
	const int64_t dst = out_ptr[L] + fill[L];
	for (int64_t k0 = 0; k0 < n; k0 += 256) {
		int32_t r[4];
		T v[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int64_t k = k0 + u * 64 + lane;
			if (k < n) { r[u] = bidx[b + k]; v[u] = bval[b + k]; }
		}
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int64_t k = k0 + u * 64 + lane;
			if (k < n) { out_idx[dst + k] = r[u] + add; out_val[dst + k] = v[u]; }
		}
	}
	if (lane == 0) fill[L] += n;
}

static void launch_box_place(int Rtype, const int64_t *bptr, const int32_t *bidx, const void *bval, int64_t nleaf,
			     int64_t first, const int64_t *out_ptr, int64_t *fill, int32_t *out_idx, void *out_val, hipStream_t s)
{
	svt_by_rtype(Rtype, bval, out_val, [&](auto *v, auto *o) {
		hipLaunchKernelGGL(box_place_kernel, dim3((unsigned) ((nleaf + 3) / 4)), dim3(256), 0, s, bptr, bidx, v, nleaf,
				   (int32_t) first, out_ptr, fill, out_idx, o);
	});
}

// The cuts, shared by the two boxed drivers, over a pointer array ptr[0 .. n] with ptr[n] = nnz (col_ptr for t(); for
// aperm() the nonzeros per index of the axis that becomes the rows): box_cut_kernel, its table copied to the host,
// whatever else the driver queues with queue_more() (work that does not depend on the cuts), then the one stream
// synchronisation of a boxed call; *bd = the boxes' boundaries (index, ptr there), ascending, each once.
typedef std::vector<std::pair<int64_t, int64_t>> BoxBounds;
template <class F>
static int box_boundaries(const char *who, const int64_t *ptr, int64_t n, int64_t nnz, int64_t bsz, int64_t W,
			  int64_t npts_max, int64_t *pts, hipStream_t s, BoxBounds *bd, F queue_more)
{
	const int64_t nk = (nnz - 1) / bsz, nw = (n - 1) / W, npts = nk + nw;
	if (npts > npts_max)
		return svt_set_error("%s: internal error (box cuts)", who);
	std::vector<int64_t> hp((size_t) npts * 3 + 1);
	if (npts > 0) {
		hipLaunchKernelGGL(box_cut_kernel, dim3((unsigned) ((npts + 255) / 256)), dim3(256), 0, s, ptr, n, nk, bsz, W, npts, pts);
		HIP_TRY(hipGetLastError());
		HIP_TRY(hipMemcpyAsync(hp.data(), pts, (size_t) npts * 24, hipMemcpyDeviceToHost, s));
	}
	if (queue_more())
		return -1;
	HIP_TRY(hipStreamSynchronize(s));
	bd->reserve((size_t) npts * 2 + 2);
	bd->push_back({0, 0});
	bd->push_back({n, nnz});
	for (int64_t i = 0; i < npts; i++) {
		bd->push_back({hp[3 * i], hp[3 * i + 1]});
		bd->push_back({hp[3 * i] + 1, hp[3 * i + 2]});
	}
	std::sort(bd->begin(), bd->end());
	bd->erase(std::unique(bd->begin(), bd->end()), bd->end());
	return 0;
}

size_t transpose_ws_bytes_box(int64_t nrow, int64_t nnz, int64_t box_limit)
{
	if (!box_taken(nnz, box_limit))
		return transpose_ws_bytes(nrow, nnz);
	return box_layout(nrow, nnz, box_limit).total;
}

static int launch_transpose_boxed(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
				  int64_t nrow, int64_t ncol, int64_t nnz, int64_t *out_ptr, int32_t *out_idx,
				  void *out_val, void *ws, int64_t box_limit, hipStream_t s)
{
	if (ncol > 0x7FFFFFFFLL)
		return svt_set_error("svt_dev_transpose: more than 2^31-1 columns");
	const BoxLayout Ly = box_layout(nrow, nnz, box_limit);
	char *w = (char *) ws;
	int64_t *pts = (int64_t *) (w + Ly.pts), *fill = (int64_t *) (w + Ly.fill);
	int64_t *bcp = (int64_t *) (w + Ly.bcp), *bptr = (int64_t *) (w + Ly.bptr);
	int32_t *bidx = (int32_t *) (w + Ly.bidx);
	void *bval = w + Ly.bval, *rws = w + Ly.route;
	const size_t esz = Rtype == SVT_REALSXP ? 8 : 4;
	// lengths of the output leaves -> out_ptr
	HIP_TRY(hipMemsetAsync(out_ptr, 0, (size_t) (nrow + 1) * 8, s));
	HIP_TRY(hipMemsetAsync(fill, 0, (size_t) nrow * 8, s));
	// (rows counted in LDS where the 128 KB of counters can be had, else memory atomics; the kernel decides by nrow)
	bool lds = nrow <= BOX_HIST_LDS;
	if (lds && hipFuncSetAttribute((const void *) box_row_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
				       BOX_HIST_LDS * 4) != hipSuccess) {
		(void) hipGetLastError();
		lds = false;
	}
	int64_t nbh = (nnz + BOX_HIST_NT * 4 - 1) / (BOX_HIST_NT * 4);
	if (nbh > 1024) nbh = 1024;                         // (a workgroup counts < 2^32 entries per row up to 4e12 nonzeros)
	hipLaunchKernelGGL(box_row_hist_kernel, dim3((unsigned) nbh), dim3(BOX_HIST_NT), lds ? (size_t) nrow * 4 : 0, s,
			   row_idx, nnz, nrow, lds ? 1 : 0, (unsigned long long *) out_ptr);
	HIP_TRY(hipGetLastError());
	if (launch_exclusive_scan_i64(out_ptr, nrow + 1, w + Ly.scan, s))
		return -1;
	// the cuts, read back once
	BoxBounds bd;                                       // (column, col_ptr there)
	if (box_boundaries("svt_dev_transpose", col_ptr, ncol, nnz, Ly.bsz, Ly.W, Ly.npts_max, pts, s, &bd, [] { return 0; }))
		return -1;
	for (size_t b = 0; b + 1 < bd.size(); b++) {
		const int64_t c0 = bd[b].first, c1 = bd[b + 1].first, p0 = bd[b].second, nb = bd[b + 1].second - p0;
		if (nb == 0)
			continue;
		if (nb > Ly.bmax || c1 - c0 > Ly.W)
			return svt_set_error("svt_dev_transpose: internal error (box of %lld nonzeros, %lld columns)",
					     (long long) nb, (long long) (c1 - c0));
		hipLaunchKernelGGL(box_rebase_kernel, dim3((unsigned) ((c1 - c0 + 1 + 255) / 256)), dim3(256), 0, s,
				   col_ptr, c0, c1 - c0, p0, bcp);
		if (launch_transpose(bcp, row_idx + p0, (const char *) val + (size_t) p0 * esz, Rtype, nrow, c1 - c0, nb,
				     bptr, bidx, bval, rws, s))
			return -1;
		launch_box_place(Rtype, bptr, bidx, bval, nrow, c0, out_ptr, fill, out_idx, out_val, s);
		HIP_TRY(hipGetLastError());
	}
	g_boxed_calls++;
	return 0;
}

// t(A) with the box limit of the call (read once by the caller: box_nnz_get()): the boxed driver past it, else the
// routes above exactly as they are.
int launch_transpose_box(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
			 int64_t nrow, int64_t ncol, int64_t nnz, int64_t *out_ptr, int32_t *out_idx,
			 void *out_val, void *ws, int64_t box_limit, hipStream_t s)
{
	if (!box_taken(nnz, box_limit))
		return launch_transpose(col_ptr, row_idx, val, Rtype, nrow, ncol, nnz, out_ptr, out_idx, out_val, ws, s);
	return launch_transpose_boxed(col_ptr, row_idx, val, Rtype, nrow, ncol, nnz, out_ptr, out_idx, out_val, ws,
				      box_limit, s);
}

// ---------------------------------------------------------------------------
// N-d aperm (C_aperm_SVT, src/SparseArray_aperm.c:148-930).  The device layout knows leaves only, so the caller passes
// the array's dims.  The reference distinguishes leaf-preserving permutations (perm[1] == 1: pointer shuffle, :949-957)
// from those that shatter leaves (counting sort, :892-929).  Here: one function per route, each next to the function
// that lays out its workspace, tried in the order of launch_aperm_n(); the last resort gives every nonzero the 64-bit
// key  new_leaf * new_dim0 + new_row  (its linear index in the permuted array), sorts and gathers.
// ---------------------------------------------------------------------------
struct ApermDims {
	int ndim;
	int64_t dim[8];      // old dims
	int perm[8];         // 0-based: new axis a takes old axis perm[a]
	int64_t mul[8];      // multiplier of old axis a in the new linear index
};

__global__ void aperm_key_kernel(const int64_t *__restrict__ col_ptr,
				 const int32_t *__restrict__ row_idx, int64_t ncol, int64_t nnz,
				 ApermDims d, unsigned long long *__restrict__ keys,
				 uint32_t *__restrict__ pos)
{
	const int64_t k = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= nnz) return;
	int64_t lo = 0, hi = ncol;                  // leaf of position k
	while (lo < hi) {
		const int64_t mid = (lo + hi + 1) >> 1;
		if (col_ptr[mid] <= k) lo = mid; else hi = mid - 1;
	}
	unsigned long long key = (unsigned long long) row_idx[k] * (unsigned long long) d.mul[0];
	int64_t rest = lo;
	for (int a = 1; a < d.ndim; a++) {
		const int64_t ia = rest % d.dim[a];
		rest /= d.dim[a];
		key += (unsigned long long) ia * (unsigned long long) d.mul[a];
	}
	keys[k] = key;
	pos[k] = (uint32_t) k;
}

template <typename T>
__global__ void aperm_gather_kernel(const unsigned long long *__restrict__ skeys,
				    const uint32_t *__restrict__ perm, const T *__restrict__ val,
				    int64_t nnz, int64_t dim0, int32_t *__restrict__ out_idx,
				    T *__restrict__ out_val)
{
	const int64_t i = xcd_chunk((nnz + blockDim.x - 1) / blockDim.x) * blockDim.x + threadIdx.x;
	if (i >= nnz) return;
	out_idx[i] = (int32_t) (skeys[i] % (unsigned long long) dim0);
	out_val[i] = val[perm[i]];
}

// ---- leaf-preserving permutations (perm[1] == 1 in R's numbering): the leaves stay what they are and
// only change places -- the reference shuffles pointers (src/SparseArray_aperm.c:949-957); here: the
// length of every new leaf from the old col_ptr, a scan, one streaming copy.  No keys, no sort.
struct LeafMap {
	int ndim;
	int64_t new_dim[8];      // extents of the new axes 1 .. ndim-1
	int64_t old_stride[8];   // leaf stride, in the OLD layout, of the old axis that new axis a takes
};

__device__ inline int64_t old_leaf_of(const LeafMap &m, int64_t jn)
{
	int64_t j = 0;
	for (int a = 1; a < m.ndim; a++) {
		const int64_t ia = jn % m.new_dim[a];
		jn /= m.new_dim[a];
		j += ia * m.old_stride[a];
	}
	return j;
}

__global__ void aperm_leaf_count_kernel(const int64_t *__restrict__ col_ptr, int64_t nleaves, LeafMap m,
					int64_t *__restrict__ cnt)
{
	const int64_t jn = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (jn > nleaves) return;
	if (jn == nleaves) { cnt[jn] = 0; return; }
	const int64_t j = old_leaf_of(m, jn);
	cnt[jn] = col_ptr[j + 1] - col_ptr[j];
}

// One wavefront per four new leaves, their bounds and their runs in flight together (a leaf at a time is
// a chain of three memory latencies per ~100 nonzeros: 1.1 ms for the 3 GB of BASELINE config 5).
#define APERM_LU 4
template <typename T>
__global__ void __launch_bounds__(256)
aperm_leaf_copy_kernel(const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ row_idx,
		       const T *__restrict__ val, int64_t nleaves, LeafMap m,
		       const int64_t *__restrict__ out_ptr, int32_t *__restrict__ out_idx, T *__restrict__ out_val)
{
	const int lane = threadIdx.x & 63;
	const int64_t j0 = ((int64_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * APERM_LU;
	if (j0 >= nleaves) return;
	int64_t src[APERM_LU], dst[APERM_LU], n[APERM_LU];
#pragma unroll
	for (int u = 0; u < APERM_LU; u++) {
		const int64_t jn = j0 + u;
		src[u] = dst[u] = n[u] = 0;
		if (jn < nleaves) {
			src[u] = col_ptr[old_leaf_of(m, jn)];
			dst[u] = out_ptr[jn];
			n[u] = out_ptr[jn + 1] - dst[u];
		}
	}
	bool more = true;
	for (int64_t k = lane; more; k += 64) {
		int32_t r[APERM_LU];
		T v[APERM_LU];
#pragma unroll
		for (int u = 0; u < APERM_LU; u++)
			if (k < n[u]) { r[u] = row_idx[src[u] + k]; v[u] = val[src[u] + k]; }
		more = false;
#pragma unroll
		for (int u = 0; u < APERM_LU; u++)
			if (k < n[u]) {
				out_idx[dst[u] + k] = r[u];
				out_val[dst[u] + k] = v[u];
				more |= k + 64 < n[u];
			}
		more = __any(more);
	}
}

// count, scan, copy: whole leaves to their new places (scan_ws: exclusive_scan_ws_bytes(nleaves + 1))
static int launch_leaf_move(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype, int64_t nleaves,
			    const LeafMap &lm, int64_t *out_ptr, int32_t *out_idx, void *out_val, void *scan_ws, hipStream_t s)
{
	hipLaunchKernelGGL(aperm_leaf_count_kernel, dim3((unsigned) ((nleaves + 1 + 255) / 256)), dim3(256), 0, s, col_ptr, nleaves, lm, out_ptr);
	if (launch_exclusive_scan_i64(out_ptr, nleaves + 1, scan_ws, s))
		return -1;
	const unsigned nbc = (unsigned) ((nleaves + 4 * APERM_LU - 1) / (4 * APERM_LU));
	svt_by_rtype(Rtype, val, out_val, [&](auto *v, auto *o) {
		hipLaunchKernelGGL(aperm_leaf_copy_kernel, dim3(nbc), dim3(256), 0, s, col_ptr, row_idx, v, nleaves, lm, out_ptr, out_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

// One aperm() call as its routes see it.  A route returns 0 (done), -1 (error), or one of the two below, on which the
// dispatcher (launch_aperm_n) goes on to the next route.
struct ApermCall {
	const int64_t *col_ptr; const int32_t *row_idx; const void *val; int Rtype;
	int64_t ncol, nnz; const int64_t *dim; int ndim; const int *perm;
	int64_t *out_ptr; int32_t *out_idx; void *out_val; void *ws; hipStream_t s;
};
enum { APERM_NA = 1, APERM_REFUSED = 2 };              // not this route's shape / its shape, refused on seeing the data
static int launch_aperm_n(const ApermCall &c, int nested);

// workspace of the leaf-preserving form: the scratch of a scan over the new leaves' counts (0: too many leaves for it)
static size_t aperm_leaf_scan_bytes(const int64_t *dim, int ndim)
{
	const double nl = extent_prod(dim, 1, ndim);
	return nl < LEAVES_MAX ? exclusive_scan_ws_bytes((int64_t) nl + 1) : 0;
}

static int aperm_leaf_preserving(const ApermCall &c, int64_t new_nleaves)
{
	LeafMap lm;
	lm.ndim = c.ndim;
	int64_t os[8], st = 1;
	for (int a = 1; a < c.ndim; a++) { os[a] = st; st *= c.dim[a]; }      // leaf strides of the old axes
	for (int a = 1; a < c.ndim; a++) { lm.new_dim[a] = c.dim[c.perm[a]]; lm.old_stride[a] = os[c.perm[a]]; }
	g_route[R_LEAF_PRESERVING]++;
	// counts into out_ptr, exclusive scan in place
	return launch_leaf_move(c.col_ptr, c.row_idx, c.val, c.Rtype, new_nleaves, lm, c.out_ptr, c.out_idx, c.out_val, c.ws, c.s);
}

// ---- leaf-shattering permutations, 32-bit keys.  A stable sort by the NEW LEAF index alone is enough:
// two nonzeros of one new leaf differ only in the coordinate that becomes the new row, and the input order
// (old leaves in order, offsets ascending) already ascends in that coordinate for fixed other ones.  So the
// key is ceil(log2(new leaves)) bits instead of ceil(log2(prod(dim))): 29 instead of 35 at BASELINE config 5,
// 32-bit keys, one radix pass less, and the new row travels beside the sort instead of through it.
__global__ void aperm_key32_kernel(const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ row_idx,
				   const uint32_t *__restrict__ hint, int64_t ncol, int64_t nnz, ApermDims d,
				   uint32_t *__restrict__ keys, uint32_t *__restrict__ pos, int32_t *__restrict__ newrow)
{
	const int64_t k = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= nnz) return;
	int64_t lo = hint[k >> HINT_SHIFT], hi = hint[(k >> HINT_SHIFT) + 1];      // old leaf of position k
	if (hi > ncol - 1) hi = ncol - 1;
	while (lo < hi) {
		const int64_t mid = (lo + hi + 1) >> 1;
		if (col_ptr[mid] <= k) lo = mid; else hi = mid - 1;
	}
	// d.mul[a] = multiplier of old axis a in the new linear index; new leaf = (linear - new row) / new dim0
	const int64_t r = row_idx[k];
	unsigned long long lin = (unsigned long long) r * (unsigned long long) d.mul[0];
	int64_t nr = d.perm[0] == 0 ? r : 0, rest = lo;
	for (int a = 1; a < d.ndim; a++) {
		const int64_t ia = rest % d.dim[a];
		rest /= d.dim[a];
		lin += (unsigned long long) ia * (unsigned long long) d.mul[a];
		if (d.perm[0] == a) nr = ia;
	}
	keys[k] = (uint32_t) ((lin - (unsigned long long) nr) / (unsigned long long) d.dim[d.perm[0]]);
	pos[k] = (uint32_t) k;
	newrow[k] = (int32_t) nr;
}

// out_ptr[j] = first sorted position whose leaf is >= j, j = 0 .. nleaves.  Most new leaves are empty when leaves
// shatter, so the work is WRITING the pointers (20 GB for the 2.56e9 leaves of aperm(x, c(3,2,4,1)) of a 2e4 x 2e3 x
// 10 x 64 array), not finding them.  Rounds 1-5: one binary search over the sorted keys per new leaf on the 64-bit
// route (48 ms there).  Round 6, first form: every sorted element fills the leaves between its predecessor's and its
// own (9.6 ms: a lane's run of leaves is contiguous, a wavefront's store instruction is not).  Now: a workgroup takes
// 256 consecutive sorted elements (plus the sentinel "element" nnz with leaf nleaves), keeps their leaves in LDS and
// fills the range of leaves they cover with consecutive lanes on consecutive leaves -- coalesced stores --, each lane
// finding its leaf's element by a binary search in LDS.  K = uint32_t: the key is the leaf; unsigned long long:
// leaf * dim0 + row.
#define PTRFILL_NT 256
template <typename K>
__global__ void __launch_bounds__(PTRFILL_NT)
aperm_ptr_fill_kernel(const K *__restrict__ skeys, int64_t nnz, int64_t nleaves, unsigned long long dim0,
		      int64_t *__restrict__ out_ptr)
{
	__shared__ int64_t s_leaf[PTRFILL_NT];
	__shared__ int64_t s_first;
	const int tid = threadIdx.x;
	const int64_t i0 = (int64_t) blockIdx.x * PTRFILL_NT, i = i0 + tid;
	// element i covers the leaves (leaf(i - 1), leaf(i)]; past the sentinel: nothing (a leaf no search will stop at)
	s_leaf[tid] = i < nnz ? (int64_t) ((unsigned long long) skeys[i] / dim0) : (i == nnz ? nleaves : nleaves + 1);
	if (tid == 0)
		s_first = i0 == 0 ? 0 : (int64_t) ((unsigned long long) skeys[i0 - 1] / dim0) + 1;
	__syncthreads();
	const int nvalid = (int) (nnz + 1 - i0 < PTRFILL_NT ? nnz + 1 - i0 : PTRFILL_NT);
	const int64_t first = s_first, last = s_leaf[nvalid - 1];
	for (int64_t j = first + tid; j <= last; j += PTRFILL_NT) {
		int lo = 0, hi = nvalid - 1;                    // smallest t with s_leaf[t] >= j (exists: s_leaf[nvalid - 1] = last >= j)
		while (lo < hi) {
			const int mid = (lo + hi) >> 1;
			if (s_leaf[mid] < j) lo = mid + 1; else hi = mid;
		}
		out_ptr[j] = i0 + lo;
	}
}

template <typename T>
__global__ void aperm_gather32_kernel(const uint32_t *__restrict__ spos, const int32_t *__restrict__ newrow,
				      const T *__restrict__ val, int64_t nnz, int32_t *__restrict__ out_idx,
				      T *__restrict__ out_val)
{
	const int64_t i = xcd_chunk((nnz + blockDim.x - 1) / blockDim.x) * blockDim.x + threadIdx.x;
	if (i >= nnz) return;
	const uint32_t k = spos[i];
	out_idx[i] = newrow[k];
	out_val[i] = val[k];
}

static ApermDims aperm_dims(const ApermCall &c)
{
	ApermDims d;
	d.ndim = c.ndim;
	int64_t m = 1;                                      // multiplier of old axis perm[a] = product of the new dims below new axis a
	for (int a = 0; a < c.ndim; a++) {
		d.dim[a] = c.dim[a];
		d.perm[a] = c.perm[a];
		d.mul[c.perm[a]] = m;
		m *= c.dim[c.perm[a]];
	}
	return d;
}

// [keys][sorted keys][pos][sorted pos][new row][second buffers of the sort's passes, twice], nnz*4 each, [leaf hints]
// [the sort's scratch] + 256.  Depends on the nonzero count alone.
struct Sort32Layout { size_t keys, skeys, pos, spos, newrow, ktmp, ptmp, hint, sort, total; };
static Sort32Layout aperm_sort32_layout(int64_t nnz)
{
	const size_t a4 = t2_a((size_t) (nnz > 0 ? nnz : 1), 4), sort = 7 * a4 + hint_bytes(nnz);
	return Sort32Layout{0, a4, 2 * a4, 3 * a4, 4 * a4, 5 * a4, 6 * a4, 7 * a4, sort, sort + svt_sort_ws_bytes(nnz) + 256};
}
static size_t aperm_key_sort_bytes(int64_t nnz) { return aperm_sort32_layout(nnz).total; }

static int aperm_sort32(const ApermCall &c, int64_t new_nleaves)
{
	const Sort32Layout L = aperm_sort32_layout(c.nnz);
	char *w = (char *) c.ws;
	uint32_t *keys = (uint32_t *) (w + L.keys), *skeys = (uint32_t *) (w + L.skeys), *pos = (uint32_t *) (w + L.pos);
	uint32_t *spos = (uint32_t *) (w + L.spos), *ktmp = (uint32_t *) (w + L.ktmp), *ptmp = (uint32_t *) (w + L.ptmp);
	uint32_t *hint = (uint32_t *) (w + L.hint);
	int32_t *newrow = (int32_t *) (w + L.newrow);
	int bits = 1;
	while (bits < 32 && ((int64_t) 1 << bits) < new_nleaves) bits++;
	const int64_t nblk = (c.nnz >> HINT_SHIFT) + 1;
	g_route[R_SORT32]++;
	hipLaunchKernelGGL(col_hint_kernel, dim3(blocks256(nblk + 1)), dim3(256), 0, c.s, c.col_ptr, c.ncol, nblk, hint);
	hipLaunchKernelGGL(aperm_key32_kernel, dim3(blocks256(c.nnz)), dim3(256), 0, c.s, c.col_ptr, c.row_idx, hint, c.ncol, c.nnz,
			   aperm_dims(c), keys, pos, newrow);
	if (svt_sort_pairs<uint32_t>(keys, skeys, ktmp, pos, spos, ptmp, c.nnz, bits, w + L.sort, c.s))
		return -1;
	hipLaunchKernelGGL(aperm_ptr_fill_kernel, dim3((unsigned) ((c.nnz + 1 + PTRFILL_NT - 1) / PTRFILL_NT)), dim3(PTRFILL_NT), 0, c.s,
			   skeys, c.nnz, new_nleaves, 1ULL, c.out_ptr);
	svt_by_rtype(c.Rtype, c.val, c.out_val, [&](auto *v, auto *o) {
		hipLaunchKernelGGL(aperm_gather32_kernel, dim3(blocks256_xcd(c.nnz)), dim3(256), 0, c.s, spos, newrow, v, c.nnz, c.out_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

// ---- 64-bit keys, the new linear index (aperm_key_kernel): results of 2^31 - 1 leaves or more.
// [keys nnz*8][sorted keys nnz*8][pos nnz*4][sorted pos nnz*4][second buffers of the sort's passes nnz*8, nnz*4]
// [the sort's scratch] + 256.  Depends on the nonzero count alone.
struct Sort64Layout { size_t keys, skeys, pos, spos, ktmp, ptmp, sort, total; };
static Sort64Layout aperm_sort64_layout(int64_t nnz)
{
	const size_t n = (size_t) (nnz > 0 ? nnz : 1), a8 = t2_a(n, 8), a4 = t2_a(n, 4), sort = 3 * a8 + 3 * a4;
	return Sort64Layout{0, a8, 2 * a8, 2 * a8 + a4, 2 * a8 + 2 * a4, 3 * a8 + 2 * a4, sort, sort + svt_sort_ws_bytes(nnz) + 256};
}

static int aperm_sort64(const ApermCall &c, int64_t new_nleaves)
{
	typedef unsigned long long u64;
	const Sort64Layout L = aperm_sort64_layout(c.nnz);
	char *w = (char *) c.ws;
	u64 *keys = (u64 *) (w + L.keys), *skeys = (u64 *) (w + L.skeys), *ktmp = (u64 *) (w + L.ktmp);
	uint32_t *pos = (uint32_t *) (w + L.pos), *spos = (uint32_t *) (w + L.spos), *ptmp = (uint32_t *) (w + L.ptmp);
	const int64_t new_dim0 = c.dim[c.perm[0]];
	const double tot = extent_prod(c.dim, 0, c.ndim);
	int bits = 1;                                       // of the new linear index
	while (bits < 64 && ldexp(1.0, bits) < tot) bits++;
	g_route[R_SORT64]++;
	hipLaunchKernelGGL(aperm_key_kernel, dim3(blocks256(c.nnz)), dim3(256), 0, c.s, c.col_ptr, c.row_idx, c.ncol, c.nnz, aperm_dims(c),
			   keys, pos);
	if (svt_sort_pairs<u64>(keys, skeys, ktmp, pos, spos, ptmp, c.nnz, bits, w + L.sort, c.s))
		return -1;
	hipLaunchKernelGGL(aperm_ptr_fill_kernel, dim3((unsigned) ((c.nnz + 1 + PTRFILL_NT - 1) / PTRFILL_NT)), dim3(PTRFILL_NT), 0, c.s,
			   skeys, c.nnz, new_nleaves, (u64) (new_dim0 > 0 ? new_dim0 : 1), c.out_ptr);
	svt_by_rtype(c.Rtype, c.val, c.out_val, [&](auto *v, auto *o) {
		hipLaunchKernelGGL(aperm_gather_kernel, dim3(blocks256_xcd(c.nnz)), dim3(256), 0, c.s, skeys, spos, v, c.nnz, new_dim0, c.out_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

// ---- slab form: the new leading axis is an old outer axis q of small extent, the old rows become new
// axis 1 (aperm(x, c(3, 1, 2)) of a 2e4 x 2e4 x 64 array).  For every index of the remaining axes (a slab)
// the sub-array is a d0 x dq matrix held in dq whole old leaves, to be transposed into d0 new leaves of at
// most dq entries each, which follow one another in the output.  One workgroup per slab: the slab's
// nonzeros (a few thousand) are sorted by old row in LDS -- a stable block radix sort on the row alone; the
// input order, leaf after leaf, already ascends in the index that becomes the new row -- and leave as one
// coalesced run; the leaf pointers of the slab's d0 new leaves are filled from the sorted rows.  Traffic:
// the nonzeros once in, once out, and the new leaf pointers (most new leaves are empty: 3.2 GB of
// pointers for 1.5 GB of nonzeros at BASELINE config 5).  7.8 ms through the global key sort.
// ---------------------------------------------------------------------------
#define SLAB_NT 512
#define SLAB_ITEMS 16
#define SLAB_CAP (SLAB_NT * SLAB_ITEMS)
struct SlabMap {
	int nother;              // axes besides old 0 and old q
	int64_t new_ext[8];      // their extents, in the order of the new axes 2 .. ndim-1
	int64_t old_stride[8];   // their leaf strides in the OLD layout
};

__device__ inline int64_t slab_base_leaf(const SlabMap &m, int64_t g)
{
	int64_t j = 0;
	for (int t = 0; t < m.nother; t++) {
		const int64_t it = g % m.new_ext[t];
		g /= m.new_ext[t];
		j += it * m.old_stride[t];
	}
	return j;
}

// cnt[g] = nonzeros of slab g (cnt[nslab] = 0), *maxcnt = the largest
__global__ void aperm_slab_count_kernel(const int64_t *__restrict__ col_ptr, SlabMap m, int64_t nslab,
					int64_t dq, int64_t osq, int64_t *__restrict__ cnt,
					unsigned long long *__restrict__ maxcnt)
{
	const int64_t g = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (g > nslab) return;
	if (g == nslab) { cnt[g] = 0; return; }
	const int64_t j0 = slab_base_leaf(m, g);
	int64_t n = 0;
	for (int64_t k = 0; k < dq; k++) {
		const int64_t j = j0 + k * osq;
		n += col_ptr[j + 1] - col_ptr[j];
	}
	cnt[g] = n;
	atomicMax(maxcnt, (unsigned long long) n);
}

template <typename T>
__global__ void __launch_bounds__(SLAB_NT)
aperm_slab_kernel(const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ row_idx,
		  const T *__restrict__ val, SlabMap m, int64_t nslab, int64_t d0, int dq, int64_t osq,
		  int bits, int64_t nnz, const int64_t *__restrict__ slab_base, int64_t *__restrict__ out_ptr,
		  int32_t *__restrict__ out_idx, T *__restrict__ out_val)
{
	typedef rocprim::block_radix_sort<uint32_t, SLAB_NT, SLAB_ITEMS, uint32_t, 1, 1, 4> Sort;        // (4-bit digits; 5-bit ones, three passes over 15 row bits, need twice the LDS: 3.15 against 2.9 ms)
	__shared__ typename Sort::storage_type sort_tmp;
	__shared__ int32_t off[1025];                   // first slab-local index of every old leaf
	__shared__ int64_t lbeg[1024];                  // its first position in the old arrays
	extern __shared__ uint32_t skey[];              // SLAB_CAP sorted rows
	const int tid = threadIdx.x;
	const int64_t g = blockIdx.x;
	const int64_t sb = slab_base[g];
	const int n = (int) (slab_base[g + 1] - sb);
	const int64_t j0 = slab_base_leaf(m, g);
	for (int k = tid; k < dq; k += SLAB_NT) {
		const int64_t j = j0 + (int64_t) k * osq;
		lbeg[k] = col_ptr[j];
		off[k + 1] = (int32_t) (col_ptr[j + 1] - col_ptr[j]);
	}
	if (tid == 0) off[0] = 0;
	__syncthreads();
	if (tid == 0)                                   // (dq <= 1024 additions; the leaves are few)
		for (int k = 1; k <= dq; k++) off[k] += off[k - 1];
	__syncthreads();
	auto leaf_of = [&](const int e) {               // last k with off[k] <= e
		int lo = 0, hi = dq - 1;
		while (lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if (off[mid] <= e) lo = mid; else hi = mid - 1;
		}
		return lo;
	};
	uint32_t key[SLAB_ITEMS], pay[SLAB_ITEMS];
	// padding items sort behind every row: the all-ones value of `bits` bits unless that is a row itself
	const bool spare = d0 < ((int64_t) 1 << bits);
	const uint32_t pad = spare ? (1u << bits) - 1u : 1u << bits;
	const int sort_bits = spare ? bits : bits + 1;
#pragma unroll
	for (int u = 0; u < SLAB_ITEMS; u++) {
		const int e = tid * SLAB_ITEMS + u;             // blocked: the input order is the tie-break
		pay[u] = (uint32_t) e;
		if (e < n) {
			const int k = leaf_of(e);
			pay[u] |= (uint32_t) k << 13;               // (e < 8192, k < 1024: the leaf rides along)
			key[u] = (uint32_t) row_idx[lbeg[k] + (e - off[k])];
		} else {
			key[u] = pad;                               // past every row
		}
	}
	Sort().sort_to_striped(key, pay, sort_tmp, 0u, (unsigned) sort_bits);
#pragma unroll
	for (int u = 0; u < SLAB_ITEMS; u++) skey[u * SLAB_NT + tid] = key[u];
	__syncthreads();
	const int64_t lp0 = g * d0;                     // first new leaf of the slab
#pragma unroll
	for (int u = 0; u < SLAB_ITEMS; u++) {
		const int sidx = u * SLAB_NT + tid;             // striped: consecutive lanes, consecutive outputs
		if (sidx >= n) continue;
		const int e = (int) (pay[u] & 8191u), k = (int) (pay[u] >> 13);
		out_idx[sb + sidx] = k;
		out_val[sb + sidx] = val[lbeg[k] + (e - off[k])];
		// leaf pointers: every new leaf from the previous entry's row (exclusive) up to this one's starts here
		const int64_t i = key[u], prev = sidx > 0 ? (int64_t) skey[sidx - 1] : -1;
		for (int64_t ii = prev + 1; ii <= i; ii++) out_ptr[lp0 + ii] = sb + sidx;
	}
	const int64_t last = n > 0 ? (int64_t) skey[n - 1] : -1;
	for (int64_t ii = last + 1 + tid; ii < d0; ii += SLAB_NT) out_ptr[lp0 + ii] = sb + n;
	if (g == nslab - 1 && tid == 0) out_ptr[nslab * d0] = nnz;
}

// Head of the slab form's workspace: [nonzeros per slab (nslab + 2) * 8, scanned in place][the largest: 8 bytes of 256][scan scratch]
struct SlabHead { size_t cnt, maxcnt, scan, total; };
static SlabHead aperm_slab_head(int64_t nslab)
{
	const size_t maxcnt = t2_a((size_t) (nslab + 2), 8);
	return SlabHead{0, maxcnt, maxcnt + 256, maxcnt + 256 + exclusive_scan_ws_bytes(nslab + 1)};
}

// new axis 0 = an old outer axis of <= 1024 entries, new axis 1 = the old rows, slabs of a few thousand nonzeros.  The
// largest slab is read back (one synchronisation of the stream): with a slab over the cap the form refuses.
static int aperm_slab(const ApermCall &c)
{
	const int ndim = c.ndim, *perm = c.perm;
	const int64_t *dim = c.dim, nnz = c.nnz;
	if (!(ndim >= 3 && perm[1] == 0 && perm[0] >= 1 && dim[perm[0]] <= 1024 && dim[0] < ((int64_t) 1 << 30)))
		return APERM_NA;
	const int q = perm[0];
	int64_t os[8], st = 1;
	for (int a = 1; a < ndim; a++) { os[a] = st; st *= dim[a]; }
	SlabMap sm;
	sm.nother = ndim - 2;
	int64_t nslab = 1;
	for (int t = 0; t < ndim - 2; t++) {
		sm.new_ext[t] = dim[perm[2 + t]];
		sm.old_stride[t] = os[perm[2 + t]];
		nslab *= dim[perm[2 + t]];
	}
	if (!(nslab >= 1 && nslab < 2147483646LL && nnz / nslab <= SLAB_CAP * 9 / 10))
		return APERM_NA;
	// The form has no budget of its own: its head must fit in front of the second buffers of the 32-bit key sort
	// (Sort32Layout::ktmp = five arrays of nnz * 4 bytes).  Safe for every caller: aperm_ws_core() gives a top-level call
	// at least aperm_sort32_layout(nnz).total, a step of a composed route gets aperm_ws_core() behind its caller's
	// intermediates (aperm_ws_bytes()), a box of the boxed driver aperm_key_sort_bytes() -- and the sort layouts depend
	// on nnz alone, which no step changes.  The bound is part of the route decision: it stays at ktmp, not .total.
	const SlabHead H = aperm_slab_head(nslab);
	if (H.total > aperm_sort32_layout(nnz).ktmp)
		return APERM_NA;
	char *w = (char *) c.ws;
	int64_t *base = (int64_t *) (w + H.cnt);
	unsigned long long *maxcnt = (unsigned long long *) (w + H.maxcnt), mx = 0;
	hipStream_t s = c.s;
	HIP_TRY(hipMemsetAsync(maxcnt, 0, 8, s));
	hipLaunchKernelGGL(aperm_slab_count_kernel, dim3((unsigned) ((nslab + 1 + 255) / 256)), dim3(256), 0, s,
			   c.col_ptr, sm, nslab, dim[q], os[q], base, maxcnt);
	HIP_TRY(hipMemcpyAsync(&mx, maxcnt, 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	if (mx > SLAB_CAP) {
		g_route[R_SLAB_REFUSED]++;
		return APERM_REFUSED;
	}
	g_route[R_SLAB]++;
	if (launch_exclusive_scan_i64(base, nslab + 1, w + H.scan, s))
		return -1;
	const int bits = key_bits(dim[0]);
	svt_by_rtype(c.Rtype, c.val, c.out_val, [&](auto *v, auto *o) {
		hipLaunchKernelGGL(aperm_slab_kernel, dim3((unsigned) nslab), dim3(SLAB_NT), (size_t) SLAB_CAP * 4, s, c.col_ptr,
				   c.row_idx, v, sm, nslab, dim[0], (int) dim[q], os[q], bits, nnz, base, c.out_ptr, c.out_idx, o);
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

// aperm(x, c(2, 1, 3, ...)): the first two axes change places inside every slab of the remaining ones -- prod(dim[2..])
// independent transpositions of dim[0] x dim[1] matrices that follow one another in the operand's leaves: the bucketed
// transposition, batched (T2Shape).  Returns the workspace it needs (0: the shape does not suit it) and fills *sh,
// *reserve: [t2_head() + 256, rounded up][t2_body() with all (ncoarse + 1) * columns coarse-bucket starts].
static size_t aperm_swap01_bytes(int64_t nnz, const int64_t *dim, int ndim, T2Shape *sh, size_t *reserve)
{
	if (ndim < 3 || nnz <= 0 || nnz >= ((int64_t) 1 << 31))
		return 0;
	const double ns = extent_prod(dim, 2, ndim, -1, false);
	if (ns < 1.0 || ns > 1.0e9)
		return 0;
	if (!t2_shape(dim[0], dim[1], nnz, sh, (int64_t) ns))
		return 0;
	const size_t res = t2_a(t2_head(*sh).total + 256, 1);
	if (reserve) *reserve = res;
	return t2_body(res, (size_t) nnz, (size_t) (sh->ncoarse + 1) * (size_t) (sh->nslab * sh->scol)).total;
}

// svt_dev_transpose_plan (include/svt_hip.h): the decision of launch_transpose() (nslab = 1) or of aperm_swap01_bytes()
// (nslab > 1: `nslab` matrices of nrow x ncol, nnz nonzeros in all), by the same functions.  No launch, no device.
extern "C" int svt_dev_transpose_plan(int64_t nrow, int64_t ncol, int64_t nnz, int64_t nslab, int64_t out[8])
{
	if (out == NULL || nslab < 1)
		return svt_set_error("svt_dev_transpose_plan: NULL result or nslab < 1");
	T2Shape sh;
	memset(&sh, 0, sizeof(sh));
	int why;
	if (nnz <= 0 || nnz >= ((int64_t) 1 << 31)) {
		why = 1;                                            // (no nonzeros: a memset; 2^31 and more: the boxed driver)
	} else if (nslab == 1) {
		size_t reserve = 0;
		why = t_route(nrow, ncol, nnz, &sh, &reserve);
	} else {
		const int64_t dim[3] = {nrow, ncol, nslab};
		why = aperm_swap01_bytes(nnz, dim, 3, &sh, NULL) > 0 ? 0 : 1;
	}
	out[0] = why == 0;
	out[1] = why == 1 ? -1 : sh.fbits;
	out[2] = why == 1 ? -1 : sh.cbits;
	out[3] = why == 1 ? 0 : sh.nfb;
	out[4] = why == 1 ? 0 : sh.ncoarse;
	out[5] = why == 1 ? 0 : sh.ngroups;
	out[6] = (key_bits(nrow) + 7) / 8;
	out[7] = why;
	return 0;
}

// the first two axes change places, the others stay: one batched bucketed transposition, no sort
static int aperm_swap01(const ApermCall &c)
{
	bool swap01 = c.ndim >= 3 && c.perm[0] == 1 && c.perm[1] == 0;
	for (int a = 2; a < c.ndim && swap01; a++) swap01 = c.perm[a] == a;
	T2Shape sh;
	size_t reserve = 0;
	if (!swap01 || aperm_swap01_bytes(c.nnz, c.dim, c.ndim, &sh, &reserve) == 0)
		return APERM_NA;
	g_route[R_SWAP01]++;
	return launch_transpose_bucketed(c.col_ptr, c.row_idx, c.val, c.Rtype, c.dim[0], c.ncol, c.nnz, sh, c.out_ptr, c.out_idx,
					 c.out_val, c.ws, reserve, c.s);
}

// ---- composed routes: steps through intermediate arrays in the workspace.  One such array:
// [leaf pointers (leaves + 1) * 8][row indices nnz*4][values nnz*8]
static size_t aperm_inter_bytes(int64_t leaves, int64_t nnz)
{
	return t2_a((size_t) leaves + 1, 8) + t2_a((size_t) (nnz > 0 ? nnz : 1), 4) + t2_a((size_t) (nnz > 0 ? nnz : 1), 8);
}

// the array at *p, in the order of aperm_inter_bytes(); moves *p past it
struct InterArray { int64_t *col_ptr; int32_t *row_idx; void *val; };
static InterArray aperm_inter_carve(char **p, int64_t leaves, int64_t nnz)
{
	char *idx = *p + t2_a((size_t) leaves + 1, 8);
	const InterArray x = {(int64_t *) *p, (int32_t *) idx, idx + t2_a((size_t) nnz, 4)};
	*p += aperm_inter_bytes(leaves, nnz);
	return x;
}

// a step reads `x` (leaves, dim)
static void aperm_from(ApermCall *n, const InterArray &x, int64_t leaves, const int64_t *dim)
{
	n->col_ptr = x.col_ptr; n->row_idx = x.row_idx; n->val = x.val; n->ncol = leaves; n->dim = dim;
}

// 3-d arrays: the two permutations that neither keep axis 1 nor are one of the forms above are two of those in a row --
// c(2,3,1) = c(2,1,3) then c(1,3,2); c(3,2,1) = c(2,1,3) then c(3,1,2) -- through an intermediate array in the workspace
// (9.3 and 11.5 ms through the library key sort at BASELINE config 5).  Bytes of that intermediate (0: not applicable).
static size_t aperm_via_bytes(int64_t nnz, const int64_t *dim, int ndim)
{
	if (ndim != 3 || nnz <= 0)
		return 0;
	const double nly = (double) dim[0] * (double) dim[2];
	if (nly >= LEAVES_MAX)
		return 0;
	return aperm_inter_bytes((int64_t) nly, nnz);
}

static int aperm_via_3d(const ApermCall &c)
{
	const int *perm = c.perm;
	const int64_t *dim = c.dim;
	if (!(c.ndim == 3 && ((perm[0] == 1 && perm[1] == 2 && perm[2] == 0) || (perm[0] == 2 && perm[1] == 1 && perm[2] == 0 && dim[2] <= 1024))))
		return APERM_NA;
	T2Shape sh;
	size_t reserve = 0;
	if (aperm_via_bytes(c.nnz, dim, 3) == 0 || aperm_swap01_bytes(c.nnz, dim, 3, &sh, &reserve) == 0)
		return APERM_NA;
	g_route[R_VIA_3D]++;
	const int64_t nly = dim[0] * dim[2];
	char *p = (char *) c.ws;
	const InterArray y = aperm_inter_carve(&p, nly, c.nnz);         // (p: what is left, for both steps)
	const int rc = launch_transpose_bucketed(c.col_ptr, c.row_idx, c.val, c.Rtype, dim[0], c.ncol, c.nnz, sh, y.col_ptr,
						 y.row_idx, y.val, p, reserve, c.s);
	if (rc)
		return rc;
	const int64_t dimy[3] = {dim[1], dim[0], dim[2]};
	const int p231[3] = {0, 2, 1}, p321[3] = {2, 0, 1};
	ApermCall n = c;
	aperm_from(&n, y, nly, dimy);
	n.perm = perm[0] == 1 ? p231 : p321;
	n.ws = p;
	return launch_aperm_n(n, 1);
}

// General permutation of an array with three or more axes (round 5; rounds 1-4: a device-wide key sort):
//   A  aperm(x, c(1, q, others))   old axis q = perm[0] next to the rows; axis 1 stays: whole leaves move (no step when q = 2)
//   B  aperm(., c(2, 1, 3, ...))   the first two axes change places: the batched bucketed transposition
//   C  aperm(., c(1, ...))         the remaining axes into their final order: whole leaves move (no step when they are in order)
// through up to two intermediate arrays in the workspace.  aperm_general_plan() fills the steps for a given perm and returns
// false when the shape does not suit (leaf counts past 2^31, or a first-two-axes matrix the bucketed transposition refuses):
// those arrays take the library's own radix sort of (new linear index, position) pairs (svt_sort.h).
struct ApermPlan3 {
	bool a_id, c_id;
	bool swap_ok;             // step B as the batched bucketed transposition
	bool slab_first;          // steps A + B in one: aperm(x, c(q, 1, others)) by the slab form (one workgroup per slab), tried first
	int pa[8], pc[8];
	int64_t dim_a[8], dim_b[8];
	int64_t leaves_a, leaves_b;
};

static bool aperm_general_plan(int64_t nnz, const int64_t *dim, int ndim, const int *perm, ApermPlan3 *pl)
{
	if (ndim < 3 || perm[0] == 0 || nnz <= 0)
		return false;
	const int q = perm[0];
	pl->pa[0] = 0; pl->pa[1] = q;
	for (int a = 1, i = 2; a < ndim; a++)
		if (a != q) pl->pa[i++] = a;
	pl->a_id = q == 1;
	for (int i = 0; i < ndim; i++) pl->dim_a[i] = dim[pl->pa[i]];
	for (int i = 0; i < ndim; i++) pl->dim_b[i] = i == 0 ? pl->dim_a[1] : i == 1 ? pl->dim_a[0] : pl->dim_a[i];
	const double la = extent_prod(pl->dim_a, 1, ndim, -1, false), lb = extent_prod(pl->dim_b, 1, ndim, -1, false);
	if (la >= LEAVES_MAX || lb >= LEAVES_MAX || la < 1.0 || lb < 1.0)
		return false;
	pl->leaves_a = (int64_t) la; pl->leaves_b = (int64_t) lb;
	// a leaf-preserving step reads and writes every leaf pointer a few times: with many more leaves than nonzeros (a short
	// new leading axis: 4e8 leaves of at most 64 entries for aperm(x, c(4,3,2,1)) of a 2e4 x 2e3 x 10 x 64 array) the
	// steps cost more than the sort of the nonzeros (41 against 28 ms there)
	if (la > 2.0 * (double) nnz + 1024.0 || lb > 2.0 * (double) nnz + 1024.0)
		return false;
	// axes of the array after step B, by old axis: l2 = (q, 0, pa[2], pa[3], ...)
	pl->c_id = true;
	pl->pc[0] = 0;
	for (int a = 1; a < ndim; a++) {
		int at = -1;
		for (int i = 1; i < ndim; i++) {
			const int old_axis = i == 1 ? 0 : pl->pa[i];
			if (old_axis == perm[a]) at = i;
		}
		if (at < 0)
			return false;
		pl->pc[a] = at;
		if (at != a) pl->c_id = false;
	}
	T2Shape sh;
	pl->swap_ok = aperm_swap01_bytes(nnz, pl->dim_a, ndim, &sh, NULL) > 0;
	// many small slabs (which the batched transposition refuses) are what the slab form is for; it serves a request
	// that still has a step C to do -- c(q, 1, others) itself has met the slab form on its way here
	pl->slab_first = !pl->c_id && dim[q] <= 1024 && dim[0] < ((int64_t) 1 << 30) &&
			 (double) nnz / (lb / (double) dim[0]) <= 0.9 * 8192.0;
	return pl->swap_ok || pl->slab_first;
}

// Workspace of the three-step form over all permutations of `dim`: the two intermediates + the largest step.
static size_t aperm_general_bytes(int64_t nnz, const int64_t *dim, int ndim, size_t *inter_max)
{
	*inter_max = 0;
	if (ndim < 3 || nnz <= 0)
		return 0;
	size_t need = 0;
	// The plan depends on perm through q = perm[0] and through whether a step C is left to do: only then may the slab form
	// stand in for a refused step B (slab_first).  Both kinds of every q: c(q, 1, others) and c(q, others, 1).  (Sized from
	// the first kind alone, a slab_first plan whose step B is refused carved its intermediate out of a workspace that had
	// none set aside, and the step's key sort behind it wrote past the end.)
	for (int qc = 2; qc < 2 * ndim; qc++) {
		const int q = qc / 2, with_c = qc & 1;
		int perm[8], i = 1;
		perm[0] = q;
		if (!with_c) perm[i++] = 0;
		for (int a = 1; a < ndim; a++)
			if (a != q) perm[i++] = a;
		if (with_c) perm[i++] = 0;
		ApermPlan3 pl;
		if (!aperm_general_plan(nnz, dim, ndim, perm, &pl))
			continue;
		T2Shape sh;
		size_t step = aperm_swap01_bytes(nnz, pl.dim_a, ndim, &sh, NULL);
		const size_t sa = exclusive_scan_ws_bytes(pl.leaves_a + 1) + 256, sb = exclusive_scan_ws_bytes(pl.leaves_b + 1) + 256;
		if (sa > step) step = sa;
		if (sb > step) step = sb;
		const size_t inter = aperm_inter_bytes(pl.leaves_a, nnz) + aperm_inter_bytes(pl.leaves_b, nnz) + 512;
		if (inter > *inter_max) *inter_max = inter;
		if (inter + step > need) need = inter + step;
	}
	return need;
}

// the general form: leaf-preserving step, first two axes swapped (or both in one by the slab form), leaf-preserving step
static int aperm_general(const ApermCall &c)
{
	ApermPlan3 pl;
	if (!aperm_general_plan(c.nnz, c.dim, c.ndim, c.perm, &pl))
		return APERM_NA;
	g_route[R_GENERAL]++;
	const InterArray out = {c.out_ptr, c.out_idx, c.out_val};
	char *p = (char *) c.ws;
	InterArray x = {NULL, NULL, NULL}, y = out;
	if (!pl.a_id && !pl.slab_first) x = aperm_inter_carve(&p, pl.leaves_a, c.nnz);     // (the slab form goes from the operand to y in one step)
	if (!pl.c_id) y = aperm_inter_carve(&p, pl.leaves_b, c.nnz);
	ApermCall n = c;                                    // the steps: nested, in what is left of the workspace
	n.ws = p;
	auto step = [&n](const int *perm, const InterArray &into) {
		n.perm = perm; n.out_ptr = into.col_ptr; n.out_idx = into.row_idx; n.out_val = into.val;
		return launch_aperm_n(n, 1);
	};
	int rc, p1[8], pb[8];
	if (pl.slab_first) {
		// c(q, 1, others) in one go (slab form; if a slab turns out too long the step takes the key sort), then step C
		p1[0] = c.perm[0]; p1[1] = 0;
		for (int a = 2; a < c.ndim; a++) p1[a] = pl.pa[a];
		if ((rc = step(p1, y)) != 0)
			return rc;
	} else {
		if (!pl.a_id) {
			if ((rc = step(pl.pa, x)) != 0)
				return rc;
			aperm_from(&n, x, pl.leaves_a, pl.dim_a);
		}
		for (int a = 0; a < c.ndim; a++) pb[a] = a == 0 ? 1 : a == 1 ? 0 : a;
		n.dim = pl.dim_a;
		if ((rc = step(pb, y)) != 0 || pl.c_id)
			return rc;
	}
	aperm_from(&n, y, pl.leaves_b, pl.dim_b);
	return step(pl.pc, out);
}

// the forms that need no intermediate: the largest of the key sorts and the batched transposition (+ 256 each) + the leaf-preserving form's
static size_t aperm_ws_core(int64_t nnz, const int64_t *dim, int ndim)
{
	T2Shape sh;
	size_t need = aperm_swap01_bytes(nnz, dim, ndim, &sh, NULL) + 256;
	need = std::max(need, std::max(aperm_sort32_layout(nnz).total, aperm_sort64_layout(nnz).total));
	return need + aperm_leaf_scan_bytes(dim, ndim);
}

size_t aperm_ws_bytes(int64_t nnz, const int64_t *dim, int ndim)
{
	if (nnz >= ((int64_t) 1 << 31))                         // only the leaf-preserving form takes such an operand
		return aperm_leaf_scan_bytes(dim, ndim) + 256;
	size_t need = aperm_ws_core(nnz, dim, ndim);
	{
		// (a step of the general form may itself fall back to the forms that aperm_ws_core() sizes: the intermediates
		// come on top of the larger of the two)
		size_t inter = 0;
		const size_t gen = aperm_general_bytes(nnz, dim, ndim, &inter);
		if (gen > need + inter) need = gen; else need += inter;
	}
	const size_t via = aperm_via_bytes(nnz, dim, ndim);
	if (via > 0) {
		const int64_t dimy[3] = {dim[1], dim[0], dim[2]};
		const size_t second = aperm_ws_core(nnz, dimy, 3);
		need = via + (need > second ? need : second);
	}
	return need;
}

static bool aperm_perm_ok(int ndim, const int *perm)
{
	if (ndim < 1 || ndim > 8)
		return false;
	bool seen[8] = {false, false, false, false, false, false, false, false};
	for (int a = 0; a < ndim; a++) {
		if (perm[a] < 0 || perm[a] >= ndim || seen[perm[a]])
			return false;
		seen[perm[a]] = true;
	}
	return true;
}

// The dispatcher: the routes in the order they are tried.
// nested != 0: a step of a composed route (aperm_via_3d, aperm_general).  Such a call gets what is left of the
// workspace behind its caller's intermediates, which aperm_ws_bytes() sizes by aperm_ws_core() alone: it must not carve
// intermediates of its own (a slab form that refused at run time used to re-enter the general form inside the rest and
// write past the workspace).  So a nested call reaches aperm_leaf_preserving (aperm_leaf_scan_bytes), aperm_swap01
// (aperm_swap01_bytes), aperm_slab (aperm_slab_head, within aperm_sort32_layout) and the two key sorts
// (aperm_sort32_layout, aperm_sort64_layout) -- the terms of aperm_ws_core(), none of which calls back into here.
// nested == 2: a box of the boxed driver whose preferred route needs more than the driver's route area: the
// leaf-preserving form or the key sort alone, whose need depends on the nonzero count only.
static int launch_aperm_n(const ApermCall &c, int nested)
{
	if (c.ndim < 1 || c.ndim > 8)
		return svt_set_error("aperm: between 1 and 8 dimensions are supported");
	if (!aperm_perm_ok(c.ndim, c.perm))
		return svt_set_error("'perm' must be a permutation of 1:%d", c.ndim);
	if (extent_prod(c.dim, 0, c.ndim) >= 9.2e18)
		return svt_set_error("aperm: array too large for 64-bit linear indices");
	int64_t new_nleaves = 1;
	for (int a = 1; a < c.ndim; a++) new_nleaves *= c.dim[c.perm[a]];
	if (c.nnz == 0) {
		HIP_TRY(hipMemsetAsync(c.out_ptr, 0, (size_t) (new_nleaves + 1) * 8, c.s));
		return 0;
	}
	if (c.perm[0] == 0 && new_nleaves < ((int64_t) 1 << 31) - 1)
		return aperm_leaf_preserving(c, new_nleaves);
	// (the leaf-preserving form above counts positions in 64 bits; the others do not)
	if (c.nnz >= ((int64_t) 1 << 31))
		return svt_set_unsupported("aperm: more than 2^31-1 nonzeros");
	int rc;
	if (!nested && (rc = aperm_via_3d(c)) != APERM_NA)
		return rc;
	if (nested < 2 && (rc = aperm_swap01(c)) != APERM_NA)
		return rc;
	if (nested < 2 && (rc = aperm_slab(c)) <= 0)            // (APERM_NA or APERM_REFUSED: on to the forms below)
		return rc;
	if (!nested && (rc = aperm_general(c)) != APERM_NA)
		return rc;
	return new_nleaves < ((int64_t) 1 << 31) - 1 ? aperm_sort32(c, new_nleaves) : aperm_sort64(c, new_nleaves);
}

// ---------------------------------------------------------------------------
// aperm(x, perm) with perm[1] != 1 past 2^31 nonzeros: the boxed driver, the N-d counterpart of launch_transpose_boxed.
// Let q = perm[0] be the old axis that becomes the rows of the result.  Inside every leaf of the result the entries are
// ordered by their index i_q along q and no two share one.  A BOX is a range [q0, q1) of indices of axis q holding at
// most `box` nonzeros, or a single index (at most one entry per result leaf: <= new_nleaves < 2^31 - 1 nonzeros).  The
// sub-array x[..., q0:q1, ...] is an operand of its own below 2^31 nonzeros; permuted with the SAME perm by the
// unchanged routes it has the leaves of the full result and rows 0 .. q1 - q0:
//   axis    nonzeros per index of axis q from col_ptr alone (one thread per old leaf, 64-bit counters, privatised in
//           LDS when dim[q] allows), scanned into qptr[dim[q] + 1]: the "col_ptr" of axis q.
//   cuts    box_cut_kernel over qptr, as for t(): the index holding every multiple of `box` is a box of its own; indices
//           Wq apart are cut too, so that a box's own leaves (Wq * leaves per index) stay within the workspace.  The
//           cuts are read back: one stream synchronisation per call.
//   count   the lengths of the result's leaves: one wavefront per old leaf, one 64-bit atomic per nonzero (the entries
//           of one old leaf hit distinct counters), scanned in place into out_ptr; fill[] = 0.
//   per box gather: the leaves with i_q in [q0, q1) -- a run of (q1 - q0) * stride_q leaves for every index of the axes
//           outside q -- are copied with a rebased col_ptr into a box-sized temporary by the leaf-preserving form's own
//           kernels (64-bit source positions, coalesced runs); when q is outermost the box is a slice of the operand
//           and only its col_ptr is rebased.  Route: launch_aperm_n on (temporary, dims with q1 - q0 on axis q, perm)
//           into a second temporary of new_nleaves + 1 pointers.  Placement: box_place_kernel, adding q0 to the rows.
// Why the result is exact: boxes are taken in ascending q0, so every box contributes ONE contiguous run to every result
// leaf and the runs come in box order = i_q order; only copies happen, and the permuted array has one representation.
// Workspace: abox_layout() -- not O(nnz).  Its route area R is the larger of aperm_key_sort_bytes() and aperm_ws_bytes() at the
// largest box.  The routes' needs depend on the box's dims, which are not known before the data is seen: a box whose preferred
// route needs more than R takes the key sort (nested = 2), whose need depends on the box's nonzero count alone.
// ---------------------------------------------------------------------------
#define ABOX_DEFAULT ((int64_t) 1 << 28)
#define ABOX_LEAVES ((int64_t) 1 << 20)  // a box spans at most max(this, new_nleaves) old leaves (or one index of axis q)
#define ABOX_CNT_NT 256
#define ABOX_CNT_LDS 8192                // indices of axis q counted in LDS (64 KB of 64-bit counters); more: memory atomics

struct ABoxLayout {
	bool ok;                 // the result has fewer than 2^31 - 1 leaves and no extent is 0
	bool outer;              // q is the outermost axis with an extent over 1: a box is a slice of the operand
	int64_t bsz, bmax, Wq, npts_max, new_nl, slice_nl, osq, nouter, box_leaves;
	size_t pts, qptr, scan, fill, bcp, gidx, gval, bptr, bidx, bval, route, route_bytes, total;
};

static ABoxLayout abox_layout(int64_t nnz, const int64_t *dim, int ndim, int q, int64_t box_limit)
{
	ABoxLayout L;
	memset(&L, 0, sizeof(L));
	for (int a = 0; a < ndim; a++)
		if (dim[a] <= 0) return L;
	const double nl = extent_prod(dim, 0, ndim, q);
	if (nl >= LEAVES_MAX) return L;
	L.ok = true;
	L.new_nl = (int64_t) nl;
	L.slice_nl = L.new_nl / dim[0];                         // old leaves per index of axis q
	L.osq = 1;
	for (int a = 1; a < q; a++) L.osq *= dim[a];
	L.nouter = L.slice_nl / L.osq;
	L.outer = L.nouter == 1;
	L.bsz = box_size(box_limit, ABOX_DEFAULT);
	L.bmax = L.bsz > L.new_nl ? L.bsz : L.new_nl;           // a box: <= bsz nonzeros, or one index of axis q
	if (L.bmax > nnz) L.bmax = nnz > 0 ? nnz : 1;
	const int64_t lcap = L.new_nl > ABOX_LEAVES ? L.new_nl : ABOX_LEAVES;
	L.Wq = lcap / L.slice_nl > 1 ? lcap / L.slice_nl : 1;
	if (L.Wq > dim[q]) L.Wq = dim[q];
	L.box_leaves = L.Wq * L.slice_nl;
	L.npts_max = (nnz + L.bsz - 1) / L.bsz + (dim[q] + L.Wq - 1) / L.Wq + 1;
	size_t sc = exclusive_scan_ws_bytes(dim[q] + 1), t;
	if ((t = exclusive_scan_ws_bytes(L.new_nl + 1)) > sc) sc = t;
	if ((t = exclusive_scan_ws_bytes(L.box_leaves + 1)) > sc) sc = t;
	L.route_bytes = aperm_ws_bytes(L.bmax, dim, ndim);
	if ((t = aperm_key_sort_bytes(L.bmax)) > L.route_bytes) L.route_bytes = t;
	size_t o = 0;
	L.pts = o;   o += t2_a((size_t) L.npts_max * 3, 8);
	L.qptr = o;  o += t2_a((size_t) dim[q] + 1, 8);
	L.scan = o;  o += t2_a(sc, 1);
	L.fill = o;  o += t2_a((size_t) L.new_nl + 1, 8);
	L.bcp = o;   o += t2_a((size_t) L.box_leaves + 1, 8);
	L.gidx = o;  o += L.outer ? 0 : t2_a((size_t) L.bmax, 4);
	L.gval = o;  o += L.outer ? 0 : t2_a((size_t) L.bmax, 8);
	L.bptr = o;  o += t2_a((size_t) L.new_nl + 1, 8);
	L.bidx = o;  o += t2_a((size_t) L.bmax, 4);
	L.bval = o;  o += t2_a((size_t) L.bmax, 8);
	L.route = o; o += L.route_bytes;
	L.total = o + 256;
	return L;
}

// the need of one permutation (0-based perm, valid) under the box limit of the call
size_t aperm_perm_ws_bytes_box(int64_t nnz, const int64_t *dim, int ndim, const int *perm, int64_t box_limit)
{
	if (!box_taken(nnz, box_limit) || !aperm_perm_ok(ndim, perm))
		return aperm_ws_bytes(nnz, dim, ndim);
	if (perm[0] == 0) {
		// leaf-preserving, never boxed: the scratch of a scan over the leaf counts (with 2^31 - 1 leaves or more
		// the call goes to the 64-bit key sort, or is refused)
		const size_t scan_b = aperm_leaf_scan_bytes(dim, ndim);
		return scan_b > 0 ? scan_b + 256 : aperm_ws_bytes(nnz, dim, ndim);
	}
	if (ndim == 2)
		return transpose_ws_bytes_box(dim[0], nnz, box_limit);
	const ABoxLayout L = abox_layout(nnz, dim, ndim, perm[0], box_limit);
	return L.ok ? L.total : 256;                            // (not ok: the call is refused before it touches the workspace)
}

// at least the need of every permutation; what aperm_ws_bytes() returns whenever the boxed driver is not taken
size_t aperm_ws_bytes_box(int64_t nnz, const int64_t *dim, int ndim, int64_t box_limit)
{
	if (!box_taken(nnz, box_limit) || ndim < 1 || ndim > 8)
		return aperm_ws_bytes(nnz, dim, ndim);
	int perm[8];
	for (int a = 0; a < ndim; a++) perm[a] = a;
	size_t need = aperm_perm_ws_bytes_box(nnz, dim, ndim, perm, box_limit);
	for (int q = 1; q < ndim; q++) {
		perm[0] = q; perm[q] = 0;                           // (the need depends on perm through perm[0] alone)
		const size_t t = aperm_perm_ws_bytes_box(nnz, dim, ndim, perm, box_limit);
		if (t > need) need = t;
		perm[0] = 0; perm[q] = q;
	}
	return need;
}

// cnt[i] += nonzeros of the old leaves whose index along axis q is i (cnt zeroed by the caller); grid-stride over leaves
__global__ void __launch_bounds__(ABOX_CNT_NT)
abox_axis_count_kernel(const int64_t *__restrict__ col_ptr, int64_t nleaves, int64_t osq, int64_t dq, int use_lds,
		       unsigned long long *__restrict__ cnt)
{
	extern __shared__ unsigned long long hq[];
	const bool lds = use_lds != 0;                  // (dq <= ABOX_CNT_LDS counters of dynamic LDS)
	if (lds) {
		for (int64_t i = threadIdx.x; i < dq; i += ABOX_CNT_NT) hq[i] = 0;
		__syncthreads();
	}
	const int64_t stride = (int64_t) gridDim.x * ABOX_CNT_NT;
	for (int64_t l = (int64_t) blockIdx.x * ABOX_CNT_NT + threadIdx.x; l < nleaves; l += stride) {
		const int64_t n = col_ptr[l + 1] - col_ptr[l];
		if (n == 0) continue;
		const int64_t iq = (l / osq) % dq;
		if (lds) atomicAdd(&hq[iq], (unsigned long long) n);
		else atomicAdd(&cnt[iq], (unsigned long long) n);
	}
	if (lds) {
		__syncthreads();
		for (int64_t i = threadIdx.x; i < dq; i += ABOX_CNT_NT)
			if (hq[i]) atomicAdd(&cnt[i], hq[i]);
	}
}

struct ABoxMap {
	int ndim;
	int64_t dim[8];      // old extents
	int64_t nmul[8];     // stride of old axis a in the NEW leaf index (0 for the axis that becomes the rows)
};

// len[new leaf] += 1 for every nonzero (len zeroed by the caller): one wavefront per old leaf, whose entries differ in
// the old row and so hit distinct counters
__global__ void __launch_bounds__(256)
abox_leaf_len_kernel(const int64_t *__restrict__ col_ptr, const int32_t *__restrict__ row_idx, int64_t nleaves,
		     ABoxMap m, unsigned long long *__restrict__ len)
{
	const int lane = threadIdx.x & 63;
	const int64_t stride = (int64_t) gridDim.x * 4;
	for (int64_t l = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6); l < nleaves; l += stride) {
		const int64_t b = col_ptr[l], n = col_ptr[l + 1] - b;
		if (n == 0) continue;
		int64_t base = 0, rest = l;
		for (int a = 1; a < m.ndim; a++) {
			const int64_t ia = rest % m.dim[a];
			rest /= m.dim[a];
			base += ia * m.nmul[a];
		}
		for (int64_t k = lane; k < n; k += 64)
			atomicAdd(&len[base + (int64_t) row_idx[b + k] * m.nmul[0]], 1ull);
	}
}

// count: the lengths of the result's leaves, scanned in place into out_ptr; fill[] = 0
static int abox_leaf_lengths(const int64_t *col_ptr, const int32_t *row_idx, int64_t ncol, const int64_t *dim, int ndim,
			     const int *perm, int64_t new_nl, int64_t *out_ptr, int64_t *fill, void *scan_ws, hipStream_t s)
{
	ABoxMap mp;
	memset(&mp, 0, sizeof(mp));
	mp.ndim = ndim;
	for (int a = 0; a < ndim; a++) mp.dim[a] = dim[a];
	int64_t st = 1;
	for (int a = 1; a < ndim; a++) { mp.nmul[perm[a]] = st; st *= dim[perm[a]]; }
	HIP_TRY(hipMemsetAsync(out_ptr, 0, (size_t) (new_nl + 1) * 8, s));
	HIP_TRY(hipMemsetAsync(fill, 0, (size_t) new_nl * 8, s));
	int64_t nbl = (ncol + 3) / 4;
	if (nbl > ((int64_t) 1 << 22)) nbl = (int64_t) 1 << 22;
	hipLaunchKernelGGL(abox_leaf_len_kernel, dim3((unsigned) nbl), dim3(256), 0, s, col_ptr, row_idx, ncol, mp, (unsigned long long *) out_ptr);
	HIP_TRY(hipGetLastError());
	return launch_exclusive_scan_i64(out_ptr, new_nl + 1, scan_ws, s);
}

static int launch_aperm_boxed(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
			      int64_t ncol, int64_t nnz, const int64_t *dim, int ndim, const int *perm,
			      int64_t *out_ptr, int32_t *out_idx, void *out_val, void *ws, int64_t box_limit, hipStream_t s)
{
	const int q = perm[0];
	const ABoxLayout Ly = abox_layout(nnz, dim, ndim, q, box_limit);
	if (!Ly.ok)
		return svt_set_unsupported("aperm: the permuted array has %.0f leaves, 2^31-1 or more", extent_prod(dim, 0, ndim, q, false));
	char *w = (char *) ws;
	int64_t *pts = (int64_t *) (w + Ly.pts), *qptr = (int64_t *) (w + Ly.qptr), *fill = (int64_t *) (w + Ly.fill);
	int64_t *bcp = (int64_t *) (w + Ly.bcp), *bptr = (int64_t *) (w + Ly.bptr);
	int32_t *gidx = (int32_t *) (w + Ly.gidx), *bidx = (int32_t *) (w + Ly.bidx);
	void *gval = w + Ly.gval, *bval = w + Ly.bval, *rws = w + Ly.route, *scan_ws = w + Ly.scan;
	const size_t esz = Rtype == SVT_REALSXP ? 8 : 4;
	const int64_t dq = dim[q], new_nl = Ly.new_nl;
	// nonzeros per index of axis q -> qptr
	HIP_TRY(hipMemsetAsync(qptr, 0, (size_t) (dq + 1) * 8, s));
	bool lds = dq <= ABOX_CNT_LDS;
	if (lds && hipFuncSetAttribute((const void *) abox_axis_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
				       ABOX_CNT_LDS * 8) != hipSuccess) {
		(void) hipGetLastError();
		lds = false;
	}
	int64_t nbc = (ncol + ABOX_CNT_NT - 1) / ABOX_CNT_NT;
	if (nbc > 1024) nbc = 1024;
	hipLaunchKernelGGL(abox_axis_count_kernel, dim3((unsigned) nbc), dim3(ABOX_CNT_NT), lds ? (size_t) dq * 8 : 0, s,
			   col_ptr, ncol, Ly.osq, dq, lds ? 1 : 0, (unsigned long long *) qptr);
	HIP_TRY(hipGetLastError());
	if (launch_exclusive_scan_i64(qptr, dq + 1, scan_ws, s))
		return -1;
	// the cuts, read back once; the lengths of the result's leaves -> out_ptr are queued before the wait for them
	BoxBounds bd;                                       // (index of axis q, qptr there)
	if (box_boundaries("aperm", qptr, dq, nnz, Ly.bsz, Ly.Wq, Ly.npts_max, pts, s, &bd, [&] {
		    return abox_leaf_lengths(col_ptr, row_idx, ncol, dim, ndim, perm, new_nl, out_ptr, fill, scan_ws, s); }))
		return -1;
	int64_t bdim[8];
	for (int a = 0; a < ndim; a++) bdim[a] = dim[a];
	LeafMap lm;                                         // box leaf (inner, i_q - q0, outer) -> old leaf, from leaf q0 * osq on
	memset(&lm, 0, sizeof(lm));
	lm.ndim = 4;
	lm.new_dim[1] = Ly.osq;    lm.old_stride[1] = 1;
	lm.new_dim[3] = Ly.nouter; lm.old_stride[3] = Ly.osq * dq;
	lm.old_stride[2] = Ly.osq;
	for (size_t b = 0; b + 1 < bd.size(); b++) {
		const int64_t q0 = bd[b].first, wq = bd[b + 1].first - q0, p0 = bd[b].second, nb = bd[b + 1].second - p0;
		if (nb == 0)
			continue;
		if (nb > Ly.bmax || wq > Ly.Wq)
			return svt_set_error("aperm: internal error (box of %lld nonzeros, %lld indices)", (long long) nb,
					     (long long) wq);
		const int64_t bl = wq * Ly.slice_nl;                // the box's leaves
		const int64_t *lcp = col_ptr + q0 * Ly.osq;
		const int32_t *bri = gidx;
		const void *bv = gval;
		if (Ly.outer) {
			hipLaunchKernelGGL(box_rebase_kernel, dim3((unsigned) ((bl + 1 + 255) / 256)), dim3(256), 0, s,
					   lcp, (int64_t) 0, bl, p0, bcp);
			HIP_TRY(hipGetLastError());
			bri = row_idx + p0;
			bv = (const char *) val + (size_t) p0 * esz;
		} else {
			lm.new_dim[2] = wq;
			if (launch_leaf_move(lcp, row_idx, val, Rtype, bl, lm, bcp, gidx, gval, scan_ws, s))
				return -1;
		}
		bdim[q] = wq;
		// the box's preferred route where the route area holds it, else the key sort (whose need is part of the area)
		const bool fits = aperm_ws_bytes(nb, bdim, ndim) <= Ly.route_bytes;
		if (!fits && aperm_key_sort_bytes(nb) > Ly.route_bytes)
			return svt_set_error("aperm: internal error (route area of a box)");
		const ApermCall box = {bcp, bri, bv, Rtype, bl, nb, bdim, ndim, perm, bptr, bidx, bval, rws, s};
		if (launch_aperm_n(box, fits ? 0 : 2))
			return -1;
		launch_box_place(Rtype, bptr, bidx, bval, new_nl, q0, out_ptr, fill, out_idx, out_val, s);
		HIP_TRY(hipGetLastError());
	}
	g_boxed_calls++;
	return 0;
}

// aperm with the box limit of the call (read once by the caller): a permutation that moves the rows takes the boxed
// driver past the limit (a 2-d one: the boxed t()); everything else the routes above exactly as they are.
int launch_aperm_box(const int64_t *col_ptr, const int32_t *row_idx, const void *val, int Rtype,
		     int64_t ncol, int64_t nnz, const int64_t *dim, int ndim, const int *perm,
		     int64_t *out_ptr, int32_t *out_idx, void *out_val, void *ws, int64_t box_limit, hipStream_t s)
{
	if (!box_taken(nnz, box_limit) || ndim < 2 || !aperm_perm_ok(ndim, perm) || perm[0] == 0) {
		const ApermCall c = {col_ptr, row_idx, val, Rtype, ncol, nnz, dim, ndim, perm, out_ptr, out_idx, out_val, ws, s};
		return launch_aperm_n(c, 0);
	}
	if (ndim == 2)
		return launch_transpose_box(col_ptr, row_idx, val, Rtype, dim[0], ncol, nnz, out_ptr, out_idx, out_val, ws,
					    box_limit, s);
	if (extent_prod(dim, 0, ndim) >= 9.2e18)
		return svt_set_error("aperm: array too large for 64-bit linear indices");
	return launch_aperm_boxed(col_ptr, row_idx, val, Rtype, ncol, nnz, dim, ndim, perm, out_ptr, out_idx, out_val, ws,
				  box_limit, s);
}
