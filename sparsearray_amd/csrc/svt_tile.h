// What the copy kernels over tiles of consecutive nonzeros share (kernels_subset.hip: the column gather; kernels_abind.hip:
// the copy of abind): a tile is SVT_TILE = 4096 consecutive entries, one trip of a 256-thread workgroup, entry
// it * 256 + tid of the tile in trip `it`; it is cut into 64 chunks of 64 consecutive entries, one per wavefront and trip,
// so that ONE wavefront scans the table over the chunks with shuffles.  The segments (columns, pieces) a tile touches are
// a contiguous range found by binary searches over their starts; one lane per segment boundary inside the tile marks it
// in LDS, and a max-scan spreads the mark over the segment's entries.
#pragma once

#include "svt_common.h"

#define SVT_TILE_NT 256
#define SVT_TILE_ITEMS 16
#define SVT_TILE (SVT_TILE_NT * SVT_TILE_ITEMS)
#define SVT_TILE_CHUNKS (SVT_TILE / SVT_WAVE)
#define SVT_TILE_SHIFT 12
static_assert(SVT_TILE == 1 << SVT_TILE_SHIFT && SVT_TILE_CHUNKS == SVT_WAVE, "one wavefront scans the chunk table of a tile");

// the last q in [0, n] with ptr[q] <= x (ptr[0 .. n] ascending, ptr[0] = 0 <= x): for x < ptr[n] the column that holds
// entry x -- a non-empty one, the empty columns that start at the same place come before it
__device__ inline int64_t sub_last_le(const int64_t *ptr, int64_t n, int64_t x)
{
	int64_t lo = 0, hi = n + 1;
	while (hi - lo > 1) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (ptr[mid] <= x) lo = mid; else hi = mid;
	}
	return lo;
}
// the first q in [0, n] with ptr[q] >= x (x <= ptr[n])
__device__ inline int64_t sub_first_ge(const int64_t *ptr, int64_t n, int64_t x)
{
	int64_t lo = -1, hi = n;
	while (hi - lo > 1) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (ptr[mid] >= x) hi = mid; else lo = mid;
	}
	return hi;
}

// seg[SVT_TILE]: at the first entry of every segment that starts inside the tile the segment's number (relative to the
// segment of the tile's first entry, so > 0), 0 elsewhere; complete and visible (a barrier after the last write).
// Afterwards the segment of entry it * 256 + tid is max(v[it], cmax[it * 4 + w]), w the thread's wavefront: v the
// inclusive max-scan inside the entry's chunk (shuffles), cmax[SVT_TILE_CHUNKS] the exclusive max-scan of the 64 chunk
// maxima (the first wavefront).  Ends with a barrier; the caller puts one before seg and cmax are written again.
__device__ inline void svt_tile_max_scan(const int *seg, int *cmax, int (&v)[SVT_TILE_ITEMS])
{
	const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
	for (int it = 0; it < SVT_TILE_ITEMS; it++) {
		int x = seg[it * SVT_TILE_NT + tid];
		for (int o = 1; o < SVT_WAVE; o <<= 1) {
			const int t = __shfl_up(x, o, SVT_WAVE);
			if (lane >= o && t > x) x = t;
		}
		v[it] = x;
		if (lane == SVT_WAVE - 1) cmax[it * (SVT_TILE_NT / SVT_WAVE) + w] = x;
	}
	__syncthreads();
	if (tid < SVT_WAVE) {                      // exclusive max-scan of the chunk maxima, in place
		int x = cmax[tid];
		for (int o = 1; o < SVT_WAVE; o <<= 1) {
			const int t = __shfl_up(x, o, SVT_WAVE);
			if (lane >= o && t > x) x = t;
		}
		const int e = __shfl_up(x, 1, SVT_WAVE);
		cmax[tid] = lane == 0 ? 0 : e;
	}
	__syncthreads();
}
