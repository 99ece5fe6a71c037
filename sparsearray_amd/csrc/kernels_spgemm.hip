// C = A %*% B for two sparse operands in the CSC device layout, with a SPARSE result: the product whose dense form
// cannot exist (1e6 x 1e4 at 1 % times a 1e4 x 1e4 matrix with a few nonzeros per column: 80 GB dense, a few GB
// sparse), and the one that keeps a chain of resident operations on the device.  kernels_spmm.hip is the same
// product with a dense result.
//
// THE RULE.  For every cell (i, k):  C[i, k] = the sum, IN ASCENDING ORDER OF THE INNER INDEX j, of
// (double) A[i, j] * (double) B[j, k] over the j where A stores an entry at (i, j) and B one at (j, k); the
// accumulator starts from +0.0, every product is rounded and then added (no fused multiply-add: the file is built
// with -ffp-contract=off like the rest of the library), an integer value goes over as svt_rule_as_double() takes it
// (NA_integer_ -> NA_real_).  The cell is stored when at least one pair meets in it and the sum is not == 0 (-0.0
// and a sum that cancels are dropped, a NaN stays; a stored zero of an operand is an ordinary value): Arith's rule.
//
// THE FIXED ORDER IS WHAT THE PLACEMENT RESTS ON.  The result is placed by a count pass and a fill pass that each
// form the sums on their own (keeping them between the passes would be the dense result).  Whether a cell is stored
// depends on its sum (1e16 + 1 - 1e16 is 0, 1e16 - 1e16 + 1 is 1): two passes that added in different orders
// could disagree about nnz, and the fill pass would write past what the count pass set aside.  With one fixed
// order both passes see the same bits, and so do two runs.
//
// Shape.  One WAVEFRONT per item (result column k, row panel q of P = 2^ps rows); its part of LDS holds the panel's
// image (P doubles) and one byte per cell that says whether a pair has reached it.  The wavefront walks the nonzeros
// (j, b) of column k of B in stored order -- ascending j -- and takes, for each, the run of leaf j of A inside panel
// q from the table of run bounds (launch_rowpanel_table_scan, kernels_rowstats.hip: one pass over A's offsets that
// also looks at A's values for the not-finite flag).  Its 64 lanes stride over the run: the rows of one run are
// distinct, so no two lanes meet in a cell, and the additions of two pairs into one cell are ordered by the
// wavefront's program order (LDS operations of a wavefront complete in order; a wavefront-scope fence between the
// pairs keeps the compiler from moving them).  No atomic, no barrier.  A cell reached for the first time is
// written, not added to: the image needs no clearing, only the P bytes do, and the closing look at the cells reads
// a double only where the byte is up -- an item costs what it touches, not P.
// The metadata of 64 pairs (j, b, run bounds) is fetched by the 64 lanes at once and handed round by shuffles; the
// first 64 elements of SPGEMM_U runs are fetched together before any of them is added (a run holds ~20 elements at
// 1 % and P = 2048: one pair at a time would wait for one short load after the other).
//
// Count pass: after the walk, trip x of the closing look has lane l at cell x * 64 + l; a cell counts when its byte
// is up and its value is not == 0 (a NaN counts).  The count goes to counts[k * npan + q] -- column-major, so that
// ONE 64-bit exclusive scan (svt_scan.h) turns the counts into every item's base in CSC order, and out_col_ptr[k] is
// the base of item k * npan.  Fill pass: the same walk, then row and value at base + running offset + the number of
// kept cells in the lanes below of the same trip (a ballot and a popcount): rows ascend inside every result column,
// no atomic decides a position.  An item whose column of B is empty writes a zero count before it touches LDS; an
// item whose count is zero leaves the fill pass at once.
//
// Measured (profiles/spgemm_timing.txt; count + fill, ms; config 3 / A 1e6 x 1e4 @ 1 % times 1e4 x 1e4 with 2 per column):
// 2048 rows x 4 wavefronts 4.34 / 28.6 (kept); 1024 rows 4.49 / 22.4 (a table of run bounds twice as large, and its LDS
// form ends at 1.05e6 rows); 4096 rows 4.49 / 43.3; 1, 2 or 8 wavefronts per workgroup within 2 % of 4.
//
// Workspace: [head 256: int not-finite flag, int64 nnz of the result at byte 8][table of run bounds int32[(npan + 1)
// * n]][counts, then bases int64[K * npan + 1]][scratch of the scan]; the parts at multiples of 256 bytes.
#include <string.h>

#include "svt_common.h"
#include "svt_scan.h"
#include "svt_arith_rules.h"

#define SPGEMM_PS 11            // 2048-row panels: 18 KB of LDS per wavefront
#define SPGEMM_WAVES 4          // wavefronts (items) per workgroup
#define SPGEMM_U 4              // runs whose first 64 elements are in flight together

static int g_spgemm_ps = SPGEMM_PS, g_spgemm_waves = SPGEMM_WAVES;
static void spgemm_knobs(void)
{
	static bool done = false;
	if (done) return;
	done = true;
	// (tuning build only: the measurements of DESIGN.md, Appendix A)
#ifdef SVT_TUNING
	if (getenv("SVT_SPGEMM_PS")) g_spgemm_ps = atoi(getenv("SVT_SPGEMM_PS"));
	if (getenv("SVT_SPGEMM_WAVES")) g_spgemm_waves = atoi(getenv("SVT_SPGEMM_WAVES"));
#endif
	if (g_spgemm_ps < 10 || g_spgemm_ps > 12) g_spgemm_ps = SPGEMM_PS;
	if (g_spgemm_waves != 1 && g_spgemm_waves != 2 && g_spgemm_waves != 4 && g_spgemm_waves != 8) g_spgemm_waves = SPGEMM_WAVES;
}

static inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

struct SpgemmWs {
	size_t table, base, scan, total;
	int64_t npan, nitems;
	int ps;
};
static SpgemmWs spgemm_ws(int64_t nrow, int64_t ninner, int64_t K)
{
	spgemm_knobs();
	SpgemmWs L;
	L.ps = g_spgemm_ps;
	L.npan = nrow > 0 ? ((nrow - 1) >> L.ps) + 1 : 0;
	L.nitems = (K > 0 ? K : 0) * L.npan;
	L.table = 256;
	L.base = L.table + up256((size_t) (ninner > 0 ? ninner : 1) * (size_t) (L.npan + 1) * 4);
	L.scan = L.base + up256(((size_t) L.nitems + 1) * 8);
	L.total = L.scan + exclusive_scan_ws_bytes(L.nitems + 1);
	return L;
}

int spgemm_panel(void)
{
	spgemm_knobs();
	return 1 << g_spgemm_ps;
}

size_t spgemm_ws_bytes(int64_t nrow, int64_t ninner, int64_t K)
{
	return spgemm_ws(nrow, ninner, K).total;
}

// *flag = 1 when a value is NaN / +-Inf / NA_real_ (doubles) or NA_integer_ (ints)
template <typename T>
__global__ void __launch_bounds__(256)
spgemm_scan_values_kernel(const T *__restrict__ val, int64_t n, int *__restrict__ flag)
{
	bool bad = false;
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
		bad |= !svt_is_finite(svt_rule_as_double(val[i]));
	if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) *flag = 1;
}

static void spgemm_scan_values(const void *val, int Rtype, int64_t n, int *flag, hipStream_t s)
{
	if (n <= 0) return;
	int64_t nb = (n + 256 * 8 - 1) / (256 * 8);
	if (nb > 256 * 16) nb = 256 * 16;
	if (Rtype == SVT_REALSXP)
		hipLaunchKernelGGL(spgemm_scan_values_kernel<double>, dim3((unsigned) nb), dim3(256), 0, s, (const double *) val, n, flag);
	else
		hipLaunchKernelGGL(spgemm_scan_values_kernel<int32_t>, dim3((unsigned) nb), dim3(256), 0, s, (const int32_t *) val, n, flag);
}

// what one pair has written, the next pair's lanes read: the order of the rule
__device__ inline void spgemm_wave_order(void)
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one product into cell r of the wavefront's image (r outside the panel: an operand whose rows do not ascend; not followed)
__device__ inline void spgemm_add(double *acc, unsigned char *seen, int r, int P, double p)
{
	if ((unsigned) r >= (unsigned) P)
		return;
	if (seen[r]) {
		acc[r] += p;
	} else {
		acc[r] = 0.0 + p;
		seen[r] = 1;
	}
}

struct SpgemmKernelArgs {
	const int64_t *a_ptr; const int32_t *a_idx; const void *a_val; int64_t nrow, ninner;
	const int64_t *b_ptr; const int32_t *b_idx; const void *b_val;
	const int32_t *pt; int64_t npan, nitems; int ps;
	int64_t *base;                      // count pass: the counts (written); fill pass: the bases (read)
	int32_t *out_row_idx; double *out_val;
};

template <typename TA, typename TB, bool FILL>
__global__ void __launch_bounds__(64 * 8)
spgemm_kernel(SpgemmKernelArgs a)
{
	extern __shared__ double spgemm_lds[];          // per wavefront [P doubles][P bytes]
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = blockDim.x >> 6;
	const int64_t item = (int64_t) blockIdx.x * W + w;
	if (item >= a.nitems)                           // (per wavefront; the kernel has no barrier)
		return;
	const int64_t k = item / a.npan, q = item - k * a.npan;
	const int64_t bb = a.b_ptr[k], be = a.b_ptr[k + 1];
	int64_t base = 0;
	if (FILL) {
		base = a.base[item];
		if (a.base[item + 1] == base)
			return;
	} else if (be <= bb) {
		if (lane == 0) a.base[item] = 0;
		return;
	}
	const int P = 1 << a.ps, C = P >> 6;            // C: cells per lane, 16 / 32 / 64
	double *acc = spgemm_lds + (size_t) w * (P + (P >> 3));
	unsigned char *seen = (unsigned char *) (acc + P);
	for (int x = 0; x < C; x += 16)
		*(uint4 *) (seen + lane * C + x) = make_uint4(0, 0, 0, 0);
	spgemm_wave_order();

	const int64_t r0 = q << a.ps;
	const int32_t *__restrict__ pt0 = a.pt + q * a.ninner, *__restrict__ pt1 = pt0 + a.ninner;
	const TA *__restrict__ av = (const TA *) a.a_val;
	const TB *__restrict__ bv = (const TB *) a.b_val;
	for (int64_t c0 = bb; c0 < be; c0 += 64) {
		// the metadata of 64 pairs, one per lane
		int64_t xb = 0;
		int len = 0;
		double b = 0.0;
		if (c0 + lane < be) {
			const int64_t j = a.b_idx[c0 + lane];
			b = svt_rule_as_double(bv[c0 + lane]);
			if ((uint64_t) j < (uint64_t) a.ninner) {
				const int lo = pt0[j], hi = pt1[j];
				xb = a.a_ptr[j] + lo;
				len = hi - lo;
			}
		}
		const int np = (int) (be - c0 < 64 ? be - c0 : 64);
		for (int t0 = 0; t0 < np; t0 += SPGEMM_U) {
			int64_t pxb[SPGEMM_U];
			int plen[SPGEMM_U], r[SPGEMM_U];
			double pb[SPGEMM_U], v[SPGEMM_U];
#pragma unroll
			for (int u = 0; u < SPGEMM_U; u++) {        // (t0 + u <= 63; the lanes past np hold len == 0)
				pxb[u] = __shfl(xb, t0 + u, 64);
				plen[u] = __shfl(len, t0 + u, 64);
				pb[u] = __shfl(b, t0 + u, 64);
				r[u] = -1; v[u] = 0.0;
				if (lane < plen[u]) {
					r[u] = (int) ((int64_t) a.a_idx[pxb[u] + lane] - r0);
					v[u] = svt_rule_as_double(av[pxb[u] + lane]);
				}
			}
#pragma unroll
			for (int u = 0; u < SPGEMM_U; u++) {        // pair after pair: ascending j
				if (lane < plen[u])
					spgemm_add(acc, seen, r[u], P, v[u] * pb[u]);
				for (int x = 64; x < plen[u]; x += 64)      // (plen is the same in every lane)
					if (x + lane < plen[u]) {
						const int rr = (int) ((int64_t) a.a_idx[pxb[u] + x + lane] - r0);
						spgemm_add(acc, seen, rr, P, svt_rule_as_double(av[pxb[u] + x + lane]) * pb[u]);
					}
				spgemm_wave_order();
			}
		}
	}

	// the closing look: trip x has lane l at cell x * 64 + l
	int64_t placed = 0;
	for (int x = 0; x < C; x++) {
		const int cell = x * 64 + lane;
		const bool up = seen[cell] != 0;
		if (__ballot(up) == 0)
			continue;
		const double val = up ? acc[cell] : 0.0;
		const bool keep = up && !(val == 0.0);
		const unsigned long long m = __ballot(keep);
		if (FILL && keep) {
			const int64_t pos = base + placed + __popcll(m & ((1ull << lane) - 1ull));
			a.out_row_idx[pos] = (int32_t) (r0 + cell);
			a.out_val[pos] = val;
		}
		placed += __popcll(m);
	}
	if (!FILL && lane == 0) a.base[item] = placed;
}

// out_col_ptr[k] = the base of item k * npan (k == K: the total); the head of the workspace and the caller's flag word
__global__ void __launch_bounds__(256)
spgemm_publish_kernel(const int64_t *__restrict__ base, int64_t K, int64_t npan, int64_t nitems,
		      int64_t *__restrict__ out_col_ptr, int64_t *__restrict__ head, int *__restrict__ not_finite)
{
	for (int64_t k = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; k <= K; k += (int64_t) gridDim.x * blockDim.x)
		out_col_ptr[k] = k == K ? base[nitems] : base[k * npan];
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		head[1] = base[nitems];
		if (not_finite != NULL) *not_finite = *(const int *) head;
	}
}

static SpgemmKernelArgs spgemm_kernel_args(const SpgemmArgs &a, const SpgemmWs &L, char *w)
{
	SpgemmKernelArgs k;
	k.a_ptr = a.a_ptr; k.a_idx = a.a_idx; k.a_val = a.a_val; k.nrow = a.nrow; k.ninner = a.ninner;
	k.b_ptr = a.b_ptr; k.b_idx = a.b_idx; k.b_val = a.b_val;
	k.pt = (const int32_t *) (w + L.table); k.npan = L.npan; k.nitems = L.nitems; k.ps = L.ps;
	k.base = (int64_t *) (w + L.base);
	k.out_row_idx = NULL; k.out_val = NULL;
	return k;
}

template <bool FILL>
static int spgemm_launch(const SpgemmArgs &a, const SpgemmKernelArgs &k, bool dry, hipStream_t s)
{
	const int W = g_spgemm_waves;
	const size_t P = (size_t) 1 << k.ps, lds = (size_t) W * (P * 8 + P);
	const int64_t nblocks = (k.nitems + W - 1) / W;
	if (nblocks >= (int64_t) 2147483647)
		return svt_set_unsupported("sparse x sparse product with a sparse result: too many (column, row panel) items for one launch");
#define SPGEMM_GO(TA, TB) do { \
		static size_t granted = 0;                  /* (per instantiation: asked once per size) */ \
		if (lds > 64 * 1024 && granted != lds && \
		    hipFuncSetAttribute((const void *) spgemm_kernel<TA, TB, FILL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds) != hipSuccess) { \
			(void) hipGetLastError(); \
			return svt_set_unsupported("sparse x sparse product with a sparse result: %zu bytes of LDS per workgroup are not to be had", lds); \
		} \
		if (lds > 64 * 1024) granted = lds; \
		if (!dry && nblocks > 0) \
			hipLaunchKernelGGL((spgemm_kernel<TA, TB, FILL>), dim3((unsigned) nblocks), dim3(64 * W), lds, s, k); } while (0)
	if (a.a_type == SVT_REALSXP && a.b_type == SVT_REALSXP) SPGEMM_GO(double, double);
	else if (a.a_type == SVT_INTSXP && a.b_type == SVT_INTSXP) SPGEMM_GO(int32_t, int32_t);
	else if (a.a_type == SVT_REALSXP && a.b_type == SVT_INTSXP) SPGEMM_GO(double, int32_t);
	else if (a.a_type == SVT_INTSXP && a.b_type == SVT_REALSXP) SPGEMM_GO(int32_t, double);
	else return svt_set_error("sparse x sparse product with a sparse result: unsupported operand types");
#undef SPGEMM_GO
	return 0;
}

// What can refuse the launch, before anything is written: the operand types, the grid, the LDS request.
int spgemm_check(const SpgemmArgs &a)
{
	const SpgemmWs L = spgemm_ws(a.nrow, a.ninner, a.K);
	SpgemmKernelArgs k;
	memset(&k, 0, sizeof(k));
	k.nitems = L.nitems; k.ps = L.ps;
	return spgemm_launch<false>(a, k, true, NULL) || spgemm_launch<true>(a, k, true, NULL);
}

int launch_spgemm_count(const SpgemmArgs &a, int64_t a_nnz, int64_t b_nnz, int64_t *out_col_ptr, int *not_finite, void *ws,
			hipStream_t s)
{
	const SpgemmWs L = spgemm_ws(a.nrow, a.ninner, a.K);
	char *w = (char *) ws;
	int *flag = (int *) w;
	const SpgemmKernelArgs k = spgemm_kernel_args(a, L, w);
	HIP_TRY(hipMemsetAsync(w, 0, 16, s));
	HIP_TRY(hipMemsetAsync(k.base + L.nitems, 0, 8, s));
	// the table of run bounds, with a look at every value of A on the way (or in a pass of its own)
	if (L.npan > 0 && a.ninner > 0 &&
	    !launch_rowpanel_table_scan(a.a_ptr, a.a_idx, a.a_val, a.a_type, a.ninner, a_nnz, L.npan, L.ps, (int32_t *) (w + L.table),
					NULL, flag, s))
		spgemm_scan_values(a.a_val, a.a_type, a_nnz, flag, s);
	spgemm_scan_values(a.b_val, a.b_type, b_nnz, flag, s);
	if (L.nitems > 0) {
		if (spgemm_launch<false>(a, k, false, s))
			return -1;
		if (launch_exclusive_scan_i64(k.base, L.nitems + 1, w + L.scan, s))
			return -1;
	}
	const int64_t K = a.K > 0 ? a.K : 0;
	int64_t nb = (K + 1 + 255) / 256;
	if (nb > 1024) nb = 1024;
	hipLaunchKernelGGL(spgemm_publish_kernel, dim3((unsigned) nb), dim3(256), 0, s, (const int64_t *) k.base, K, L.npan, L.nitems,
			   out_col_ptr, (int64_t *) w, not_finite);
	HIP_TRY(hipGetLastError());
	return 0;
}

int launch_spgemm_fill(const SpgemmArgs &a, int32_t *out_row_idx, double *out_val, const void *ws, hipStream_t s)
{
	const SpgemmWs L = spgemm_ws(a.nrow, a.ninner, a.K);
	if (L.nitems <= 0)
		return 0;
	SpgemmKernelArgs k = spgemm_kernel_args(a, L, (char *) ws);
	k.out_row_idx = out_row_idx; k.out_val = out_val;
	if (spgemm_launch<true>(a, k, false, s))
		return -1;
	HIP_TRY(hipGetLastError());
	return 0;
}
