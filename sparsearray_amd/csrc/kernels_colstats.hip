// col* matrixStats and whole-array summarization on the CSC device layout.
//
// Reference: C_colStats_SVT / REC_colStats_SVT (src/SparseArray_matrixStats.c:
// 200-284) call _summarize_SVT() (src/SparseArray_summarization.c:89-109) once
// per "generalized column".  On the device a generalized column is a run of
// `inner` consecutive leaves, i.e. one contiguous slice of val[]; the op is a
// streaming segmented reduction over that slice (row_idx is never read).
//
// Six launch forms (colstats_route, svt_common.h) in three kernel families:
//   colstats_kernel<T, NT, CAP>, NT lanes per segment
//     NT = 16  : 16 segments per 256-thread workgroup
//                (short leaves: config 1 / config 5, ~100 nz per leaf)
//     NT = 64  : one wavefront per segment, 4 segments per workgroup
//     NT = 256 : one workgroup per segment (long leaves: config 2, ~1e4 nz),
//                register-cached (CAP = 48) or streaming (CAP = 0)
//   colstats_thread_kernel : one thread per segment (fewer than ~4 nz each)
//   colstats_chunk_kernel + colstats_combine_kernel : few very long segments,
//                cut into chunks (launch_colstats_split)
// All of them share one statement of each rule: colstats_step1 / colstats_step2
// (what a value does to the state in pass 1 / to the centred sum in pass 2),
// colstats_center and colstats_final (the post-processing).
//
// Sequential NA/NaN rules of src/Rvector_summarization.c:177-734 restated as
// order-independent predicates (valid because every rule is of the form "any
// NA anywhere wins, else any NaN wins, else the plain IEEE reduction"):
//   flags & F_NA   some value is R's NA (payload 1954 / INT_MIN)
//   flags & F_NAN  some value is a NaN that is not NA
// Roofline: HBM; algorithmic bytes = 8 (f64) or 4 (i32) per nonzero.
#include "svt_common.h"

#define F_NA    1
#define F_NAN   2
#define F_TRUE  4   // a non-NA value != 0
#define F_ZERO  8   // a stored value == 0 (not expected in a valid SVT)
#define F_HAVE 16   // at least one non-NA value went into min/max

// One value per lane -> f over the NT lanes of a segment, in every lane of it.  The order is fixed, so results are
// bit-reproducible:
//   NT = 16  : xor butterflies, which stay inside the aligned 16-lane group
//   NT = 64  : the __shfl_down ladder, then lane 0 broadcast
//   NT = 256 : the ladder, lane 0 of each wavefront to sm[w], then f(... f(f(init, sm[0]), sm[1]) ..., sm[3])
// `init` is the identity of f and the serial pass starts from it, not from sm[0]: 0.0 + (-0.0) is +0.0, the sign a
// workgroup's sum of negative zeros has always had.  (+-Inf under min / max gives back sm[0] itself, which is never NaN.)
template <int NT, typename V, typename F>
__device__ __forceinline__ V red(V v, double *sm, const V init, F f)
{
	if (NT == 16) {
#pragma unroll
		for (int m = 8; m >= 1; m >>= 1) v = f(v, __shfl_xor(v, m, SVT_WAVE));
		return v;
	}
	for (int o = 32; o > 0; o >>= 1) v = f(v, __shfl_down(v, o, SVT_WAVE));   // valid in lane 0
	if (NT == SVT_WAVE)
		return __shfl(v, 0, SVT_WAVE);
	V *s = (V *) sm;
	const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
	__syncthreads();
	if (l == 0) s[w] = v;
	__syncthreads();
	V t = init;
	for (int i = 0; i < NT / SVT_WAVE; i++) t = f(t, s[i]);
	return t;
}
template <int NT>
__device__ __forceinline__ double red_sum(double v, double *sm)
{
	return red<NT>(v, sm, 0.0, [](double a, double b) { return a + b; });
}

template <typename T> struct ValTraits;
template <> struct ValTraits<double> {
	static __device__ inline bool is_missing(double v) { return v != v; }
	static __device__ inline bool is_na(double v) { return svt_is_na(v); }
	static __device__ inline double as_double(double v) { return v; }
};
template <> struct ValTraits<int> {
	static __device__ inline bool is_missing(int v) { return v == NA_INT; }
	static __device__ inline bool is_na(int v) { return v == NA_INT; }
	static __device__ inline double as_double(int v) { return (double) v; }
};

// What pass 1 leaves of a segment, a chunk of one or one lane's share
struct ColState {
	int flags;
	int pad;
	long long nacnt;
	double acc;       // sum or product
	double mm;        // extremum
};

__host__ __device__ inline bool colstats_two_pass(int oc)
{
	return oc == SVT_OP_CENTERED_X2_SUM || oc == SVT_OP_VAR1 || oc == SVT_OP_SD1;
}

__device__ __forceinline__ ColState colstats_init(const int oc)
{
	ColState st;
	st.flags = 0; st.pad = 0; st.nacnt = 0;
	st.acc = (oc == SVT_OP_PROD) ? 1.0 : 0.0;
	st.mm = (oc == SVT_OP_MIN) ? INFINITY : -INFINITY;
	return st;
}

// ---- pass 1 of one value: flags, NA count, sum / product / extremum --------
template <typename T>
__device__ __forceinline__ void colstats_step1(ColState &st, const T v, const int oc, const bool narm)
{
	typedef ValTraits<T> VT;
	if (VT::is_missing(v)) {
		st.nacnt++;
		st.flags |= VT::is_na(v) ? F_NA : F_NAN;
		// na.rm = FALSE: NaN/NA of doubles take part in the IEEE reduction
		// (ints: the value is never used once F_NA is set)
		if (narm || sizeof(T) != 8)
			return;
	} else {
		st.flags |= (v != (T) 0) ? F_TRUE : F_ZERO;
		st.flags |= F_HAVE;
	}
	const double d = VT::as_double(v);
	const bool is_min = oc == SVT_OP_MIN, is_minmax = is_min | (oc == SVT_OP_MAX);
	if (oc == SVT_OP_PROD) st.acc *= d;
	else if (is_minmax) { if (d == d) st.mm = is_min ? (d < st.mm ? d : st.mm) : (d > st.mm ? d : st.mm); }
	else st.acc += d;
}

// ---- pass 2 of one value: the centred square, missing values as in pass 1 --
template <typename T>
__device__ __forceinline__ void colstats_step2(double &acc2, const T v, const double c, const bool narm)
{
	typedef ValTraits<T> VT;
	if (VT::is_missing(v) && (narm || sizeof(T) != 8))
		return;
	const double d = VT::as_double(v) - c;
	acc2 += d * d;
}

// the lanes' states -> the state of their segment (or chunk), in every lane
template <int NT>
__device__ __forceinline__ void colstats_reduce(ColState &st, const int oc, double *sm)
{
	st.flags = red<NT>(st.flags, sm, 0, [](int a, int b) { return a | b; });
	st.nacnt = red<NT>(st.nacnt, sm, 0LL, [](long long a, long long b) { return a + b; });
	const bool is_min = oc == SVT_OP_MIN, is_minmax = is_min | (oc == SVT_OP_MAX);
	if (oc == SVT_OP_PROD)
		st.acc = red<NT>(st.acc, sm, 1.0, [](double a, double b) { return a * b; });
	else if (is_minmax)
		st.mm = is_min ? red<NT>(st.mm, sm, (double) INFINITY, [](double a, double b) { return b < a ? b : a; })
			       : red<NT>(st.mm, sm, (double) -INFINITY, [](double a, double b) { return b > a ? b : a; });
	else
		st.acc = red_sum<NT>(st.acc, sm);
}

// The effective count and the breaking NA need only flags and nacnt.  A kernel takes both once per segment, in every
// lane, and hands them to colstats_center and colstats_final: n_eff is then ready before the sum it divides is reduced.
//
// effective count: na.rm takes the missing values out, and an NaArray's implicit NAs with them
__device__ __forceinline__ double colstats_neff(const StatsArgs &a, const ColState &st, int64_t nz)
{
	const bool narm = a.na_rm != 0, nabg = a.na_bg != 0;
	return narm ? (double) ((nabg ? nz : a.seg_len) - st.nacnt) : (double) a.seg_len;
}

// "breaking value" NA: a stored NA, or an implicit one of an NaArray, without na.rm
__device__ __forceinline__ bool colstats_brk(const StatsArgs &a, const ColState &st, int64_t nz)
{
	int flags = st.flags;
	if (a.na_bg && a.seg_len - nz > 0 && !a.na_rm) flags |= F_NA;
	return (flags & F_NA) && !a.na_rm;
}

// centre used by the two-pass ops.  src/SparseArray_summarization.c:70-109: without a center the mean comes from a
// first full pass (acc = st.acc)
__device__ __forceinline__ double colstats_center(const StatsArgs &a, double acc, bool brk_na, double n_eff)
{
	double c = a.center;
	if (c != c)
		c = (brk_na && !a.dgc) ? svt_na_real() : acc / n_eff;
	return c;
}

// The post-processing of _postprocess_SummarizeResult (Rvector_summarization.c:1078-1177) for segment g: result and
// warn word.  One lane per segment calls it.
__device__ __forceinline__ void colstats_final(const StatsArgs &a, int64_t g, const ColState &st, int64_t nz,
					       bool brk_na, double n_eff, double c, double acc2, bool is_dbl)
{
	const int oc = a.opcode;
	const bool narm = a.na_rm != 0, nabg = a.na_bg != 0;
	// NaArray (a.na_bg): the zerocount implicit values are NAs -- they count as
	// NAs, one NA is fed to the op unless na.rm, and no implicit zero takes part
	// (Rvector_summarization.c:1086-1106)
	const int64_t zerocount = a.seg_len - nz;
	const int64_t implicit_na = nabg ? zerocount : 0;
	const int64_t zeros = nabg ? 0 : zerocount;            // implicit zeros
	const int flags = st.flags;
	const double NAr = svt_na_real();
	const bool is_minmax = oc == SVT_OP_MIN || oc == SVT_OP_MAX, is_min = oc == SVT_OP_MIN;
	double rd = 0.0, mm = st.mm;
	int ri = 0, warn = 0;
	switch (oc) {
	case SVT_OP_ANYNA:
		ri = ((flags & (F_NA | F_NAN)) || implicit_na > 0) ? 1 : 0;
		break;
	case SVT_OP_COUNTNAS:
		rd = (double) (st.nacnt + implicit_na);
		break;
	case SVT_OP_ANY:      // src/Rvector_summarization.c:260-284
		ri = (flags & F_TRUE) ? 1 : (brk_na ? NA_INT : 0);
		break;
	case SVT_OP_ALL:      // :289-313 plus the implicit zero of :1100-1106
		ri = ((flags & F_ZERO) || zeros > 0) ? 0 : (brk_na ? NA_INT : 1);
		break;
	case SVT_OP_SUM:
		rd = brk_na ? NAr : st.acc;
		break;
	case SVT_OP_MEAN:
		rd = brk_na ? NAr : st.acc / n_eff;
		break;
	case SVT_OP_PROD:
		rd = brk_na ? NAr : (zeros > 0 ? st.acc * 0.0 : st.acc);
		break;
	case SVT_OP_MIN: case SVT_OP_MAX:
		if (is_dbl) {
			if (brk_na) { rd = NAr; break; }
			if ((flags & F_NAN) && !narm) { rd = NAN; break; }
			if (zeros > 0) mm = is_min ? (0.0 < mm ? 0.0 : mm) : (0.0 > mm ? 0.0 : mm);
			rd = mm;
		} else {
			if (brk_na) { ri = NA_INT; break; }
			bool have = (flags & F_HAVE) != 0;
			if (zeros > 0) {
				mm = have ? (is_min ? (0.0 < mm ? 0.0 : mm) : (0.0 > mm ? 0.0 : mm)) : 0.0;
				have = true;
			}
			if (!have) { ri = NA_INT; warn = 1; }   // :1108-1128
			else ri = (int) mm;
		}
		break;
	case SVT_OP_CENTERED_X2_SUM: case SVT_OP_VAR1: case SVT_OP_SD1:
		if (a.dgc) {      // col_var(), src/sparseMatrix_utils.c:190-203: IEEE all the way
			rd = (c * c * (double) zeros + acc2) / (n_eff - 1.0);
			break;
		}
		if (brk_na) { rd = NAr; break; }
		rd = acc2 + c * c * (double) zeros;
		if (oc == SVT_OP_CENTERED_X2_SUM) break;
		if (n_eff <= 1.0) { rd = NAr; break; }
		rd /= (n_eff - 1.0);
		if (oc == SVT_OP_SD1) rd = sqrt(rd);
		break;
	default:
		break;
	}
	const bool out_is_int = oc == SVT_OP_ANYNA || oc == SVT_OP_ANY || oc == SVT_OP_ALL ||
		(is_minmax && !is_dbl);
	if (out_is_int) ((int *) a.out)[g] = ri;
	else ((double *) a.out)[g] = rd;
	if (warn && a.warn_flag) *a.warn_flag = 1;
}

// CAP > 0: the first pass keeps the
// column in registers (CAP values per thread, all loads in flight at once) and
// the centred second pass runs from there instead of re-reading it -- the
// two-pass arithmetic of the reference (src/SparseArray_summarization.c:70-109)
// with one trip to memory.  Columns longer than NT*CAP take the re-read path.
template <typename T, int NT, int CAP>
__global__ void __launch_bounds__(256)
colstats_kernel(StatsArgs a)
{
	__shared__ double sm[256 / SVT_WAVE];   // red<256>: one slot per wavefront
	const int per_block = 256 / NT;
	const int sub = NT == 256 ? 0 : (NT == 16 ? (threadIdx.x >> 4) : (threadIdx.x >> 6));
	const int tid = NT == 256 ? threadIdx.x : (threadIdx.x & (NT - 1));
	const int64_t g = (int64_t) blockIdx.x * per_block + sub;
	if (NT <= SVT_WAVE && g >= a.nseg)
		return;   // whole wave / 16-lane group exits together; no barriers on this path
	const T *__restrict__ val = (const T *) a.val;
	const int64_t beg = a.col_ptr[g * a.inner];
	const int64_t end = a.col_ptr[(g + 1) * a.inner];
	const int64_t nz = end - beg;
	const int oc = a.opcode;
	const bool narm = a.na_rm != 0;

	ColState st = colstats_init(oc);
	T cache[CAP > 0 ? CAP : 1];
	const bool cached = CAP > 0 && nz <= (int64_t) NT * CAP;   // uniform per column
	if (cached) {
#pragma unroll
		for (int i = 0; i < CAP; i++) {
			const int64_t k = beg + tid + (int64_t) i * NT;
			cache[i] = k < end ? val[k] : (T) 0;
		}
#pragma unroll
		for (int i = 0; i < CAP; i++)
			if (beg + tid + (int64_t) i * NT < end) colstats_step1(st, cache[i], oc, narm);
	} else {
		for (int64_t k = beg + tid; k < end; k += NT)
			colstats_step1(st, val[k], oc, narm);
	}
	colstats_reduce<NT>(st, oc, sm);
	const bool brk_na = colstats_brk(a, st, nz);
	const double n_eff = colstats_neff(a, st, nz);

	double c = 0.0, acc2 = 0.0;
	if (colstats_two_pass(oc)) {
		c = colstats_center(a, st.acc, brk_na, n_eff);
		if (cached) {
#pragma unroll
			for (int i = 0; i < CAP; i++)
				if (beg + tid + (int64_t) i * NT < end) colstats_step2(acc2, cache[i], c, narm);
		} else {
			for (int64_t k = beg + tid; k < end; k += NT)
				colstats_step2(acc2, val[k], c, narm);
		}
		acc2 = red_sum<NT>(acc2, sm);
	}
	if (tid == 0)
		colstats_final(a, g, st, nz, brk_na, n_eff, c, acc2, sizeof(T) == 8);
}

// --------------------------------------------------------------------------
// Few, very long segments (whole-array sum(), colSums(dims = ndim - 1) of a 3-d
// array, ...): one workgroup per segment would leave the chip idle, so every
// segment is cut into NCHUNK element ranges, one workgroup each, whose partial
// states are combined in chunk order by a small second kernel.  var1 / sd1 /
// centered sums keep the reference's two passes (mean first,
// src/SparseArray_summarization.c:70-109): state + mean, then the centred
// squares, 4 launches.
// --------------------------------------------------------------------------
// one workgroup's walk over its chunk, from k: 8 loads in flight per thread
template <typename T, typename F>
__device__ __forceinline__ void chunk_each(const T *__restrict__ val, int64_t k, const int64_t end, F step)
{
	for (; k + 7 * 256 < end; k += 8 * 256) {
		T v[8];
#pragma unroll
		for (int u = 0; u < 8; u++) v[u] = val[k + u * 256];
#pragma unroll
		for (int u = 0; u < 8; u++) step(v[u]);
	}
	for (; k < end; k += 256) step(val[k]);
}

// PASS 1: state of one chunk;  PASS 2: centred squares of one chunk
template <typename T, int PASS>
__global__ void __launch_bounds__(256)
colstats_chunk_kernel(StatsArgs a, int nchunk, ColState *__restrict__ st, const double *__restrict__ centers,
		      double *__restrict__ acc2_out)
{
	__shared__ double sm[256 / SVT_WAVE];
	const int64_t g = blockIdx.y;
	const int ch = blockIdx.x, tid = threadIdx.x;
	const T *__restrict__ val = (const T *) a.val;
	const int64_t sbeg = a.col_ptr[g * a.inner], send = a.col_ptr[(g + 1) * a.inner];
	const int64_t nz = send - sbeg;
	const int64_t beg = sbeg + nz * ch / nchunk, end = sbeg + nz * (ch + 1) / nchunk;
	const int oc = a.opcode;
	const bool narm = a.na_rm != 0;
	if (PASS == 1) {
		ColState o = colstats_init(oc);
		chunk_each(val, beg + tid, end, [&](const T v) { colstats_step1(o, v, oc, narm); });
		colstats_reduce<256>(o, oc, sm);
		if (tid == 0) st[g * nchunk + ch] = o;
	} else {
		const double c = centers[g];
		double acc2 = 0.0;
		chunk_each(val, beg + tid, end, [&](const T v) { colstats_step2(acc2, v, c, narm); });
		acc2 = red_sum<256>(acc2, sm);
		if (tid == 0) acc2_out[g * nchunk + ch] = acc2;
	}
}

// STAGE 1: combine the chunk states (chunk order); final result, or the centre for
// pass 2.  STAGE 2: combine the centred squares, final result.
template <int STAGE>
__global__ void colstats_combine_kernel(StatsArgs a, int nchunk, ColState *__restrict__ st,
					double *__restrict__ centers, const double *__restrict__ acc2_in,
					int two_pass, int is_dbl)
{
	const int64_t g = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.nseg) return;
	const int64_t nz = a.col_ptr[(g + 1) * a.inner] - a.col_ptr[g * a.inner];
	if (STAGE == 1) {
		const int oc = a.opcode;
		const bool is_min = oc == SVT_OP_MIN;
		ColState t = st[g * nchunk];
		for (int c = 1; c < nchunk; c++) {
			const ColState u = st[g * nchunk + c];
			t.flags |= u.flags;
			t.nacnt += u.nacnt;
			if (oc == SVT_OP_PROD) t.acc *= u.acc; else t.acc += u.acc;
			t.mm = is_min ? (u.mm < t.mm ? u.mm : t.mm) : (u.mm > t.mm ? u.mm : t.mm);
		}
		const bool brk_na = colstats_brk(a, t, nz);
		const double n_eff = colstats_neff(a, t, nz);
		if (two_pass) {
			st[g * nchunk] = t;
			centers[g] = colstats_center(a, t.acc, brk_na, n_eff);
		} else {
			colstats_final(a, g, t, nz, brk_na, n_eff, 0.0, 0.0, is_dbl != 0);
		}
	} else {
		double acc2 = 0.0;
		for (int c = 0; c < nchunk; c++) acc2 += acc2_in[g * nchunk + c];
		const ColState t = st[g * nchunk];
		colstats_final(a, g, t, nz, colstats_brk(a, t, nz), colstats_neff(a, t, nz), centers[g], acc2, is_dbl != 0);
	}
}

// Very short segments (fewer than ~4 nonzeros on average: arrays with a short first extent,
// leaf-shattering permutations): one THREAD per segment, sequential like the reference; what
// it streams is mostly col_ptr.
template <typename T>
__global__ void __launch_bounds__(256)
colstats_thread_kernel(StatsArgs a)
{
	const int64_t g = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.nseg) return;
	const T *__restrict__ val = (const T *) a.val;
	const int64_t beg = a.col_ptr[g * a.inner], end = a.col_ptr[(g + 1) * a.inner];
	const int oc = a.opcode;
	const bool narm = a.na_rm != 0;
	ColState st = colstats_init(oc);
	for (int64_t k = beg; k < end; k++)
		colstats_step1(st, val[k], oc, narm);
	const bool brk_na = colstats_brk(a, st, end - beg);
	const double n_eff = colstats_neff(a, st, end - beg);
	double c = 0.0, acc2 = 0.0;
	if (colstats_two_pass(oc)) {
		c = colstats_center(a, st.acc, brk_na, n_eff);
		for (int64_t k = beg; k < end; k++)
			colstats_step2(acc2, val[k], c, narm);
	}
	colstats_final(a, g, st, end - beg, brk_na, n_eff, c, acc2, sizeof(T) == 8);
}

static int launch_colstats_split(const StatsArgs &a, int nchunk, hipStream_t s)
{
	const bool is_dbl = a.Rtype == SVT_REALSXP;
	const bool two_pass = colstats_two_pass(a.opcode);
	const size_t n = (size_t) a.nseg * nchunk;
	const size_t b_st = (n * sizeof(ColState) + 255) / 256 * 256, b_c = ((size_t) a.nseg * 8 + 255) / 256 * 256;
	char *scr = NULL;
	HIP_TRY(hipMallocAsync((void **) &scr, b_st + b_c + n * 8 + 256, s));   // stream-ordered scratch
	ColState *st = (ColState *) scr;
	double *centers = (double *) (scr + b_st), *acc2 = (double *) (scr + b_st + b_c);
	dim3 grid((unsigned) nchunk, (unsigned) a.nseg), cgrid((unsigned) ((a.nseg + 255) / 256));
	if (is_dbl) hipLaunchKernelGGL((colstats_chunk_kernel<double, 1>), grid, dim3(256), 0, s, a, nchunk, st, centers, acc2);
	else hipLaunchKernelGGL((colstats_chunk_kernel<int, 1>), grid, dim3(256), 0, s, a, nchunk, st, centers, acc2);
	hipLaunchKernelGGL(colstats_combine_kernel<1>, cgrid, dim3(256), 0, s, a, nchunk, st, centers, acc2,
			   (int) two_pass, (int) is_dbl);
	if (two_pass) {
		if (is_dbl) hipLaunchKernelGGL((colstats_chunk_kernel<double, 2>), grid, dim3(256), 0, s, a, nchunk, st, centers, acc2);
		else hipLaunchKernelGGL((colstats_chunk_kernel<int, 2>), grid, dim3(256), 0, s, a, nchunk, st, centers, acc2);
		hipLaunchKernelGGL(colstats_combine_kernel<2>, cgrid, dim3(256), 0, s, a, nchunk, st, centers, acc2,
				   (int) two_pass, (int) is_dbl);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipFreeAsync(scr, s));
	return 0;
}

// The launch form of a shape: decided from the number of generalized columns and their AVERAGE length alone
// (a column far from the average still takes the form of its launch; inside colstats_kernel<T, NT, CAP> it
// then picks the register-cached or the re-read branch by its own length, nz <= NT * CAP).
ColStatsRoute colstats_route(int64_t nseg, int64_t nnz)
{
	ColStatsRoute rt = { COLSTATS_LANES16, 1 };
	if (nseg <= 0)
		return rt;
	const int64_t avg = nnz / nseg;
	if (nseg < 512 && avg >= 65536 && nseg <= 65535) {
		// few long segments: ~1024 workgroups in all, >= 16K elements each
		int64_t nchunk = (1024 + nseg - 1) / nseg;
		if (nchunk > avg / 16384) nchunk = avg / 16384;
		if (nchunk >= 2) {
			rt.form = COLSTATS_SPLIT;
			rt.nchunk = (int) nchunk;
			return rt;
		}
	}
	if (avg >= 1024)                             // (cached: also faster for one-pass ops, all loads in flight)
		rt.form = avg <= 256 * 40 ? COLSTATS_GROUP_CACHED : COLSTATS_GROUP_STREAM;
	else if (avg < 4 && nseg >= 4096)
		rt.form = COLSTATS_THREAD;
	else if (avg < 160)                          // short leaves (config 1 / config 5, ~100 nonzeros)
		rt.form = COLSTATS_LANES16;
	else
		rt.form = COLSTATS_WAVE;
	return rt;
}

template <int NT, int CAP>
static void launch_colstats_form(const StatsArgs &a, hipStream_t s)
{
	const dim3 grid((unsigned) ((a.nseg + 256 / NT - 1) / (256 / NT))), block(256);
	if (a.Rtype == SVT_REALSXP) hipLaunchKernelGGL((colstats_kernel<double, NT, CAP>), grid, block, 0, s, a);
	else hipLaunchKernelGGL((colstats_kernel<int, NT, CAP>), grid, block, 0, s, a);
}

int launch_colstats(const StatsArgs &a, int64_t nnz, hipStream_t s)
{
	if (a.nseg <= 0)
		return 0;
	if (a.nseg > 0x7FFFFFFFLL)
		return svt_set_error("too many generalized columns");
	const ColStatsRoute rt = colstats_route(a.nseg, nnz);
	switch (rt.form) {
	case COLSTATS_SPLIT:
		return launch_colstats_split(a, rt.nchunk, s);
	case COLSTATS_GROUP_CACHED: launch_colstats_form<256, 48>(a, s); break;
	case COLSTATS_GROUP_STREAM: launch_colstats_form<256, 0>(a, s); break;
	case COLSTATS_WAVE: launch_colstats_form<64, 16>(a, s); break;
	case COLSTATS_LANES16: launch_colstats_form<16, 16>(a, s); break;
	case COLSTATS_THREAD: {
		const dim3 gridt((unsigned) ((a.nseg + 255) / 256)), block(256);
		if (a.Rtype == SVT_REALSXP) hipLaunchKernelGGL(colstats_thread_kernel<double>, gridt, block, 0, s, a);
		else hipLaunchKernelGGL(colstats_thread_kernel<int>, gridt, block, 0, s, a);
		break;
	}
	}
	HIP_TRY(hipGetLastError());
	return 0;
}
