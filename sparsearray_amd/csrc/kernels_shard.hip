// Kernels of the sharded host entry points (svt_hip.cpp, svt_set_devices): the fixed-order sum of the
// reduce-scatter that assembles crossprod(A, Y) from the row shards' partial results, and the rebase of a row
// block's offsets after its upload.
#include "svt_common.h"

// out[i] = ((p_0[i] + p_1[i]) + p_2[i]) + ... + p_{nparts-1}[i], part t at parts + t * stride.  One order for every
// cell, no atomics: the result depends on the number of parts and on what each holds, never on timing.  Two
// doubles per lane (16-byte loads and stores); stride is even and the buffers come from hipMalloc, so every
// part is 16-byte aligned.  Each partial is read once.
__global__ void shard_sum_kernel(const double *__restrict__ parts, int nparts, int64_t stride, int64_t n,
				 double *__restrict__ out)
{
	const int64_t npair = n >> 1;
	const int64_t step = (int64_t) gridDim.x * blockDim.x;
	for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < npair; i += step) {
		double2 acc = ((const double2 *) parts)[i];
		for (int t = 1; t < nparts; t++) {
			const double2 v = ((const double2 *) (parts + (int64_t) t * stride))[i];
			acc.x += v.x;
			acc.y += v.y;
		}
		((double2 *) out)[i] = acc;
	}
	if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
		double acc = parts[n - 1];
		for (int t = 1; t < nparts; t++) acc += parts[(int64_t) t * stride + n - 1];
		out[n - 1] = acc;
	}
}

int launch_shard_sum(const double *parts, int nparts, int64_t stride, int64_t n, double *out, hipStream_t s)
{
	if (n <= 0) return 0;
	if (nparts < 1 || (stride & 1) || stride < n)
		return svt_set_error("launch_shard_sum: bad part layout");
	const int64_t npair = n >> 1;
	int64_t blocks = (npair + 255) / 256;
	if (blocks < 1) blocks = 1;
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(shard_sum_kernel, dim3((unsigned) blocks), dim3(256), 0, s, parts, nparts, stride, n, out);
	HIP_TRY(hipGetLastError());
	return 0;
}

// idx[k] -= base: the offsets of a row block [r0, r1) uploaded as they are, rebased to 0.  Four offsets per lane
// (16-byte accesses; hipMalloc'd buffer), the n % 4 tail by the first lanes.
__global__ void rebase_rows_kernel(int32_t *__restrict__ idx, int64_t n, int32_t base)
{
	const int64_t nq = n >> 2;
	const int64_t step = (int64_t) gridDim.x * blockDim.x;
	const int64_t t0 = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
	for (int64_t i = t0; i < nq; i += step) {
		int4 v = ((int4 *) idx)[i];
		v.x -= base; v.y -= base; v.z -= base; v.w -= base;
		((int4 *) idx)[i] = v;
	}
	if (t0 < (n & 3))
		idx[(nq << 2) + t0] -= base;
}

int launch_rebase_rows(int32_t *idx, int64_t n, int32_t base, hipStream_t s)
{
	if (n <= 0 || base == 0) return 0;
	int64_t blocks = ((n >> 2) + 255) / 256;
	if (blocks < 1) blocks = 1;
	if (blocks > 4096) blocks = 4096;
	hipLaunchKernelGGL(rebase_rows_kernel, dim3((unsigned) blocks), dim3(256), 0, s, idx, n, base);
	HIP_TRY(hipGetLastError());
	return 0;
}
