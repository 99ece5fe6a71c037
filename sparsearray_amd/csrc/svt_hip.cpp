// Host side of libsvt_hip.so: the C ABI of include/svt_hip.h.
//
// Host-level functions restate the argument checks and dispatch of the
// reference's .Call entry points (file:line at each function), marshal the
// SVT leaves into the CSC device layout (model:
// dump_SVT_to_CsparseMatrix_slots, src/SVT_SparseArray_class.c:598-633),
// launch the kernels and copy the result back.  No arithmetic of the hot path
// happens on the host.
#include "svt_common.h"
#include "svt_arith_rules.h"
#include "svt_coerce_rules.h"
#include <unistd.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <thread>
#include <type_traits>
#include <vector>

static thread_local char g_err[1024];
static int g_device = -1;
static char g_arch[64] = "";

int svt_set_error(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return -1;
}

// "Not supported here" (include/svt_hip.h: status > 0): inside the library it unwinds like an error (-1, with the
// message), and the entry point that hands a status to the caller turns it into 1 (svt_status).  A caller inside
// the library that recovers from it (another route) clears the mark.
static thread_local int g_unsupported = 0;
int svt_set_unsupported(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	g_unsupported = 1;
	return -1;
}
void svt_clear_unsupported(void) { g_unsupported = 0; }
static inline int svt_status(int rc)
{
	return rc < 0 && g_unsupported ? 1 : rc;
}
// The status an entry point hands to its caller: f() run with the mark cleared, a refusal turned into 1.
template <class F> static int abi_status(F f)
{
	g_unsupported = 0;
	return svt_status(f());
}

extern "C" const char *svt_last_error(void) { return g_err; }
extern "C" const char *svt_device_arch(void) { return g_arch; }

static int select_device(int device)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
		return svt_set_error("libsvt_hip: no HIP device visible -- the SVT "
				     "backend has no CPU fallback");
	if (device < 0 || device >= n)
		return svt_set_error("libsvt_hip: device %d out of range (0..%d)",
				     device, n - 1);
	HIP_TRY(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIP_TRY(hipGetDeviceProperties(&prop, device));
	snprintf(g_arch, sizeof(g_arch), "%s", prop.gcnArchName);
	if (strncmp(g_arch, "gfx950", 6) != 0)
		return svt_set_error("libsvt_hip: device %d is %s; this library "
				     "carries gfx950 (MI355X) code only", device, g_arch);
	g_device = device;
	return 0;
}

// ---- the device list of the host-level entry points (svt_set_devices) --------------------------------
// One entry (what svt_init() sets): every entry point runs on that device, as it always did.  More entries:
// the four sharded entry points split their operand over them, one host thread per entry (repeated ordinals
// are separate shards on one device); the others run on the first entry.
#define SVT_MAX_SHARDS 16
static std::vector<int> g_devices;             // empty until svt_init()
static int g_init_device = -1;                 // device of the last svt_init()
// Operands with fewer nonzeros stay on the first device.  A guess, not a measurement: no run on more than one
// physical device exists yet; below ~1.6e7 nonzeros the upload of one shard is a few ms over one PCIe link.
static int64_t g_shard_min_nnz = (int64_t) 1 << 24;

extern "C" int svt_init(int device)
{
	if (select_device(device))
		return -1;
	g_devices.assign(1, device);
	g_init_device = device;
	return 0;
}

extern "C" int svt_set_devices(const int *ordinals, int n)
{
	if (n == 0)
		return svt_init(g_init_device >= 0 ? g_init_device : 0);
	if (n < 0 || n > SVT_MAX_SHARDS || ordinals == NULL)
		return svt_set_error("svt_set_devices: between 1 and %d devices", SVT_MAX_SHARDS);
	int cnt = 0;
	if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
		return svt_set_error("libsvt_hip: no HIP device visible -- the SVT "
				     "backend has no CPU fallback");
	for (int i = 0; i < n; i++) {
		const int d = ordinals[i];
		if (d < 0 || d >= cnt)
			return svt_set_error("svt_set_devices: device %d out of range (0..%d)", d, cnt - 1);
		hipDeviceProp_t prop;
		HIP_TRY(hipGetDeviceProperties(&prop, d));
		if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
			return svt_set_error("svt_set_devices: device %d is %s; this library "
					     "carries gfx950 (MI355X) code only", d, prop.gcnArchName);
	}
	// peer access between distinct ordinals (the reduce-scatter's copies); a pair without it still copies,
	// through the runtime
	std::vector<int> distinct;
	for (int i = 0; i < n; i++)
		if (std::find(distinct.begin(), distinct.end(), ordinals[i]) == distinct.end())
			distinct.push_back(ordinals[i]);
	for (int a : distinct)
		for (int b : distinct) {
			int ok = 0;
			if (a == b || hipDeviceCanAccessPeer(&ok, a, b) != hipSuccess || !ok) continue;
			if (hipSetDevice(a) == hipSuccess && hipDeviceEnablePeerAccess(b, 0) != hipSuccess)
				(void) hipGetLastError();        // hipErrorPeerAccessAlreadyEnabled among them
		}
	if (select_device(ordinals[0])) {
		if (g_device >= 0) (void) hipSetDevice(g_device);
		return -1;
	}
	g_devices.assign(ordinals, ordinals + n);
	return 0;
}

extern "C" int svt_get_devices(int *ordinals, int cap)
{
	const int n = (int) g_devices.size();
	for (int i = 0; i < n && i < cap; i++)
		if (ordinals) ordinals[i] = g_devices[(size_t) i];
	return n;
}

extern "C" void svt_set_shard_min_nnz(int64_t nnz)
{
	g_shard_min_nnz = nnz > 0 ? nnz : 0;
}

// The shard a worker thread of a sharded call runs (NULL on every other thread): its slot, the number of
// shards, its device.  Stager, marshalling team and helper threads follow it.
struct ShardCtx {
	int slot, nshard, device;
};
static thread_local const ShardCtx *t_shard = NULL;

static int cur_device() { return t_shard ? t_shard->device : g_device; }

// ---- thread control (src/thread_control.c:47-66) ---------------------------------
static int g_max_threads = 0;
extern "C" int svt_get_num_procs(void)
{
	const long n = sysconf(_SC_NPROCESSORS_ONLN);
	return n > 0 ? (int) n : 0;
}
extern "C" int svt_get_max_threads(void)
{
	return g_max_threads > 0 ? g_max_threads : svt_get_num_procs();
}
extern "C" int svt_set_max_threads(int nthread)
{
	const int prev = svt_get_max_threads();
	if (nthread > 0) g_max_threads = nthread;
	return prev;
}

static int ensure_init()
{
	if (g_device >= 0)
		return 0;
	return svt_init(0);
}

// ---- host -> device staging ----------------------------------------------------------
// .Call hands over pageable host memory.  hipMemcpy() from pageable memory runs at a
// few GB/s; instead the bytes go through two pinned buffers: a small thread team
// gathers the next chunk (for an SVT: the leaves' nzoffs / nzvals, scattered over
// the R heap) into one buffer while the previous one is in flight on a copy stream
// (the reference's counterpart is the leaf walk of
// src/SVT_SparseArray_class.c:598-633, which never leaves the host).
struct Stager {
	static const size_t CHUNK = (size_t) 48 << 20;      // bytes per pinned buffer
	size_t chunk = CHUNK;                                // (a shard's stager: CHUNK / number of shards)
	int dev = -1;                                        // device of `stream` (shard stagers)
	char *buf[2] = {NULL, NULL};
	hipEvent_t done[2];
	hipStream_t stream = NULL;
	bool ok = false;
	int next = 0;
	bool busy[2] = {false, false};

	int init()
	{
		if (ok) return 0;
		for (int i = 0; i < 2; i++) {
			HIP_TRY(hipHostMalloc((void **) &buf[i], chunk, hipHostMallocDefault));
			HIP_TRY(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
		}
		HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
		ok = true;
		return 0;
	}
	// a free pinned buffer (waits for the copy that last used it)
	int acquire(char **p, int *slot)
	{
		if (init()) return -1;
		const int i = next;
		next ^= 1;
		if (busy[i]) { HIP_TRY(hipEventSynchronize(done[i])); busy[i] = false; }
		*p = buf[i]; *slot = i;
		return 0;
	}
	int send(int slot, void *dst, size_t off_in_buf, size_t n)
	{
		if (n) HIP_TRY(hipMemcpyAsync(dst, buf[slot] + off_in_buf, n, hipMemcpyHostToDevice, stream));
		return 0;
	}
	int commit(int slot)
	{
		HIP_TRY(hipEventRecord(done[slot], stream));
		busy[slot] = true;
		return 0;
	}
	int drain()
	{
		if (!ok) return 0;
		HIP_TRY(hipStreamSynchronize(stream));
		busy[0] = busy[1] = false;
		return 0;
	}
	// a shard stager: buffers of `bytes` on device `d` -- kept from call to call, rebuilt when either changes
	void use(size_t bytes, int d)
	{
		if (ok && (bytes != chunk || d != dev)) {
			(void) hipStreamSynchronize(stream);
			(void) hipStreamDestroy(stream);
			for (int i = 0; i < 2; i++) {
				(void) hipEventDestroy(done[i]);
				(void) hipHostFree(buf[i]);
				buf[i] = NULL;
			}
			ok = false;
			next = 0;
			busy[0] = busy[1] = false;
		}
		chunk = bytes;
		dev = d;
	}
};
// The one-device path stages through g_stager (2 x 48 MB pinned).  Shard s of a sharded call stages through
// g_shard_stager[s], whose two buffers hold 48 MB / N each: 96 MB pinned for all shards together whatever N
// (2 x 6 MB per shard at N = 8), next to the 96 MB of g_stager.
static Stager g_stager;
static Stager g_shard_stager[SVT_MAX_SHARDS];
static Stager &cur_stager() { return t_shard ? g_shard_stager[t_shard->slot] : g_stager; }

// Bytes of a pinned buffer used per trip.  SVT_STAGING_CHUNK (bytes, read once) lowers it so
// that a test can drive the multi-chunk paths -- a leaf longer than a chunk among them --
// with small inputs.
static size_t g_stager_chunk()
{
	static size_t v = 0;
	if (v == 0) {
		v = Stager::CHUNK;
		const char *e = getenv("SVT_STAGING_CHUNK");
		if (e != NULL) {
			const long long t = atoll(e);
			if (t >= 4096 && (size_t) t < Stager::CHUNK) v = (size_t) t / 4096 * 4096;
		}
	}
	return v < cur_stager().chunk ? v : cur_stager().chunk;
}

// run fn(t, nt) on a small team (the calling thread is one of them)
static void team_run(int nt, const std::function<void(int, int)> &fn)
{
	std::vector<std::thread> th;
	for (int t = 1; t < nt; t++) th.emplace_back(fn, t, nt);
	fn(0, nt);
	for (auto &x : th) x.join();
}

static int team_size(size_t bytes)
{
	int nt = svt_get_max_threads();
	if (t_shard) nt /= t_shard->nshard;                 // the shards' teams share the caller's thread count
	if (nt > 8) nt = 8;
	if (bytes < ((size_t) 4 << 20) || nt < 1) nt = 1;
	return nt;
}

// contiguous host array -> device, through the pinned buffers
static int staged_copy(void *dst, const void *src, size_t n)
{
	if (n < ((size_t) 1 << 20)) {
		if (n) HIP_TRY(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
		return 0;
	}
	Stager &st = cur_stager();
	for (size_t off = 0; off < n; off += st.chunk) {
		const size_t len = n - off < st.chunk ? n - off : st.chunk;
		char *b; int slot;
		if (st.acquire(&b, &slot)) return -1;
		const char *s0 = (const char *) src + off;
		team_run(team_size(len), [&](int t, int nt) {
			const size_t a = len * t / nt, e = len * (t + 1) / nt;
			memcpy(b + a, s0 + a, e - a);
		});
		if (st.send(slot, (char *) dst + off, 0, len) || st.commit(slot)) return -1;
	}
	return st.drain();
}

// ncols runs of `run` bytes, `ld` bytes apart on the host (rows [r0, r1) of a column-major matrix), -> one
// contiguous device array, through the pinned buffers
static int staged_copy_2d(void *dst, const void *src, size_t run, size_t ncols, size_t ld)
{
	if (run == ld || ncols <= 1)
		return staged_copy(dst, src, run * ncols);
	const size_t n = run * ncols;
	Stager &st = cur_stager();
	for (size_t off = 0; off < n; off += st.chunk) {
		const size_t len = n - off < st.chunk ? n - off : st.chunk;
		char *b; int slot;
		if (st.acquire(&b, &slot)) return -1;
		team_run(team_size(len), [&](int t, int nt) {
			size_t a = off + len * t / nt;
			const size_t e = off + len * (t + 1) / nt;
			while (a < e) {                     // piece of column a / run
				const size_t c = a / run, in = a - c * run;
				const size_t m = std::min(run - in, e - a);
				memcpy(b + (a - off), (const char *) src + c * ld + in, m);
				a += m;
			}
		});
		if (st.send(slot, (char *) dst + off, 0, len) || st.commit(slot)) return -1;
	}
	return st.drain();
}

// device -> contiguous host array: D2H into one pinned buffer while the thread team
// copies the previous chunk out of the other (results can be large: the 1e6 x 128
// product of BASELINE config 3 is 1 GB)
static int staged_download(void *dst, const void *src, size_t n)
{
	if (n < ((size_t) 4 << 20)) {
		if (n) HIP_TRY(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
		return 0;
	}
	Stager &st = cur_stager();
	if (st.init() || st.drain()) return -1;
	HIP_TRY(hipDeviceSynchronize());            // the producer kernels ran on other streams
	const size_t C = st.chunk;
	const size_t nchunk = (n + C - 1) / C;
	for (size_t c = 0; c <= nchunk; c++) {
		if (c < nchunk) {                   // start chunk c into buffer c & 1
			const size_t off = c * C, len = n - off < C ? n - off : C;
			HIP_TRY(hipMemcpyAsync(st.buf[c & 1], (const char *) src + off, len,
					       hipMemcpyDeviceToHost, st.stream));
			HIP_TRY(hipEventRecord(st.done[c & 1], st.stream));
		}
		if (c > 0) {                        // chunk c - 1 has landed: copy it out
			const size_t off = (c - 1) * C, len = n - off < C ? n - off : C;
			HIP_TRY(hipEventSynchronize(st.done[(c - 1) & 1]));
			const char *b = st.buf[(c - 1) & 1];
			char *d0 = (char *) dst + off;
			team_run(team_size(len), [&](int t, int nt) {
				const size_t a = len * t / nt, e = len * (t + 1) / nt;
				memcpy(d0 + a, b + a, e - a);
			});
		}
	}
	return 0;
}

// ---- small RAII device buffer --------------------------------------------------
struct DevBuf {
	void *p = nullptr;
	size_t bytes = 0;
	DevBuf() {}
	DevBuf(const DevBuf &) = delete;
	~DevBuf() { if (p) (void) hipFree(p); }
	int alloc(size_t n)
	{
		if (n == 0) n = 16;
		HIP_TRY(hipMalloc(&p, n));
		bytes = n;
		return 0;
	}
	int upload(const void *src, size_t n)
	{
		if (alloc(n)) return -1;
		return staged_copy(p, src, n);
	}
	int zero()
	{
		HIP_TRY(hipMemset(p, 0, bytes));
		return 0;
	}
	template <typename T> T *as() { return (T *) p; }
};

// The device word a launch raises (warn, overflow, workspace too small), zeroed.  read() ORs it into a host flag;
// what a raised flag means is the caller's business.
struct DevFlag {
	DevBuf W;
	int init() { return W.alloc(16) || W.zero(); }
	int *ptr() { return W.as<int>(); }
	int read(int *into)
	{
		int w = 0;
		HIP_TRY(hipMemcpy(&w, W.p, 4, hipMemcpyDeviceToHost));
		if (w) *into = 1;
		return 0;
	}
};

static void split_dims(const svt_view *x, int dims, int64_t *inner, int64_t *outer)
{
	*inner = *outer = 1;
	for (int a = 1; a < dims; a++) *inner *= x->dim[a];
	for (int a = dims; a < x->ndim; a++) *outer *= x->dim[a];
}

// The view of `n` empty segments on the structure of A: what a statistic over zero-extent dims summarizes, once per
// result.  P holds the offsets; a NULL col_ptr in the answer says that they could not be uploaded.
static svt_dev_csc empty_segments(const svt_dev_csc *A, int64_t n, DevBuf &P)
{
	const std::vector<int64_t> cp((size_t) n + 1, 0);
	svt_dev_csc E = *A;
	E.owned = 0; E.ncol = n; E.nnz = 0; E.nrow = 0;
	E.col_ptr = P.upload(cp.data(), cp.size() * 8) ? NULL : P.as<int64_t>();
	return E;
}

// ---- SVT -> CSC marshal ----------------------------------------------------------
static size_t elt_size(int Rtype) { return Rtype == SVT_REALSXP ? 8 : 4; }

static int check_view(const svt_view *x)
{
	if (x == NULL || x->ndim < 1 || x->dim == NULL)
		return svt_set_error("invalid svt_view");
	if (x->Rtype != SVT_REALSXP && x->Rtype != SVT_INTSXP &&
	    x->Rtype != SVT_LGLSXP)
		return svt_set_error("does not support SparseArray objects of "
				     "type code %d", x->Rtype);
	int64_t n = 1;
	for (int a = 1; a < x->ndim; a++) n *= x->dim[a];
	if (n != x->nleaves)
		return svt_set_error("svt_view: nleaves does not match dim");
	return 0;
}

// counts within [0, dim0], no NULL offsets behind a positive count
static int check_leaves(const svt_view *x)
{
	if (x->svt_is_null) return 0;
	const int dim0 = x->dim[0];
	for (int64_t j = 0; j < x->nleaves; j++) {
		const int c = x->nzcount[j];
		if (c < 0 || c > dim0)
			return svt_set_error("invalid SVT leaf (nzcount %d, dim %d)", c, dim0);
		if (c > 0 && x->nzoffs[j] == NULL)
			return svt_set_error("invalid SVT leaf (NULL nzoffs)");
	}
	return 0;
}

extern "C" svt_dev_csc *svt_upload(const svt_view *x)
{
	if (ensure_init() || check_view(x))
		return NULL;
	const int64_t n = x->nleaves;
	const size_t esz = elt_size(x->Rtype);
	const int dim0 = x->dim[0];
	std::vector<int64_t> col_ptr((size_t) n + 1, 0);
	for (int64_t j = 0; j < n; j++) {
		const int c = x->svt_is_null ? 0 : x->nzcount[j];
		if (c < 0 || c > dim0) {
			svt_set_error("invalid SVT leaf (nzcount %d, dim %d)", c, dim0);
			return NULL;
		}
		if (c > 0 && x->nzoffs[j] == NULL) {
			svt_set_error("invalid SVT leaf (NULL nzoffs)");
			return NULL;
		}
		col_ptr[j + 1] = col_ptr[j] + c;
	}
	svt_dev_csc *d = (svt_dev_csc *) calloc(1, sizeof(*d));
	d->Rtype = x->Rtype;
	d->owned = 1;
	d->na_background = x->na_background != 0;
	d->nrow = dim0;
	d->ncol = n;
	d->nnz = col_ptr[(size_t) n];
	const size_t nn = (size_t) (d->nnz > 0 ? d->nnz : 1);
	if (hipMalloc((void **) &d->col_ptr, (size_t) (d->ncol + 1) * 8) != hipSuccess ||
	    hipMalloc((void **) &d->row_idx, nn * 4) != hipSuccess ||
	    hipMalloc(&d->val, nn * esz) != hipSuccess) {
		svt_set_error("hipMalloc failed while uploading an SVT (%lld nnz)",
			      (long long) d->nnz);
		svt_release(d);
		return NULL;
	}
	bool ok = hipMemcpy(d->col_ptr, col_ptr.data(), (size_t) (d->ncol + 1) * 8,
			    hipMemcpyHostToDevice) == hipSuccess;
	// nonzeros k0 .. k0+cnt-1 per trip: as many as fit one pinned buffer
	// ([offsets of the chunk][values of the chunk], 4 + esz bytes per nonzero).  Chunks are
	// cut in nonzeros, not in leaves: one leaf may be longer than a buffer (dim0 only has to
	// exceed CHUNK / 12), and the team splits a chunk evenly whatever the leaf lengths are.
	const int64_t cap = (int64_t) (g_stager_chunk() / (4 + esz));
	const int64_t nnz = d->nnz;
	Stager &st = cur_stager();
	for (int64_t k0 = 0; ok && k0 < nnz; k0 += cap) {
		const int64_t cnt = nnz - k0 < cap ? nnz - k0 : cap;
		char *b; int slot;
		if (st.acquire(&b, &slot)) { ok = false; break; }
		int32_t *so = (int32_t *) b;
		char *sv = b + (size_t) cnt * 4;
		team_run(team_size((size_t) cnt * (4 + esz)), [&](int t, int nt) {
			const int64_t ka = k0 + cnt * t / nt, kb = k0 + cnt * (t + 1) / nt;
			if (ka >= kb) return;
			// first leaf that reaches past ka
			int64_t j = std::upper_bound(col_ptr.begin(), col_ptr.end(), ka) - col_ptr.begin() - 1;
			for (; j < n && col_ptr[j] < kb; j++) {
				const int64_t a = col_ptr[j] > ka ? col_ptr[j] : ka;
				const int64_t e = col_ptr[j + 1] < kb ? col_ptr[j + 1] : kb;
				if (e <= a) continue;
				const int64_t in_leaf = a - col_ptr[j], s = a - k0, c = e - a;
				memcpy(so + s, x->nzoffs[j] + in_leaf, (size_t) c * 4);
				const void *v = x->nzvals[j];
				if (v != NULL) {
					memcpy(sv + (size_t) s * esz, (const char *) v + (size_t) in_leaf * esz,
					       (size_t) c * esz);
				} else if (esz == 8) {      // lacunar leaf: all ones
					double *o = (double *) sv + s;
					for (int64_t k = 0; k < c; k++) o[k] = 1.0;
				} else {
					int *o = (int *) sv + s;
					for (int64_t k = 0; k < c; k++) o[k] = 1;
				}
			}
		});
		ok = st.send(slot, d->row_idx + k0, 0, (size_t) cnt * 4) == 0 &&
		     st.send(slot, (char *) d->val + (size_t) k0 * esz, (size_t) cnt * 4,
				   (size_t) cnt * esz) == 0 &&
		     st.commit(slot) == 0;
	}
	if (ok) ok = st.drain() == 0;
	if (!ok) {
		if (svt_last_error()[0] == '\0') svt_set_error("H2D copy failed");
		svt_release(d);
		return NULL;
	}
	return d;
}

extern "C" svt_dev_csc *svt_wrap_device_csc(int Rtype, int64_t nrow, int64_t ncol,
					    int64_t nnz, int64_t *col_ptr,
					    int32_t *row_idx, void *val)
{
	svt_dev_csc *d = (svt_dev_csc *) calloc(1, sizeof(*d));
	d->Rtype = Rtype;
	d->owned = 0;
	d->nrow = nrow;
	d->ncol = ncol;
	d->nnz = nnz;
	d->col_ptr = col_ptr;
	d->row_idx = row_idx;
	d->val = val;
	return d;
}

extern "C" void svt_release(svt_dev_csc *h)
{
	if (h == NULL)
		return;
	if (h->owned) {
		if (h->col_ptr) (void) hipFree(h->col_ptr);
		if (h->row_idx) (void) hipFree(h->row_idx);
		if (h->val) (void) hipFree(h->val);
	}
	free(h);
}

// ---- resident operands (opt-in) -------------------------------------------------------
// R code keeps calling the entry points on the same object (colSums(x); colVars(x);
// crossprod(x, y1); crossprod(x, y2) ...), and every call marshals and uploads the whole
// tree again (26 ms of a 54 ms crossprod at BASELINE config 2).  With a byte limit set
// (svt_resident_set_limit), the host-level entry points keep the device copy of an
// operand -- and the layouts derived from it: panel-blocked records, t(x) -- and find it
// again through a fingerprint of the view: dims, type, and per leaf the two host
// pointers, the count and eight evenly spread (offset, value) samples.  R vectors are
// immutable once shared, so equal pointers + counts + samples mean equal contents for
// well-behaved callers; code that overwrites leaves in place must call
// svt_resident_clear().  Off by default.  
struct Resident {
	uint64_t key;
	svt_dev_csc *csc;
	svt_dev_pbc *pbc;        // panel-blocked layout of csc, built on first use
	svt_dev_csc *tr;         // t(csc), built on first use
	svt_dev_pbc *tr_pbc;     // layout of t(csc)
	size_t bytes;
	uint64_t stamp;
	int pins;
};
static std::vector<Resident> g_res;
static std::mutex g_res_mu;
static size_t g_res_limit = 0, g_res_bytes = 0;
static uint64_t g_res_clock = 0, g_res_hits = 0, g_res_misses = 0;

static size_t csc_bytes(const svt_dev_csc *c)
{
	return (size_t) (c->ncol + 1) * 8 + (size_t) c->nnz * (4 + elt_size(c->Rtype));
}

static size_t pbc_bytes(const svt_dev_pbc *P) { return svt_dev_pbc_bytes(P); }

static void resident_free(Resident &r)
{
	if (r.pbc) svt_dev_pbc_release(r.pbc);
	if (r.tr_pbc) svt_dev_pbc_release(r.tr_pbc);
	svt_release(r.tr);
	svt_release(r.csc);
}

// drop least-recently-used unpinned entries until `need` more bytes fit
static void resident_make_room(size_t need)
{
	while (g_res_bytes + need > g_res_limit) {
		int victim = -1;
		for (size_t i = 0; i < g_res.size(); i++)
			if (g_res[i].pins == 0 && (victim < 0 || g_res[i].stamp < g_res[victim].stamp))
				victim = (int) i;
		if (victim < 0) return;
		g_res_bytes -= g_res[victim].bytes;
		resident_free(g_res[victim]);
		g_res.erase(g_res.begin() + victim);
	}
}

extern "C" int svt_resident_set_limit(size_t bytes)
{
	std::lock_guard<std::mutex> lk(g_res_mu);
	g_res_limit = bytes;
	resident_make_room(0);
	return 0;
}

extern "C" void svt_resident_clear(void)
{
	std::lock_guard<std::mutex> lk(g_res_mu);
	const size_t keep = g_res_limit;
	g_res_limit = 0;
	resident_make_room(0);
	g_res_limit = keep;
}

extern "C" void svt_resident_stats(size_t *bytes, int64_t *entries, int64_t *hits, int64_t *misses)
{
	std::lock_guard<std::mutex> lk(g_res_mu);
	if (bytes) *bytes = g_res_bytes;
	if (entries) *entries = (int64_t) g_res.size();
	if (hits) *hits = (int64_t) g_res_hits;
	if (misses) *misses = (int64_t) g_res_misses;
}

static inline uint64_t fp_mix(uint64_t h, uint64_t v)
{
	h ^= v + 0x9E3779B97F4A7C15ULL + (h << 6) + (h >> 2);
	h *= 0xFF51AFD7ED558CCDULL;
	return h ^ (h >> 33);
}

static uint64_t view_fingerprint(const svt_view *x)
{
	uint64_t h = fp_mix(0x5356545F48495031ULL, (uint64_t) x->Rtype);
	h = fp_mix(h, (uint64_t) x->ndim);
	for (int a = 0; a < x->ndim; a++) h = fp_mix(h, (uint64_t) x->dim[a]);
	h = fp_mix(h, (uint64_t) x->svt_is_null * 2 + (uint64_t) (x->na_background != 0));
	h = fp_mix(h, (uint64_t) x->nleaves);
	if (x->svt_is_null) return h;
	const size_t esz = elt_size(x->Rtype);
	for (int64_t j = 0; j < x->nleaves; j++) {
		const int n = x->nzcount[j];
		h = fp_mix(h, (uint64_t) n);
		if (n <= 0) continue;
		h = fp_mix(h, (uint64_t) (uintptr_t) x->nzoffs[j]);
		h = fp_mix(h, (uint64_t) (uintptr_t) x->nzvals[j]);
		int at[8];
		for (int t = 0; t < 8; t++) at[t] = (int) ((int64_t) (n - 1) * t / 7);
		for (int t = 0; t < 8; t++) {
			uint64_t v = (uint64_t) (uint32_t) x->nzoffs[j][at[t]];
			if (x->nzvals[j] != NULL) {               // (NULL: lacunar leaf, all ones)
				uint64_t bits = 0;
				memcpy(&bits, (const char *) x->nzvals[j] + (size_t) at[t] * esz, esz);
				v ^= bits * 0x9E3779B97F4A7C15ULL;
			}
			h = fp_mix(h, v);
		}
	}
	return h;
}

// An operand of a host-level call: resident if the cache is on (found or inserted, pinned
// for the lifetime of the guard), else uploaded for this call and released with the guard.
struct CscGuard {
	svt_dev_csc *h;
	uint64_t key;            // != 0: h belongs to the resident set
	explicit CscGuard(svt_dev_csc *p) : h(p), key(0) {}
	explicit CscGuard(const svt_view *x) : h(NULL), key(0)
	{
		if (g_res_limit == 0) { h = svt_upload(x); return; }
		if (check_view(x) || check_leaves(x)) return;      // (the fingerprint reads the leaves)
		const uint64_t k = view_fingerprint(x) | 1;
		{
			std::lock_guard<std::mutex> lk(g_res_mu);
			for (Resident &r : g_res)
				if (r.key == k) {
					r.pins++; r.stamp = ++g_res_clock; g_res_hits++;
					h = r.csc; key = k;
					return;
				}
			g_res_misses++;
		}
		h = svt_upload(x);
		if (h == NULL) return;
		std::lock_guard<std::mutex> lk(g_res_mu);
		const size_t nb = csc_bytes(h);
		resident_make_room(nb);
		if (g_res_bytes + nb > g_res_limit) return;        // does not fit: one-call operand
		Resident r = { k, h, NULL, NULL, NULL, nb, ++g_res_clock, 1 };
		g_res.push_back(r);
		g_res_bytes += nb;
		key = k;
	}
	~CscGuard()
	{
		if (key == 0) { svt_release(h); return; }
		std::lock_guard<std::mutex> lk(g_res_mu);
		for (Resident &r : g_res)
			if (r.key == key) { r.pins--; return; }
	}
	void drop()              // a one-call operand that is no longer needed
	{
		if (key == 0) { svt_release(h); h = NULL; }
	}
	CscGuard(const CscGuard &) = delete;
	CscGuard &operator=(const CscGuard &) = delete;
};

// index of the resident entry that owns the device handle A (as its operand or as its
// transposed copy), or -1; call with g_res_mu held
static int resident_find(const svt_dev_csc *A)
{
	for (size_t i = 0; i < g_res.size(); i++)
		if (g_res[i].csc == A || g_res[i].tr == A) return (int) i;
	return -1;
}

// The panel-blocked layout of a resident operand lives with it; for a one-call operand it
// is built and released by the caller.  *owned tells which.
static svt_dev_pbc *pbc_for(const svt_dev_csc *A, int *owned)
{
	*owned = 1;
	{
		std::lock_guard<std::mutex> lk(g_res_mu);
		for (Resident &r : g_res)
			if (r.csc == A || r.tr == A) {
				svt_dev_pbc *&slot = r.csc == A ? r.pbc : r.tr_pbc;
				if (slot != NULL) { *owned = 0; return slot; }
				break;
			}
	}
	svt_dev_pbc *P = svt_dev_pbc_build(A, 0, 0, 0);        // layout by density (pbc_auto_layout)
	if (P == NULL) return NULL;
	std::lock_guard<std::mutex> lk(g_res_mu);
	if (resident_find(A) >= 0) {
		const size_t nb = pbc_bytes(P);
		resident_make_room(nb);                   // (the entry itself is pinned by its guard)
		// make_room() erases entries: look the operand up again, never keep a reference across it
		const int i = resident_find(A);
		if (i >= 0 && g_res_bytes + nb <= g_res_limit) {
			Resident &r = g_res[(size_t) i];
			(r.csc == A ? r.pbc : r.tr_pbc) = P;
			r.bytes += nb; g_res_bytes += nb;
			*owned = 0;
		}
	}
	return P;
}

// ==================================================================================
// Device level
// ==================================================================================
extern "C" size_t svt_dev_crossprod_ws_bytes(int64_t nrow, int64_t ncol, int K)
{
	return crossprod_ws_bytes(nrow, ncol, K);
}

extern "C" int svt_dev_crossprod_csc_dense(const svt_dev_csc *A, const void *Y,
					   int64_t ldY, int K, int tr_y, double *out,
					   int64_t out_stride_c, int64_t out_stride_k,
					   void *ws, size_t ws_bytes, void *stream)
{
	CrossprodArgs a;
	a.col_ptr = A->col_ptr; a.row_idx = A->row_idx; a.val = A->val;
	a.Rtype = A->Rtype == SVT_REALSXP ? SVT_REALSXP : SVT_INTSXP;
	a.nrow = A->nrow; a.ncol = A->ncol;
	a.Y = Y; a.ldY = ldY; a.K = K; a.tr_y = tr_y;
	a.out = out; a.out_stride_c = out_stride_c; a.out_stride_k = out_stride_k;
	a.ws = ws; a.ws_bytes = ws_bytes;
	return launch_crossprod_csc_dense(a, (hipStream_t) stream);
}

extern "C" int svt_dev_dense_prepare(const void *Y, int64_t ldY, int64_t nrow, int K,
				     int tr_y, int Rtype, void *ws, size_t ws_bytes,
				     void *stream)
{
	CrossprodArgs a;
	memset(&a, 0, sizeof(a));
	a.Rtype = Rtype == SVT_REALSXP ? SVT_REALSXP : SVT_INTSXP;
	a.nrow = nrow; a.Y = Y; a.ldY = ldY; a.K = K; a.tr_y = tr_y;
	a.ws = ws; a.ws_bytes = ws_bytes;
	return launch_dense_prepare(a, (hipStream_t) stream);
}

extern "C" int svt_dev_crossprod_prepared(const svt_dev_csc *A, const void *ws, int K,
					  double *out, int64_t out_stride_c,
					  int64_t out_stride_k, void *stream)
{
	CrossprodArgs a;
	memset(&a, 0, sizeof(a));
	a.col_ptr = A->col_ptr; a.row_idx = A->row_idx; a.val = A->val;
	a.Rtype = A->Rtype == SVT_REALSXP ? SVT_REALSXP : SVT_INTSXP;
	a.nrow = A->nrow; a.ncol = A->ncol; a.K = K;
	a.out = out; a.out_stride_c = out_stride_c; a.out_stride_k = out_stride_k;
	a.ws = (void *) ws;
	return launch_crossprod_prepared(a, (hipStream_t) stream);
}

static int check_stat_op(int opcode, int Rtype)
{
	// _get_summarize_opcode(), src/Rvector_summarization.c:19-78
	if (opcode < SVT_OP_ANYNA || opcode > SVT_OP_SD2)
		return svt_set_error("'op' must be one of: \"anyNA\", \"countNAs\", "
				     "\"any\", \"all\", \"min\", \"max\", \"range\", \"sum\", "
				     "\"prod\", \"mean\", \"centered_X2_sum\", \"sum_X_X2\", "
				     "\"var1\", \"var2\", \"sd1\", \"sd2\"");
	if ((opcode == SVT_OP_ANY || opcode == SVT_OP_ALL) && Rtype == SVT_REALSXP)
		return svt_set_error("%s() does not support SparseArray objects of "
				     "type() \"double\"", opcode == SVT_OP_ANY ? "any" : "all");
	return 0;
}

extern "C" int svt_colStats_out_Rtype(int opcode, int in_Rtype)
{
	// _init_SummarizeResult(), src/Rvector_summarization.c:97-165
	switch (opcode) {
	case SVT_OP_ANYNA: case SVT_OP_ANY: case SVT_OP_ALL:
		return SVT_LGLSXP;
	case SVT_OP_MIN: case SVT_OP_MAX: case SVT_OP_RANGE:
		return in_Rtype == SVT_REALSXP ? SVT_REALSXP : SVT_INTSXP;
	default:
		if (opcode < SVT_OP_ANYNA || opcode > SVT_OP_SD2)
			return svt_set_error("unknown opcode %d", opcode);
		return SVT_REALSXP;
	}
}

static int device_op_supported(int opcode)
{
	if (opcode == SVT_OP_RANGE || opcode == SVT_OP_SUM_X_X2 ||
	    opcode == SVT_OP_VAR2 || opcode == SVT_OP_SD2)
		return svt_set_unsupported("op code %d is not reachable from the R API for "
					   "col/row stats and is not implemented on the device",
					   opcode);
	return 0;
}

static int dev_colstats_ex(const svt_dev_csc *A, int opcode, int na_rm, double center,
			   int64_t inner, void *out, int *warn_flag, void *stream, int dgc)
{
	if (check_stat_op(opcode, A->Rtype) || device_op_supported(opcode))
		return -1;
	if (inner <= 0 || A->ncol % inner != 0)
		return svt_set_error("'inner' must divide the number of leaves");
	StatsArgs a;
	a.col_ptr = A->col_ptr; a.val = A->val; a.Rtype = A->Rtype;
	a.nseg = A->ncol / inner; a.inner = inner; a.seg_len = inner * A->nrow;
	a.opcode = opcode; a.na_rm = na_rm; a.center = center;
	a.out = out; a.warn_flag = warn_flag; a.na_bg = A->na_background;
	a.dgc = dgc;
	return launch_colstats(a, A->nnz, (hipStream_t) stream);
}

extern "C" int svt_dev_colstats(const svt_dev_csc *A, int opcode, int na_rm,
				double center, int64_t inner, void *out,
				int *warn_flag, void *stream)
{
	return abi_status([&] { return dev_colstats_ex(A, opcode, na_rm, center, inner, out, warn_flag, stream, 0); });
}

extern "C" int svt_dev_colstats_form(int64_t nseg, int64_t nnz, int *nchunk)
{
	const ColStatsRoute rt = colstats_route(nseg, nnz);
	if (nchunk) *nchunk = rt.nchunk;
	return rt.form;
}

extern "C" size_t svt_dev_colmedians_ws_bytes(int64_t nnz, int64_t ncol)
{
	(void) nnz;
	return order_stat_ws_bytes(ORDER_MEDIANS, ncol);
}

extern "C" size_t svt_dev_colquantiles_ws_bytes(int64_t nnz, int64_t ncol, int nprobs)
{
	(void) nnz; (void) nprobs;
	return order_stat_ws_bytes(ORDER_QUANTILES, ncol);
}

extern "C" size_t svt_dev_colmads_ws_bytes(int64_t nnz, int64_t ncol)
{
	(void) nnz;
	return order_stat_ws_bytes(ORDER_MADS, ncol);
}

// The names of an order statistic (ORDER_*): its col and row methods, and its device entry point.
static const char *const order_stat_names[3][3] = {
	{ "colMedians", "rowMedians", "colmedians" },
	{ "colQuantiles", "rowQuantiles", "colquantiles" },
	{ "colMads", "rowMads", "colmads" },
};

// vec: the probs (ORDER_QUANTILES) or the centers, NULL for the medians (ORDER_MADS), on the device.
static int dev_order_stat_impl(const svt_dev_csc *A, int what, const double *vec, int nprobs, double constant, int na_rm,
				  double *out, void *ws, size_t ws_bytes, void *stream)
{
	const bool quant = what == ORDER_QUANTILES;
	if (A->na_background)
		return svt_set_error("%s() is not supported on NaArray objects", order_stat_names[what][0]);
	if (quant && nprobs < 0)
		return svt_set_error("svt_dev_colquantiles: 'nprobs' must be >= 0");
	if (ws_bytes < order_stat_ws_bytes(what, A->ncol))
		return svt_set_error("svt_dev_%s: workspace too small", order_stat_names[what][2]);
	return launch_order_stat(what, A->col_ptr, A->val, A->Rtype, A->nrow, A->ncol, A->nnz, vec, nprobs, constant, na_rm,
				 out, ws, (hipStream_t) stream);
}
extern "C" int svt_dev_colmedians(const svt_dev_csc *A, int na_rm, double *out, void *ws,
				  size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		return dev_order_stat_impl(A, ORDER_MEDIANS, NULL, 0, 0.0, na_rm, out, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_colquantiles(const svt_dev_csc *A, const double *probs, int nprobs, int na_rm, double *out,
				    void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		return dev_order_stat_impl(A, ORDER_QUANTILES, probs, nprobs, 0.0, na_rm, out, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_colmads(const svt_dev_csc *A, const double *center, double constant, int na_rm, double *out,
			       void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		return dev_order_stat_impl(A, ORDER_MADS, center, 0, constant, na_rm, out, ws, ws_bytes, stream);
	});
}

// colRanks in the compact form (kernels_ranks.hip)
extern "C" int svt_dev_colranks_form(int64_t col_nnz) { return ranks_form(col_nnz); }
extern "C" size_t svt_dev_colranks_ws_bytes(int64_t ncol, int64_t long_nnz) { return ranks_ws_bytes(ncol, long_nnz); }

static int check_ties(int ties)
{
	if (ties != SVT_TIES_MAX && ties != SVT_TIES_AVERAGE && ties != SVT_TIES_MIN && ties != SVT_TIES_DENSE)
		return svt_set_error("'ties.method' must be \"max\", \"average\", \"min\" or \"dense\"");
	return 0;
}

extern "C" int svt_dev_colranks(const svt_dev_csc *A, int ties, void *rank_nz, void *zero_rank, int *flag, void *ws,
				size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		if (flag == NULL)
			return svt_set_error("svt_dev_colranks: 'flag' must be a device word");
		// (the flag is cleared on every call, before any early return)
		HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), (hipStream_t) stream));
		if (A->na_background)
			return svt_set_error("colRanks() is not supported on NaArray objects");
		if (check_ties(ties))
			return -1;
		return launch_ranks(A->col_ptr, A->val, A->Rtype, A->nrow, A->ncol, A->nnz, ties, rank_nz, zero_rank, flag, ws,
				    ws_bytes, (hipStream_t) stream);
	});
}

extern "C" size_t svt_dev_rowstats_ws_bytes(int64_t nrow, int64_t ncol)
{
	return rowstats_panel_ws_bytes(nrow, ncol);
}

// the operand and the operation of a row statistic; the caller adds center, scratch, warn_flag and table_mode
static RowStatsArgs rowstats_args(const svt_dev_csc *A, int opcode, int na_rm, int64_t inner, int64_t nstrata, void *out)
{
	RowStatsArgs a;
	memset(&a, 0, sizeof(a));
	a.col_ptr = A->col_ptr; a.row_idx = A->row_idx; a.val = A->val;
	a.Rtype = A->Rtype; a.ncol = A->ncol; a.nrow = A->nrow;
	a.inner = inner; a.nstrata = nstrata; a.out_len = inner * A->nrow;
	a.opcode = opcode; a.na_rm = na_rm; a.out = out; a.nnz_hint = A->nnz;
	a.na_bg = A->na_background != 0;
	return a;
}

static int dev_rowsums(const svt_dev_csc *A, int na_rm, int64_t inner, double *out, void *ws, size_t ws_bytes,
		       void *stream, int table_mode)
{
	if (inner <= 0 || A->ncol % inner != 0)
		return svt_set_error("'inner' must divide the number of leaves");
	if (ws_bytes < rowstats_panel_ws_bytes(A->nrow, A->ncol))
		return svt_set_error("svt_dev_rowsums: workspace too small");
	RowStatsArgs a = rowstats_args(A, SVT_OP_SUM, na_rm, inner, A->ncol / inner, out);
	a.table_mode = table_mode;
	return launch_rowstats_panel(a, ws, (hipStream_t) stream);
}

extern "C" int svt_dev_rowsums(const svt_dev_csc *A, int na_rm, int64_t inner,
			       double *out, void *ws, size_t ws_bytes, void *stream)
{
	return dev_rowsums(A, na_rm, inner, out, ws, ws_bytes, stream, ROWSTATS_TABLE_BUILD);
}

// The table of run bounds per row panel depends on the operand alone (one pass over its offsets, a quarter of
// a rowSums at BASELINE config 2): built once into `ws`, then any number of svt_dev_rowsums_prepared() calls on
// the same operand with the same `inner` read it.
extern "C" int svt_dev_rowsums_prepare(const svt_dev_csc *A, int64_t inner, void *ws, size_t ws_bytes, void *stream)
{
	return dev_rowsums(A, 0, inner, NULL, ws, ws_bytes, stream, ROWSTATS_TABLE_ONLY);
}

extern "C" int svt_dev_rowsums_prepared(const svt_dev_csc *A, int na_rm, int64_t inner,
					double *out, void *ws, size_t ws_bytes, void *stream)
{
	return dev_rowsums(A, na_rm, inner, out, ws, ws_bytes, stream, ROWSTATS_TABLE_READY);
}

// ---- every row statistic in one call (svt_dev_rowstats, svt_rowStatsFull_SVT) ----
static bool rowstats_reference_op(int opcode)       // the six of C_rowStats_SVT
{
	return opcode == SVT_OP_COUNTNAS || opcode == SVT_OP_ANYNA || opcode == SVT_OP_MIN || opcode == SVT_OP_MAX ||
		opcode == SVT_OP_SUM || opcode == SVT_OP_CENTERED_X2_SUM;
}
static bool rowstats_fused_op(int opcode)
{
	return opcode == SVT_OP_MEAN || opcode == SVT_OP_VAR1 || opcode == SVT_OP_SD1;
}
// the checks of C_rowStats_SVT for the thirteen operations taken here
static int check_rowstats_op(int opcode, int Rtype, int na_background)
{
	if (check_stat_op(opcode, Rtype))
		return -1;
	if (opcode == SVT_OP_SUM_X_X2 || opcode == SVT_OP_VAR2 || opcode == SVT_OP_SD2)
		return svt_set_unsupported("op code %d is not reachable from the R API for col/row stats and is not "
					   "implemented on the device", opcode);
	// :639-642; rowAnys / Alls / Prods / Means / Vars / Sds have no NaArray methods (R/NaArray-matrixStats.R:187-330)
	if (na_background && opcode != SVT_OP_RANGE && (opcode == SVT_OP_CENTERED_X2_SUM || !rowstats_reference_op(opcode)))
		return svt_set_error("operation not yet supported on NaArray objects");
	return 0;
}

// workspace: the table of run bounds | sums, NA counts, center (mean / var1 / sd1) | the min / max scratch of the
// memory-atomic route (more than 65535 output columns)
static size_t rowstats_ws_table_bytes(const svt_dev_csc *A)
{
	return (rowstats_panel_ws_bytes(A->nrow, A->ncol) + 255) / 256 * 256;
}
extern "C" size_t svt_dev_rowstats_ws_bytes_op(const svt_dev_csc *A, int opcode, int64_t inner)
{
	const int64_t out_len = inner > 0 ? inner * A->nrow : 0;
	size_t n = rowstats_ws_table_bytes(A);
	if (rowstats_fused_op(opcode)) n += rowstats_fused_ws_bytes(out_len);
	if (inner > 65535) n += rowstats_scratch_bytes(opcode, out_len);
	return n;
}

static int dev_rowstats_impl(const svt_dev_csc *A, int opcode, int na_rm, const double *center, int64_t inner, void *out,
			     int *warn_flag, void *ws, size_t ws_bytes, void *stream)
{
	if (check_rowstats_op(opcode, A->Rtype, A->na_background))
		return -1;
	if (inner <= 0 || A->ncol % inner != 0)
		return svt_set_error("'inner' must divide the number of leaves");
	const int64_t nstrata = A->ncol / inner;
	if (nstrata > 0xFFFFFFFFLL)
		return svt_set_unsupported("too many strata for the device coverage counters");
	if (inner > 65535 && A->na_background)
		return svt_set_unsupported("row statistics of NaArray objects: more than 65535 output columns");
	if (inner > 65535 && !rowstats_reference_op(opcode))
		return svt_set_unsupported("row statistics: this operation is not served with more than 65535 output columns");
	if (ws_bytes < svt_dev_rowstats_ws_bytes_op(A, opcode, inner))
		return svt_set_error("svt_dev_rowstats: workspace too small");
	RowStatsArgs a = rowstats_args(A, opcode, na_rm, inner, nstrata, out);
	a.center = opcode == SVT_OP_CENTERED_X2_SUM || rowstats_fused_op(opcode) ? center : NULL;
	a.warn_flag = warn_flag;
	char *after_table = (char *) ws + rowstats_ws_table_bytes(A);
	if (inner > 65535) {
		a.scratch = after_table;
		return launch_rowstats(a, (hipStream_t) stream);
	}
	if (rowstats_fused_op(opcode))
		return launch_rowstats_fused(a, ws, after_table, (hipStream_t) stream);
	return launch_rowstats_panel(a, ws, (hipStream_t) stream);
}

extern "C" int svt_dev_rowstats(const svt_dev_csc *A, int opcode, int na_rm, const double *center, int64_t inner,
				void *out, int *warn_flag, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] { return dev_rowstats_impl(A, opcode, na_rm, center, inner, out, warn_flag, ws, ws_bytes, stream); });
}

extern "C" int svt_dev_rowstats_form(int64_t nrow, int64_t ncol, int64_t nnz, int na_background, int opcode,
				     int64_t inner, int *panel_shift, int64_t *nsplit)
{
	int ps = 0;
	int64_t ns = 1;
	int form = 4;           // more than 65535 output columns: memory atomics (dev_rowstats_impl)
	if (inner <= 65535) {
		svt_dev_csc A;
		memset(&A, 0, sizeof(A));
		A.nrow = nrow; A.ncol = ncol; A.nnz = nnz; A.na_background = na_background;
		const RowStatsArgs a = rowstats_args(&A, opcode, 0, inner, inner > 0 ? ncol / inner : 0, NULL);
		form = rowstats_panel_form(a, &ps, &ns);
	}
	if (panel_shift) *panel_shift = ps;
	if (nsplit) *nsplit = ns;
	return form;
}

extern "C" size_t svt_dev_transpose_ws_bytes(int64_t nrow, int64_t nnz)
{
	return transpose_ws_bytes_box(nrow, nnz, box_nnz_get());
}

static int dev_transpose_impl(const svt_dev_csc *A, int64_t *out_col_ptr, int32_t *out_row_idx,
				 void *out_val, void *ws, size_t ws_bytes, void *stream)
{
	const int64_t box = box_nnz_get();                  // (once: the size check and the launch agree)
	if (ws_bytes < transpose_ws_bytes_box(A->nrow, A->nnz, box))
		return svt_set_error("svt_dev_transpose: workspace too small");
	return launch_transpose_box(A->col_ptr, A->row_idx, A->val, A->Rtype, A->nrow, A->ncol, A->nnz,
				    out_col_ptr, out_row_idx, out_val, ws, box, (hipStream_t) stream);
}

extern "C" void svt_dev_set_box_nnz(int64_t n)
{
	box_nnz_set(n);
}

extern "C" int64_t svt_dev_boxed_calls(int reset)
{
	return boxed_calls(reset);
}
extern "C" int svt_dev_transpose(const svt_dev_csc *A, int64_t *out_col_ptr, int32_t *out_row_idx,
				 void *out_val, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] { return dev_transpose_impl(A, out_col_ptr, out_row_idx, out_val, ws, ws_bytes, stream); });
}

// ---- x[i, j] by an N-index (kernels_subset.hip; C_subset_SVT_by_Nindex, src/SparseArray_subsetting.c:223-297) ----
enum { SUBSET_GATHER = 0, SUBSET_FILTER = 1, SUBSET_GENERAL = 2 };
static std::atomic<int64_t> g_subset_route[3];

extern "C" int svt_dev_subset_tile(void)
{
	return subset_tile();
}

extern "C" void svt_dev_subset_route_counts(int64_t *counts, int reset)
{
	for (int i = 0; i < 3; i++) {
		if (counts) counts[i] = g_subset_route[i].load();
		if (reset) g_subset_route[i] = 0;
	}
}

// what a count launcher left in the first `nwords` (2 or 3) 64-bit words of its workspace: one copy, the call's one
// synchronisation
struct WsHead {
	int flag = 0;                // the low half of word 0
	int64_t total = 0;           // word 1: the result's nonzeros
	int64_t third = 0;           // word 2, as it is (sweep: the refused element; the L-index placement: unsorted)
	int read(const void *ws, hipStream_t s, int nwords = 2)
	{
		int64_t head[3] = { 0, 0, 0 };
		HIP_TRY(hipMemcpyAsync(head, ws, (size_t) nwords * 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(hipStreamSynchronize(s));
		flag = (int) (head[0] & 0xFFFFFFFFLL);
		total = head[1];
		third = head[2];
		return 0;
	}
	static int total_of(const void *ws, hipStream_t s, int64_t *out_nnz)      // for a count that raises no flag
	{
		WsHead head;
		if (head.read(ws, s))
			return -1;
		*out_nnz = head.total;
		return 0;
	}
};

extern "C" size_t svt_dev_subset_cols_ws_bytes(int64_t ncols_sel)
{
	return subset_cols_ws_bytes(ncols_sel);
}

static int dev_subset_cols_count_impl(const svt_dev_csc *A, const int32_t *cols, int64_t ncols_sel, int64_t *out_col_ptr,
				      int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	if (ncols_sel < 0 || ncols_sel > 0x7FFFFFFELL)
		return svt_set_error("svt_dev_subset_cols_count: between 0 and 2^31-2 columns");
	if (ws_bytes < subset_cols_ws_bytes(ncols_sel))
		return svt_set_error("svt_dev_subset_cols_count: workspace too small");
	if (ncols_sel == 0) {
		HIP_TRY(hipMemsetAsync(out_col_ptr, 0, 8, (hipStream_t) stream));
		*out_nnz = 0;
		return 0;
	}
	if (launch_subset_cols_count(A->col_ptr, A->ncol, cols, ncols_sel, out_col_ptr, ws, (hipStream_t) stream))
		return -1;
	WsHead head;
	if (head.read(ws, (hipStream_t) stream))
		return -1;
	if (head.flag)
		return svt_set_error("subscript out of bounds");
	*out_nnz = head.total;
	return 0;
}
extern "C" int svt_dev_subset_cols_count(const svt_dev_csc *A, const int32_t *cols, int64_t ncols_sel, int64_t *out_col_ptr,
					 int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] { return dev_subset_cols_count_impl(A, cols, ncols_sel, out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}

static int dev_subset_cols_fill_impl(const svt_dev_csc *A, const int32_t *cols, int64_t ncols_sel, const int64_t *out_col_ptr,
				     int32_t *out_row_idx, void *out_val, void *stream)
{
	g_subset_route[SUBSET_GATHER]++;
	if (ncols_sel <= 0 || A->nnz == 0)
		return 0;
	return launch_subset_cols_fill(A->col_ptr, A->row_idx, A->val, A->Rtype, A->ncol, A->nnz, cols, ncols_sel, out_col_ptr,
				       out_row_idx, out_val, (hipStream_t) stream);
}
extern "C" int svt_dev_subset_cols_fill(const svt_dev_csc *A, const int32_t *cols, int64_t ncols_sel, const int64_t *out_col_ptr,
					int32_t *out_row_idx, void *out_val, void *stream)
{
	return abi_status([&] { return dev_subset_cols_fill_impl(A, cols, ncols_sel, out_col_ptr, out_row_idx, out_val, stream); });
}

extern "C" size_t svt_dev_subset_rows_ws_bytes(int64_t nrow, int64_t ncol, int64_t nnz)
{
	return subset_rows_ws_bytes(nrow, ncol, nnz);
}

static int dev_subset_rows_count_impl(const svt_dev_csc *A, const int32_t *rows, int64_t nrows_sel, int64_t *out_col_ptr,
				      int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	if (nrows_sel < 0)
		return svt_set_error("svt_dev_subset_rows_count: 'nrows_sel' must be >= 0");
	if (ws_bytes < subset_rows_ws_bytes(A->nrow, A->ncol, A->nnz))
		return svt_set_error("svt_dev_subset_rows_count: workspace too small");
	if (launch_subset_rows_count(A->col_ptr, A->row_idx, A->nrow, A->ncol, A->nnz, rows, nrows_sel, out_col_ptr, ws,
				     (hipStream_t) stream))
		return -1;
	WsHead head;
	if (head.read(ws, (hipStream_t) stream))
		return -1;
	if (head.flag & 1)
		return svt_set_error("subscript out of bounds");
	if (head.flag)
		return svt_set_unsupported("svt_dev_subset_rows_count: the subscript is not strictly increasing");
	*out_nnz = head.total;
	return 0;
}
extern "C" int svt_dev_subset_rows_count(const svt_dev_csc *A, const int32_t *rows, int64_t nrows_sel, int64_t *out_col_ptr,
					 int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] { return dev_subset_rows_count_impl(A, rows, nrows_sel, out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}

static int dev_subset_rows_fill_impl(const svt_dev_csc *A, int32_t *out_row_idx, void *out_val, const void *ws,
				     size_t ws_bytes, void *stream)
{
	if (ws_bytes < subset_rows_ws_bytes(A->nrow, A->ncol, A->nnz))
		return svt_set_error("svt_dev_subset_rows_fill: workspace too small");
	g_subset_route[SUBSET_FILTER]++;
	return launch_subset_rows_fill(A->row_idx, A->val, A->Rtype, A->nrow, A->ncol, A->nnz, out_row_idx, out_val, ws,
				       (hipStream_t) stream);
}
extern "C" int svt_dev_subset_rows_fill(const svt_dev_csc *A, const int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val,
					const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the tile prefixes in `ws` place the entries)
	return abi_status([&] { return dev_subset_rows_fill_impl(A, out_row_idx, out_val, ws, ws_bytes, stream); });
}

// ---- the protocol of every entry point that leaves a new sparse operand behind, stated once ----
// Every array -- the result's three, intermediates, workspaces -- comes from the caller's allocator: col_ptr and the
// workspace first, then the count step (its read of the workspace head is the call's one synchronisation), row_idx and
// val for the nonzeros it found, the fill step; the three arrays go to the caller, everything else is released on every
// exit.  The families differ in their checks (each keeps its own order of refusals), their count and their fill.
static int need_allocator(const char *who, svt_dev_alloc_fn alloc, svt_dev_free_fn release)
{
	return alloc == NULL || release == NULL ? svt_set_error("%s: an allocator is needed", who) : 0;
}
struct ResultDest {              // the caller's allocator and where the result's nonzero count and three arrays go
	svt_dev_alloc_fn alloc;
	svt_dev_free_fn release;
	void *ctx;
	int64_t *nnz;
	int64_t **col_ptr;
	int32_t **row_idx;
	void **val;
};
struct ResultMem {
	const char *who;             // the entry point a failed allocation names
	svt_dev_alloc_fn alloc;
	svt_dev_free_fn release;
	void *ctx;
	ResultMem(const char *w, const ResultDest &to) : who(w), alloc(to.alloc), release(to.release), ctx(to.ctx) {}
	void *get(size_t n)
	{
		void *p = alloc(n > 0 ? n : 16, ctx);
		if (p == NULL) svt_set_error("%s: device allocation failed (%zu bytes)", who, n);
		return p;
	}
	void put(void *p) { if (p) release(p, ctx); }
};
struct ResultCsc {               // a CSC of three such arrays, given back with this object unless handed over
	ResultMem &mem;
	svt_dev_csc c;
	explicit ResultCsc(ResultMem &m) : mem(m) { memset(&c, 0, sizeof(c)); }
	ResultCsc(const ResultCsc &) = delete;
	~ResultCsc() { drop(); }
	void drop()
	{
		mem.put(c.col_ptr); mem.put(c.row_idx); mem.put(c.val);
		c.col_ptr = NULL; c.row_idx = NULL; c.val = NULL;
	}
	int shape(int Rtype, int na_background, int64_t nrow, int64_t ncol)
	{
		drop();
		c.Rtype = Rtype; c.na_background = na_background;
		c.nrow = nrow; c.ncol = ncol; c.nnz = 0;
		c.col_ptr = (int64_t *) mem.get(((size_t) ncol + 1) * 8);
		return c.col_ptr ? 0 : -1;
	}
	int entries(int64_t nnz)
	{
		const size_t n = nnz > 0 ? (size_t) nnz : 1;
		c.nnz = nnz;
		c.row_idx = (int32_t *) mem.get(n * 4);
		c.val = mem.get(n * elt_size(c.Rtype));
		return c.row_idx && c.val ? 0 : -1;
	}
	void hand_over(const ResultDest &to)
	{
		*to.nnz = c.nnz;
		*to.col_ptr = c.col_ptr; *to.row_idx = c.row_idx; *to.val = c.val;
		c.col_ptr = NULL; c.row_idx = NULL; c.val = NULL;   // taken
	}
};
struct ResultWs {
	ResultMem &mem;
	void *p = NULL;
	size_t n = 0;
	explicit ResultWs(ResultMem &m) : mem(m) {}
	ResultWs(const ResultWs &) = delete;
	~ResultWs() { mem.put(p); }
	int get(size_t bytes) { p = mem.get(bytes); n = bytes; return p ? 0 : -1; }
};

// The driver, into an operand that stays with the composition: count(col_ptr, &nnz, ws, ws_bytes), then
// fill(R.c, ws, ws_bytes); a status of `count` other than 0 ends the call and is returned as it is.
template <class Count, class Fill>
static int compose_into(ResultCsc &R, int Rtype, int na_background, int64_t nrow, int64_t ncol, size_t ws_bytes, Count count, Fill fill)
{
	ResultWs ws(R.mem);
	int64_t nnz = 0;
	if (R.shape(Rtype, na_background, nrow, ncol) || ws.get(ws_bytes))
		return -1;
	if (const int rc = count(R.c.col_ptr, &nnz, ws.p, ws.n))
		return rc;
	if (R.entries(nnz))
		return -1;
	return fill(R.c, ws.p, ws.n);
}
// The driver, for the result that goes to the caller
template <class Count, class Fill>
static int compose_result(const char *who, const ResultDest &to, int Rtype, int na_background, int64_t nrow, int64_t ncol,
			  size_t ws_bytes, Count count, Fill fill)
{
	ResultMem mem(who, to);
	ResultCsc R(mem);
	if (compose_into(R, Rtype, na_background, nrow, ncol, ws_bytes, count, fill))
		return -1;
	R.hand_over(to);
	return 0;
}

// The composition x[rows, cols], stated once: columns first (cheap, and it shrinks the operand), then the rows by the
// filter when the subscript is strictly increasing, else t() -> column gather with the row subscript -> t().
static int subset_gather_into(const svt_dev_csc *A, const int32_t *cols, int64_t n, ResultCsc &out, void *s)
{
	return compose_into(out, A->Rtype, A->na_background, A->nrow, n, subset_cols_ws_bytes(n),
		[&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t ws_bytes) {
			return dev_subset_cols_count_impl(A, cols, n, col_ptr, nnz, ws, ws_bytes, s);
		},
		[&](const svt_dev_csc &R, const void *, size_t) {
			return dev_subset_cols_fill_impl(A, cols, n, R.col_ptr, R.row_idx, R.val, s);
		});
}

static int subset_transpose_into(const svt_dev_csc *A, ResultCsc &out, void *s)
{
	ResultWs ws(out.mem);
	if (out.shape(A->Rtype, A->na_background, A->ncol, A->nrow) || out.entries(A->nnz) ||
	    ws.get(transpose_ws_bytes_box(A->nrow, A->nnz, box_nnz_get())))
		return -1;
	return dev_transpose_impl(A, out.c.col_ptr, out.c.row_idx, out.c.val, ws.p, ws.n, s);
}

// 0 done, -1 error, 1 the subscript is in range but not strictly increasing (nothing of `out` is of use)
static int subset_filter_into(const svt_dev_csc *A, const int32_t *rows, int64_t n, ResultCsc &out, void *s)
{
	return compose_into(out, A->Rtype, A->na_background, n, A->ncol, subset_rows_ws_bytes(A->nrow, A->ncol, A->nnz),
		[&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t ws_bytes) {
			if (dev_subset_rows_count_impl(A, rows, n, col_ptr, nnz, ws, ws_bytes, s) == 0) return 0;
			if (!g_unsupported) return -1;
			svt_clear_unsupported();
			return 1;
		},
		[&](const svt_dev_csc &R, const void *ws, size_t ws_bytes) {
			return dev_subset_rows_fill_impl(A, R.row_idx, R.val, ws, ws_bytes, s);
		});
}

// rows in any order, with repeats (all in range: the filter's count call has looked): a column gather on t(A)
static int subset_rows_general_into(const svt_dev_csc *A, const int32_t *rows, int64_t n, ResultCsc &out, void *s)
{
	g_subset_route[SUBSET_GENERAL]++;
	if (A->nnz == 0) {
		if (out.shape(A->Rtype, A->na_background, n, A->ncol) || out.entries(0))
			return -1;
		HIP_TRY(hipMemsetAsync(out.c.col_ptr, 0, ((size_t) A->ncol + 1) * 8, (hipStream_t) s));
		return 0;
	}
	ResultCsc T(out.mem), G(out.mem);
	if (subset_transpose_into(A, T, s) || subset_gather_into(&T.c, rows, n, G, s))
		return -1;
	T.drop();
	return subset_transpose_into(&G.c, out, s);
}

static int dev_subset_impl(const svt_dev_csc *A, const int32_t *rows, int64_t nrows_sel, const int32_t *cols, int64_t ncols_sel,
			   const ResultDest &to, void *stream)
{
	const char *who = "svt_dev_subset";
	if (need_allocator(who, to.alloc, to.release))
		return -1;
	ResultMem mem(who, to);
	ResultCsc B(mem), R(mem);
	const svt_dev_csc *cur = A;
	if (ncols_sel >= 0) {
		if (subset_gather_into(A, cols, ncols_sel, B, stream))
			return -1;
		cur = &B.c;
	}
	if (nrows_sel >= 0) {
		const int rc = subset_filter_into(cur, rows, nrows_sel, R, stream);
		if (rc < 0 || (rc > 0 && subset_rows_general_into(cur, rows, nrows_sel, R, stream)))
			return -1;
	} else if (cur == A) {                              // x[, ]: a copy
		hipStream_t s = (hipStream_t) stream;
		if (R.shape(A->Rtype, A->na_background, A->nrow, A->ncol) || R.entries(A->nnz))
			return -1;
		HIP_TRY(hipMemcpyAsync(R.c.col_ptr, A->col_ptr, ((size_t) A->ncol + 1) * 8, hipMemcpyDeviceToDevice, s));
		if (A->nnz > 0) {
			HIP_TRY(hipMemcpyAsync(R.c.row_idx, A->row_idx, (size_t) A->nnz * 4, hipMemcpyDeviceToDevice, s));
			HIP_TRY(hipMemcpyAsync(R.c.val, A->val, (size_t) A->nnz * elt_size(A->Rtype), hipMemcpyDeviceToDevice, s));
		}
	} else {
		std::swap(R.c, B.c);
	}
	R.hand_over(to);
	return 0;
}
extern "C" int svt_dev_subset(const svt_dev_csc *A, const int32_t *rows, int64_t nrows_sel, const int32_t *cols,
			      int64_t ncols_sel, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int64_t *out_nnz,
			      int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val, void *stream)
{
	return abi_status([&] {
		return dev_subset_impl(A, rows, nrows_sel, cols, ncols_sel, { alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val },
				       stream);
	});
}

// ---- Arith and Math (kernels_arith.hip; the element rules in svt_arith_rules.h) ----
extern "C" int svt_dev_arith_tile(void)
{
	return arith_tile();
}
extern "C" int svt_dev_arith_out_Rtype(int kind, int op, int x_Rtype, int y_Rtype)
{
	return svt_rule_out_Rtype(kind, op, x_Rtype, y_Rtype);
}
extern "C" size_t svt_dev_arith_merge_ws_bytes(int64_t ncol, int64_t x_nnz, int64_t y_nnz)
{
	return arith_ws_bytes(ncol, (x_nnz > 0 ? x_nnz : 0) + (y_nnz > 0 ? y_nnz : 0), 1);
}
extern "C" size_t svt_dev_arith_map_ws_bytes(int64_t ncol, int64_t nnz)
{
	return arith_ws_bytes(ncol, nnz, 0);
}

// the statuses that depend on the operation and the operands alone; *out_Rtype <- the type of the result
static int arith_check(const char *who, int kind, int op, const svt_dev_csc *x, const svt_dev_csc *y, int s_Rtype, int *out_Rtype)
{
	if (x == NULL || (kind == SVT_ARITH_MERGE && y == NULL))
		return svt_set_error("%s: an operand is needed", who);
	if (x->Rtype == SVT_LGLSXP || (y != NULL && y->Rtype == SVT_LGLSXP))
		return svt_set_error("arithmetic operation not supported on SparseArray object of type() \"logical\"");
	if (y != NULL && (x->nrow != y->nrow || x->ncol != y->ncol))
		return svt_set_error("non-conformable arrays");
	if (kind == SVT_ARITH_MATH && op >= SVT_MATH_ABS && op <= SVT_MATH_SIGNIF && x->Rtype != SVT_REALSXP)
		return svt_set_error("%s: Math operations take operands of type \"double\" only", who);
	const int rt = svt_rule_out_Rtype(kind, op, x->Rtype, y != NULL ? y->Rtype : s_Rtype);
	if (rt == 0 && !(kind == SVT_ARITH_MATH && op > SVT_MATH_EXPM1 && op <= SVT_MATH_SIGNIF))
		return svt_set_error("%s: unknown operation (kind %d, opcode %d) or operand type", who, kind, op);
	if (x->na_background || (y != NULL && y->na_background))
		return svt_set_unsupported("%s: NaArray operands are not supported here", who);
	if (rt == 0)
		return svt_set_unsupported("%s: Math opcode %d is not supported here", who, op);
	*out_Rtype = rt;
	return 0;
}

// The same for Compare and Logic (`rule`: ARI_RULE_COMPARE / _LOGIC; `kind`: SVT_ARITH_MERGE for x op y, SVT_ARITH_SCALAR
// for the map x op s).  Nothing here looks at a value on the device: every refusal comes before anything is launched.
static inline bool logical_family_type(int Rtype)
{
	return Rtype == SVT_LGLSXP || Rtype == SVT_INTSXP || Rtype == SVT_REALSXP;
}
static int compare_check(const char *who, int rule, int kind, int op, const svt_dev_csc *x, const svt_dev_csc *y, double s,
			 int s_Rtype)
{
	const bool merge = kind == SVT_ARITH_MERGE;
	if (x == NULL || merge != (y != NULL))
		return svt_set_error("%s: an operand is needed", who);
	if (y != NULL && (x->nrow != y->nrow || x->ncol != y->ncol))
		return svt_set_error("non-conformable arrays");
	if (!logical_family_type(x->Rtype) || (y != NULL && !logical_family_type(y->Rtype)))
		return svt_set_error("%s: operands must be of type \"logical\", \"integer\" or \"double\"", who);
	if (rule == ARI_RULE_LOGIC) {
		if (x->Rtype != SVT_LGLSXP || y->Rtype != SVT_LGLSXP)
			return svt_set_error("'Logic' operation \"&\" and \"|\" not supported on SparseArray object of type() other than "
					     "\"logical\"");
		if (op != SVT_LOGIC_AND && op != SVT_LOGIC_OR)
			return svt_set_error("%s: unknown operation (opcode %d)", who, op);
	} else {
		if (op < SVT_COMPARE_EQ || op > SVT_COMPARE_GT)
			return svt_set_error("%s: unknown operation (opcode %d)", who, op);
		if (merge && op != SVT_COMPARE_NE && op != SVT_COMPARE_LT && op != SVT_COMPARE_GT)
			return svt_set_error("%s: only \"!=\", \"<\" and \">\" are supported between two sparse operands (result wouldn't be "
					     "sparse in general)", who);
		if (!merge) {
			if (!logical_family_type(s_Rtype))
				return svt_set_error("%s: the scalar must be of type \"logical\", \"integer\" or \"double\"", who);
			if (svt_rule_compare(op, 0.0, s) != 0)
				return svt_set_error("%s: 0 compared with the scalar is not FALSE (result wouldn't be sparse)", who);
		}
	}
	if (x->na_background || (y != NULL && y->na_background))
		return svt_set_unsupported("%s: NaArray operands are not supported here", who);
	return 0;
}
// the scalar of a Compare map as the double the rule sees: an integer or logical NA arrives as INT_MIN
static inline double compare_scalar(double s, int s_Rtype)
{
	return s_Rtype != SVT_REALSXP && s == -2147483648.0 ? svt_rule_na_real() : s;
}

// The same for the subassignment merge (ARI_RULE_ASSIGN): y is the placed operand; *out_Rtype <- the wider type
static int assign_check(const char *who, const svt_dev_csc *x, const svt_dev_csc *y, int *out_Rtype)
{
	if (x == NULL || y == NULL)
		return svt_set_error("%s: an operand is needed", who);
	if (x->nrow != y->nrow || x->ncol != y->ncol)
		return svt_set_error("%s: the placed operand must have the extents of x", who);
	const int rt = svt_rule_assign_out_Rtype(x->Rtype, y->Rtype);
	if (rt == 0)
		return svt_set_error("%s: operands must be of type \"logical\", \"integer\" or \"double\"", who);
	if (x->na_background || y->na_background)
		return svt_set_unsupported("%s: NaArray operands are not supported here", who);
	*out_Rtype = rt;
	return 0;
}

// The same for pmin / pmax (ARI_RULE_PMINMAX; `kind` as for Compare; `s`: the scalar as the rule sees it) and for is.na /
// is.nan / is.infinite (ARI_RULE_ISFUN, a map without a scalar); *out_Rtype <- the type of the result
static int pminmax_check(const char *who, int rule, int kind, int op, const svt_dev_csc *x, const svt_dev_csc *y, double s,
			 int s_Rtype, int *out_Rtype)
{
	const bool merge = kind == SVT_ARITH_MERGE;
	if (x == NULL || merge != (y != NULL))
		return svt_set_error("%s: an operand is needed", who);
	if (y != NULL && (x->nrow != y->nrow || x->ncol != y->ncol))
		return svt_set_error("non-conformable arrays");
	if (!logical_family_type(x->Rtype) || (y != NULL && !logical_family_type(y->Rtype)))
		return svt_set_error("%s: operands must be of type \"logical\", \"integer\" or \"double\"", who);
	if (rule == ARI_RULE_ISFUN) {
		if (op != SVT_IS_NA && op != SVT_IS_NAN && op != SVT_IS_INFINITE)
			return svt_set_error("%s: unknown operation (opcode %d)", who, op);
		*out_Rtype = SVT_LGLSXP;
	} else {
		if ((op & ~SVT_PMINMAX_NA_RM) != SVT_PMINMAX_MIN && (op & ~SVT_PMINMAX_NA_RM) != SVT_PMINMAX_MAX)
			return svt_set_error("%s: unknown operation (opcode %d)", who, op);
		if (!merge) {
			if (!logical_family_type(s_Rtype))
				return svt_set_error("%s: the scalar must be of type \"logical\", \"integer\" or \"double\"", who);
			if (s_Rtype != SVT_REALSXP && s == s && (s != trunc(s) || s < -2147483647.0 || s > 2147483647.0))
				return svt_set_error("%s: the scalar is not a value of its integer or logical type", who);
			if (!svt_rule_pminmax_keeps_sparse(op, s, SVT_REALSXP))
				return svt_set_error("%s: %s of 0 and the scalar is not 0 (result wouldn't be sparse)", who,
						     (op & ~SVT_PMINMAX_NA_RM) == SVT_PMINMAX_MIN ? "pmin" : "pmax");
		}
		*out_Rtype = svt_rule_assign_out_Rtype(x->Rtype, merge ? y->Rtype : s_Rtype);
	}
	if (x->na_background || (y != NULL && y->na_background))
		return svt_set_unsupported("%s: NaArray operands are not supported here", who);
	return 0;
}

static ArithMergeArgs arith_merge_args(const svt_dev_csc *x, const svt_dev_csc *y, int op)
{
	ArithMergeArgs a;
	a.x_col_ptr = x->col_ptr; a.x_row_idx = x->row_idx; a.x_val = x->val; a.x_Rtype = x->Rtype; a.x_nnz = x->nnz;
	a.y_col_ptr = y->col_ptr; a.y_row_idx = y->row_idx; a.y_val = y->val; a.y_Rtype = y->Rtype; a.y_nnz = y->nnz;
	a.nrow = x->nrow; a.ncol = x->ncol; a.op = op;
	return a;
}
static ArithMapArgs arith_map_args(const svt_dev_csc *x, int kind, int op, double s, int out_Rtype)
{
	ArithMapArgs a;
	a.col_ptr = x->col_ptr; a.row_idx = x->row_idx; a.val = x->val; a.Rtype = x->Rtype; a.ncol = x->ncol; a.nnz = x->nnz;
	a.kind = kind; a.op = op; a.sd = s; a.out_Rtype = out_Rtype;
	a.si = out_Rtype == SVT_INTSXP && kind == SVT_ARITH_SCALAR ? (int32_t) s : 0;
	return a;
}

// One operation of either family (y == NULL: the map), the one statement of the checks and of count / fill.
struct ArithCall {
	const char *who;
	int kind, op;
	const svt_dev_csc *x, *y;
	double s;
	int s_Rtype;
	int out_Rtype = 0;
	int rule = ARI_RULE_ARITH;      // ARI_RULE_COMPARE / _LOGIC: `kind` says merge or map, the result is LGLSXP, no overflow word
					// (ARI_RULE_PMINMAX / _ISFUN: the same, the result typed by pminmax_check)
	const unsigned char *cover_row = NULL, *cover_leaf = NULL;      // ARI_RULE_ASSIGN (a merge): the two tables, NULL = the whole axis
									// (ARI_RULE_ASSIGN_CELLS, a merge too, reads neither)
	ArithMergeArgs merge_args() const
	{
		ArithMergeArgs a = arith_merge_args(x, y, op);
		a.rule = rule;
		a.cover_row = cover_row; a.cover_leaf = cover_leaf;
		return a;
	}
	ArithMapArgs map_args() const
	{
		ArithMapArgs a = arith_map_args(x, kind, op, s, out_Rtype);
		a.rule = rule;
		if (rule == ARI_RULE_COMPARE || rule == ARI_RULE_PMINMAX) a.sd = compare_scalar(s, s_Rtype);
		if (rule == ARI_RULE_PMINMAX) a.si = out_Rtype != SVT_REALSXP ? (int32_t) s : 0;       // (an NA or out-of-range scalar was refused)
		return a;
	}
	size_t need() const
	{
		return y != NULL ? svt_dev_arith_merge_ws_bytes(x->ncol, x->nnz, y->nnz) : arith_ws_bytes(x->ncol, x->nnz, 0);
	}
	int check(size_t ws_bytes)
	{
		if (rule == ARI_RULE_ASSIGN || rule == ARI_RULE_ASSIGN_CELLS) {
			if (const int rc = assign_check(who, x, y, &out_Rtype))
				return rc;
		} else if (rule == ARI_RULE_PMINMAX || rule == ARI_RULE_ISFUN) {
			if (const int rc = pminmax_check(who, rule, kind, op, x, y, compare_scalar(s, s_Rtype), s_Rtype, &out_Rtype))
				return rc;
		} else if (rule != ARI_RULE_ARITH) {
			if (const int rc = compare_check(who, rule, kind, op, x, y, compare_scalar(s, s_Rtype), s_Rtype))
				return rc;
			out_Rtype = SVT_LGLSXP;
		} else if (const int rc = arith_check(who, kind, op, x, y, s_Rtype, &out_Rtype)) {
			return rc;
		}
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		return 0;
	}
	int count(int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
	{
		if (const int rc = check(ws_bytes))
			return rc;
		hipStream_t st = (hipStream_t) stream;
		if (y != NULL ? launch_arith_merge_count(merge_args(), out_col_ptr, ws, st)
			      : launch_arith_map_count(map_args(), out_col_ptr, ws, st))
			return -1;
		return WsHead::total_of(ws, st, out_nnz);
	}
	int fill(int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, size_t ws_bytes, void *stream)
	{
		if (const int rc = check(ws_bytes))
			return rc;
		hipStream_t st = (hipStream_t) stream;
		return y != NULL ? launch_arith_merge_fill(merge_args(), out_row_idx, out_val, ovflow, ws, st)
				 : launch_arith_map_fill(map_args(), out_row_idx, out_val, ovflow, ws, st);
	}
	int compose(const ResultDest &to, int *out_Rtype_p, int *ovflow, void *stream)
	{
		if (need_allocator(who, to.alloc, to.release) || check(need()))
			return -1;
		if (compose_result(who, to, out_Rtype, x->na_background, x->nrow, x->ncol, need(),
				   [&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t n) { return count(col_ptr, nnz, ws, n, stream); },
				   [&](const svt_dev_csc &R, const void *ws, size_t n) { return fill(R.row_idx, R.val, ovflow, ws, n, stream); }))
			return -1;
		*out_Rtype_p = out_Rtype;
		return 0;
	}
};

// The typed outputs of an entry point brought to the form compose() takes -- V int32_t: Compare, Logic and is*(), whose
// result is logical and which have no 'out_Rtype'; V void: pmin / pmax -- with the status the caller gets
template <class V, class Compose>
static int typed_compose(const char *who, int *out_Rtype, V **out_val, Compose compose)
{
	return abi_status([&] {
		const bool lgl = std::is_same<V, int32_t>::value;
		if (out_val == NULL || (!lgl && out_Rtype == NULL))
			return svt_set_error(lgl ? "%s: 'out_val' is needed" : "%s: 'out_Rtype' and 'out_val' are needed", who);
		int rt = 0;
		void *val = NULL;
		const int rc = compose(&rt, &val);
		if (rc == 0) {
			*out_val = (V *) val;
			if (!lgl) *out_Rtype = rt;
		}
		return rc;
	});
}

extern "C" int svt_dev_arith_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int op, int64_t *out_col_ptr,
					 int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	ArithCall c = { "svt_dev_arith_merge_count", SVT_ARITH_MERGE, op, x, y, 0.0, 0 };
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_arith_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, int op, const int64_t *out_col_ptr,
					int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, size_t ws_bytes,
					void *stream)
{
	(void) out_col_ptr;                                 // (the tile prefixes in `ws` place the entries)
	ArithCall c = { "svt_dev_arith_merge_fill", SVT_ARITH_MERGE, op, x, y, 0.0, 0 };
	return abi_status([&] { return c.fill(out_row_idx, out_val, ovflow, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_arith_merge(const svt_dev_csc *x, const svt_dev_csc *y, int op, svt_dev_alloc_fn alloc,
				   svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr,
				   int32_t **out_row_idx, void **out_val, int *ovflow, void *stream)
{
	ArithCall c = { "svt_dev_arith_merge", SVT_ARITH_MERGE, op, x, y, 0.0, 0 };
	return abi_status([&] {
		return c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, out_Rtype, ovflow, stream);
	});
}
extern "C" int svt_dev_arith_map_count(const svt_dev_csc *x, int kind, int op, double s, int s_Rtype, int64_t *out_col_ptr,
				       int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	ArithCall c = { "svt_dev_arith_map_count", kind == SVT_ARITH_MERGE ? -1 : kind, op, x, NULL, s, s_Rtype };
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_arith_map_fill(const svt_dev_csc *x, int kind, int op, double s, int s_Rtype, const int64_t *out_col_ptr,
				      int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, size_t ws_bytes,
				      void *stream)
{
	(void) out_col_ptr;
	ArithCall c = { "svt_dev_arith_map_fill", kind == SVT_ARITH_MERGE ? -1 : kind, op, x, NULL, s, s_Rtype };
	return abi_status([&] { return c.fill(out_row_idx, out_val, ovflow, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_arith_map(const svt_dev_csc *x, int kind, int op, double s, int s_Rtype, svt_dev_alloc_fn alloc,
				 svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr,
				 int32_t **out_row_idx, void **out_val, int *ovflow, void *stream)
{
	ArithCall c = { "svt_dev_arith_map", kind == SVT_ARITH_MERGE ? -1 : kind, op, x, NULL, s, s_Rtype };
	return abi_status([&] {
		return c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, out_Rtype, ovflow, stream);
	});
}

// ---- Compare and Logic: the same call object under another rule; the result is LGLSXP, there is no overflow word ----
static ArithCall compare_call(const char *who, int rule, int kind, int op, const svt_dev_csc *x, const svt_dev_csc *y, double s,
			      int s_Rtype)
{
	ArithCall c = { who, kind, op, x, y, s, s_Rtype };
	c.rule = rule;
	return c;
}
// typed_compose() around the composition of such a call: 'out_Rtype' NULL for Compare, Logic and is*(), given for pmin / pmax
template <class V>
static int compare_compose(ArithCall c, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz,
			   int64_t **out_col_ptr, int32_t **out_row_idx, V **out_val, void *stream)
{
	return typed_compose(c.who, out_Rtype, out_val, [&](int *rt, void **val) {
		return c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, val }, rt, NULL, stream);
	});
}

extern "C" int svt_dev_compare_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int op, int64_t *out_col_ptr,
					   int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	ArithCall c = compare_call("svt_dev_compare_merge_count", ARI_RULE_COMPARE, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_compare_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, int op, const int64_t *out_col_ptr,
					  int32_t *out_row_idx, int32_t *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the tile prefixes in `ws` place the entries)
	ArithCall c = compare_call("svt_dev_compare_merge_fill", ARI_RULE_COMPARE, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_compare_merge(const svt_dev_csc *x, const svt_dev_csc *y, int op, svt_dev_alloc_fn alloc,
				     svt_dev_free_fn release, void *ctx, int64_t *out_nnz, int64_t **out_col_ptr,
				     int32_t **out_row_idx, int32_t **out_val, void *stream)
{
	ArithCall c = compare_call("svt_dev_compare_merge", ARI_RULE_COMPARE, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return compare_compose(c, alloc, release, ctx, NULL, out_nnz, out_col_ptr, out_row_idx, out_val, stream);
}
extern "C" int svt_dev_compare_map_count(const svt_dev_csc *x, int op, double s, int s_Rtype, int64_t *out_col_ptr,
					 int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	ArithCall c = compare_call("svt_dev_compare_map_count", ARI_RULE_COMPARE, SVT_ARITH_SCALAR, op, x, NULL, s, s_Rtype);
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_compare_map_fill(const svt_dev_csc *x, int op, double s, int s_Rtype, const int64_t *out_col_ptr,
					int32_t *out_row_idx, int32_t *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;
	ArithCall c = compare_call("svt_dev_compare_map_fill", ARI_RULE_COMPARE, SVT_ARITH_SCALAR, op, x, NULL, s, s_Rtype);
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_compare_map(const svt_dev_csc *x, int op, double s, int s_Rtype, svt_dev_alloc_fn alloc,
				   svt_dev_free_fn release, void *ctx, int64_t *out_nnz, int64_t **out_col_ptr,
				   int32_t **out_row_idx, int32_t **out_val, void *stream)
{
	ArithCall c = compare_call("svt_dev_compare_map", ARI_RULE_COMPARE, SVT_ARITH_SCALAR, op, x, NULL, s, s_Rtype);
	return compare_compose(c, alloc, release, ctx, NULL, out_nnz, out_col_ptr, out_row_idx, out_val, stream);
}
extern "C" int svt_dev_logic_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int op, int64_t *out_col_ptr,
					 int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	ArithCall c = compare_call("svt_dev_logic_merge_count", ARI_RULE_LOGIC, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_logic_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, int op, const int64_t *out_col_ptr,
					int32_t *out_row_idx, int32_t *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;
	ArithCall c = compare_call("svt_dev_logic_merge_fill", ARI_RULE_LOGIC, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_logic_merge(const svt_dev_csc *x, const svt_dev_csc *y, int op, svt_dev_alloc_fn alloc,
				   svt_dev_free_fn release, void *ctx, int64_t *out_nnz, int64_t **out_col_ptr,
				   int32_t **out_row_idx, int32_t **out_val, void *stream)
{
	ArithCall c = compare_call("svt_dev_logic_merge", ARI_RULE_LOGIC, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return compare_compose(c, alloc, release, ctx, NULL, out_nnz, out_col_ptr, out_row_idx, out_val, stream);
}

// ---- pmin / pmax and is.na / is.nan / is.infinite: the same call object under two more rules; no overflow word ----
extern "C" int svt_dev_pminmax_out_Rtype(int x_Rtype, int y_Rtype)
{
	return svt_rule_assign_out_Rtype(x_Rtype, y_Rtype);
}
extern "C" int svt_dev_pminmax_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int op, int64_t *out_col_ptr,
					   int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	ArithCall c = compare_call("svt_dev_pminmax_merge_count", ARI_RULE_PMINMAX, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_pminmax_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, int op, const int64_t *out_col_ptr,
					  int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the tile prefixes in `ws` place the entries)
	ArithCall c = compare_call("svt_dev_pminmax_merge_fill", ARI_RULE_PMINMAX, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_pminmax_merge(const svt_dev_csc *x, const svt_dev_csc *y, int op, svt_dev_alloc_fn alloc,
				     svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr,
				     int32_t **out_row_idx, void **out_val, void *stream)
{
	ArithCall c = compare_call("svt_dev_pminmax_merge", ARI_RULE_PMINMAX, SVT_ARITH_MERGE, op, x, y, 0.0, 0);
	return compare_compose(c, alloc, release, ctx, out_Rtype, out_nnz, out_col_ptr, out_row_idx, out_val, stream);
}
extern "C" int svt_dev_pminmax_map_count(const svt_dev_csc *x, int op, double s, int s_Rtype, int64_t *out_col_ptr,
					 int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	ArithCall c = compare_call("svt_dev_pminmax_map_count", ARI_RULE_PMINMAX, SVT_ARITH_SCALAR, op, x, NULL, s, s_Rtype);
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_pminmax_map_fill(const svt_dev_csc *x, int op, double s, int s_Rtype, const int64_t *out_col_ptr,
					int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;
	ArithCall c = compare_call("svt_dev_pminmax_map_fill", ARI_RULE_PMINMAX, SVT_ARITH_SCALAR, op, x, NULL, s, s_Rtype);
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_pminmax_map(const svt_dev_csc *x, int op, double s, int s_Rtype, svt_dev_alloc_fn alloc,
				   svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr,
				   int32_t **out_row_idx, void **out_val, void *stream)
{
	ArithCall c = compare_call("svt_dev_pminmax_map", ARI_RULE_PMINMAX, SVT_ARITH_SCALAR, op, x, NULL, s, s_Rtype);
	return compare_compose(c, alloc, release, ctx, out_Rtype, out_nnz, out_col_ptr, out_row_idx, out_val, stream);
}
extern "C" int svt_dev_isfun_map_count(const svt_dev_csc *x, int op, int64_t *out_col_ptr, int64_t *out_nnz, void *ws,
				       size_t ws_bytes, void *stream)
{
	ArithCall c = compare_call("svt_dev_isfun_map_count", ARI_RULE_ISFUN, SVT_ARITH_SCALAR, op, x, NULL, 0.0, 0);
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_isfun_map_fill(const svt_dev_csc *x, int op, const int64_t *out_col_ptr, int32_t *out_row_idx,
				      int32_t *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;
	ArithCall c = compare_call("svt_dev_isfun_map_fill", ARI_RULE_ISFUN, SVT_ARITH_SCALAR, op, x, NULL, 0.0, 0);
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_isfun_map(const svt_dev_csc *x, int op, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx,
				 int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, int32_t **out_val, void *stream)
{
	ArithCall c = compare_call("svt_dev_isfun_map", ARI_RULE_ISFUN, SVT_ARITH_SCALAR, op, x, NULL, 0.0, 0);
	return compare_compose(c, alloc, release, ctx, NULL, out_nnz, out_col_ptr, out_row_idx, out_val, stream);
}

// ---- sweep: x op stats[k], Arith or Compare with one element of a device vector per row or per leaf ----
// One operation of the third family: the one statement of its checks and of count / fill / compose.  The statuses are
// those of the maps; what is added is the geometry of the vector and the element the device refused.
struct SweepCall {
	const char *who;
	int rule, op;
	const svt_dev_csc *x;
	const void *stats;
	int stats_Rtype;
	int64_t stats_len;
	int with_rows;
	int64_t stride, len;
	int out_Rtype = 0;

	size_t need() const { return arith_ws_bytes(x->ncol, x->nnz, 0); }
	int check(size_t ws_bytes)
	{
		if (x == NULL)
			return svt_set_error("%s: an operand is needed", who);
		if (rule == ARI_RULE_COMPARE) {
			if (!logical_family_type(x->Rtype) || !logical_family_type(stats_Rtype))
				return svt_set_error("%s: the operand and the vector must be of type \"logical\", \"integer\" or \"double\"", who);
			if (op < SVT_COMPARE_EQ || op > SVT_COMPARE_GT)
				return svt_set_error("%s: unknown operation (opcode %d)", who, op);
			out_Rtype = SVT_LGLSXP;
		} else if (rule == ARI_RULE_PMINMAX) {
			if (!logical_family_type(x->Rtype) || !logical_family_type(stats_Rtype))
				return svt_set_error("%s: the operand and the vector must be of type \"logical\", \"integer\" or \"double\"", who);
			if ((op & ~SVT_PMINMAX_NA_RM) != SVT_PMINMAX_MIN && (op & ~SVT_PMINMAX_NA_RM) != SVT_PMINMAX_MAX)
				return svt_set_error("%s: unknown operation (opcode %d)", who, op);
			out_Rtype = svt_rule_assign_out_Rtype(x->Rtype, stats_Rtype);
		} else {
			if (x->Rtype == SVT_LGLSXP)
				return svt_set_error("arithmetic operation not supported on SparseArray object of type() \"logical\"");
			if (op == SVT_ARITH_ADD || op == SVT_ARITH_SUB)
				return svt_set_error("%s: \"%s\" is not supported between a SparseArray object and a vector (result wouldn't be "
						     "sparse in general)", who, op == SVT_ARITH_ADD ? "+" : "-");
			out_Rtype = svt_rule_out_Rtype(SVT_ARITH_SCALAR, op, x->Rtype, stats_Rtype);
			if (out_Rtype == 0)
				return svt_set_error("%s: unknown operation (opcode %d) or operand type", who, op);
		}
		// the vector against the three integers of the index k = (with_rows ? row : 0) + (with_rows ? nrow : 1) * ((leaf / stride) % len)
		if ((with_rows != 0 && with_rows != 1) || stride < 1 || len < 0 || stats_len < 0)
			return svt_set_error("%s: invalid vector geometry", who);
		if (x->ncol > 0 && (len < 1 || stride > x->ncol || len > x->ncol / stride || x->ncol % (stride * len) != 0))
			return svt_set_error("%s: 'stride' and 'len' do not divide the operand's leaves", who);
		const int64_t mult = with_rows ? x->nrow : 1;
		if ((len != 0 && mult > INT64_MAX / len) || stats_len != mult * len)
			return svt_set_error("%s: the vector's length does not match the extents it sweeps (%lld, expected %lld)", who,
					     (long long) stats_len, (long long) (len != 0 && mult > INT64_MAX / len ? -1 : mult * len));
		if (stats_len > 0 && stats == NULL)
			return svt_set_error("%s: the vector is needed", who);
		if (x->na_background)
			return svt_set_unsupported("%s: NaArray operands are not supported here", who);
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		return 0;
	}
	ArithSweepArgs args() const
	{
		ArithSweepArgs a;
		a.col_ptr = x->col_ptr; a.row_idx = x->row_idx; a.val = x->val; a.Rtype = x->Rtype;
		a.nrow = x->nrow; a.ncol = x->ncol; a.nnz = x->nnz;
		a.rule = rule; a.op = op; a.stats = stats; a.stats_Rtype = stats_Rtype;
		a.with_rows = with_rows; a.stride = stride; a.len = len; a.out_Rtype = out_Rtype;
		return a;
	}
	int count(int64_t *out_col_ptr, int64_t *out_nnz, int64_t *bad_index, void *ws, size_t ws_bytes, void *stream)
	{
		if (bad_index != NULL) *bad_index = -1;
		if (const int rc = check(ws_bytes))
			return rc;
		hipStream_t st = (hipStream_t) stream;
		if (launch_arith_sweep_count(args(), out_col_ptr, ws, st))
			return -1;
		WsHead head;                                        // (the third word: the refused element)
		if (head.read(ws, st, 3))
			return -1;
		if (head.third != -1) {
			if (bad_index != NULL) *bad_index = head.third;
			return svt_set_error("%s: element %lld of the vector does not keep the result sparse", who, (long long) head.third);
		}
		*out_nnz = head.total;
		return 0;
	}
	int fill(int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, size_t ws_bytes, void *stream)
	{
		if (const int rc = check(ws_bytes))
			return rc;
		return launch_arith_sweep_fill(args(), out_row_idx, out_val, ovflow, ws, (hipStream_t) stream);
	}
	int compose(const ResultDest &to, int *out_Rtype_p, int *ovflow, int64_t *bad_index, void *stream)
	{
		if (bad_index != NULL) *bad_index = -1;
		if (need_allocator(who, to.alloc, to.release) || (x == NULL ? check(0) : check(need())))
			return -1;
		if (compose_result(who, to, out_Rtype, x->na_background, x->nrow, x->ncol, need(),
				   [&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t n) { return count(col_ptr, nnz, bad_index, ws, n, stream); },
				   [&](const svt_dev_csc &R, const void *ws, size_t n) { return fill(R.row_idx, R.val, ovflow, ws, n, stream); }))
			return -1;
		*out_Rtype_p = out_Rtype;
		return 0;
	}
};

extern "C" size_t svt_dev_sweep_ws_bytes(int64_t ncol, int64_t nnz)
{
	return arith_ws_bytes(ncol, nnz, 0);
}
extern "C" int svt_dev_arith_sweep_count(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
					 int with_rows, int64_t stride, int64_t len, int64_t *out_col_ptr, int64_t *out_nnz,
					 int64_t *bad_index, void *ws, size_t ws_bytes, void *stream)
{
	SweepCall c = { "svt_dev_arith_sweep_count", ARI_RULE_ARITH, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, bad_index, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_arith_sweep_fill(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
					int with_rows, int64_t stride, int64_t len, const int64_t *out_col_ptr, int32_t *out_row_idx,
					void *out_val, int *ovflow, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the tile prefixes in `ws` place the entries)
	SweepCall c = { "svt_dev_arith_sweep_fill", ARI_RULE_ARITH, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return abi_status([&] { return c.fill(out_row_idx, out_val, ovflow, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_arith_sweep(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
				   int with_rows, int64_t stride, int64_t len, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
				   void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx,
				   void **out_val, int *ovflow, int64_t *bad_index, void *stream)
{
	SweepCall c = { "svt_dev_arith_sweep", ARI_RULE_ARITH, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return abi_status([&] {
		return c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, out_Rtype, ovflow, bad_index, stream);
	});
}
extern "C" int svt_dev_compare_sweep_count(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
					   int with_rows, int64_t stride, int64_t len, int64_t *out_col_ptr, int64_t *out_nnz,
					   int64_t *bad_index, void *ws, size_t ws_bytes, void *stream)
{
	SweepCall c = { "svt_dev_compare_sweep_count", ARI_RULE_COMPARE, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, bad_index, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_compare_sweep_fill(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
					  int with_rows, int64_t stride, int64_t len, const int64_t *out_col_ptr, int32_t *out_row_idx,
					  int32_t *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;
	SweepCall c = { "svt_dev_compare_sweep_fill", ARI_RULE_COMPARE, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_compare_sweep(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
				     int with_rows, int64_t stride, int64_t len, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
				     void *ctx, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, int32_t **out_val,
				     int64_t *bad_index, void *stream)
{
	SweepCall c = { "svt_dev_compare_sweep", ARI_RULE_COMPARE, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return typed_compose(c.who, NULL, out_val, [&](int *rt, void **val) {
		return c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, val }, rt, NULL, bad_index, stream);
	});
}
extern "C" int svt_dev_pminmax_sweep_count(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
					   int with_rows, int64_t stride, int64_t len, int64_t *out_col_ptr, int64_t *out_nnz,
					   int64_t *bad_index, void *ws, size_t ws_bytes, void *stream)
{
	SweepCall c = { "svt_dev_pminmax_sweep_count", ARI_RULE_PMINMAX, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, bad_index, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_pminmax_sweep_fill(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
					  int with_rows, int64_t stride, int64_t len, const int64_t *out_col_ptr, int32_t *out_row_idx,
					  void *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;
	SweepCall c = { "svt_dev_pminmax_sweep_fill", ARI_RULE_PMINMAX, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_pminmax_sweep(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
				     int with_rows, int64_t stride, int64_t len, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
				     void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx,
				     void **out_val, int64_t *bad_index, void *stream)
{
	SweepCall c = { "svt_dev_pminmax_sweep", ARI_RULE_PMINMAX, op, x, stats, stats_Rtype, stats_len, with_rows, stride, len };
	return typed_compose(c.who, out_Rtype, out_val, [&](int *rt, void **val) {
		return c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, val }, rt, NULL, bad_index, stream);
	});
}

// ---- abind / cbind / rbind (kernels_abind.hip; C_abind_SVT_SparseArray_objects, src/SparseArray_abind.c) ----
extern "C" int svt_dev_abind_tile(void)
{
	return abind_tile();
}
extern "C" size_t svt_dev_abind_ws_bytes(int nobj, int64_t out_nleaves, int rows_form)
{
	if (nobj < 0) nobj = 0;
	if (out_nleaves < 0) out_nleaves = 0;
	return abind_ws_bytes(nobj, rows_form ? out_nleaves * nobj : out_nleaves);
}

static inline int abind_type_rank(int Rtype)
{
	return Rtype == SVT_LGLSXP ? 0 : Rtype == SVT_INTSXP ? 1 : Rtype == SVT_REALSXP ? 2 : -1;
}

// One call: every check that needs no GPU, the result's extents and the table of objects the count kernels read.
struct AbindCall {
	const char *who;
	std::vector<AbindObj> table;
	AbindArgs a;
	int64_t out_nrow = 0;
	int na_background = 0;

	int plan(const svt_dev_csc *const *objs, int nobj, int64_t inner, const int64_t *ext, int ans_Rtype)
	{
		memset(&a, 0, sizeof(a));
		if (nobj < 1 || objs == NULL)
			return svt_set_error("%s: at least one object is needed", who);
		for (int n = 0; n < nobj; n++)
			if (objs[n] == NULL)
				return svt_set_error("%s: object %d is NULL", who, n + 1);
		if (abind_type_rank(ans_Rtype) < 0)
			return svt_set_error("invalid requested type");
		a.uniform = 1;
		for (int n = 0; n < nobj; n++) {
			const int r = abind_type_rank(objs[n]->Rtype);
			if (r < 0)
				return svt_set_error("%s: object %d has a type that is not logical, integer or double", who, n + 1);
			if (r > abind_type_rank(ans_Rtype))
				return svt_set_error("%s: the requested type is narrower than the type of object %d", who, n + 1);
			if (elt_size(objs[n]->Rtype) != elt_size(ans_Rtype)) a.uniform = 0;
			if ((objs[n]->na_background != 0) != (objs[0]->na_background != 0))
				return svt_set_error("%s: NaArray objects and ordinary objects cannot be bound together", who);
			if (objs[n]->nrow < 0 || objs[n]->ncol < 0 || objs[n]->nnz < 0)
				return svt_set_error("%s: object %d has a negative extent", who, n + 1);
		}
		na_background = objs[0]->na_background != 0;
		a.nobj = nobj;
		a.rows_form = ext == NULL;
		a.ans_Rtype = ans_Rtype;
		table.resize((size_t) nobj);
		int64_t run = 0;                                    // off[n] / start[n]
		if (a.rows_form) {
			for (int n = 0; n < nobj; n++) {
				if (objs[n]->ncol != objs[0]->ncol)
					return svt_set_error("%s: object %d has %lld leaves, object 1 has %lld", who, n + 1,
							     (long long) objs[n]->ncol, (long long) objs[0]->ncol);
				table[(size_t) n].shift = run;
				run += objs[n]->nrow;
				if (run > 0x7FFFFFFFLL)
					return svt_set_error("%s: the rows of the objects sum past 2^31 - 1", who);
			}
			out_nrow = run;
			a.out_nleaves = objs[0]->ncol;
			if (a.out_nleaves > 0x7FFFFFFELL / nobj)
				return svt_set_error("%s: more than 2^31 - 2 pieces", who);
			a.npieces = a.out_nleaves * nobj;
		} else {
			if (inner < 0)
				return svt_set_error("%s: 'inner' must be >= 0", who);
			int64_t outer = -1;
			for (int n = 0; n < nobj; n++) {
				if (ext[n] < 0)
					return svt_set_error("%s: object %d has a negative extent", who, n + 1);
				if (objs[n]->nrow != objs[0]->nrow)
					return svt_set_error("%s: object %d has %lld rows, object 1 has %lld", who, n + 1,
							     (long long) objs[n]->nrow, (long long) objs[0]->nrow);
				const int64_t slab = inner * ext[n];        // (svt_dev_csc counts leaves in int64; ext and inner come from int dims)
				if (slab == 0 ? objs[n]->ncol != 0 : objs[n]->ncol % slab != 0)
					return svt_set_error("%s: the leaves of object %d are not inner * ext * outer", who, n + 1);
				if (slab != 0) {
					if (outer < 0) outer = objs[n]->ncol / slab;
					if (objs[n]->ncol / slab != outer)
						return svt_set_error("%s: the leaves of object %d are not inner * ext * outer for the outer of "
								     "the objects before it", who, n + 1);
				}
				table[(size_t) n].shift = run;
				table[(size_t) n].ext = ext[n];
				run += ext[n];
			}
			out_nrow = objs[0]->nrow;
			a.inner = inner;
			a.D = run;
			a.out_nleaves = outer > 0 ? inner * run * outer : 0;
			if (a.out_nleaves > 0x7FFFFFFELL)
				return svt_set_error("%s: more than 2^31 - 2 pieces", who);
			a.npieces = a.out_nleaves;
		}
		for (int n = 0; n < nobj; n++) {
			AbindObj &o = table[(size_t) n];
			o.col_ptr = objs[n]->col_ptr; o.row_idx = objs[n]->row_idx; o.val = objs[n]->val;
			o.nnz = objs[n]->nnz; o.nleaves = objs[n]->ncol; o.Rtype = objs[n]->Rtype; o.pad = 0;
			a.max_nnz += objs[n]->nnz;
		}
		a.objs = table.data();
		return 0;
	}
	size_t need() const { return abind_ws_bytes(a.nobj, a.npieces); }

	int count(int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
	{
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		hipStream_t st = (hipStream_t) stream;
		if (a.npieces == 0) {                               // a result without leaves: nothing to count
			HIP_TRY(hipMemsetAsync(out_col_ptr, 0, 8, st));
			*out_nnz = 0;
			return 0;
		}
		if (launch_abind_count(a, out_col_ptr, ws, st))
			return -1;
		WsHead head;
		if (head.read(ws, st))                              // (the table of objects has been copied by now)
			return -1;
		if (head.flag)
			return svt_set_error("%s: the column pointers of an object descend or pass its nonzeros", who);
		*out_nnz = head.total;
		return 0;
	}
	int fill(int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes, void *stream)
	{
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		return launch_abind_fill(a, out_row_idx, out_val, ws, (hipStream_t) stream);
	}
	int compose(const ResultDest &to, void *stream)
	{
		if (need_allocator(who, to.alloc, to.release))
			return -1;
		return compose_result(who, to, a.ans_Rtype, na_background, out_nrow, a.out_nleaves, need(),
			[&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t n) { return count(col_ptr, nnz, ws, n, stream); },
			[&](const svt_dev_csc &R, const void *ws, size_t n) { return fill(R.row_idx, R.val, ws, n, stream); });
	}
};

// x as it is in the type `rt`, the one-object case of abind: the result of a subassignment that selects nothing
static int compose_coerced(const char *who, const svt_dev_csc *x, int rt, const ResultDest &to, int *out_Rtype, void *stream)
{
	AbindCall c = { who };
	const svt_dev_csc *objs[1] = { x };
	if (c.plan(objs, 1, 0, NULL, rt) || c.compose(to, stream))
		return -1;
	*out_Rtype = rt;
	return 0;
}

extern "C" int svt_dev_abind_count(const svt_dev_csc *const *objs, int nobj, int64_t inner, const int64_t *ext, int ans_Rtype,
				   int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		AbindCall c = { "svt_dev_abind_count" };
		if (c.plan(objs, nobj, inner, ext, ans_Rtype)) return -1;
		return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_abind_fill(const svt_dev_csc *const *objs, int nobj, int64_t inner, const int64_t *ext, int ans_Rtype,
				  const int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val, const void *ws,
				  size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the piece starts in `ws` place the entries)
	return abi_status([&] {
		AbindCall c = { "svt_dev_abind_fill" };
		if (c.plan(objs, nobj, inner, ext, ans_Rtype)) return -1;
		return c.fill(out_row_idx, out_val, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_abind(const svt_dev_csc *const *objs, int nobj, int64_t inner, const int64_t *ext, int ans_Rtype,
			     svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int64_t *out_nrow, int64_t *out_nleaves,
			     int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val, void *stream)
{
	return abi_status([&] {
		AbindCall c = { "svt_dev_abind" };
		if (c.plan(objs, nobj, inner, ext, ans_Rtype) ||
		    c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, stream))
			return -1;
		*out_nrow = c.out_nrow;
		*out_nleaves = c.a.out_nleaves;
		return 0;
	});
}

// ---- coercions dense array <-> operand, nzwhich (kernels_coerce.hip; C_build_SVT_from_Rarray,
// C_from_SVT_SparseArray_to_Rarray, C_nzwhich_SVT, src/SVT_SparseArray_class.c) ----
extern "C" int svt_dev_coerce_tile(void)
{
	return coerce_tile();
}
extern "C" size_t svt_dev_from_dense_ws_bytes(int64_t ncells)
{
	return from_dense_ws_bytes(ncells);
}

// `from` to `to`: 0 the same type or a wider one; a narrower one is "not supported here", another type an error
static int coerce_type_check(const char *who, int from_Rtype, int to_Rtype)
{
	const int st = svt_rule_coerce_status(from_Rtype, to_Rtype);
	if (st < 0)
		return svt_set_error("%s: the types must be logical, integer or double", who);
	if (st > 0)
		return svt_set_unsupported("%s: coercion to a narrower type is not supported here", who);
	return 0;
}

// One call of dense -> sparse: every check that needs no GPU, then count / fill / their composition.
struct FromDenseCall {
	const char *who;
	FromDenseArgs a;

	int plan(const void *x, int x_Rtype, int64_t nrow, int64_t nleaves, int ans_Rtype, int na_background)
	{
		memset(&a, 0, sizeof(a));
		if (const int rc = coerce_type_check(who, x_Rtype, ans_Rtype))
			return rc;
		if (nrow < 0 || nleaves < 0)
			return svt_set_error("%s: negative extent", who);
		if (nrow > 0x7FFFFFFFLL)
			return svt_set_error("%s: more than 2^31 - 1 rows", who);
		if (nleaves > 0 && nrow > INT64_MAX / nleaves)
			return svt_set_error("%s: nrow * nleaves overflows 64 bits", who);
		a.x = x; a.x_Rtype = x_Rtype;
		a.nrow = nrow; a.nleaves = nleaves; a.ncells = nrow * nleaves;
		a.ans_Rtype = ans_Rtype; a.na_background = na_background != 0;
		if (a.ncells > 0 && x == NULL)
			return svt_set_error("%s: 'x' is NULL", who);
		return 0;
	}
	size_t need() const { return from_dense_ws_bytes(a.ncells); }

	int count(int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
	{
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		hipStream_t st = (hipStream_t) stream;
		if (a.ncells == 0) {                                // no rows or no leaves: nothing to count, every pointer is 0
			HIP_TRY(hipMemsetAsync(out_col_ptr, 0, ((size_t) a.nleaves + 1) * 8, st));
			*out_nnz = 0;
			return 0;
		}
		if (launch_from_dense_count(a, out_col_ptr, ws, st))
			return -1;
		return WsHead::total_of(ws, st, out_nnz);
	}
	int fill(int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes, void *stream)
	{
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		return launch_from_dense_fill(a, out_row_idx, out_val, ws, (hipStream_t) stream);
	}
	int compose(const ResultDest &to, void *stream)
	{
		if (need_allocator(who, to.alloc, to.release))
			return -1;
		return compose_result(who, to, a.ans_Rtype, a.na_background, a.nrow, a.nleaves, need(),
			[&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t n) { return count(col_ptr, nnz, ws, n, stream); },
			[&](const svt_dev_csc &R, const void *ws, size_t n) { return fill(R.row_idx, R.val, ws, n, stream); });
	}
};

extern "C" int svt_dev_from_dense_count(const void *x, int x_Rtype, int64_t nrow, int64_t nleaves, int ans_Rtype, int na_background,
					int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		FromDenseCall c = { "svt_dev_from_dense_count" };
		if (c.plan(x, x_Rtype, nrow, nleaves, ans_Rtype, na_background)) return -1;
		return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_from_dense_fill(const void *x, int x_Rtype, int64_t nrow, int64_t nleaves, int ans_Rtype, int na_background,
				       const int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val, const void *ws,
				       size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the tile bases in `ws` place the entries)
	return abi_status([&] {
		FromDenseCall c = { "svt_dev_from_dense_fill" };
		if (c.plan(x, x_Rtype, nrow, nleaves, ans_Rtype, na_background)) return -1;
		return c.fill(out_row_idx, out_val, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_from_dense(const void *x, int x_Rtype, int64_t nrow, int64_t nleaves, int ans_Rtype, int na_background,
				  svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int64_t *out_nnz,
				  int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val, void *stream)
{
	return abi_status([&] {
		FromDenseCall c = { "svt_dev_from_dense" };
		if (c.plan(x, x_Rtype, nrow, nleaves, ans_Rtype, na_background)) return -1;
		return c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, stream);
	});
}

// ---- poissonSparseArray() and simple_rpois() (C_poissonSparseArray, C_simple_rpois, src/randomSparseArray.c): the
// compaction of dense -> sparse over generated cells (kernels_coerce.hip, svt_random_rules.h) ----
extern "C" int svt_poisson_ticks(double lambda, double *ticks32)
{
	double local[SVT_POISSON_MAX_TICKS];
	return svt_rule_poisson_ticks(lambda, ticks32 != NULL ? ticks32 : local);
}
extern "C" size_t svt_dev_poisson_ws_bytes(int64_t ncells)
{
	return from_dense_ws_bytes(ncells);
}
static int poisson_table(const char *who, double lambda, svt_poisson_table *t)
{
	memset(t, 0, sizeof(*t));
	if (!(lambda >= 0.0))
		return svt_set_error("%s: 'lambda' must be a non-negative number", who);
	t->n = svt_rule_poisson_ticks(lambda, t->ticks);
	if (t->n < 0)
		return svt_set_error("'lambda' too big?");
	return 0;
}

// One call of the generator: every check that needs no GPU, then count / fill / their composition.
struct PoissonCall {
	const char *who;
	PoissonArgs a;

	int plan(double lambda, int64_t seed, int64_t nrow, int64_t first_leaf, int64_t nleaves)
	{
		memset(&a, 0, sizeof(a));
		if (poisson_table(who, lambda, &a.table))
			return -1;
		if (nrow < 0 || nleaves < 0 || first_leaf < 0)
			return svt_set_error("%s: negative extent", who);
		if (nrow > 0x7FFFFFFFLL)
			return svt_set_error("%s: more than 2^31 - 1 rows", who);
		if (first_leaf > INT64_MAX - nleaves || (nrow > 0 && first_leaf + nleaves > INT64_MAX / nrow))
			return svt_set_error("%s: (first_leaf + nleaves) * nrow overflows 64 bits", who);
		a.seed = (uint64_t) seed;
		a.nrow = nrow; a.first_leaf = first_leaf; a.nleaves = nleaves; a.ncells = nrow * nleaves;
		return 0;
	}
	size_t need() const { return from_dense_ws_bytes(a.ncells); }

	int count(int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
	{
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		hipStream_t st = (hipStream_t) stream;
		if (a.ncells == 0) {                                // no rows or no leaves: nothing to count, every pointer is 0
			HIP_TRY(hipMemsetAsync(out_col_ptr, 0, ((size_t) a.nleaves + 1) * 8, st));
			*out_nnz = 0;
			return 0;
		}
		if (launch_poisson_count(a, out_col_ptr, ws, st))
			return -1;
		return WsHead::total_of(ws, st, out_nnz);
	}
	int fill(int32_t *out_row_idx, int32_t *out_val, const void *ws, size_t ws_bytes, void *stream)
	{
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		return launch_poisson_fill(a, out_row_idx, out_val, ws, (hipStream_t) stream);
	}
	int compose(const ResultDest &to, void *stream)
	{
		if (need_allocator(who, to.alloc, to.release))
			return -1;
		return compose_result(who, to, SVT_INTSXP, 0, a.nrow, a.nleaves, need(),
			[&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t n) { return count(col_ptr, nnz, ws, n, stream); },
			[&](const svt_dev_csc &R, const void *ws, size_t n) { return fill(R.row_idx, (int32_t *) R.val, ws, n, stream); });
	}
};

extern "C" int svt_dev_poisson_count(double lambda, int64_t seed, int64_t nrow, int64_t first_leaf, int64_t nleaves,
				     int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		PoissonCall c = { "svt_dev_poisson_count" };
		if (c.plan(lambda, seed, nrow, first_leaf, nleaves)) return -1;
		return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_poisson_fill(double lambda, int64_t seed, int64_t nrow, int64_t first_leaf, int64_t nleaves,
				    const int64_t *out_col_ptr, int32_t *out_row_idx, int32_t *out_val, const void *ws,
				    size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the tile bases in `ws` place the entries)
	return abi_status([&] {
		PoissonCall c = { "svt_dev_poisson_fill" };
		if (c.plan(lambda, seed, nrow, first_leaf, nleaves)) return -1;
		return c.fill(out_row_idx, out_val, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_poisson(double lambda, int64_t seed, int64_t nrow, int64_t first_leaf, int64_t nleaves,
			       svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int64_t *out_nnz, int64_t **out_col_ptr,
			       int32_t **out_row_idx, void **out_val, void *stream)
{
	return abi_status([&] {
		PoissonCall c = { "svt_dev_poisson" };
		if (c.plan(lambda, seed, nrow, first_leaf, nleaves)) return -1;
		return c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, stream);
	});
}
extern "C" int svt_dev_rpois(double lambda, int64_t seed, int64_t first, int64_t n, int32_t *out, void *stream)
{
	const char *who = "svt_dev_rpois";
	return abi_status([&] {
		svt_poisson_table t;
		if (poisson_table(who, lambda, &t))
			return -1;
		if (n < 0)
			return svt_set_error("'n' cannot be negative");
		if (first < 0 || first > INT64_MAX - n)
			return svt_set_error("%s: 'first' is negative or first + n overflows 64 bits", who);
		if (n > 0 && out == NULL)
			return svt_set_error("%s: 'out' is NULL", who);
		return launch_rpois(t, (uint64_t) seed, first, n, out, (hipStream_t) stream);
	});
}

extern "C" int svt_dev_to_dense(const svt_dev_csc *A, int na_background, int out_Rtype, void *out, int *bad, void *stream)
{
	const char *who = "svt_dev_to_dense";
	return abi_status([&] {
		if (A == NULL)
			return svt_set_error("%s: the operand is NULL", who);
		if (const int rc = coerce_type_check(who, A->Rtype, out_Rtype))
			return rc;
		if (A->nrow < 0 || A->ncol < 0 || A->nnz < 0 || A->nrow > 0x7FFFFFFFLL)
			return svt_set_error("%s: the operand has a negative extent or more than 2^31 - 1 rows", who);
		if (A->ncol > 0 && A->nrow > INT64_MAX / A->ncol)
			return svt_set_error("%s: nrow * ncol overflows 64 bits", who);
		if (A->nrow == 0 || A->ncol == 0)
			return 0;                                   // an output without cells
		if (out == NULL || ((uintptr_t) out & 15) != 0)
			return svt_set_error("%s: 'out' must be aligned to 16 bytes", who);
		return launch_to_dense(A->col_ptr, A->row_idx, A->val, A->Rtype, A->nrow, A->ncol, A->nnz, na_background != 0,
				       out_Rtype, out, bad, (hipStream_t) stream);
	});
}

extern "C" int svt_dev_nzwhich(const svt_dev_csc *A, int ndim, const int64_t *dim, int arr_ind, void *out, void *stream)
{
	const char *who = "svt_dev_nzwhich";
	return abi_status([&] {
		if (A == NULL)
			return svt_set_error("%s: the operand is NULL", who);
		if (ndim < 1 || ndim > 8 || dim == NULL)
			return svt_set_error("%s: between 1 and 8 dimensions", who);
		int64_t leaves = 1;
		for (int k = 0; k < ndim; k++) {
			if (dim[k] < 0 || dim[k] > 0x7FFFFFFFLL)
				return svt_set_error("%s: an extent outside 0 .. 2^31 - 1", who);
			if (k > 0) {
				if (dim[k] != 0 && leaves > INT64_MAX / dim[k])
					return svt_set_error("%s: 'dim' does not match the operand's rows and leaves", who);
				leaves *= dim[k];
			}
		}
		if (dim[0] != A->nrow || leaves != A->ncol)
			return svt_set_error("%s: 'dim' does not match the operand's rows and leaves", who);
		if (A->ncol > 0x7FFFFFFFLL)                         // (a tile's leaves are numbered in 32 bits)
			return svt_set_error("%s: more than 2^31 - 1 leaves", who);
		if (A->nnz < 0 || (A->nnz > 0 && (A->nrow == 0 || A->ncol == 0)))
			return svt_set_error("%s: nonzeros in an operand without cells", who);
		if (arr_ind && A->nnz > 0x7FFFFFFFLL)
			return svt_set_error("too many nonzero elements in SVT_SparseArray object to return their \"array coordinates\" "
					     "(n-tuples) in a matrix");
		if (A->nnz > 0 && out == NULL)
			return svt_set_error("%s: 'out' is NULL", who);
		return launch_nzwhich(A->col_ptr, A->row_idx, A->nrow, A->ncol, A->nnz, ndim, dim, arr_ind != 0, out,
				      (hipStream_t) stream);
	});
}

// ---- subassignment x[i, j] <- value: kernels_subassign.hip places the new values as an operand Y and marks what the
// subscripts cover, the merge of kernels_arith.hip under ARI_RULE_ASSIGN (svt_rule_assign) makes the result ----
extern "C" int svt_dev_subassign_tile(void)
{
	return subassign_tile();
}
extern "C" size_t svt_dev_subassign_place_ws_bytes(int64_t nrow, int64_t ncol)
{
	return subassign_ws_bytes(nrow, ncol);
}

// The merge that writes the placed operand y over x, under the two cover tables or (no tables) under the rule of the cells
static ArithCall assign_call(const char *who, const svt_dev_csc *x, const svt_dev_csc *y, const unsigned char *cover_row,
			     const unsigned char *cover_leaf, int rule = ARI_RULE_ASSIGN)
{
	ArithCall c = { who, SVT_ARITH_MERGE, 0, x, y, 0.0, 0 };
	c.rule = rule;
	c.cover_row = cover_row; c.cover_leaf = cover_leaf;
	return c;
}
static ArithCall assign_cells_call(const char *who, const svt_dev_csc *x, const svt_dev_csc *y)
{
	return assign_call(who, x, y, NULL, NULL, ARI_RULE_ASSIGN_CELLS);
}
// what a composed subassignment refuses about x and the value's type before it places anything; *rt <- the wider type
static int assign_out_Rtype(const char *who, const svt_dev_csc *x, int v_Rtype, int *rt)
{
	*rt = svt_rule_assign_out_Rtype(x->Rtype, v_Rtype);
	if (*rt == 0)
		return svt_set_error("%s: operands must be of type \"logical\", \"integer\" or \"double\"", who);
	if (x->na_background)
		return svt_set_unsupported("%s: NaArray operands are not supported here", who);
	return 0;
}

// One placement, of either form (v != NULL: the SVT form): every check that needs no GPU, then count / fill.
struct SubassignCall {
	const char *who;
	SubassignArgs a;

	int plan(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel, const int32_t *leaves, int64_t nleaves_sel,
		 const void *vals, int64_t nvals, int v_Rtype, const svt_dev_csc *v, bool svt_form)
	{
		memset(&a, 0, sizeof(a));
		if (nrow < 0 || nrow > 0x7FFFFFFFLL || ncol < 0 || ncol > 0x7FFFFFFELL)
			return svt_set_error("%s: extents outside 0 .. 2^31 - 1 rows, 0 .. 2^31 - 2 leaves", who);
		if (nrows_sel > 0x7FFFFFFFLL || nleaves_sel > 0x7FFFFFFELL)
			return svt_set_error("%s: at most 2^31 - 1 row subscripts and 2^31 - 2 leaves", who);
		if ((nrows_sel > 0 && rows == NULL) || (nleaves_sel > 0 && leaves == NULL))
			return svt_set_error("%s: a subscript is needed (a length < 0 stands for the whole axis)", who);
		if (svt_form) {
			if (v == NULL)
				return svt_set_error("%s: the value operand is needed", who);
			v_Rtype = v->Rtype;
		} else if (nvals < 1 || vals == NULL) {
			return svt_set_error("replacement has length zero");
		}
		if (!logical_family_type(v_Rtype))
			return svt_set_error("%s: the value must be of type \"logical\", \"integer\" or \"double\"", who);
		if (svt_form) {
			if (v->nrow != (nrows_sel < 0 ? nrow : nrows_sel) || v->ncol != (nleaves_sel < 0 ? ncol : nleaves_sel))
				return svt_set_error("the selection and supplied value must have the same dimensions");
			if (v->na_background)
				return svt_set_unsupported("%s: NaArray operands are not supported here", who);
			a.v_col_ptr = v->col_ptr; a.v_row_idx = v->row_idx; a.v_val = v->val; a.v_nnz = v->nnz;
		}
		a.nrow = nrow; a.ncol = ncol;
		a.rows = rows; a.nrows_sel = nrows_sel < 0 ? -1 : nrows_sel;
		a.leaves = leaves; a.nleaves_sel = nleaves_sel < 0 ? -1 : nleaves_sel;
		a.vals = vals; a.nvals = nvals; a.v_Rtype = v_Rtype;
		return 0;
	}
	size_t need() const { return subassign_ws_bytes(a.nrow, a.ncol); }
	int count(int64_t *y_col_ptr, unsigned char *cover_row, unsigned char *cover_leaf, int64_t *y_nnz, void *ws, size_t ws_bytes,
		  void *stream)
	{
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		if (y_col_ptr == NULL || y_nnz == NULL || (cover_row == NULL && a.nrows_sel >= 0) || (cover_leaf == NULL && a.nleaves_sel >= 0))
			return svt_set_error("%s: 'y_col_ptr', 'y_nnz' and a cover table per subscript are needed", who);
		hipStream_t st = (hipStream_t) stream;
		if (launch_subassign_count(a, y_col_ptr, cover_row, cover_leaf, ws, st))
			return -1;
		WsHead head;
		if (head.read(ws, st))
			return -1;
		if (head.flag & 1)
			return svt_set_error("subscript contains out-of-bound indices or NAs");
		if (head.flag)
			return svt_set_unsupported("%s: the row subscript is not strictly increasing, or a leaf is repeated", who);
		*y_nnz = head.total;
		return 0;
	}
	int fill(const int64_t *y_col_ptr, int64_t y_nnz, int32_t *y_row_idx, void *y_val, const void *ws, size_t ws_bytes, void *stream)
	{
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		return launch_subassign_fill(a, y_col_ptr, y_nnz, y_row_idx, y_val, ws, (hipStream_t) stream);
	}
	// place -> merge over the caller's allocator: the whole of x[rows, leaves] <- value
	int compose(const svt_dev_csc *x, const ResultDest &to, int *out_Rtype, void *stream)
	{
		int rt = 0;
		if (need_allocator(who, to.alloc, to.release) || assign_out_Rtype(who, x, a.v_Rtype, &rt))
			return -1;
		if (a.nrows_sel == 0 || a.nleaves_sel == 0)         // nothing selected
			return compose_coerced(who, x, rt, to, out_Rtype, stream);
		ResultMem mem(who, to);
		ResultCsc Y(mem);
		ResultWs cover(mem);                                // the two tables, the merge reads them: allocated third, kept to the end
		const size_t row_bytes = ((size_t) x->nrow + 255) / 256 * 256;
		unsigned char *cover_row = NULL, *cover_leaf = NULL;
		if (compose_into(Y, a.v_Rtype, 0, x->nrow, x->ncol, need(),
				 [&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t n) {
					 if (cover.get(row_bytes + (size_t) x->ncol)) return -1;
					 if (a.nrows_sel >= 0) cover_row = (unsigned char *) cover.p;
					 if (a.nleaves_sel >= 0) cover_leaf = (unsigned char *) cover.p + row_bytes;
					 return count(col_ptr, cover_row, cover_leaf, nnz, ws, n, stream);
				 },
				 [&](const svt_dev_csc &R, const void *ws, size_t n) {
					 return fill(R.col_ptr, R.nnz, R.row_idx, R.val, ws, n, stream);
				 }))
			return -1;
		return assign_call(who, x, &Y.c, cover_row, cover_leaf).compose(to, out_Rtype, NULL, stream);
	}
};

extern "C" int svt_dev_subassign_place_vector_count(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel,
						    const int32_t *leaves, int64_t nleaves_sel, const void *vals, int64_t nvals,
						    int v_Rtype, int64_t *y_col_ptr, unsigned char *cover_row, unsigned char *cover_leaf,
						    int64_t *y_nnz, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		SubassignCall c = { "svt_dev_subassign_place_vector_count" };
		if (c.plan(nrow, ncol, rows, nrows_sel, leaves, nleaves_sel, vals, nvals, v_Rtype, NULL, false)) return -1;
		return c.count(y_col_ptr, cover_row, cover_leaf, y_nnz, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_subassign_place_vector_fill(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel,
						   const int32_t *leaves, int64_t nleaves_sel, const void *vals, int64_t nvals,
						   int v_Rtype, const int64_t *y_col_ptr, int64_t y_nnz, int32_t *y_row_idx, void *y_val,
						   const void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		SubassignCall c = { "svt_dev_subassign_place_vector_fill" };
		if (c.plan(nrow, ncol, rows, nrows_sel, leaves, nleaves_sel, vals, nvals, v_Rtype, NULL, false)) return -1;
		return c.fill(y_col_ptr, y_nnz, y_row_idx, y_val, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_subassign_place_svt_count(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel,
						 const int32_t *leaves, int64_t nleaves_sel, const svt_dev_csc *v, int64_t *y_col_ptr,
						 unsigned char *cover_row, unsigned char *cover_leaf, int64_t *y_nnz, void *ws,
						 size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		SubassignCall c = { "svt_dev_subassign_place_svt_count" };
		if (c.plan(nrow, ncol, rows, nrows_sel, leaves, nleaves_sel, NULL, 0, 0, v, true)) return -1;
		return c.count(y_col_ptr, cover_row, cover_leaf, y_nnz, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_subassign_place_svt_fill(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel,
						const int32_t *leaves, int64_t nleaves_sel, const svt_dev_csc *v, const int64_t *y_col_ptr,
						int64_t y_nnz, int32_t *y_row_idx, void *y_val, const void *ws, size_t ws_bytes,
						void *stream)
{
	return abi_status([&] {
		SubassignCall c = { "svt_dev_subassign_place_svt_fill" };
		if (c.plan(nrow, ncol, rows, nrows_sel, leaves, nleaves_sel, NULL, 0, 0, v, true)) return -1;
		return c.fill(y_col_ptr, y_nnz, y_row_idx, y_val, ws, ws_bytes, stream);
	});
}

extern "C" int svt_dev_assign_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, const unsigned char *cover_row,
					  const unsigned char *cover_leaf, int64_t *out_col_ptr, int64_t *out_nnz, void *ws,
					  size_t ws_bytes, void *stream)
{
	ArithCall c = assign_call("svt_dev_assign_merge_count", x, y, cover_row, cover_leaf);
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_assign_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, const unsigned char *cover_row,
					 const unsigned char *cover_leaf, const int64_t *out_col_ptr, int32_t *out_row_idx,
					 void *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the tile prefixes in `ws` place the entries)
	ArithCall c = assign_call("svt_dev_assign_merge_fill", x, y, cover_row, cover_leaf);
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}

extern "C" int svt_dev_subassign_vector(const svt_dev_csc *x, const int32_t *rows, int64_t nrows_sel, const int32_t *leaves,
					int64_t nleaves_sel, const void *vals, int64_t nvals, int v_Rtype, svt_dev_alloc_fn alloc,
					svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr,
					int32_t **out_row_idx, void **out_val, void *stream)
{
	return abi_status([&] {
		SubassignCall c = { "svt_dev_subassign_vector" };
		if (x == NULL) return svt_set_error("%s: an operand is needed", c.who);
		if (c.plan(x->nrow, x->ncol, rows, nrows_sel, leaves, nleaves_sel, vals, nvals, v_Rtype, NULL, false)) return -1;
		return c.compose(x, { alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, out_Rtype, stream);
	});
}
extern "C" int svt_dev_subassign_svt(const svt_dev_csc *x, const int32_t *rows, int64_t nrows_sel, const int32_t *leaves,
				     int64_t nleaves_sel, const svt_dev_csc *v, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
				     void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx,
				     void **out_val, void *stream)
{
	return abi_status([&] {
		SubassignCall c = { "svt_dev_subassign_svt" };
		if (x == NULL) return svt_set_error("%s: an operand is needed", c.who);
		if (c.plan(x->nrow, x->ncol, rows, nrows_sel, leaves, nleaves_sel, NULL, 0, 0, v, true)) return -1;
		return c.compose(x, { alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, out_Rtype, stream);
	});
}

// ---- subsetting and subassignment by an L-index or M-index: kernels_lindex.hip gathers, or places the new values as an
// operand Y with one entry per assigned cell; the merge of kernels_arith.hip under ARI_RULE_ASSIGN_CELLS
// (svt_rule_assign_cells) makes the result ----
enum { LINDEX_SORTED = 0, LINDEX_UNSORTED = 1 };
static std::atomic<int64_t> g_lindex_route[2];

extern "C" void svt_dev_lindex_route_counts(int64_t *counts, int reset)
{
	for (int i = 0; i < 2; i++) {
		if (counts) counts[i] = g_lindex_route[i].load();
		if (reset) g_lindex_route[i] = 0;
	}
}
extern "C" size_t svt_dev_subassign_place_lindex_ws_bytes(int64_t K, int64_t ncol)
{
	return lindex_place_ws_bytes(K, ncol);
}
extern "C" int svt_dev_lindex_sort_passes(int64_t nrow, int64_t ncol)
{
	return lindex_sort_passes(nrow, ncol);
}

// One index of either form (ndim == 0: an L-index) over an array of nrow x ncol cells: every check that needs no GPU,
// then the gather, or the placement's count / fill and the composition with the merge.
struct LindexCall {
	const char *who;
	LindexArgs a;

	int plan(int64_t nrow, int64_t ncol, const void *index, int64_t K, int ndim, const int64_t *dim)
	{
		memset(&a, 0, sizeof(a));
		if (nrow < 0 || nrow > 0x7FFFFFFFLL || ncol < 0 || ncol > 0x7FFFFFFELL)
			return svt_set_error("%s: extents outside 0 .. 2^31 - 1 rows, 0 .. 2^31 - 2 leaves", who);
		if (K < 0 || (K > 0 && index == NULL))
			return svt_set_error("%s: an index of K >= 0 elements is needed", who);
		if (K > 0x7FFFFFFFLL * 256)
			return svt_set_error("%s: too many indices", who);
		if (ndim < 0 || ndim > 8 || (ndim > 0 && dim == NULL))
			return svt_set_error("%s: an M-index takes between 1 and 8 dimensions", who);
		if (ndim > 0) {
			int64_t leaves = 1;
			for (int k = 0; k < ndim; k++) {
				if (dim[k] < 0 || dim[k] > 0x7FFFFFFFLL)
					return svt_set_error("%s: an extent outside 0 .. 2^31 - 1", who);
				if (k > 0) {
					if (dim[k] != 0 && leaves > INT64_MAX / dim[k])
						return svt_set_error("%s: 'dim' does not match the operand's rows and leaves", who);
					leaves *= dim[k];
				}
				a.dim[k] = dim[k];
			}
			if (dim[0] != nrow || leaves != ncol)
				return svt_set_error("%s: 'dim' does not match the operand's rows and leaves", who);
		}
		a.index = index; a.K = K; a.ndim = ndim; a.nrow = nrow; a.ncol = ncol;
		return 0;
	}
	const char *bad_index_message() const
	{
		return a.ndim == 0 ? "linear index (L-index) contains out-of-bound indices or NAs"
				   : "matrix subscript (M-index) contains out-of-bound indices or NAs";
	}
	int gather(const svt_dev_csc *A, void *out, int *bad, void *stream)
	{
		if (!logical_family_type(A->Rtype))
			return svt_set_error("%s: the operand must be of type \"logical\", \"integer\" or \"double\"", who);
		if (A->nnz < 0)
			return svt_set_error("%s: the operand has a negative nonzero count", who);
		if (a.K == 0)
			return 0;
		if (out == NULL || bad == NULL)
			return svt_set_error("%s: 'out' and 'bad' are needed", who);
		return launch_lindex_gather(a, A->col_ptr, A->row_idx, A->val, A->Rtype, A->nnz, A->na_background != 0, out, bad,
					    (hipStream_t) stream);
	}

	size_t need() const { return lindex_place_ws_bytes(a.K, a.ncol); }
	int check_values(const void *vals, int64_t nvals, int v_Rtype, size_t ws_bytes) const
	{
		if (nvals < 1 || vals == NULL)
			return svt_set_error("replacement has length zero");
		if (!logical_family_type(v_Rtype))
			return svt_set_error("%s: the value must be of type \"logical\", \"integer\" or \"double\"", who);
		if (a.K > 0x7FFFFFFFLL)                             // (the sort's payload, the position, is 32 bits)
			return svt_set_unsupported("%s: more than 2^31 - 1 indices are not supported here", who);
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		return 0;
	}
	int count(const void *vals, int64_t nvals, int v_Rtype, int64_t *y_col_ptr, int64_t *y_nnz, void *ws, size_t ws_bytes, void *stream)
	{
		if (const int rc = check_values(vals, nvals, v_Rtype, ws_bytes))
			return rc;
		if (y_col_ptr == NULL || y_nnz == NULL)
			return svt_set_error("%s: 'y_col_ptr' and 'y_nnz' are needed", who);
		hipStream_t st = (hipStream_t) stream;
		if (launch_lindex_check(a, ws, st))
			return -1;
		WsHead head;                                        // (the third word: unsorted, the route)
		if (head.read(ws, st, 3))
			return -1;
		if (head.flag)
			return svt_set_error("%s", bad_index_message());
		const int unsorted = (head.third & 0xFFFFFFFFLL) != 0;
		g_lindex_route[unsorted ? LINDEX_UNSORTED : LINDEX_SORTED]++;
		if (launch_lindex_place(a, unsorted, y_col_ptr, ws, st))
			return -1;
		*y_nnz = a.K;                                       // the sorted route: every index is an entry
		return unsorted ? WsHead::total_of(ws, st, y_nnz) : 0;
	}
	int fill(const void *vals, int64_t nvals, int v_Rtype, int64_t y_nnz, int32_t *y_row_idx, void *y_val, const void *ws, size_t ws_bytes,
		 void *stream)
	{
		if (const int rc = check_values(vals, nvals, v_Rtype, ws_bytes))
			return rc;
		if (y_nnz > 0 && (y_row_idx == NULL || y_val == NULL))
			return svt_set_error("%s: 'y_row_idx' and 'y_val' are needed", who);
		return launch_lindex_fill(a, vals, nvals, v_Rtype, y_nnz, y_row_idx, y_val, ws, (hipStream_t) stream);
	}
	// place -> merge over the caller's allocator: the whole of x[index] <- vals
	int compose(const svt_dev_csc *x, const void *vals, int64_t nvals, int v_Rtype, const ResultDest &to, int *out_Rtype, void *stream)
	{
		int rt = 0;
		if (need_allocator(who, to.alloc, to.release) || check_values(vals, nvals, v_Rtype, need()) ||
		    assign_out_Rtype(who, x, v_Rtype, &rt))
			return -1;
		if (a.K == 0)                                       // nothing assigned
			return compose_coerced(who, x, rt, to, out_Rtype, stream);
		ResultMem mem(who, to);
		ResultCsc Y(mem);
		if (compose_into(Y, v_Rtype, 0, x->nrow, x->ncol, need(),
				 [&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t n) {
					 return count(vals, nvals, v_Rtype, col_ptr, nnz, ws, n, stream);
				 },
				 [&](const svt_dev_csc &R, const void *ws, size_t n) {
					 return fill(vals, nvals, v_Rtype, R.nnz, R.row_idx, R.val, ws, n, stream);
				 }))
			return -1;
		return assign_cells_call(who, x, &Y.c).compose(to, out_Rtype, NULL, stream);
	}
};

extern "C" int svt_dev_subset_lindex(const svt_dev_csc *A, const int64_t *lindex, int64_t K, void *out, int *bad, void *stream)
{
	return abi_status([&] {
		LindexCall c = { "svt_dev_subset_lindex" };
		if (A == NULL) return svt_set_error("%s: an operand is needed", c.who);
		if (c.plan(A->nrow, A->ncol, lindex, K, 0, NULL)) return -1;
		return c.gather(A, out, bad, stream);
	});
}
extern "C" int svt_dev_subset_mindex(const svt_dev_csc *A, const int32_t *mindex, int64_t K, int ndim, const int64_t *dim, void *out,
				     int *bad, void *stream)
{
	return abi_status([&] {
		LindexCall c = { "svt_dev_subset_mindex" };
		if (A == NULL) return svt_set_error("%s: an operand is needed", c.who);
		if (ndim < 1) return svt_set_error("%s: an M-index takes between 1 and 8 dimensions", c.who);
		if (c.plan(A->nrow, A->ncol, mindex, K, ndim, dim)) return -1;
		return c.gather(A, out, bad, stream);
	});
}
extern "C" int svt_dev_subassign_place_lindex_count(int64_t nrow, int64_t ncol, const void *index, int64_t K, int ndim,
						    const int64_t *dim, const void *vals, int64_t nvals, int v_Rtype, int64_t *y_col_ptr,
						    int64_t *y_nnz, void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] {
		LindexCall c = { "svt_dev_subassign_place_lindex_count" };
		if (c.plan(nrow, ncol, index, K, ndim, dim)) return -1;
		return c.count(vals, nvals, v_Rtype, y_col_ptr, y_nnz, ws, ws_bytes, stream);
	});
}
extern "C" int svt_dev_subassign_place_lindex_fill(int64_t nrow, int64_t ncol, const void *index, int64_t K, int ndim,
						   const int64_t *dim, const void *vals, int64_t nvals, int v_Rtype, const int64_t *y_col_ptr,
						   int64_t y_nnz, int32_t *y_row_idx, void *y_val, const void *ws, size_t ws_bytes,
						   void *stream)
{
	(void) y_col_ptr;                                   // (the scanned run ends in `ws` place the entries)
	return abi_status([&] {
		LindexCall c = { "svt_dev_subassign_place_lindex_fill" };
		if (c.plan(nrow, ncol, index, K, ndim, dim)) return -1;
		return c.fill(vals, nvals, v_Rtype, y_nnz, y_row_idx, y_val, ws, ws_bytes, stream);
	});
}

extern "C" int svt_dev_assign_cells_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int64_t *out_col_ptr, int64_t *out_nnz,
						void *ws, size_t ws_bytes, void *stream)
{
	ArithCall c = assign_cells_call("svt_dev_assign_cells_merge_count", x, y);
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_assign_cells_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, const int64_t *out_col_ptr,
					       int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the tile prefixes in `ws` place the entries)
	ArithCall c = assign_cells_call("svt_dev_assign_cells_merge_fill", x, y);
	return abi_status([&] { return c.fill(out_row_idx, out_val, NULL, ws, ws_bytes, stream); });
}

extern "C" int svt_dev_subassign_lindex(const svt_dev_csc *x, const int64_t *lindex, int64_t K, const void *vals, int64_t nvals,
					int v_Rtype, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int *out_Rtype,
					int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val, void *stream)
{
	return abi_status([&] {
		LindexCall c = { "svt_dev_subassign_lindex" };
		if (x == NULL) return svt_set_error("%s: an operand is needed", c.who);
		if (c.plan(x->nrow, x->ncol, lindex, K, 0, NULL)) return -1;
		return c.compose(x, vals, nvals, v_Rtype, { alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, out_Rtype, stream);
	});
}
extern "C" int svt_dev_subassign_mindex(const svt_dev_csc *x, const int32_t *mindex, int64_t K, int ndim, const int64_t *dim,
					const void *vals, int64_t nvals, int v_Rtype, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
					void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx,
					void **out_val, void *stream)
{
	return abi_status([&] {
		LindexCall c = { "svt_dev_subassign_mindex" };
		if (x == NULL) return svt_set_error("%s: an operand is needed", c.who);
		if (ndim < 1) return svt_set_error("%s: an M-index takes between 1 and 8 dimensions", c.who);
		if (c.plan(x->nrow, x->ncol, mindex, K, ndim, dim)) return -1;
		return c.compose(x, vals, nvals, v_Rtype, { alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, out_val }, out_Rtype, stream);
	});
}

// A %*% B, both sparse (kernels_spmm.hip): out[r + k * ldo], r < A->nrow, k < B->ncol.
extern "C" size_t svt_dev_matmul_csc_csc_ws_bytes(const svt_dev_csc *A)
{
	return spmm_ws_bytes(A->nrow, A->ncol) + 256;       // [flag][table of run bounds]
}

static SpmmArgs spmm_args(const svt_dev_csc *A, const svt_dev_csc *B, double *out, int64_t ldo, int *flag)
{
	SpmmArgs a;
	memset(&a, 0, sizeof(a));
	a.a_ptr = A->col_ptr; a.a_idx = A->row_idx; a.a_val = A->val; a.a_type = A->Rtype;
	a.nrow = A->nrow; a.ninner = A->ncol;
	a.b_ptr = B->col_ptr; a.b_idx = B->row_idx; a.b_val = B->val; a.b_type = B->Rtype; a.K = B->ncol;
	a.out = out; a.ldo = ldo; a.flag = flag;
	return a;
}

// ws: [int: A holds a non-finite value / an NA][int: the same for the last product, B included][...][table at 256]
extern "C" int svt_dev_matmul_csc_csc_prepare(const svt_dev_csc *A, void *ws, size_t ws_bytes, void *stream)
{
	if (ws_bytes < svt_dev_matmul_csc_csc_ws_bytes(A))
		return svt_set_error("svt_dev_matmul_csc_csc: workspace too small");
	hipStream_t s = (hipStream_t) stream;
	HIP_TRY(hipMemsetAsync(ws, 0, 8, s));
	svt_dev_csc none;
	memset(&none, 0, sizeof(none));
	return launch_spmm_prepare(spmm_args(A, &none, NULL, 0, (int *) ws), A->nnz, (char *) ws + 256, s);
}

static int dev_matmul_csc_csc_prepared_impl(const svt_dev_csc *A, const svt_dev_csc *B, double *out, int64_t ldo,
					       void *ws, size_t ws_bytes, int *not_finite, void *stream)
{
	if (A->ncol != B->nrow)
		return svt_set_error("svt_dev_matmul_csc_csc: non-conformable operands");
	if (ws_bytes < svt_dev_matmul_csc_csc_ws_bytes(A))
		return svt_set_error("svt_dev_matmul_csc_csc: workspace too small");
	if (ldo < A->nrow)
		return svt_set_error("svt_dev_matmul_csc_csc: leading dimension of the result too small");
	hipStream_t s = (hipStream_t) stream;
	int *flag = (int *) ws + 1;
	HIP_TRY(hipMemcpyAsync(flag, ws, 4, hipMemcpyDeviceToDevice, s));
	if (launch_spmm_product(spmm_args(A, B, out, ldo, flag), A->nnz, B->nnz, (char *) ws + 256, s))
		return -1;
	if (not_finite != NULL)
		HIP_TRY(hipMemcpyAsync(not_finite, flag, 4, hipMemcpyDeviceToDevice, s));
	return 0;
}
extern "C" int svt_dev_matmul_csc_csc_prepared(const svt_dev_csc *A, const svt_dev_csc *B, double *out, int64_t ldo,
					       void *ws, size_t ws_bytes, int *not_finite, void *stream)
{
	return abi_status([&] { return dev_matmul_csc_csc_prepared_impl(A, B, out, ldo, ws, ws_bytes, not_finite, stream); });
}

static int dev_matmul_csc_csc_impl(const svt_dev_csc *A, const svt_dev_csc *B, double *out, int64_t ldo,
				      void *ws, size_t ws_bytes, int *not_finite, void *stream)
{
	if (A->ncol != B->nrow)
		return svt_set_error("svt_dev_matmul_csc_csc: non-conformable operands");
	if (ws_bytes < svt_dev_matmul_csc_csc_ws_bytes(A))
		return svt_set_error("svt_dev_matmul_csc_csc: workspace too small");
	if (ldo < A->nrow)
		return svt_set_error("svt_dev_matmul_csc_csc: leading dimension of the result too small");
	// one product: the table pass looks only at the leaves of A that B does not refer to, the product kernel at
	// the values it reads (kernels_spmm.hip); ws[0] is left as "not known for A alone" -- this ws is not a
	// prepared one afterwards
	hipStream_t s = (hipStream_t) stream;
	int *flag = (int *) ws + 1;
	const SpmmArgs a = spmm_args(A, B, out, ldo, flag);
	// (the two flag words are zeroed by the first kernel of the pass: a memset in front of it is a blit kernel of its own)
	if (launch_spmm_prepare_for(a, A->nnz, B->nnz, (char *) ws + 256, s, (int *) ws))
		return -1;
	if (launch_spmm_product(a, A->nnz, B->nnz, (char *) ws + 256, s))
		return -1;
	if (not_finite != NULL)
		HIP_TRY(hipMemcpyAsync(not_finite, flag, 4, hipMemcpyDeviceToDevice, s));
	return 0;
}
extern "C" int svt_dev_matmul_csc_csc(const svt_dev_csc *A, const svt_dev_csc *B, double *out, int64_t ldo,
				      void *ws, size_t ws_bytes, int *not_finite, void *stream)
{
	return abi_status([&] { return dev_matmul_csc_csc_impl(A, B, out, ldo, ws, ws_bytes, not_finite, stream); });
}

// A %*% B, both sparse, with a sparse result (kernels_spgemm.hip): the one statement of the checks and of count / fill
extern "C" int svt_dev_spgemm_panel(int64_t nrow)
{
	(void) nrow;                                        // (one height for every operand today)
	return spgemm_panel();
}
extern "C" size_t svt_dev_spgemm_ws_bytes(const svt_dev_csc *A, int64_t K)
{
	return spgemm_ws_bytes(A->nrow, A->ncol, K);
}

struct SpgemmCall {
	const char *who;
	const svt_dev_csc *A, *B;
	SpgemmArgs args() const
	{
		SpgemmArgs a;
		a.a_ptr = A->col_ptr; a.a_idx = A->row_idx; a.a_val = A->val; a.a_type = A->Rtype; a.nrow = A->nrow; a.ninner = A->ncol;
		a.b_ptr = B->col_ptr; a.b_idx = B->row_idx; a.b_val = B->val; a.b_type = B->Rtype; a.K = B->ncol;
		return a;
	}
	size_t need() const { return svt_dev_spgemm_ws_bytes(A, B->ncol); }
	int check(size_t ws_bytes) const
	{
		if (A == NULL || B == NULL)
			return svt_set_error("%s: two operands are needed", who);
		if (A->ncol != B->nrow)
			return svt_set_error("%s: non-conformable arguments", who);
		if ((A->Rtype != SVT_REALSXP && A->Rtype != SVT_INTSXP) || (B->Rtype != SVT_REALSXP && B->Rtype != SVT_INTSXP))
			return svt_set_error("%s: operands must be of type \"integer\" or \"double\"", who);
		if (ws_bytes < need())
			return svt_set_error("%s: workspace too small", who);
		if (A->na_background || B->na_background)
			return svt_set_unsupported("%s: NaArray operands are not supported here", who);
		// the limit of launch_spmm_product, kept for its sparse-result sibling
		if (B->nnz >= (int64_t) 2147483647)
			return svt_set_unsupported("%s: the second operand holds 2^31 - 1 nonzeros or more", who);
		return spgemm_check(args());
	}
	int count(int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, int *not_finite, void *stream) const
	{
		if (const int rc = check(ws_bytes))
			return rc;
		hipStream_t st = (hipStream_t) stream;
		if (launch_spgemm_count(args(), A->nnz, B->nnz, out_col_ptr, not_finite, ws, st))
			return -1;
		return WsHead::total_of(ws, st, out_nnz);
	}
	int fill(int32_t *out_row_idx, double *out_val, const void *ws, size_t ws_bytes, void *stream) const
	{
		if (const int rc = check(ws_bytes))
			return rc;
		return launch_spgemm_fill(args(), out_row_idx, out_val, ws, (hipStream_t) stream);
	}
	int compose(const ResultDest &to, int *not_finite, void *stream) const
	{
		if (need_allocator(who, to.alloc, to.release))
			return -1;
		if (A == NULL || B == NULL)
			return svt_set_error("%s: two operands are needed", who);
		if (check(need()))
			return -1;
		return compose_result(who, to, SVT_REALSXP, 0, A->nrow, B->ncol, need(),
			[&](int64_t *col_ptr, int64_t *nnz, void *ws, size_t n) { return count(col_ptr, nnz, ws, n, not_finite, stream); },
			[&](const svt_dev_csc &R, const void *ws, size_t n) { return fill(R.row_idx, (double *) R.val, ws, n, stream); });
	}
};

extern "C" int svt_dev_spgemm_count(const svt_dev_csc *A, const svt_dev_csc *B, int64_t *out_col_ptr, int64_t *out_nnz, void *ws,
				    size_t ws_bytes, int *not_finite, void *stream)
{
	const SpgemmCall c = { "svt_dev_spgemm_count", A, B };
	return abi_status([&] { return c.count(out_col_ptr, out_nnz, ws, ws_bytes, not_finite, stream); });
}
extern "C" int svt_dev_spgemm_fill(const svt_dev_csc *A, const svt_dev_csc *B, const int64_t *out_col_ptr, int32_t *out_row_idx,
				   double *out_val, const void *ws, size_t ws_bytes, void *stream)
{
	(void) out_col_ptr;                                 // (the item bases in `ws` place the entries)
	const SpgemmCall c = { "svt_dev_spgemm_fill", A, B };
	return abi_status([&] { return c.fill(out_row_idx, out_val, ws, ws_bytes, stream); });
}
extern "C" int svt_dev_spgemm(const svt_dev_csc *A, const svt_dev_csc *B, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
			      void *ctx, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, double **out_val,
			      int *not_finite, void *stream)
{
	const SpgemmCall c = { "svt_dev_spgemm", A, B };
	return abi_status([&] {
		void *val = NULL;                                   // (the result is double: 'out_val' is typed)
		const int rc = c.compose({ alloc, release, ctx, out_nnz, out_col_ptr, out_row_idx, &val }, not_finite, stream);
		if (rc == 0) *out_val = (double *) val;
		return rc;
	});
}

// crossprod(X, Y) of two sparse operands on t(X) and Y (kernels_gram.hip)
extern "C" size_t svt_dev_crossprod_csc_csc_ws_bytes(const svt_dev_csc *Xt)
{
	return gram_ws_bytes(Xt->nrow, Xt->ncol, Xt->nnz);
}

extern "C" void svt_dev_crossprod_csc_csc_set_panel(int one_block_max, int log2_panel)
{
	gram_set_panel(one_block_max, log2_panel);
}

static int dev_crossprod_csc_csc_impl(const svt_dev_csc *Xt, const svt_dev_csc *Y, int sym, double *out,
					 int64_t ldo, void *ws, size_t ws_bytes, int *not_finite, void *stream)
{
	if (Xt->ncol != Y->nrow)
		return svt_set_error("svt_dev_crossprod_csc_csc: non-conformable operands");
	if (sym && Xt->nrow != Y->ncol)
		return svt_set_error("svt_dev_crossprod_csc_csc: the symmetric form needs t(Y) and Y");
	if (ws_bytes < svt_dev_crossprod_csc_csc_ws_bytes(Xt))
		return svt_set_error("svt_dev_crossprod_csc_csc: workspace too small");
	if (ldo < Xt->nrow)
		return svt_set_error("svt_dev_crossprod_csc_csc: leading dimension of the result too small");
	if ((Xt->Rtype != SVT_REALSXP && Xt->Rtype != SVT_INTSXP) || (Y->Rtype != SVT_REALSXP && Y->Rtype != SVT_INTSXP))
		return svt_set_error("svt_dev_crossprod_csc_csc: double or integer operands");
	hipStream_t s = (hipStream_t) stream;
	GramArgs a;
	memset(&a, 0, sizeof(a));
	a.a_ptr = Xt->col_ptr; a.a_idx = Xt->row_idx; a.a_val = Xt->val; a.a_type = Xt->Rtype;
	a.nx = Xt->nrow; a.nrow = Xt->ncol;
	a.b_ptr = Y->col_ptr; a.b_idx = Y->row_idx; a.b_val = Y->val; a.b_type = Y->Rtype; a.ny = Y->ncol;
	a.out = out; a.ldo = ldo; a.sym = sym != 0;
	if (launch_gram(a, Xt->nnz, Y->nnz, ws, s))
		return -1;
	if (not_finite != NULL)
		HIP_TRY(hipMemcpyAsync(not_finite, ws, 4, hipMemcpyDeviceToDevice, s));
	return 0;
}
extern "C" int svt_dev_crossprod_csc_csc(const svt_dev_csc *Xt, const svt_dev_csc *Y, int sym, double *out,
					 int64_t ldo, void *ws, size_t ws_bytes, int *not_finite, void *stream)
{
	return abi_status([&] { return dev_crossprod_csc_csc_impl(Xt, Y, sym, out, ldo, ws, ws_bytes, not_finite, stream); });
}

extern "C" void svt_dev_aperm_route_counts(int64_t *counts, int reset)
{
	aperm_route_counts(counts, reset);
}

static int aperm_args(int ndim, const int *perm, int *perm0)
{
	if (ndim < 1 || ndim > 8)
		return svt_set_error("aperm: between 1 and 8 dimensions are supported");
	for (int a = 0; a < ndim; a++) {
		if (perm[a] < 1 || perm[a] > ndim)
			return svt_set_error("'perm' must be a permutation of 1:%d", ndim);
		perm0[a] = perm[a] - 1;
	}
	return 0;
}

extern "C" size_t svt_dev_aperm_ws_bytes(int64_t nnz, int ndim, const int64_t *dim)
{
	return aperm_ws_bytes_box(nnz, dim, ndim, box_nnz_get());
}

extern "C" size_t svt_dev_aperm_perm_ws_bytes(int64_t nnz, int ndim, const int64_t *dim, const int *perm)
{
	int perm0[8];
	if (ndim < 1 || ndim > 8)
		return aperm_ws_bytes_box(nnz, dim, ndim, box_nnz_get());
	for (int a = 0; a < ndim; a++) perm0[a] = perm[a] - 1;      // (not a permutation: the need of every permutation)
	return aperm_perm_ws_bytes_box(nnz, dim, ndim, perm0, box_nnz_get());
}

static int dev_aperm_impl(const svt_dev_csc *A, int ndim, const int64_t *dim, const int *perm,
			     int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val,
			     void *ws, size_t ws_bytes, void *stream)
{
	int perm0[8];
	if (aperm_args(ndim, perm, perm0))
		return -1;
	int64_t nl = 1;
	for (int a = 1; a < ndim; a++) nl *= dim[a];
	if (dim[0] != A->nrow || nl != A->ncol)
		return svt_set_error("aperm: 'dim' does not match the operand");
	const int64_t box = box_nnz_get();                  // (once: the size check and the launch agree)
	if (ws_bytes < aperm_perm_ws_bytes_box(A->nnz, dim, ndim, perm0, box))
		return svt_set_error("svt_dev_aperm: workspace too small");
	return launch_aperm_box(A->col_ptr, A->row_idx, A->val, A->Rtype, A->ncol, A->nnz, dim, ndim,
				perm0, out_col_ptr, out_row_idx, out_val, ws, box, (hipStream_t) stream);
}
extern "C" int svt_dev_aperm(const svt_dev_csc *A, int ndim, const int64_t *dim, const int *perm,
			     int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val,
			     void *ws, size_t ws_bytes, void *stream)
{
	return abi_status([&] { return dev_aperm_impl(A, ndim, dim, perm, out_col_ptr, out_row_idx, out_val, ws, ws_bytes, stream); });
}

// C_aperm_SVT, src/SparseArray_aperm.c:935-970
static int aperm_SVT_impl(const svt_view *x, const int *perm, int64_t *out_col_ptr,
			     int32_t *out_row_idx, void *out_val)
{
	if (ensure_init() || check_view(x))
		return -1;
	int perm0[8];
	if (aperm_args(x->ndim, perm, perm0))
		return -1;
	int64_t dim[8], new_nl = 1;
	for (int a = 0; a < x->ndim; a++) dim[a] = x->dim[a];
	for (int a = 1; a < x->ndim; a++) new_nl *= dim[perm0[a]];
	CscGuard A(x);
	if (A.h == NULL) return -1;
	const size_t esz = elt_size(x->Rtype);
	const size_t nn = (size_t) (A.h->nnz > 0 ? A.h->nnz : 1);
	const int64_t box = box_nnz_get();
	DevBuf P, I, V, W;
	if (P.alloc((size_t) (new_nl + 1) * 8) || I.alloc(nn * 4) || V.alloc(nn * esz) ||
	    W.alloc(aperm_perm_ws_bytes_box(A.h->nnz, dim, x->ndim, perm0, box)))
		return -1;
	if (launch_aperm_box(A.h->col_ptr, A.h->row_idx, A.h->val, A.h->Rtype, A.h->ncol, A.h->nnz, dim,
			     x->ndim, perm0, P.as<int64_t>(), I.as<int32_t>(), V.p, W.p, box, 0))
		return -1;
	HIP_TRY(hipMemcpy(out_col_ptr, P.p, (size_t) (new_nl + 1) * 8, hipMemcpyDeviceToHost));
	if (A.h->nnz) {
		if (staged_download(out_row_idx, I.p, (size_t) A.h->nnz * 4) ||
		    staged_download(out_val, V.p, (size_t) A.h->nnz * esz))
			return -1;
	}
	return 0;
}
extern "C" int svt_aperm_SVT(const svt_view *x, const int *perm, int64_t *out_col_ptr,
			     int32_t *out_row_idx, void *out_val)
{
	return abi_status([&] { return aperm_SVT_impl(x, perm, out_col_ptr, out_row_idx, out_val); });
}

// the operand, the groups and the result of a rowsum / colsum; the caller adds scratch and ovflow_flag.
// col_ptr32: the int32 'p' slot of a dgCMatrix in place of A->col_ptr
static GroupSumArgs groupsum_args(const svt_dev_csc *A, const int32_t *col_ptr32, const int *group, int ngroup,
				  int na_rm, void *out)
{
	GroupSumArgs a;
	memset(&a, 0, sizeof(a));
	a.col_ptr64 = col_ptr32 ? NULL : A->col_ptr; a.col_ptr32 = col_ptr32;
	a.row_idx = A->row_idx; a.val = A->val; a.Rtype = A->Rtype;
	a.nrow = A->nrow; a.ncol = A->ncol; a.nnz = A->nnz;
	a.group = group; a.ngroup = ngroup; a.na_rm = na_rm; a.out = out;
	return a;
}

extern "C" int svt_dev_rowsum(const svt_dev_csc *A, const int *group, int ngroup,
			      int na_rm, double *out, void *stream)
{
	if (A->Rtype != SVT_REALSXP)
		return svt_set_error("svt_dev_rowsum: f64 input only");
	return launch_rowsum(groupsum_args(A, NULL, group, ngroup, na_rm, out), (hipStream_t) stream);
}

// rowsum(x, group) for a (x, group) pair that is used more than once: the group of every nonzero, as a 16-bit
// 0-based id (NA -> ngroup - 1), is written to `gid` (svt_dev_rowsum_gid_bytes(A) bytes) once; the prepared call
// then streams values and ids -- 10 bytes per nonzero, no lookup in the group table.
extern "C" size_t svt_dev_rowsum_gid_bytes(const svt_dev_csc *A)
{
	return (size_t) (A->nnz > 0 ? A->nnz : 1) * 2 + 16;
}

extern "C" int svt_dev_rowsum_prepare(const svt_dev_csc *A, const int *group, int ngroup, void *gid,
				      size_t gid_bytes, void *stream)
{
	if (ngroup < 1 || ngroup > 65535)
		return svt_set_error("svt_dev_rowsum_prepare: between 1 and 65535 groups");
	if (gid_bytes < svt_dev_rowsum_gid_bytes(A))
		return svt_set_error("svt_dev_rowsum_prepare: id buffer too small");
	return launch_rowsum_gid(groupsum_args(A, NULL, group, ngroup, 0, NULL), (uint16_t *) gid, (hipStream_t) stream);
}

extern "C" int svt_dev_rowsum_prepared(const svt_dev_csc *A, const void *gid, int ngroup, int na_rm,
				       double *out, void *stream)
{
	if (A->Rtype != SVT_REALSXP)
		return svt_set_error("svt_dev_rowsum: f64 input only");
	if (ngroup < 1 || ngroup > 65535)
		return svt_set_error("svt_dev_rowsum_prepared: between 1 and 65535 groups");
	if ((int64_t) ngroup * 8 > 160 * 1024)
		return svt_set_error("svt_dev_rowsum_prepared: more groups than a workgroup's LDS holds (20480)");
	const int rc = launch_rowsum_prepared(groupsum_args(A, NULL, NULL, ngroup, na_rm, out), (const uint16_t *) gid,
					      (hipStream_t) stream);
	if (rc > 0)
		return svt_set_error("svt_dev_rowsum_prepared: unsupported shape");
	return rc;
}

extern "C" int svt_dev_rowsum_form(int64_t nrow, int64_t ncol, int64_t nnz, int ngroup, int Rtype, int col_ptr32,
				  int *cols_per_wg, int64_t *window_rows)
{
	const RowsumRoute rt = rowsum_route(nrow, ncol, nnz, ngroup, Rtype, col_ptr32 != 0);
	if (cols_per_wg) *cols_per_wg = rt.cols_per_wg;
	if (window_rows) *window_rows = rowsum_window_rows();
	return rt.form;
}

extern "C" int svt_dev_rowsum_prepare_form(int64_t nrow, int64_t ncol, int64_t nnz, int ngroup, int *cols_per_wg)
{
	const RowsumRoute rt = rowsum_gid_route(nrow, ncol, nnz, ngroup, false);
	if (cols_per_wg) *cols_per_wg = rt.cols_per_wg;
	return rt.form;
}

extern "C" int svt_dev_rowsum_prepared_form(int64_t ncol, int ngroup, int *cols_per_wg)
{
	int C = 0;
	const int rc = rowsum_prepared_route(ncol, ngroup, false, &C);
	if (cols_per_wg) *cols_per_wg = C;
	return rc;
}

// ==================================================================================
// Sharded host entry points (svt_set_devices)
// ==================================================================================
// With more than one device in the list and an operand of at least svt_set_shard_min_nnz() nonzeros,
// crossprod2_SVT_mat and matmul_SVT_mat split the operand into row blocks, colStats and rowsum into leaf ranges.
// Shard s runs on a host thread of its own, on device g_devices[s], with its own stager and 1/N of the marshalling
// threads.  It uploads its part of the operand and frees it again: sharded calls do not use the resident cache.
static int64_t view_nzcount(const svt_view *x);

static bool shard_applies(const svt_view *x)
{
	return t_shard == NULL && g_devices.size() > 1 && view_nzcount(x) >= g_shard_min_nnz;
}

// Runs fn(s) for every shard and joins every thread.  Status: a shard < 0 makes the call < 0 with that shard's
// message (the first in shard order); else a shard refused (> 0 at the ABI) makes the call refused.
// SVT_SHARD_REFUSE=<slot> (read at every call; tests) makes that shard refuse.
template <class F> static int run_shards(const std::vector<int> &devs, F fn)
{
	const int N = (int) devs.size();
	struct Res {
		int rc, unsupported;
		char err[sizeof(g_err)];
	};
	std::vector<Res> res((size_t) N);
	const size_t chunk = Stager::CHUNK / (size_t) N / 4096 * 4096;
	const char *refuse = getenv("SVT_SHARD_REFUSE");
	const int refuse_slot = refuse != NULL && refuse[0] != '\0' ? atoi(refuse) : -1;
	auto body = [&](int s) {
		const ShardCtx ctx = { s, N, devs[(size_t) s] };
		t_shard = &ctx;
		g_err[0] = '\0';
		g_unsupported = 0;
		int rc;
		if (s == refuse_slot) {
			rc = svt_set_unsupported("shard %d refused the call (SVT_SHARD_REFUSE)", s);
		} else if (hipSetDevice(ctx.device) != hipSuccess) {
			rc = svt_set_error("shard %d: hipSetDevice(%d) failed", s, ctx.device);
		} else {
			g_shard_stager[s].use(chunk, ctx.device);
			rc = fn(s);
		}
		Res &r = res[(size_t) s];
		r.rc = rc;
		r.unsupported = rc < 0 && g_unsupported;
		memcpy(r.err, g_err, sizeof(g_err));
		t_shard = NULL;
	};
	std::vector<std::thread> th;
	for (int s = 0; s < N; s++) th.emplace_back(body, s);
	for (auto &t : th) t.join();
	int failed = -1, refused = -1;
	for (int s = 0; s < N; s++) {
		const Res &r = res[(size_t) s];
		if (r.rc < 0 && !r.unsupported && failed < 0) failed = s;
		if (r.rc < 0 && r.unsupported && refused < 0) refused = s;
	}
	const int pick = failed >= 0 ? failed : refused;
	if (pick < 0) return 0;
	memcpy(g_err, res[(size_t) pick].err, sizeof(g_err));
	g_unsupported = failed < 0;
	return -1;
}

// Part of a view: rows [r0, r1) of every leaf of a 2-d operand (offsets as they are: row_block_upload() rebases them
// on the device), or leaves [c0, c1).  Pointers into the caller's leaves; nothing is copied.
struct SubView {
	svt_view v;
	int32_t dim[2];
	std::vector<int32_t> cnt;
	std::vector<const int32_t *> offs;
	std::vector<const void *> vals;
};

static void row_block_view(const svt_view *x, int r0, int r1, SubView &sv)
{
	sv.v = *x;
	sv.dim[0] = r1 - r0;
	sv.dim[1] = x->dim[1];
	sv.v.dim = sv.dim;
	if (x->svt_is_null) return;
	const size_t n = (size_t) x->nleaves, esz = elt_size(x->Rtype);
	sv.cnt.assign(n, 0);
	sv.offs.assign(n, NULL);
	sv.vals.assign(n, NULL);
	for (size_t j = 0; j < n; j++) {
		const int c = x->nzcount[j];
		if (c <= 0) continue;
		// offsets ascend inside a leaf (src/leaf_utils.h:12-15)
		const int32_t *o = x->nzoffs[j];
		const int32_t *lo = std::lower_bound(o, o + c, r0), *hi = std::lower_bound(lo, o + c, r1);
		sv.cnt[j] = (int32_t) (hi - lo);
		sv.offs[j] = lo;
		if (x->nzvals[j] != NULL) sv.vals[j] = (const char *) x->nzvals[j] + (size_t) (lo - o) * esz;
	}
	sv.v.nzcount = sv.cnt.data();
	sv.v.nzoffs = sv.offs.data();
	sv.v.nzvals = sv.vals.data();
}

static void col_block_view(const svt_view *x, int64_t c0, int64_t c1, SubView &sv)
{
	sv.v = *x;
	sv.v.ndim = 2;
	sv.dim[0] = x->dim[0];
	sv.dim[1] = (int32_t) (c1 - c0);
	sv.v.dim = sv.dim;
	sv.v.nleaves = c1 - c0;
	if (x->svt_is_null) return;
	sv.v.nzcount = x->nzcount + c0;
	sv.v.nzoffs = x->nzoffs + c0;
	sv.v.nzvals = x->nzvals + c0;
}

// Upload of the rows [r0, r1) of x: offsets rebased to 0 on the device.
static svt_dev_csc *row_block_upload(const svt_view *x, int64_t r0, int64_t r1)
{
	SubView sv;
	row_block_view(x, (int) r0, (int) r1, sv);
	svt_dev_csc *d = svt_upload(&sv.v);
	if (d == NULL || r0 == 0) return d;
	if (launch_rebase_rows(d->row_idx, d->nnz, (int32_t) r0, 0) || hipStreamSynchronize(0) != hipSuccess) {
		if (svt_last_error()[0] == '\0') svt_set_error("device error while rebasing a row block");
		svt_release(d);
		return NULL;
	}
	return d;
}

// Row block of shard s: the blocks of parallel.row_block(nrow, s, N, 128) -- every boundary but the last a
// multiple of 128 rows (the row panels of the product kernels); empty blocks when N exceeds the panels.
static void shard_rows(int64_t nrow, int s, int N, int64_t *r0, int64_t *r1)
{
	const int64_t units = (nrow + 127) / 128, base = units / N, rem = units % N;
	const int64_t u0 = s * base + (s < rem ? s : rem), u1 = u0 + base + (s < rem ? 1 : 0);
	*r0 = u0 * 128 < nrow ? u0 * 128 : nrow;
	*r1 = u1 * 128 < nrow ? u1 * 128 : nrow;
}

// Leaf ranges cut on unit boundaries (units of `unit` consecutive leaves: the output cells of colStats), balanced by
// weight = nonzeros + 1 per unit.  cut[s] .. cut[s + 1] are the units of shard s (possibly none).
static std::vector<int64_t> shard_cuts(const svt_view *x, int64_t unit, int64_t nunits, int N)
{
	std::vector<int64_t> pre((size_t) nunits + 1, 0);
	for (int64_t u = 0; u < nunits; u++) {
		int64_t w = 1;
		if (!x->svt_is_null)
			for (int64_t j = u * unit; j < (u + 1) * unit; j++) w += x->nzcount[j];
		pre[(size_t) u + 1] = pre[(size_t) u] + w;
	}
	const int64_t total = pre[(size_t) nunits];
	std::vector<int64_t> cut((size_t) N + 1, nunits);
	cut[0] = 0;
	for (int s = 1; s < N; s++) {
		const int64_t target = total / N * s + total % N * s / N;
		cut[(size_t) s] = std::lower_bound(pre.begin(), pre.end(), target) - pre.begin();
		if (cut[(size_t) s] > nunits) cut[(size_t) s] = nunits;
		if (cut[(size_t) s] < cut[(size_t) s - 1]) cut[(size_t) s] = cut[(size_t) s - 1];
	}
	return cut;
}

// Device buffers of the shards that outlive one run_shards() (the partial results of the reduce-scatter), freed
// on their devices.
struct ShardBufs {
	std::vector<void *> p;
	std::vector<int> dev;
	explicit ShardBufs(const std::vector<int> &devs) : p(devs.size(), nullptr), dev(devs) {}
	~ShardBufs()
	{
		for (size_t s = 0; s < p.size(); s++)
			if (p[s] && hipSetDevice(dev[s]) == hipSuccess) (void) hipFree(p[s]);
		if (g_device >= 0) (void) hipSetDevice(g_device);
	}
	ShardBufs(const ShardBufs &) = delete;
	ShardBufs &operator=(const ShardBufs &) = delete;
};

// ==================================================================================
// Host level: crossprod
// ==================================================================================
static int check_mult_view(const svt_view *x, const char *what)
{
	if (check_view(x))
		return -1;
	if (x->ndim != 2)
		return svt_set_error("%s must have 2 dimensions", what);
	// get_and_check_input_Rtype(), src/SparseMatrix_mult.c:915-928
	if (x->Rtype != SVT_REALSXP && x->Rtype != SVT_INTSXP)
		return svt_set_error("input type is not supported yet");
	if (x->na_background)      // crossprod()/%*% have no NaArray methods (R/SparseMatrix-mult.R)
		return svt_set_error("NaArray objects are not supported by this operation");
	return 0;
}

// Largest number of dense columns handled per launch so that the row-major
// staging copy of the dense operand stays below ~1 GiB.
static int chunk_K(int64_t nrow, int64_t K)
{
	const int64_t budget = (int64_t) 1 << 30;
	int64_t kc = budget / (8 * (nrow > 0 ? nrow : 1));
	kc = kc / 64 * 64;
	if (kc < 64) kc = 64;
	if (kc > K) kc = K;
	return (int) kc;
}

// The panel-blocked layout stores every (column group, 128-row panel) tile as whole batches of
// 8 records (96 bytes, at least one per tile) plus 8 bytes of tile table: a hypersparse operand
// (1e6 x 1e6 with 3e7 nonzeros: 20 GB of records for 0.36 GB of CSC) would be streamed at a
// fraction of the general kernels' speed, and the tile count must fit the 32-bit scan.  And a
// product kernel must read the layout (pbc_kind: not below 256 rows, for one).
static bool pbc_shape_ok(int64_t nrow, int64_t ncol, int64_t nnz)
{
	int cbw, wpb, logr;
	pbc_auto_layout(nrow, ncol, nnz, &cbw, &wpb, &logr);      // (very sparse operands: panels of 1024 rows)
	if (pbc_kind(nrow, cbw, wpb, logr) <= PBC_KIND_NONE)
		return false;
	const int64_t cb = (int64_t) cbw * wpb;
	const double ngroups = (double) ((ncol + cb - 1) / cb) * (double) wpb;
	const double npanels = (double) ((nrow + ((int64_t) 1 << logr) - 1) >> logr);
	const double ntiles = ngroups * npanels;
	return ntiles + 1.0 < 2147483647.0 && (double) nnz >= 4.0 * ntiles;
}

// (whatever the orientation of the dense operand: one given by rows is transposed on the device)
static bool pbc_applies(const svt_dev_csc *A, int64_t K)
{
	return A->ncol > 0 && (double) A->nnz * (double) K >= 268435456.0 && pbc_shape_ok(A->nrow, A->ncol, A->nnz);
}

// The layout build is device work (a few ms at 1e8 nonzeros) and the upload of the dense
// operand is PCIe + host threads: start the build on a helper thread, upload meanwhile.
struct PbcAhead {
	std::thread th;
	svt_dev_pbc *P = NULL;
	int own = 1;
	bool started = false, taken = false;
	void start(const svt_dev_csc *A, int64_t K)
	{
		if (A->Rtype != SVT_REALSXP || !pbc_applies(A, K)) return;
		started = true;
		const int dev = cur_device();                     // (a shard's device on a shard's thread)
		th = std::thread([this, A, dev] {
			(void) hipSetDevice(dev);
			P = pbc_for(A, &own);
		});
	}
	svt_dev_pbc *get(int *own_out)
	{
		if (th.joinable()) th.join();
		taken = true;
		*own_out = own;
		return P;
	}
	~PbcAhead()
	{
		if (th.joinable()) th.join();
		if (P && own && !taken) svt_dev_pbc_release(P);
	}
};

// n integers on the device -> a new f64 array `dst` (NA_integer_ -> NA_real_: int_to_f64_kernel)
static int widen_int(DevBuf &dst, const void *src, int64_t n)
{
	if (dst.alloc((size_t) (n > 0 ? n : 1) * 8))
		return -1;
	return launch_int_to_f64((const int *) src, n, dst.as<double>(), 0);
}

// An integer operand with f64 values: `view` is A with `val` in place of its values (owns nothing).
struct Widened {
	svt_dev_csc view;
	DevBuf val;
	int widen(const svt_dev_csc *A)
	{
		if (widen_int(val, A->val, A->nnz))
			return -1;
		view = *A;
		view.Rtype = SVT_REALSXP; view.val = val.p; view.owned = 0;
		return 0;
	}
};

// out (device) receives all K columns; the dense operand is already on the device.
static int dev_crossprod_chunked(const svt_dev_csc *A, const void *Y_dev, int64_t ldY,
				 int64_t K, int tr_y, double *out_dev,
				 int64_t sc, int64_t sk, PbcAhead *ahead = NULL)
{
	if (K <= 0 || A->ncol <= 0)
		return 0;
	// Large integer products: the same panel-blocked kernels on f64 copies of the values and
	// of the dense operand (count matrices are integer; see int_to_f64_kernel for why the
	// results, NA rules included, are those of the integer path -- bit for bit while the sums
	// stay below 2^53).
	if (A->Rtype == SVT_INTSXP && !tr_y && ldY == A->nrow && pbc_applies(A, K)) {
		Widened Af;
		DevBuf Yf;
		if (Af.widen(A) || widen_int(Yf, Y_dev, A->nrow * K))
			return -1;
		return dev_crossprod_chunked(&Af.view, Yf.p, ldY, K, 0, out_dev, sc, sk, NULL);
	}
	// Large double products with a column-major dense operand take the panel-blocked
	// kernels: the one-off layout build (a few ms at 1e8 nonzeros)
	// pays for itself within the call.  Below the threshold the general kernels run,
	// whose sums are bit-identical to the reference's sequential ones; above it the
	// row-split partial sums differ from those in the last bits (parity bar: 1e-6).
	if (A->Rtype == SVT_REALSXP && pbc_applies(A, K)) {
		int own_P = 1;
		svt_dev_pbc *P = (ahead && ahead->started) ? ahead->get(&own_P) : pbc_for(A, &own_P);
		if (P == NULL)                 // e.g. more records than 32-bit stream offsets reach:
			goto general;          // the general kernels take any size
		const int kc = K < 512 ? (int) K : 512;
		DevBuf ws;
		int rc = ws.alloc(svt_dev_crossprod_pbc_ws_bytes(P, kc));
		for (int64_t k0 = 0; rc == 0 && k0 < K; k0 += kc) {
			const int kn = (int) (K - k0 < kc ? K - k0 : kc);
			rc = svt_dev_crossprod_pbc(P, A, (const double *) Y_dev + (tr_y ? k0 : k0 * ldY), ldY, kn,
						   tr_y, out_dev + k0 * sk, sc, sk, ws.p, ws.bytes, 0);
		}
		if (rc == 0 && hipDeviceSynchronize() != hipSuccess)
			rc = svt_set_error("device error in the panel-blocked crossprod");
		if (own_P) svt_dev_pbc_release(P);
		return rc;
	}
general:
	const int kc = chunk_K(A->nrow, K);
	DevBuf ws;
	if (ws.alloc(crossprod_ws_bytes(A->nrow, A->ncol, kc)))
		return -1;
	const size_t esz = elt_size(A->Rtype);
	for (int64_t k0 = 0; k0 < K; k0 += kc) {
		const int kn = (int) (K - k0 < kc ? K - k0 : kc);
		const char *Yc = (const char *) Y_dev +
			(tr_y ? (size_t) k0 : (size_t) k0 * (size_t) ldY) * esz;
		if (svt_dev_crossprod_csc_dense(A, Yc, ldY, kn, tr_y,
						out_dev + k0 * sk, sc, sk,
						ws.p, ws.bytes, 0))
			return -1;
	}
	HIP_TRY(hipDeviceSynchronize());
	return 0;
}

// Mixed integer / double operands.  The reference's entry points refuse them ("not supported
// yet") and its R methods coerce the integer operand on the host first (type(x) <- "double",
// R/SparseMatrix-mult.R:75-120) -- a copy of the whole tree.  Here the integer side is uploaded
// as it is (4 bytes per value over PCIe) and widened on the device; as.double(NA_integer_) is
// NA_real_, which is what int_to_f64_kernel writes.
// The product of the dense-operand entry points: A times a dense operand of y_elems elements of y_Rtype, which
// put_y(dst) copies to the device (ldY, tr_y: its layout there), into O (device, zeroed; strides sc, sk).  The layout
// build of A starts first, on a helper thread, so that it overlaps the copy of Y.  (An integer A paired with a double
// Y is widened, and it has no layout to build: PbcAhead::start() does nothing for it.)
template <class PutY>
static int dense_product(const svt_dev_csc *A, int64_t K, int y_Rtype, size_t y_elems, PutY put_y, int64_t ldY,
			 int tr_y, double *O, int64_t sc, int64_t sk)
{
	PbcAhead ahead;
	ahead.start(A, K);
	DevBuf Y;
	if (Y.alloc(y_elems * elt_size(y_Rtype)) || put_y(Y.p))
		return -1;
	const void *Yp = Y.p;
	Widened Aw;
	DevBuf Yw;
	if (A->Rtype != y_Rtype) {
		if (A->Rtype == SVT_INTSXP) {             // sparse int, dense double
			if (Aw.widen(A)) return -1;
			A = &Aw.view;
		} else {                                  // sparse double, dense int
			if (widen_int(Yw, Y.p, (int64_t) y_elems)) return -1;
			Yp = Yw.p;
		}
	}
	return dev_crossprod_chunked(A, Yp, ldY, K, tr_y, O, sc, sk, &ahead);
}

static bool mult_types_ok(int a, int b)
{
	return (a == SVT_REALSXP || a == SVT_INTSXP) && (b == SVT_REALSXP || b == SVT_INTSXP);
}

// crossprod(x, y) over the device list: shard s multiplies the rows [r0, r1) of x and y into a whole ncol x K
// partial (on its device), then owns slice s of the result's cells: it fetches that slice of every partial
// (hipMemcpyPeerAsync; a device-to-device copy between shards on one device), adds them in shard order
// (kernels_shard.hip) and copies the sum into `out`.  The sums depend on N and the row blocks only.
static int crossprod2_SVT_mat_sharded(const svt_view *x, const void *y, int y_nrow, int y_ncol, int y_Rtype,
				      int tr_y, double *out)
{
	if (check_leaves(x))                                // (the row blocks read the offsets)
		return -1;
	const std::vector<int> devs = g_devices;
	const int N = (int) devs.size();
	const int64_t nrow = x->dim[0], ncol = x->dim[1], K = tr_y ? y_nrow : y_ncol;
	const size_t out_n = (size_t) ncol * (size_t) K, ysz = elt_size(y_Rtype);
	ShardBufs part(devs);
	// SVT_SHARD_TIMING=1 (tools/debug/multi_device_time.py): per-shard upload / product / reduce-scatter ms on stderr
	const bool timing = getenv("SVT_SHARD_TIMING") != NULL;
	std::vector<double> t_up((size_t) N, 0.0), t_mul((size_t) N, 0.0), t_red((size_t) N, 0.0);
	auto ms_since = [](std::chrono::steady_clock::time_point t0) {
		return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	};
	int rc = run_shards(devs, [&](int s) -> int {
		const auto t0 = std::chrono::steady_clock::now();
		int64_t r0, r1;
		shard_rows(nrow, s, N, &r0, &r1);
		const int64_t rs = r1 - r0;
		DevBuf O;
		if (O.alloc(out_n * 8) || O.zero())
			return -1;
		if (rs > 0) {
			CscGuard A(row_block_upload(x, r0, r1));
			if (A.h == NULL) return -1;
			auto put_y = [&](void *d) -> int {
				// y is K x nrow: its columns r0 .. r1 are contiguous; else its rows r0 .. r1 of every column
				const int rc = tr_y ? staged_copy(d, (const char *) y + (size_t) r0 * y_nrow * ysz,
								  (size_t) rs * y_nrow * ysz)
						    : staged_copy_2d(d, (const char *) y + (size_t) r0 * ysz, (size_t) rs * ysz,
								     (size_t) K, (size_t) y_nrow * ysz);
				t_up[(size_t) s] = ms_since(t0);
				return rc;
			};
			if (dense_product(A.h, K, y_Rtype, (size_t) rs * K, put_y, tr_y ? y_nrow : rs, tr_y, O.as<double>(), 1,
					  ncol))
				return -1;
		}
		HIP_TRY(hipDeviceSynchronize());                 // (the other shards read the partial next)
		t_mul[(size_t) s] = ms_since(t0) - t_up[(size_t) s];
		part.p[(size_t) s] = O.p;
		O.p = nullptr;
		return 0;
	});
	if (rc) return -1;
	// reduce-scatter: slice s = cells [q[s], q[s + 1]), even boundaries (16-byte accesses in the sum)
	std::vector<size_t> q((size_t) N + 1, out_n);
	for (int s = 0; s < N; s++) q[(size_t) s] = (out_n / N * s + out_n % N * s / N) & ~(size_t) 1;
	rc = run_shards(devs, [&](int s) -> int {
		const auto t0 = std::chrono::steady_clock::now();
		const size_t c0 = q[(size_t) s], len = q[(size_t) s + 1] - c0;
		if (len == 0) return 0;
		const size_t stride = (len + 1) & ~(size_t) 1;
		DevBuf F, R;
		if (F.alloc(stride * N * 8) || R.alloc(len * 8))
			return -1;
		for (int t = 0; t < N; t++) {
			double *dst = F.as<double>() + (size_t) t * stride;
			const double *src = (const double *) part.p[(size_t) t] + c0;
			if (devs[(size_t) t] == devs[(size_t) s])
				HIP_TRY(hipMemcpyAsync(dst, src, len * 8, hipMemcpyDeviceToDevice, 0));
			else
				HIP_TRY(hipMemcpyPeerAsync(dst, devs[(size_t) s], src, devs[(size_t) t], len * 8, 0));
		}
		if (launch_shard_sum(F.as<double>(), N, (int64_t) stride, (int64_t) len, R.as<double>(), 0))
			return -1;
		HIP_TRY(hipStreamSynchronize(0));
		const int rd = staged_download(out + c0, R.p, len * 8);
		t_red[(size_t) s] = ms_since(t0);
		return rd;
	});
	if (timing)
		for (int s = 0; s < N; s++)
			fprintf(stderr, "svt shard %d/%d device %d: upload %.3f ms, product %.3f ms, reduce-scatter %.3f ms\n",
				s, N, devs[(size_t) s], t_up[(size_t) s], t_mul[(size_t) s], t_red[(size_t) s]);
	return rc;
}

// C_crossprod2_SVT_mat, src/SparseMatrix_mult.c:931-982
static int crossprod2_SVT_mat_impl(const svt_view *x, const void *y, int y_nrow,
				      int y_ncol, int y_Rtype, int tr_y, double *out)
{
	if (ensure_init() || check_mult_view(x, "input objects"))
		return -1;
	const int in_nrow = x->dim[0], out_nrow = x->dim[1];
	if (in_nrow != (tr_y ? y_ncol : y_nrow))
		return svt_set_error("input objects are non-conformable");
	if (y_Rtype == SVT_LGLSXP) y_Rtype = SVT_INTSXP;
	if (!mult_types_ok(x->Rtype, y_Rtype))
		return svt_set_error("SparseArray internal error in "
				     "C_crossprod2_SVT_mat():\n"
				     "    'x_Rtype != TYPEOF(y)' not supported yet");
	const int out_ncol = tr_y ? y_nrow : y_ncol;
	const size_t out_n = (size_t) out_nrow * out_ncol;
	memset(out, 0, out_n * sizeof(double));
	if (x->svt_is_null || out_n == 0)     // :389-390
		return 0;
	if (shard_applies(x))
		return crossprod2_SVT_mat_sharded(x, y, y_nrow, y_ncol, y_Rtype, tr_y, out);
	CscGuard A(x);
	if (A.h == NULL) return -1;
	const size_t y_elems = (size_t) y_nrow * y_ncol;
	auto put_y = [&](void *d) { return staged_copy(d, y, y_elems * elt_size(y_Rtype)); };
	DevBuf O;
	if (O.alloc(out_n * 8) || O.zero() ||
	    dense_product(A.h, out_ncol, y_Rtype, y_elems, put_y, y_nrow, tr_y, O.as<double>(), 1, out_nrow))
		return -1;
	return staged_download(out, O.p, out_n * 8);
}
extern "C" int svt_crossprod2_SVT_mat(const svt_view *x, const void *y, int y_nrow,
				      int y_ncol, int y_Rtype, int tr_y, double *out)
{
	return abi_status([&] { return crossprod2_SVT_mat_impl(x, y, y_nrow, y_ncol, y_Rtype, tr_y, out); });
}

// C_crossprod2_mat_SVT, src/SparseMatrix_mult.c:985-1034
static int crossprod2_mat_SVT_impl(const void *x, int x_nrow, int x_ncol,
				      int x_Rtype, const svt_view *y, int tr_x,
				      double *out)
{
	if (ensure_init() || check_mult_view(y, "input objects"))
		return -1;
	const int in_nrow = y->dim[0], out_ncol = y->dim[1];
	if ((tr_x ? x_ncol : x_nrow) != in_nrow)
		return svt_set_error("input objects are non-conformable");
	if (x_Rtype == SVT_LGLSXP) x_Rtype = SVT_INTSXP;
	if (!mult_types_ok(x_Rtype, y->Rtype))
		return svt_set_error("input objects must have the same type() for now");
	const int out_nrow = tr_x ? x_nrow : x_ncol;
	const size_t out_n = (size_t) out_nrow * out_ncol;
	memset(out, 0, out_n * sizeof(double));
	if (y->svt_is_null || out_n == 0)     // :439-440
		return 0;
	CscGuard A(y);
	if (A.h == NULL) return -1;
	const size_t x_elems = (size_t) x_nrow * x_ncol;
	auto put_x = [&](void *d) { return staged_copy(d, x, x_elems * elt_size(x_Rtype)); };
	// result cell (i = dense vector, j = leaf) lives at out[i + j*out_nrow]
	DevBuf O;
	if (O.alloc(out_n * 8) || O.zero() ||
	    dense_product(A.h, out_nrow, x_Rtype, x_elems, put_x, x_nrow, tr_x, O.as<double>(), out_nrow, 1))
		return -1;
	return staged_download(out, O.p, out_n * 8);
}
extern "C" int svt_crossprod2_mat_SVT(const void *x, int x_nrow, int x_ncol,
				      int x_Rtype, const svt_view *y, int tr_x,
				      double *out)
{
	return abi_status([&] { return crossprod2_mat_SVT_impl(x, x_nrow, x_ncol, x_Rtype, y, tr_x, out); });
}

// Densify columns of `pp` chunk by chunk and multiply every chunk with the
// leaves of `other`: crossprod2_Lpp_* / crossprod2_Rpp_*,
// src/SparseMatrix_mult.c:728-820.  sym (crossprod(x): pp is other) computes
// only the cells that the caller's mirror does not fill.
static int dev_crossprod_pp(const svt_dev_csc *other, const svt_dev_csc *pp, bool sym,
			    double *out_dev, int64_t sc, int64_t sk)
{
	const int64_t K = pp->ncol, nrow = pp->nrow;
	if (K <= 0 || other->ncol <= 0)
		return 0;
	const bool big = pbc_applies(other, K);
	if (other->Rtype == SVT_INTSXP && big) {                         // as in dev_crossprod_chunked
		Widened of, pf;
		if (of.widen(other) || (!sym && pf.widen(pp)))
			return -1;
		return dev_crossprod_pp(&of.view, sym ? &of.view : &pf.view, sym, out_dev, sc, sk);
	}
	int kc = chunk_K(nrow, K);
	const size_t esz = elt_size(pp->Rtype);
	// large double products: panel-blocked layout of `other`, built once, against
	// every densified chunk (same threshold and caveat as dev_crossprod_chunked)
	svt_dev_pbc *P = NULL;
	int own_P = 1;
	if (other->Rtype == SVT_REALSXP && big) {
		P = pbc_for(other, &own_P);
		if (P != NULL && kc > 512) kc = 512;
	}
	DevBuf dense, ws;
	int rc = 0;
	if (dense.alloc((size_t) (nrow > 0 ? nrow : 1) * kc * esz) ||
	    ws.alloc(P ? svt_dev_crossprod_pbc_ws_bytes(P, kc)
		       : crossprod_ws_bytes(nrow, other->ncol, kc)))
		rc = -1;
	// sym: of the dense chunk [k0, k0 + kn) only the leaves c >= k0 are needed -- the cells
	// with c >= k, which the caller mirrors -- as in compute_sym_dotprods_*
	// (src/SparseMatrix_mult.c:263-296: ncol^2 / 2 dot products).
	for (int64_t k0 = 0; rc == 0 && k0 < K; k0 += kc) {
		const int kn = (int) (K - k0 < kc ? K - k0 : kc);
		if (launch_densify(pp->col_ptr, pp->row_idx, pp->val, pp->Rtype, nrow,
				   k0, kn, dense.p, 0)) {
			rc = -1;
		} else if (P) {
			rc = svt_dev_crossprod_pbc_from(P, other, (const double *) dense.p, nrow, kn, 0,
							out_dev + k0 * sk, sc, sk, ws.p, ws.bytes, 0,
							sym ? k0 : 0);
		} else if (sym && k0 > 0) {
			svt_dev_csc tail = *other;                 // leaves k0 .. ncol-1 (col_ptr entries stay absolute)
			tail.col_ptr += k0; tail.ncol -= k0; tail.owned = 0;
			rc = svt_dev_crossprod_csc_dense(&tail, dense.p, nrow, kn, 0,
							 out_dev + k0 * sk + k0 * sc, sc, sk,
							 ws.p, ws.bytes, 0);
		} else {
			rc = svt_dev_crossprod_csc_dense(other, dense.p, nrow, kn, 0,
							 out_dev + k0 * sk, sc, sk,
							 ws.p, ws.bytes, 0);
		}
	}
	if (rc == 0 && hipDeviceSynchronize() != hipSuccess)
		rc = svt_set_error("device error in the sparse x sparse crossprod");
	if (P && own_P) svt_dev_pbc_release(P);
	return rc;
}

struct OwnedCsc {            // a handle, released with this object only if this call built it
	svt_dev_csc *t;
	bool own;
	OwnedCsc(svt_dev_csc *p, bool o) : t(p), own(o) {}
	OwnedCsc(OwnedCsc &&o) : t(o.t), own(o.own) { o.own = false; }
	OwnedCsc(const OwnedCsc &) = delete;
	OwnedCsc &operator=(const OwnedCsc &) = delete;
	~OwnedCsc() { if (own) svt_release(t); }
};
static OwnedCsc transposed_for(const CscGuard &A);

// The operand of a 2-D col/row method pair (medians, quantiles, MADs, ranks).  check(): stopifnot_2D_object()
// (R/SparseArray-matrixStats.R:51-57), then the type and background rules, which name the col method for either call.
// The object puts x on the device, resident or uploaded, and gives M, the operand whose columns are worked on: x, or
// for the row method t(x) built on the device (rowMedians(x) = colMedians(t(x)), :802-815).  M == NULL: error set.
struct ColOperand {
	CscGuard A;
	OwnedCsc T;
	const svt_dev_csc *M;
	ColOperand(const svt_view *x, int by_row)
		: A(x), T(by_row && A.h ? transposed_for(A) : OwnedCsc(NULL, false)), M(by_row ? T.t : A.h) {}
	static int check(const svt_view *x, int by_row, const char *col, const char *row)
	{
		if (ensure_init() || check_view(x))
			return -1;
		if (x->ndim != 2)
			return svt_set_error("the %s() method for SparseArray objects only supports 2D "
					     "objects (i.e. SparseMatrix objects) at the moment", by_row ? row : col);
		if (x->Rtype != SVT_REALSXP && x->Rtype != SVT_INTSXP && x->Rtype != SVT_LGLSXP)
			return svt_set_error("%s(): unsupported type", col);
		if (x->na_background)
			return svt_set_error("%s() is not supported on NaArray objects", col);
		return 0;
	}
};

// The sparse-aware route (kernels_gram.hip) multiplies only the pairs of nonzeros that meet in a row -- about
// nnz(x) * nnz(y) / nrow of them (half that for the unary form), each an LDS atomic behind a gathered 12-byte read --
// where the dense-buffer route below does `dense_ops` multiply-adds (the reference's Lpp_nops / Rpp_nops,
// src/SparseMatrix_mult.c:1077-1078).  Times measured on one MI355X (tools/debug/sparse_crossprod_time.py, round 6):
// gathered pairs at 2.6e11 / s behind t(x) (2.5e-11 s per nonzero) and ~0.2 ms of launches; the dense-buffer route at
// 3e12 multiply-adds / s behind ~1 ms of allocations, layout build and synchronisation.
static double g_gram_cost = 1.0;
extern "C" void svt_sparse_crossprod_set_cost(double factor)
{
	g_gram_cost = factor;      // the sparse-aware route's estimated time is multiplied by it; < 0: never that route; 0: always
}

static double dense_route_seconds(double dense_ops) { return 1.0e-3 + dense_ops / 3.0e12; }
static double sparse_route_seconds(double pairs, int64_t nnz_x) { return 0.2e-3 + pairs / 2.6e11 + (double) nnz_x * 2.5e-11; }

static bool sparse_route_pays(int64_t nnz_x, int64_t nnz_y, int64_t nrow, double dense_ops, bool sym)
{
	if (g_gram_cost < 0.0 || nrow <= 0 || nnz_x <= 0 || nnz_y <= 0)
		return false;
	double pairs = (double) nnz_x * (double) nnz_y / (double) nrow;
	// small products stay with the general kernels of the dense-buffer route: their sums run in the reference's own
	// ascending order, bit for bit (tests/test_hip_vs_oracle.py); from the size on where that route takes the panel
	// kernels (pbc_applies) neither route is ordered like the reference and the faster one is taken
	if (g_gram_cost > 0.0 && dense_ops < 268435456.0)
		return false;
	if (sym) { pairs *= 0.5; dense_ops *= 0.5; }
	return sparse_route_seconds(pairs, nnz_x) * g_gram_cost < dense_route_seconds(dense_ops);
}

// 0: `O` holds the result; 1: a non-finite value or an NA took part (the caller takes the dense-buffer route, whose
// dirty-leaf rules are the reference's); -1: error
static int dev_crossprod_sparse_on(const svt_dev_csc *T, const svt_dev_csc *Y, bool sym, double *O, int64_t ldo, double dense_ops)
{
	DevBuf Ws;
	int bad = 1;
	if (Ws.alloc(svt_dev_crossprod_csc_csc_ws_bytes(T)))
		return -1;
	if (sym && g_gram_cost > 0.0) {
		// The choice was made on nnz^2 / (2 nrow) pairs; with t(x) at hand they can be counted: rows of very unequal
		// length hold more (sum of len^2), and an operand whose count says the other route is clearly faster goes there.
		double pairs = 0.0;
		if (launch_gram_pairs(T->col_ptr, T->ncol, (double *) Ws.p, 0))
			return -1;
		HIP_TRY(hipMemcpy(&pairs, Ws.p, 8, hipMemcpyDeviceToHost));
		if (sparse_route_seconds(pairs, 0) * g_gram_cost > 1.5 * dense_route_seconds(0.5 * dense_ops))
			return 1;
	}
	const int rc = svt_dev_crossprod_csc_csc(T, Y, sym ? 1 : 0, O, ldo, Ws.p, Ws.bytes, NULL, 0);
	if (rc > 0) { g_unsupported = 0; return 1; }      // a shape this kernel refuses: the other route
	if (rc < 0) return -1;
	HIP_TRY(hipMemcpy(&bad, Ws.p, 4, hipMemcpyDeviceToHost));
	return bad ? 1 : 0;
}

static int dev_crossprod_sparse(const CscGuard &X, const svt_dev_csc *Y, bool sym, double *O, int64_t ldo, double dense_ops)
{
	// An operand of 2^31 nonzeros or more keeps the dense-buffer route, which needs no t(x): the transposition takes
	// such operands through its boxed driver, but a t(x) of that size (plus its workspace) for the sparse-aware kernel
	// is a separate, unmeasured choice.  (The fixed bound, not the box limit of svt_dev_set_box_nnz: forcing boxes in a
	// test changes no route.)
	if (X.h->nnz >= ((int64_t) 1 << 31))
		return 1;
	const OwnedCsc T = transposed_for(X);
	if (T.t == NULL) {
		// an operand the transposition does not take (2^31 nonzeros or more): the dense-buffer route needs no t(x)
		if (g_unsupported) { g_unsupported = 0; return 1; }
		return -1;
	}
	return dev_crossprod_sparse_on(T.t, Y, sym, O, ldo, dense_ops);
}

// The dense-buffer route of crossprod(X, Y) (what the sparse x sparse entry points fall back to): O = ncol(X) x ncol(Y)
// on the device, column-major, zeroed here.  sym: the unary form crossprod(X) (Y is X), half the dot products + mirror.
// Else the columns of the operand with fewer multiply-adds are expanded (Lpp_nops / Rpp_nops,
// src/SparseMatrix_mult.c:1075-1097).
static int dense_buffer_route(const svt_dev_csc *X, const svt_dev_csc *Y, bool sym, double *O)
{
	const int64_t nx = X->ncol, ny = Y->ncol;
	HIP_TRY(hipMemset(O, 0, (size_t) nx * ny * 8));
	if (sym)
		return dev_crossprod_pp(X, X, true, O, 1, nx) || launch_mirror_lower(O, nx, 0) ? -1 : 0;
	if (Y->nnz * nx < X->nnz * ny)     // expand the columns of X, walk the leaves of Y
		return dev_crossprod_pp(Y, X, false, O, nx, 1);
	return dev_crossprod_pp(X, Y, false, O, 1, nx);     // expand the columns of Y, walk the leaves of X
}

// The dense-buffer route on resident operands (the yardstick of tools/debug/sparse_crossprod_time.py).  Y == X (the
// same handle): the unary form.  Allocates and synchronises.
extern "C" int svt_dev_crossprod_csc_csc_dense_buffer(const svt_dev_csc *X, const svt_dev_csc *Y, double *out)
{
	if (X->nrow != Y->nrow)
		return svt_set_error("svt_dev_crossprod_csc_csc_dense_buffer: non-conformable operands");
	if (X->ncol == 0 || Y->ncol == 0) return 0;
	if (dense_buffer_route(X, Y, X == Y, out)) return -1;
	HIP_TRY(hipDeviceSynchronize());
	return 0;
}

// The sparse x sparse entry points' last step, into `out` (out_n doubles): sparse(O), the sparse-aware route into the
// device buffer O (0: done; 1: declined, the route does not pay or a non-finite value took part; -1: error), then if
// it declined dense(O), the dense-buffer route.
template <class S, class D> static int sparse_then_dense(double *out, size_t out_n, S sparse, D dense)
{
	DevBuf O;
	if (O.alloc(out_n * 8))
		return -1;
	const int st = sparse(O.as<double>());
	if (st < 0 || (st > 0 && dense(O.as<double>())))
		return -1;
	return staged_download(out, O.p, out_n * 8);
}

static int64_t view_nzcount(const svt_view *x)   // _REC_nzcount_SVT, SVT_SparseArray_class.c:200-218
{
	int64_t t = 0;
	if (x->svt_is_null) return 0;
	for (int64_t j = 0; j < x->nleaves; j++) t += x->nzcount[j];
	return t;
}

// C_crossprod2_SVT_SVT, src/SparseMatrix_mult.c:1037-1101
static int crossprod2_SVT_SVT_impl(const svt_view *x, const svt_view *y, double *out)
{
	if (ensure_init() || check_mult_view(x, "input objects") ||
	    check_mult_view(y, "input objects"))
		return -1;
	const int in_nrow = x->dim[0];
	if (in_nrow != y->dim[0])
		return svt_set_error("input SVT_SparseMatrix objects are non-conformable");
	if (x->Rtype != y->Rtype)
		return svt_set_error("input SVT_SparseMatrix objects must have the "
				     "same type() for now");
	const int out_nrow = x->dim[1], out_ncol = y->dim[1];
	const size_t out_n = (size_t) out_nrow * out_ncol;
	memset(out, 0, out_n * sizeof(double));
	if (out_n == 0)
		return 0;
	const int64_t Lpp_nops = view_nzcount(y) * out_nrow;   // :1077-1078
	const int64_t Rpp_nops = view_nzcount(x) * out_ncol;
	const double dense_ops = (double) (Lpp_nops < Rpp_nops ? Lpp_nops : Rpp_nops);
	CscGuard X(x), Y(y);
	if (X.h == NULL || Y.h == NULL) return -1;
	// few pairs of nonzeros meet in a row: multiply only those (kernels_gram.hip); a non-finite value or an NA
	// anywhere sends the product down the reference's route.  (Under the resident cache crossprod(x, x) gets one
	// handle for both operands: still the two-operand form.)
	const bool pays = !x->svt_is_null && !y->svt_is_null &&
			  sparse_route_pays(X.h->nnz, Y.h->nnz, in_nrow, dense_ops, false);
	return sparse_then_dense(out, out_n,
		[&](double *O) { return pays ? dev_crossprod_sparse(X, Y.h, false, O, out_nrow, dense_ops) : 1; },
		[&](double *O) { return dense_buffer_route(X.h, Y.h, false, O); });
}
extern "C" int svt_crossprod2_SVT_SVT(const svt_view *x, const svt_view *y, double *out)
{
	return abi_status([&] { return crossprod2_SVT_SVT_impl(x, y, out); });
}

// t(A) on the device, as a handle that owns its buffers (A may be released afterwards).
static svt_dev_csc *dev_transposed(const svt_dev_csc *A)
{
	svt_dev_csc *T = (svt_dev_csc *) calloc(1, sizeof(*T));
	if (T == NULL) { svt_set_error("out of memory"); return NULL; }
	T->Rtype = A->Rtype; T->owned = 1; T->na_background = A->na_background;
	T->nrow = A->ncol; T->ncol = A->nrow; T->nnz = A->nnz;
	const size_t n = A->nnz > 0 ? (size_t) A->nnz : 1;
	const int64_t box = box_nnz_get();
	DevBuf ws;
	if (hipMalloc((void **) &T->col_ptr, ((size_t) T->ncol + 1) * 8) != hipSuccess ||
	    hipMalloc((void **) &T->row_idx, n * 4) != hipSuccess ||
	    hipMalloc(&T->val, n * elt_size(A->Rtype)) != hipSuccess ||
	    ws.alloc(transpose_ws_bytes_box(A->nrow, A->nnz, box))) {
		svt_set_error("device allocation failed (transposed operand)");
		svt_release(T);
		return NULL;
	}
	if (launch_transpose_box(A->col_ptr, A->row_idx, A->val, A->Rtype, A->nrow, A->ncol, A->nnz,
				 T->col_ptr, T->row_idx, T->val, ws.p, box, 0) ||
	    hipDeviceSynchronize() != hipSuccess) {
		if (svt_last_error()[0] == '\0') svt_set_error("device transposition failed");
		svt_release(T);
		return NULL;
	}
	return T;
}

// t(A) of an operand: kept with a resident operand, else built for this call and owned by the result.
static OwnedCsc transposed_for(const CscGuard &A)
{
	if (A.key != 0) {
		std::lock_guard<std::mutex> lk(g_res_mu);
		for (Resident &r : g_res)
			if (r.key == A.key && r.tr != NULL) return OwnedCsc(r.tr, false);
	}
	svt_dev_csc *T = dev_transposed(A.h);
	if (T == NULL || A.key == 0) return OwnedCsc(T, true);
	std::lock_guard<std::mutex> lk(g_res_mu);
	const size_t nb = csc_bytes(T);
	resident_make_room(nb);                           // may erase entries: search afterwards
	if (g_res_bytes + nb <= g_res_limit)
		for (Resident &r : g_res)
			if (r.key == A.key) {
				r.tr = T; r.bytes += nb; g_res_bytes += nb;
				return OwnedCsc(T, false);
			}
	return OwnedCsc(T, true);
}

// C_transpose_2D_SVT, src/SparseArray_aperm.c:395-423
static int transpose_2D_SVT_impl(const svt_view *x, int64_t *out_col_ptr,
				    int32_t *out_row_idx, void *out_val)
{
	if (ensure_init() || check_view(x))
		return -1;
	if (x->ndim != 2)
		return svt_set_error("object to transpose must have exactly 2 dimensions");
	const int64_t nrow = x->dim[0];
	if (x->svt_is_null || x->dim[1] == 0 || nrow == 0) {     // :405-406: nothing to move
		for (int64_t i = 0; i <= nrow; i++) out_col_ptr[i] = 0;
		return 0;
	}
	CscGuard A(x);
	if (A.h == NULL) return -1;
	const OwnedCsc TA = transposed_for(A);
	const svt_dev_csc *T = TA.t;
	if (T == NULL) return -1;
	HIP_TRY(hipMemcpy(out_col_ptr, T->col_ptr, (size_t) (nrow + 1) * 8, hipMemcpyDeviceToHost));
	if (T->nnz > 0) {
		if (staged_download(out_row_idx, T->row_idx, (size_t) T->nnz * 4) ||
		    staged_download(out_val, T->val, (size_t) T->nnz * elt_size(T->Rtype)))
			return -1;
	}
	return 0;
}
extern "C" int svt_transpose_2D_SVT(const svt_view *x, int64_t *out_col_ptr,
				    int32_t *out_row_idx, void *out_val)
{
	return abi_status([&] { return transpose_2D_SVT_impl(x, out_col_ptr, out_row_idx, out_val); });
}

// x[i, j] by an N-index (C_subset_SVT_by_Nindex, src/SparseArray_subsetting.c:223-297, 759-843; 2-D operands): the
// subscripts are checked here, on the host, before anything is uploaded; the composition is dev_subset_impl().
struct svt_subset_result {
	svt_dev_csc *h;              // owns its buffers
};

// 1-based subscript of an axis of `extent` -> 0-based, or the error of the reference's checks
static int subset_index0(const int *idx, int64_t n, int extent, std::vector<int32_t> &out)
{
	if (n < 0 || (n > 0 && idx == NULL))
		return svt_set_error("invalid subscript");
	out.resize((size_t) n);
	for (int64_t k = 0; k < n; k++) {
		const int v = idx[k];
		if (v == NA_INT)
			return svt_set_error("subscript contains NAs");
		if (v < 1 || v > extent)
			return svt_set_error("subscript out of bounds");
		out[(size_t) k] = v - 1;
	}
	return 0;
}

static void *result_hip_alloc(size_t n, void *)
{
	void *p = NULL;
	return hipMalloc(&p, n) == hipSuccess ? p : NULL;
}
static void result_hip_free(void *p, void *) { (void) hipFree(p); }

// The tail of every `begin` that leaves a result on the device, stated once: the handle that owns the result is made with
// the type and extents given, `compose(to, &Rtype)` runs on the default stream over hipMalloc / hipFree, the stream is
// synchronised; a failure without a message gets the default text, and every failure releases what there is.  Then the
// result record is made, the flag word is read where there is one (`flag`: the overflow of Arith and sweep, the
// not_finite of the product) and the outputs are published ('out_Rtype' and 'raised' may be NULL).
template <class Res, class Compose>
static int result_begin(const char *who, int Rtype, int na_background, int64_t nrow, int64_t ncol, Compose compose, DevFlag *flag,
			Res **res, int *out_Rtype, int64_t *out_nnz, int *raised)
{
	svt_dev_csc *h = (svt_dev_csc *) calloc(1, sizeof(*h));
	if (h == NULL) return svt_set_error("out of memory");
	h->Rtype = Rtype; h->owned = 1; h->na_background = na_background;
	h->nrow = nrow; h->ncol = ncol;
	if (compose(ResultDest{ result_hip_alloc, result_hip_free, NULL, &h->nnz, &h->col_ptr, &h->row_idx, &h->val }, &h->Rtype) ||
	    hipStreamSynchronize(0) != hipSuccess) {
		if (svt_last_error()[0] == '\0') svt_set_error("%s: device error", who);
		svt_release(h);
		return -1;
	}
	int w = 0;
	Res *r = (Res *) calloc(1, sizeof(*r));
	if ((flag != NULL && flag->read(&w)) || r == NULL) {
		svt_release(h);
		free(r);
		return r == NULL ? svt_set_error("out of memory") : -1;
	}
	r->h = h;
	*res = r;
	if (out_Rtype != NULL) *out_Rtype = h->Rtype;
	*out_nnz = h->nnz;
	if (raised != NULL) *raised = w;
	return 0;
}

static int subset_SVT_begin_impl(const svt_view *x, const int *rows, int64_t nrows_sel, const int *cols, int64_t ncols_sel,
				 svt_subset_result **res, int64_t *out_nnz)
{
	if (res == NULL || out_nnz == NULL)
		return svt_set_error("svt_subset_SVT_begin: 'res' and 'out_nnz' are needed");
	*res = NULL;
	if (ensure_init() || check_view(x))
		return -1;
	if (x->ndim != 2)
		return svt_set_unsupported("N-index subsetting on the device takes 2-D operands only");
	std::vector<int32_t> r0, c0;
	if ((rows != NULL && subset_index0(rows, nrows_sel, x->dim[0], r0)) ||
	    (cols != NULL && subset_index0(cols, ncols_sel, x->dim[1], c0)))
		return -1;
	CscGuard A(x);
	if (A.h == NULL) return -1;
	DevBuf dr, dc;
	if ((rows != NULL && dr.upload(r0.data(), r0.size() * 4)) || (cols != NULL && dc.upload(c0.data(), c0.size() * 4)))
		return -1;
	return result_begin("svt_subset_SVT_begin", A.h->Rtype, A.h->na_background, rows != NULL ? nrows_sel : A.h->nrow,
			    cols != NULL ? ncols_sel : A.h->ncol,
			    [&](const ResultDest &to, int *) {
				    return dev_subset_impl(A.h, dr.as<int32_t>(), rows != NULL ? nrows_sel : -1, dc.as<int32_t>(),
							   cols != NULL ? ncols_sel : -1, to, NULL);
			    },
			    NULL, res, NULL, out_nnz, NULL);
}
extern "C" int svt_subset_SVT_begin(const svt_view *x, const int *rows, int64_t nrows_sel, const int *cols, int64_t ncols_sel,
				    svt_subset_result **res, int64_t *out_nnz)
{
	return abi_status([&] { return subset_SVT_begin_impl(x, rows, nrows_sel, cols, ncols_sel, res, out_nnz); });
}

// The `end` of a begin / end pair: the result a `begin` left on the device copied out (all three outputs, or none:
// release only) and released.
static int result_end(const char *who, svt_dev_csc *h, int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val)
{
	int rc = 0;
	if (out_col_ptr != NULL || out_row_idx != NULL || out_val != NULL) {
		if (out_col_ptr == NULL || (h->nnz > 0 && (out_row_idx == NULL || out_val == NULL)))
			rc = svt_set_error("%s: all three outputs, or none", who);
		else if (hipMemcpy(out_col_ptr, h->col_ptr, ((size_t) h->ncol + 1) * 8, hipMemcpyDeviceToHost) != hipSuccess)
			rc = svt_set_error("%s: D2H copy failed", who);
		else if (h->nnz > 0 && (staged_download(out_row_idx, h->row_idx, (size_t) h->nnz * 4) ||
					staged_download(out_val, h->val, (size_t) h->nnz * elt_size(h->Rtype))))
			rc = -1;
	}
	svt_release(h);
	return rc;
}

static int subset_SVT_end_impl(svt_subset_result *res, int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val)
{
	if (res == NULL) return 0;
	const int rc = result_end("svt_subset_SVT_end", res->h, out_col_ptr, out_row_idx, out_val);
	free(res);
	return rc;
}
extern "C" int svt_subset_SVT_end(svt_subset_result *res, int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val)
{
	return abi_status([&] { return subset_SVT_end_impl(res, out_col_ptr, out_row_idx, out_val); });
}

// Arith / Math on host operands (C_Arith_SVT1_SVT2, C_Arith_SVT1_v2, C_unary_minus_SVT, C_Math_SVT): the operands go
// up through the resident cache, ArithCall::compose() runs on the first device, the result stays there until `end`.
struct svt_arith_result {
	svt_dev_csc *h;              // owns its buffers
};

static int arith_begin_impl(const char *who, int kind, int op, const svt_view *x, const svt_view *y, double s, int s_Rtype,
			    svt_arith_result **res, int *out_Rtype, int64_t *out_nnz, int *ovflow, int rule = ARI_RULE_ARITH)
{
	if (res == NULL || out_Rtype == NULL || out_nnz == NULL)
		return svt_set_error("%s: 'res', 'out_Rtype' and 'out_nnz' are needed", who);
	*res = NULL;
	if (ensure_init() || check_view(x) || (y != NULL && check_view(y)))
		return -1;
	if (y != NULL) {
		bool same = x->ndim == y->ndim;
		for (int a = 0; same && a < x->ndim; a++) same = x->dim[a] == y->dim[a];
		if (!same) return svt_set_error("non-conformable arrays");
	}
	CscGuard A(x);
	if (A.h == NULL) return -1;
	std::optional<CscGuard> B;
	if (y != NULL) {
		B.emplace(y);
		if (B->h == NULL) return -1;
	}
	DevFlag ov;
	if (ov.init()) return -1;
	ArithCall c = { who, kind, op, A.h, B ? B->h : NULL, s, s_Rtype };
	c.rule = rule;
	return result_begin(who, 0, 0, A.h->nrow, A.h->ncol,
			    [&](const ResultDest &to, int *rt) { return c.compose(to, rt, ov.ptr(), NULL); }, &ov, res, out_Rtype, out_nnz,
			    ovflow);
}
extern "C" int svt_Arith_SVT_SVT_begin(const svt_view *x, const svt_view *y, int op, svt_arith_result **res, int *out_Rtype,
				       int64_t *out_nnz, int *ovflow)
{
	return abi_status([&] {
		if (y == NULL) return svt_set_error("svt_Arith_SVT_SVT_begin: two operands are needed");
		return arith_begin_impl("svt_Arith_SVT_SVT_begin", SVT_ARITH_MERGE, op, x, y, 0.0, 0, res, out_Rtype, out_nnz, ovflow);
	});
}
extern "C" int svt_Arith_SVT_scalar_begin(const svt_view *x, int op, double s, int s_Rtype, svt_arith_result **res,
					  int *out_Rtype, int64_t *out_nnz, int *ovflow)
{
	return abi_status([&] {
		return arith_begin_impl("svt_Arith_SVT_scalar_begin", SVT_ARITH_SCALAR, op, x, NULL, s, s_Rtype, res, out_Rtype, out_nnz,
					ovflow);
	});
}
extern "C" int svt_unary_minus_SVT_begin(const svt_view *x, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz)
{
	return abi_status([&] {
		return arith_begin_impl("svt_unary_minus_SVT_begin", SVT_ARITH_NEG, 0, x, NULL, 0.0, 0, res, out_Rtype, out_nnz, NULL);
	});
}
extern "C" int svt_Math_SVT_begin(const svt_view *x, int op, double digits, svt_arith_result **res, int *out_Rtype,
				  int64_t *out_nnz)
{
	(void) digits;                                      // (round / signif: not supported here)
	return abi_status([&] {
		return arith_begin_impl("svt_Math_SVT_begin", SVT_ARITH_MATH, op, x, NULL, 0.0, 0, res, out_Rtype, out_nnz, NULL);
	});
}
// Compare / Logic on host operands (C_Compare_SVT1_SVT2, C_Compare_SVT1_v2, C_Logic_SVT1_SVT2): the same begin under
// another rule; the result is LGLSXP and svt_Arith_SVT_end ends it.
static int compare_begin(const char *who, int rule, int op, const svt_view *x, const svt_view *y, bool merge, double s, int s_Rtype,
			 svt_arith_result **res, int64_t *out_nnz)
{
	return abi_status([&] {
		int rt = 0;
		if (merge && y == NULL) return svt_set_error("%s: two operands are needed", who);
		return arith_begin_impl(who, merge ? SVT_ARITH_MERGE : SVT_ARITH_SCALAR, op, x, y, s, s_Rtype, res, &rt, out_nnz, NULL, rule);
	});
}
extern "C" int svt_Compare_SVT_SVT_begin(const svt_view *x, const svt_view *y, int op, svt_arith_result **res, int64_t *out_nnz)
{
	return compare_begin("svt_Compare_SVT_SVT_begin", ARI_RULE_COMPARE, op, x, y, true, 0.0, 0, res, out_nnz);
}
extern "C" int svt_Compare_SVT_scalar_begin(const svt_view *x, int op, double s, int s_Rtype, svt_arith_result **res,
					    int64_t *out_nnz)
{
	return compare_begin("svt_Compare_SVT_scalar_begin", ARI_RULE_COMPARE, op, x, NULL, false, s, s_Rtype, res, out_nnz);
}
extern "C" int svt_Logic_SVT_SVT_begin(const svt_view *x, const svt_view *y, int op, svt_arith_result **res, int64_t *out_nnz)
{
	return compare_begin("svt_Logic_SVT_SVT_begin", ARI_RULE_LOGIC, op, x, y, true, 0.0, 0, res, out_nnz);
}
// pmin / pmax and is.na / is.nan / is.infinite on host operands (.pminmax2, .isFUN_SVT): the same begin under the two
// other rules; svt_Arith_SVT_end ends it.
extern "C" int svt_pminmax_SVT_SVT_begin(const svt_view *x, const svt_view *y, int op, svt_arith_result **res, int *out_Rtype,
					 int64_t *out_nnz)
{
	return abi_status([&] {
		if (y == NULL) return svt_set_error("svt_pminmax_SVT_SVT_begin: two operands are needed");
		return arith_begin_impl("svt_pminmax_SVT_SVT_begin", SVT_ARITH_MERGE, op, x, y, 0.0, 0, res, out_Rtype, out_nnz, NULL,
					ARI_RULE_PMINMAX);
	});
}
extern "C" int svt_pminmax_SVT_scalar_begin(const svt_view *x, int op, double s, int s_Rtype, svt_arith_result **res,
					    int *out_Rtype, int64_t *out_nnz)
{
	return abi_status([&] {
		return arith_begin_impl("svt_pminmax_SVT_scalar_begin", SVT_ARITH_SCALAR, op, x, NULL, s, s_Rtype, res, out_Rtype, out_nnz,
					NULL, ARI_RULE_PMINMAX);
	});
}
extern "C" int svt_isFUN_SVT_begin(const svt_view *x, int op, svt_arith_result **res, int64_t *out_nnz)
{
	return compare_begin("svt_isFUN_SVT_begin", ARI_RULE_ISFUN, op, x, NULL, false, 0.0, 0, res, out_nnz);
}
// sweep(x, MARGIN, STATS, op) on host operands: the margin becomes the three integers of the device index here, the
// operand and the vector go up, SweepCall::compose() runs on the first device, the result stays there until `end`.
// `margin`: 1-based, a strictly increasing run of consecutive dimensions.  With dimension 1 in it the vector has a row
// part and the leaves of the run's other dimensions are the fastest ones (stride 1); else the run starts `stride` leaves
// apart.
static int sweep_geometry(const char *who, const svt_view *x, const int *margin, int nmargin, int *with_rows, int64_t *stride,
			  int64_t *len)
{
	if (margin == NULL || nmargin < 1 || nmargin > x->ndim)
		return svt_set_error("%s: 'margin' must name between 1 and %d dimensions", who, x->ndim);
	for (int a = 0; a < nmargin; a++)
		if (margin[a] < 1 || margin[a] > x->ndim || (a > 0 && margin[a] != margin[a - 1] + 1))
			return svt_set_error("%s: 'margin' must be a strictly increasing run of consecutive dimensions of the operand", who);
	*with_rows = margin[0] == 1;
	*stride = 1;
	*len = 1;
	for (int a = 1; a < margin[0] - 1; a++) *stride *= x->dim[a];
	for (int a = 0; a < nmargin; a++)
		if (margin[a] > 1) *len *= x->dim[margin[a] - 1];
	return 0;
}
static int sweep_begin_impl(const char *who, int rule, const svt_view *x, int op, const void *stats, int64_t stats_len, int stats_Rtype,
			    const int *margin, int nmargin, int64_t *bad_index, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz,
			    int *ovflow)
{
	if (res == NULL || out_Rtype == NULL || out_nnz == NULL)
		return svt_set_error("%s: 'res', 'out_Rtype' and 'out_nnz' are needed", who);
	*res = NULL;
	if (bad_index != NULL) *bad_index = -1;
	if (ensure_init() || check_view(x))
		return -1;
	if (!logical_family_type(stats_Rtype))
		return svt_set_error("%s: the vector must be of type \"logical\", \"integer\" or \"double\"", who);
	int with_rows = 0;
	int64_t stride = 1, len = 1;
	if (sweep_geometry(who, x, margin, nmargin, &with_rows, &stride, &len))
		return -1;
	if (stats_len < 0 || (stats_len > 0 && stats == NULL))
		return svt_set_error("%s: the vector is needed", who);
	CscGuard A(x);
	if (A.h == NULL) return -1;
	DevBuf dv;
	DevFlag ov;
	if (dv.upload(stats, (size_t) stats_len * elt_size(stats_Rtype)) || ov.init())
		return -1;
	SweepCall c = { who, rule, op, A.h, dv.p, stats_Rtype, stats_len, with_rows, stride, len };
	return result_begin(who, 0, 0, A.h->nrow, A.h->ncol,
			    [&](const ResultDest &to, int *rt) { return c.compose(to, rt, ov.ptr(), bad_index, NULL); }, &ov, res, out_Rtype,
			    out_nnz, ovflow);
}
extern "C" int svt_Arith_SVT_vector_begin(const svt_view *x, int op, const void *stats, int64_t stats_len, int stats_Rtype,
					  const int *margin, int nmargin, int64_t *bad_index, svt_arith_result **res, int *out_Rtype,
					  int64_t *out_nnz, int *ovflow)
{
	return abi_status([&] {
		return sweep_begin_impl("svt_Arith_SVT_vector_begin", ARI_RULE_ARITH, x, op, stats, stats_len, stats_Rtype, margin, nmargin,
					bad_index, res, out_Rtype, out_nnz, ovflow);
	});
}
extern "C" int svt_Compare_SVT_vector_begin(const svt_view *x, int op, const void *stats, int64_t stats_len, int stats_Rtype,
					    const int *margin, int nmargin, int64_t *bad_index, svt_arith_result **res,
					    int64_t *out_nnz)
{
	return abi_status([&] {
		int rt = 0;
		return sweep_begin_impl("svt_Compare_SVT_vector_begin", ARI_RULE_COMPARE, x, op, stats, stats_len, stats_Rtype, margin, nmargin,
					bad_index, res, &rt, out_nnz, NULL);
	});
}
extern "C" int svt_pminmax_SVT_vector_begin(const svt_view *x, int op, const void *stats, int64_t stats_len, int stats_Rtype,
					    const int *margin, int nmargin, int64_t *bad_index, svt_arith_result **res,
					    int *out_Rtype, int64_t *out_nnz)
{
	return abi_status([&] {
		return sweep_begin_impl("svt_pminmax_SVT_vector_begin", ARI_RULE_PMINMAX, x, op, stats, stats_len, stats_Rtype, margin, nmargin,
					bad_index, res, out_Rtype, out_nnz, NULL);
	});
}

// x[i, j, ...] <- value on host operands (.subassign_SVT_by_Nindex, C_subassign_SVT_with_short_Rvector): the subscripts
// are checked and those of dims 2..N expanded into the leaf list here, on the host, before anything is uploaded; the
// composition is SubassignCall::compose() on the first device, the result stays there until svt_Arith_SVT_end.
static int subassign_begin_impl(const char *who, const svt_view *x, const int *const *index, const int64_t *index_len,
				const void *vals, int64_t nvals, int v_Rtype, const svt_view *v, bool svt_form, svt_arith_result **res,
				int *out_Rtype, int64_t *out_nnz)
{
	if (res == NULL || out_Rtype == NULL || out_nnz == NULL)
		return svt_set_error("%s: 'res', 'out_Rtype' and 'out_nnz' are needed", who);
	*res = NULL;
	if (svt_form && v == NULL)
		return svt_set_error("%s: the value operand is needed", who);
	if (ensure_init() || check_view(x) || (svt_form && check_view(v)))
		return -1;
	if (x->na_background || (svt_form && v->na_background))
		return svt_set_unsupported("%s: NaArray operands are not supported here", who);
	if (!svt_form && (nvals < 1 || vals == NULL))
		return svt_set_error("replacement has length zero");
	const int ndim = x->ndim;
	std::vector<std::vector<int32_t>> sub((size_t) ndim);
	std::vector<int64_t> len((size_t) ndim);            // the selection's extent along every dimension
	bool whole_leaves = true;
	for (int a = 0; a < ndim; a++) {
		const int *idx = index != NULL ? index[a] : NULL;
		len[(size_t) a] = x->dim[a];
		if (idx == NULL) continue;
		const int64_t n = index_len != NULL ? index_len[a] : -1;
		if (n < 0) return svt_set_error("%s: a subscript needs its length", who);
		sub[(size_t) a].resize((size_t) n);
		for (int64_t k = 0; k < n; k++) {
			if (idx[k] == NA_INT || idx[k] < 1 || idx[k] > x->dim[a])
				return svt_set_error("subscript contains out-of-bound indices or NAs");
			sub[(size_t) a][(size_t) k] = idx[k] - 1;
		}
		len[(size_t) a] = n;
		if (a > 0) whole_leaves = false;
	}
	if (svt_form) {
		bool same = v->ndim == ndim;
		for (int a = 0; same && a < ndim; a++) same = v->dim[a] == len[(size_t) a];
		if (!same) return svt_set_error("the selection and supplied value must have the same dimensions");
	}
	// the selected leaves, the outermost dimension slowest -- the order of the leaves of a value of the selection's dims
	std::vector<int32_t> leaves;
	int64_t nleaves_sel = -1;
	if (!whole_leaves) {
		nleaves_sel = 1;
		for (int a = 1; a < ndim; a++) {
			if (len[(size_t) a] > 0 && nleaves_sel > 0x7FFFFFFELL / len[(size_t) a])
				return svt_set_error("%s: the subscripts select more than 2^31 - 2 leaves", who);
			nleaves_sel *= len[(size_t) a];
		}
		leaves.resize((size_t) nleaves_sel);
		for (int64_t q = 0; q < nleaves_sel; q++) {
			int64_t rest = q, leaf = 0, stride = 1;
			for (int a = 1; a < ndim; a++) {
				const int64_t k = rest % len[(size_t) a];
				rest /= len[(size_t) a];
				leaf += stride * (index[a] != NULL ? sub[(size_t) a][(size_t) k] : k);
				stride *= x->dim[a];
			}
			leaves[(size_t) q] = (int32_t) leaf;
		}
	}
	const bool whole_rows = index == NULL || index[0] == NULL;
	CscGuard A(x);
	if (A.h == NULL) return -1;
	std::optional<CscGuard> V;
	if (svt_form) {
		V.emplace(v);
		if (V->h == NULL) return -1;
	}
	DevBuf dr, dl, dv;
	if ((!whole_rows && !sub[0].empty() && dr.upload(sub[0].data(), sub[0].size() * 4)) ||
	    (!leaves.empty() && dl.upload(leaves.data(), leaves.size() * 4)) ||
	    (!svt_form && dv.upload(vals, (size_t) nvals * elt_size(v_Rtype))))
		return -1;
	SubassignCall c = { who };
	return result_begin(who, 0, 0, A.h->nrow, A.h->ncol,
			    [&](const ResultDest &to, int *rt) {
				    return c.plan(A.h->nrow, A.h->ncol, dr.as<int32_t>(), whole_rows ? -1 : len[0], dl.as<int32_t>(), nleaves_sel,
						  dv.as<char>(), nvals, v_Rtype, svt_form ? V->h : NULL, svt_form) ||
					   c.compose(A.h, to, rt, NULL);
			    },
			    NULL, res, out_Rtype, out_nnz, NULL);
}
extern "C" int svt_subassign_SVT_vector_begin(const svt_view *x, const int *const *index, const int64_t *index_len, const void *vals,
					      int64_t nvals, int v_Rtype, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz)
{
	return abi_status([&] {
		if (!logical_family_type(v_Rtype))
			return svt_set_error("svt_subassign_SVT_vector_begin: the value must be of type \"logical\", \"integer\" or \"double\"");
		return subassign_begin_impl("svt_subassign_SVT_vector_begin", x, index, index_len, vals, nvals, v_Rtype, NULL, false, res,
					    out_Rtype, out_nnz);
	});
}
extern "C" int svt_subassign_SVT_SVT_begin(const svt_view *x, const int *const *index, const int64_t *index_len, const svt_view *v,
					   svt_arith_result **res, int *out_Rtype, int64_t *out_nnz)
{
	return abi_status([&] {
		return subassign_begin_impl("svt_subassign_SVT_SVT_begin", x, index, index_len, NULL, 0, 0, v, true, res, out_Rtype, out_nnz);
	});
}

// x[Lindex], x[Mindex] and their subassignments on host operands (C_subset_SVT_by_Lindex / _by_Mindex,
// C_subassign_SVT_by_Lindex / _by_Mindex): the index is checked and brought to the 0-based cell numbers of the device
// layout here, on the host, before anything is uploaded -- an M-index becomes an L-index on the way, so one device path
// serves both.  First device of the list; not sharded.
static int view_ncells(const svt_view *x, int64_t *ncells)
{
	int64_t n = 1;
	for (int a = 0; a < x->ndim; a++) {
		if (x->dim[a] != 0 && n > INT64_MAX / x->dim[a])
			return svt_set_error("the array has more than 2^63 - 1 cells");
		n *= x->dim[a];
	}
	*ncells = n;
	return 0;
}
static int lindex_cells(const int64_t *lindex, int64_t K, int64_t ncells, bool na_ok, std::vector<int64_t> &out)
{
	if (K < 0 || (K > 0 && lindex == NULL))
		return svt_set_error("invalid linear index (L-index)");
	out.resize((size_t) K);
	for (int64_t k = 0; k < K; k++) {
		const int64_t v = lindex[k];
		if (v == INT64_MIN) {
			if (!na_ok) return svt_set_error("linear index (L-index) contains NAs");
			out[(size_t) k] = INT64_MIN;
			continue;
		}
		if (v < 1 || v > ncells)
			return svt_set_error("linear index (L-index) contains out-of-bound indices");
		out[(size_t) k] = v - 1;
	}
	return 0;
}
static int mindex_cells(const int *mindex, int64_t K, const svt_view *x, std::vector<int64_t> &out)
{
	if (K < 0 || (K > 0 && mindex == NULL))
		return svt_set_error("matrix subscript (M-index) must be a numeric matrix");
	out.resize((size_t) K);
	for (int64_t k = 0; k < K; k++) {
		int64_t cell = 0, stride = 1;
		for (int a = 0; a < x->ndim; a++) {
			const int m = mindex[k + (int64_t) a * K];
			if (m == NA_INT)
				return svt_set_error("matrix subscript (M-index) contains NAs");
			if (m < 1 || m > x->dim[a])
				return svt_set_error("matrix subscript (M-index) contains out-of-bound indices");
			cell += (int64_t) (m - 1) * stride;
			stride *= x->dim[a];
		}
		out[(size_t) k] = cell;
	}
	return 0;
}

static int subset_by_cells(const char *who, const svt_view *x, const std::vector<int64_t> &cells, void *out)
{
	const int64_t K = (int64_t) cells.size();
	if (!logical_family_type(x->Rtype))
		return svt_set_unsupported("%s: operands of type \"logical\", \"integer\" or \"double\" only", who);
	if (K == 0)
		return 0;
	if (out == NULL)
		return svt_set_error("%s: 'out' is needed", who);
	CscGuard A(x);
	if (A.h == NULL) return -1;
	DevBuf di, dout;
	DevFlag bad;
	if (di.upload(cells.data(), (size_t) K * 8) || dout.alloc((size_t) K * elt_size(x->Rtype)) || bad.init())
		return -1;
	LindexCall c = { who };
	if (c.plan(A.h->nrow, A.h->ncol, di.p, K, 0, NULL) || c.gather(A.h, dout.p, bad.ptr(), NULL))
		return -1;
	HIP_TRY(hipStreamSynchronize(0));
	int raised = 0;
	if (bad.read(&raised))
		return -1;
	if (raised)
		return svt_set_error("%s: the device refused an index or the operand's pointers", who);
	return staged_download(out, dout.p, (size_t) K * elt_size(x->Rtype));
}
extern "C" int svt_subset_SVT_by_Lindex(const svt_view *x, const int64_t *lindex, int64_t K, void *out)
{
	return abi_status([&] {
		int64_t ncells = 0;
		std::vector<int64_t> cells;
		if (ensure_init() || check_view(x) || view_ncells(x, &ncells) || lindex_cells(lindex, K, ncells, true, cells))
			return -1;
		return subset_by_cells("svt_subset_SVT_by_Lindex", x, cells, out);
	});
}
extern "C" int svt_subset_SVT_by_Mindex(const svt_view *x, const int *mindex, int64_t K, void *out)
{
	return abi_status([&] {
		int64_t ncells = 0;
		std::vector<int64_t> cells;
		if (ensure_init() || check_view(x) || view_ncells(x, &ncells) || mindex_cells(mindex, K, x, cells))
			return -1;
		return subset_by_cells("svt_subset_SVT_by_Mindex", x, cells, out);
	});
}

static int subassign_by_cells(const char *who, const svt_view *x, const std::vector<int64_t> &cells, const void *vals, int64_t nvals,
			      int v_Rtype, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz)
{
	const int64_t K = (int64_t) cells.size();
	CscGuard A(x);
	if (A.h == NULL) return -1;
	DevBuf di, dv;
	if ((K > 0 && di.upload(cells.data(), (size_t) K * 8)) || dv.upload(vals, (size_t) nvals * elt_size(v_Rtype)))
		return -1;
	LindexCall c = { who };
	return result_begin(who, 0, 0, A.h->nrow, A.h->ncol,
			    [&](const ResultDest &to, int *rt) {
				    return c.plan(A.h->nrow, A.h->ncol, di.p, K, 0, NULL) || c.compose(A.h, dv.p, nvals, v_Rtype, to, rt, NULL);
			    },
			    NULL, res, out_Rtype, out_nnz, NULL);
}
// the checks both forms share, before the index is looked at
static int subassign_by_index_head(const char *who, const svt_view *x, const void *vals, int64_t nvals, int v_Rtype,
				   svt_arith_result **res, int *out_Rtype, int64_t *out_nnz)
{
	if (res == NULL || out_Rtype == NULL || out_nnz == NULL)
		return svt_set_error("%s: 'res', 'out_Rtype' and 'out_nnz' are needed", who);
	*res = NULL;
	if (ensure_init() || check_view(x))
		return -1;
	if (!logical_family_type(v_Rtype))
		return svt_set_error("%s: the value must be of type \"logical\", \"integer\" or \"double\"", who);
	if (!logical_family_type(x->Rtype))
		return svt_set_unsupported("%s: operands of type \"logical\", \"integer\" or \"double\" only", who);
	if (x->na_background)
		return svt_set_unsupported("%s: NaArray operands are not supported here", who);
	if (nvals < 1 || vals == NULL)
		return svt_set_error("replacement has length zero");
	return 0;
}
extern "C" int svt_subassign_SVT_by_Lindex_begin(const svt_view *x, const int64_t *lindex, int64_t K, const void *vals, int64_t nvals,
						 int v_Rtype, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz)
{
	const char *who = "svt_subassign_SVT_by_Lindex_begin";
	return abi_status([&] {
		int64_t ncells = 0;
		std::vector<int64_t> cells;
		if (const int rc = subassign_by_index_head(who, x, vals, nvals, v_Rtype, res, out_Rtype, out_nnz))
			return rc;
		if (view_ncells(x, &ncells) || lindex_cells(lindex, K, ncells, false, cells))
			return -1;
		return subassign_by_cells(who, x, cells, vals, nvals, v_Rtype, res, out_Rtype, out_nnz);
	});
}
extern "C" int svt_subassign_SVT_by_Mindex_begin(const svt_view *x, const int *mindex, int64_t K, const void *vals, int64_t nvals,
						 int v_Rtype, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz)
{
	const char *who = "svt_subassign_SVT_by_Mindex_begin";
	return abi_status([&] {
		int64_t ncells = 0;
		std::vector<int64_t> cells;
		if (const int rc = subassign_by_index_head(who, x, vals, nvals, v_Rtype, res, out_Rtype, out_nnz))
			return rc;
		if (view_ncells(x, &ncells) || mindex_cells(mindex, K, x, cells))
			return -1;
		return subassign_by_cells(who, x, cells, vals, nvals, v_Rtype, res, out_Rtype, out_nnz);
	});
}

// abind on host operands (C_abind_SVT_SparseArray_objects): `along` and the dims are checked here, before anything is
// uploaded; the objects go up through the resident cache, AbindCall::compose() runs on the first device, the result
// stays there until svt_Arith_SVT_end.
static int abind_SVT_begin_impl(const svt_view *const *objs, int nobj, int along, int ans_Rtype, svt_arith_result **res,
				int64_t *out_nnz)
{
	const char *who = "svt_abind_SVT_begin";
	if (res == NULL || out_nnz == NULL)
		return svt_set_error("%s: 'res' and 'out_nnz' are needed", who);
	*res = NULL;
	if (nobj < 1 || objs == NULL)
		return svt_set_error("'objects' cannot be an empty list");
	if (ensure_init())
		return -1;
	for (int n = 0; n < nobj; n++)
		if (check_view(objs[n]))
			return -1;
	const int ndim = objs[0]->ndim;
	if (along < 1 || along > ndim)
		return svt_set_error("'along' must be >= 1 and <= the number of dimensions of the objects to bind");
	for (int n = 1; n < nobj; n++) {
		if (objs[n]->ndim != ndim)
			return svt_set_error("all the objects to bind must have the same number of dimensions");
		for (int k = 0; k < ndim; k++)
			if (k != along - 1 && objs[n]->dim[k] != objs[0]->dim[k])
				return svt_set_error("all the objects to bind must have the same extent along dimension %d (they are "
						     "bound along dimension %d)", k + 1, along);
	}
	int64_t inner = 1;
	for (int k = 1; k < along - 1; k++) inner *= objs[0]->dim[k];
	std::vector<int64_t> ext((size_t) nobj);
	for (int n = 0; n < nobj; n++) ext[(size_t) n] = objs[n]->dim[along - 1];
	std::vector<std::unique_ptr<CscGuard>> up;
	std::vector<const svt_dev_csc *> handles;
	for (int n = 0; n < nobj; n++) {
		up.emplace_back(new CscGuard(objs[n]));
		if (up.back()->h == NULL) return -1;
		handles.push_back(up.back()->h);
	}
	AbindCall c = { who };
	if (c.plan(handles.data(), nobj, inner, along == 1 ? NULL : ext.data(), ans_Rtype))
		return -1;
	return result_begin(who, ans_Rtype, c.na_background, c.out_nrow, c.a.out_nleaves,
			    [&](const ResultDest &to, int *) { return c.compose(to, NULL); }, NULL, res, NULL, out_nnz, NULL);
}
extern "C" int svt_abind_SVT_begin(const svt_view *const *objs, int nobj, int along, int ans_Rtype, svt_arith_result **res,
				   int64_t *out_nnz)
{
	return abi_status([&] { return abind_SVT_begin_impl(objs, nobj, along, ans_Rtype, res, out_nnz); });
}
// poissonSparseArray() and simple_rpois() for a host caller: nothing goes up; PoissonCall::compose() runs on the first
// device and the result stays there until svt_Arith_SVT_end, the vector of simple_rpois comes down at once.
extern "C" int svt_poissonSparseArray_begin(int64_t nrow, int64_t nleaves, double lambda, int64_t seed, svt_arith_result **res,
					    int64_t *out_nnz)
{
	const char *who = "svt_poissonSparseArray_begin";
	return abi_status([&] {
		if (res == NULL || out_nnz == NULL)
			return svt_set_error("%s: 'res' and 'out_nnz' are needed", who);
		*res = NULL;
		PoissonCall c = { who };
		if (c.plan(lambda, seed, nrow, 0, nleaves) || ensure_init())
			return -1;
		return result_begin(who, SVT_INTSXP, 0, nrow, nleaves, [&](const ResultDest &to, int *) { return c.compose(to, NULL); },
				    NULL, res, NULL, out_nnz, NULL);
	});
}
extern "C" int svt_simple_rpois(int64_t n, double lambda, int64_t seed, int32_t *out)
{
	const char *who = "svt_simple_rpois";
	return abi_status([&] {
		svt_poisson_table t;
		if (n < 0)
			return svt_set_error("'n' cannot be negative");
		if (poisson_table(who, lambda, &t))
			return -1;
		if (n == 0)
			return 0;
		if (out == NULL)
			return svt_set_error("%s: 'out' is NULL", who);
		DevBuf d;
		if (ensure_init() || d.alloc((size_t) n * 4) || launch_rpois(t, (uint64_t) seed, 0, n, (int32_t *) d.p, NULL))
			return -1;
		return staged_download(out, d.p, (size_t) n * 4);
	});
}

extern "C" int svt_Arith_SVT_end(svt_arith_result *res, int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val)
{
	return abi_status([&] {
		if (res == NULL) return 0;
		const int rc = result_end("svt_Arith_SVT_end", res->h, out_col_ptr, out_row_idx, out_val);
		free(res);
		return rc;
	});
}

// x %*% y over the device list: shard s takes the rows [r0, r1) of x, transposes them and multiplies them with the
// whole of y (replicated); its rows of the result go straight into `out` (a 2-d copy, ld = nrow).  No collective.
static int matmul_SVT_mat_sharded(const svt_view *x, const void *y, int y_nrow, int y_ncol, int y_Rtype, double *out)
{
	if (check_leaves(x))
		return -1;
	const std::vector<int> devs = g_devices;
	const int N = (int) devs.size();
	const int64_t nrow = x->dim[0], K = y_ncol;
	const size_t y_elems = (size_t) y_nrow * y_ncol;
	return run_shards(devs, [&](int s) -> int {
		int64_t r0, r1;
		shard_rows(nrow, s, N, &r0, &r1);
		const int64_t rs = r1 - r0;
		if (rs == 0) return 0;
		CscGuard A(row_block_upload(x, r0, r1));
		if (A.h == NULL) return -1;
		const OwnedCsc T = transposed_for(A);
		if (T.t == NULL) return -1;
		A.drop();
		auto put_y = [&](void *d) { return staged_copy(d, y, y_elems * elt_size(y_Rtype)); };
		DevBuf O;
		if (O.alloc((size_t) rs * K * 8) || O.zero() ||
		    dense_product(T.t, K, y_Rtype, y_elems, put_y, y_nrow, 0, O.as<double>(), 1, rs))
			return -1;
		HIP_TRY(hipMemcpy2D(out + r0, (size_t) nrow * 8, O.p, (size_t) rs * 8, (size_t) rs * 8, (size_t) K,
				    hipMemcpyDeviceToHost));
		return 0;
	});
}

// x %*% y, y an ordinary matrix: the R method (R/SparseMatrix-mult.R:195-215) is
// .crossprod2_SparseMatrix_matrix(t(x), y), i.e. C_transpose_2D_SVT on the host
// followed by C_crossprod2_SVT_mat.  Here the transposition happens on the device,
// between the upload and the product (no second marshalling of a 1e8-nonzero tree).
static int matmul_SVT_mat_impl(const svt_view *x, const void *y, int y_nrow,
				  int y_ncol, int y_Rtype, double *out)
{
	if (ensure_init() || check_mult_view(x, "input objects"))
		return -1;
	const int out_nrow = x->dim[0], in_nrow = x->dim[1];
	if (in_nrow != y_nrow)
		return svt_set_error("input objects are non-conformable");
	if (y_Rtype == SVT_LGLSXP) y_Rtype = SVT_INTSXP;
	if (!mult_types_ok(x->Rtype, y_Rtype))
		return svt_set_error("SparseArray internal error in "
				     "C_crossprod2_SVT_mat():\n"
				     "    'x_Rtype != TYPEOF(y)' not supported yet");
	const size_t out_n = (size_t) out_nrow * y_ncol;
	memset(out, 0, out_n * sizeof(double));
	if (x->svt_is_null || out_n == 0)
		return 0;
	if (shard_applies(x))
		return matmul_SVT_mat_sharded(x, y, y_nrow, y_ncol, y_Rtype, out);
	CscGuard A(x);
	if (A.h == NULL) return -1;
	const OwnedCsc T = transposed_for(A);
	if (T.t == NULL) return -1;
	A.drop();                           // a one-call operand: its untransposed copy can go now
	const size_t y_elems = (size_t) y_nrow * y_ncol;
	auto put_y = [&](void *d) { return staged_copy(d, y, y_elems * elt_size(y_Rtype)); };
	DevBuf O;
	if (O.alloc(out_n * 8) || O.zero() ||
	    dense_product(T.t, y_ncol, y_Rtype, y_elems, put_y, y_nrow, 0, O.as<double>(), 1, out_nrow))
		return -1;
	return staged_download(out, O.p, out_n * 8);
}
extern "C" int svt_matmul_SVT_mat(const svt_view *x, const void *y, int y_nrow,
				  int y_ncol, int y_Rtype, double *out)
{
	return abi_status([&] { return matmul_SVT_mat_impl(x, y, y_nrow, y_ncol, y_Rtype, out); });
}

// x %*% y, both SVT_SparseMatrix: .crossprod2_SparseMatrix_SparseMatrix(t(x), y) with
// the transposition on the device; operand to expand chosen as C_crossprod2_SVT_SVT
// does (src/SparseMatrix_mult.c:1075-1097; nzcount(t(x)) == nzcount(x)).
static int matmul_SVT_SVT_impl(const svt_view *x, const svt_view *y, double *out)
{
	if (ensure_init() || check_mult_view(x, "input objects") ||
	    check_mult_view(y, "input objects"))
		return -1;
	if (x->dim[1] != y->dim[0])
		return svt_set_error("input SVT_SparseMatrix objects are non-conformable");
	if (x->Rtype != y->Rtype)
		return svt_set_error("input SVT_SparseMatrix objects must have the "
				     "same type() for now");
	const int out_nrow = x->dim[0], out_ncol = y->dim[1];
	const size_t out_n = (size_t) out_nrow * out_ncol;
	memset(out, 0, out_n * sizeof(double));
	if (out_n == 0)
		return 0;
	CscGuard X(x);
	if (X.h == NULL) return -1;
	CscGuard Y(y);                                  // (one upload of y for both routes)
	if (Y.h == NULL) return -1;
	// y much sparser than a dense matrix (<= 5 % filled), finite operands: the row-panel kernel on x itself,
	// no transposition, no dense operand (kernels_spmm.hip); a non-finite value or an NA anywhere sends the
	// product down the reference's route below.  The kernel adds the products of a cell in the order its lane
	// groups get to them: doubles can differ in the last bits from run to run and from the reference's
	// ascending-index order (inside the 1e-6 the contract allows; integer operands are exact below 2^53).
	if (view_nzcount(y) * 20 <= (int64_t) y->dim[0] * y->dim[1]) {
		DevBuf Os, Ws;
		int bad = 1;
		if (Os.alloc(out_n * 8) || Ws.alloc(svt_dev_matmul_csc_csc_ws_bytes(X.h)))
			return -1;
		const int rc_s = svt_dev_matmul_csc_csc(X.h, Y.h, Os.as<double>(), out_nrow, Ws.p, Ws.bytes, NULL, 0);
		if (rc_s < 0)
			return -1;
		if (rc_s == 0) {
			HIP_TRY(hipMemcpy(&bad, (char *) Ws.p + 4, 4, hipMemcpyDeviceToHost));
			if (!bad)
				return staged_download(out, Os.p, out_n * 8) ? -1 : 0;
		} else
			g_unsupported = 0;                // (a shape the row-panel kernel refuses: the route below)
	}
	const OwnedCsc T = transposed_for(X);
	if (T.t == NULL) return -1;
	X.drop();
	return sparse_then_dense(out, out_n, [](double *) { return 1; },
				 [&](double *O) { return dense_buffer_route(T.t, Y.h, false, O); });
}
extern "C" int svt_matmul_SVT_SVT(const svt_view *x, const svt_view *y, double *out)
{
	return abi_status([&] { return matmul_SVT_SVT_impl(x, y, out); });
}

// x %*% y, crossprod(x, y) (tr_x) and tcrossprod(x, y) (tr_y) of two SVT_SparseMatrix objects with a SPARSE result
// (kernels_spgemm.hip): the operands go up through the resident cache, are transposed on the device where asked,
// SpgemmCall::compose() runs on the first device and the result stays there until svt_Arith_SVT_end.
static int matmul_SVT_SVT_sparse_begin_impl(const svt_view *x, const svt_view *y, int tr_x, int tr_y, svt_arith_result **res,
					    int64_t *out_nnz, int *not_finite)
{
	const char *who = "svt_matmul_SVT_SVT_sparse_begin";
	if (res == NULL || out_nnz == NULL || not_finite == NULL)
		return svt_set_error("%s: 'res', 'out_nnz' and 'not_finite' are needed", who);
	*res = NULL;
	if (ensure_init() || check_mult_view(x, "input objects") || check_mult_view(y, "input objects"))
		return -1;
	if (x->dim[tr_x ? 0 : 1] != y->dim[tr_y ? 1 : 0])
		return svt_set_error("non-conformable arguments");
	CscGuard X(x);
	if (X.h == NULL) return -1;
	CscGuard Y(y);
	if (Y.h == NULL) return -1;
	const OwnedCsc Tx = tr_x ? transposed_for(X) : OwnedCsc(NULL, false);
	const OwnedCsc Ty = tr_y ? transposed_for(Y) : OwnedCsc(NULL, false);
	const svt_dev_csc *A = tr_x ? Tx.t : X.h, *B = tr_y ? Ty.t : Y.h;
	if (A == NULL || B == NULL) return -1;
	DevFlag nf;
	if (nf.init()) return -1;
	const SpgemmCall c = { who, A, B };
	return result_begin(who, SVT_REALSXP, 0, A->nrow, B->ncol,
			    [&](const ResultDest &to, int *) { return c.compose(to, nf.ptr(), NULL); }, &nf, res, NULL, out_nnz, not_finite);
}
extern "C" int svt_matmul_SVT_SVT_sparse_begin(const svt_view *x, const svt_view *y, int tr_x, int tr_y, svt_arith_result **res,
					       int64_t *out_nnz, int *not_finite)
{
	return abi_status([&] { return matmul_SVT_SVT_sparse_begin_impl(x, y, tr_x, tr_y, res, out_nnz, not_finite); });
}

// C_crossprod1_SVT, src/SparseMatrix_mult.c:1104-1140
static int crossprod1_SVT_impl(const svt_view *x, double *out)
{
	if (ensure_init() || check_mult_view(x, "'x'"))
		return -1;
	const int n = x->dim[1];
	const size_t out_n = (size_t) n * n;
	memset(out, 0, out_n * sizeof(double));
	if (x->svt_is_null || out_n == 0)      // :880-881
		return 0;
	CscGuard X(x);
	if (X.h == NULL) return -1;
	const double dense_ops = (double) X.h->nnz * (double) n;
	const bool pays = sparse_route_pays(X.h->nnz, X.h->nnz, x->dim[0], dense_ops, true);
	return sparse_then_dense(out, out_n,
		[&](double *O) { return pays ? dev_crossprod_sparse(X, X.h, true, O, n, dense_ops) : 1; },
		[&](double *O) { return dense_buffer_route(X.h, X.h, true, O); });
}
extern "C" int svt_crossprod1_SVT(const svt_view *x, double *out)
{
	return abi_status([&] { return crossprod1_SVT_impl(x, out); });
}

// tcrossprod(x) = crossprod(t(x)) and tcrossprod(x, y) = crossprod(t(x), t(y)) of SVT_SparseMatrix objects in one call.
// The R methods (R/SparseMatrix-mult.R:165-193) take t() on the host first (C_transpose_2D_SVT: the transposed tree comes
// back as R leaves and is marshalled again by C_crossprod1_SVT / C_crossprod2_SVT_SVT).  Here the operands are uploaded as
// they are and transposed on the device; the sparse-aware kernel needs the ROWS of its first operand t(x), i.e. x itself --
// no transposition at all on that side.  Checks, messages and the route choice are those of the crossprod entry points
// applied to the transposed operands; a non-finite value or an NA anywhere takes the dense-buffer route (the reference's
// dirty-leaf rules).  out: nrow(x) x nrow(x) / nrow(x) x nrow(y) doubles, column-major.
static int tcrossprod1_SVT_impl(const svt_view *x, double *out)
{
	if (ensure_init() || check_mult_view(x, "'x'"))
		return -1;
	const int n = x->dim[0];
	const size_t out_n = (size_t) n * n;
	memset(out, 0, out_n * sizeof(double));
	if (x->svt_is_null || out_n == 0 || x->dim[1] == 0)      // (t(x)@SVT is NULL: src/SparseMatrix_mult.c:880-881)
		return 0;
	CscGuard X(x);
	if (X.h == NULL) return -1;
	const OwnedCsc TM = transposed_for(X);                  // M = t(x): ncol(x) rows, nrow(x) leaves
	const svt_dev_csc *M = TM.t;
	if (M == NULL) return -1;
	const double dense_ops = (double) M->nnz * (double) n;
	const bool pays = sparse_route_pays(M->nnz, M->nnz, M->nrow, dense_ops, true);
	return sparse_then_dense(out, out_n,
		[&](double *O) { return pays ? dev_crossprod_sparse_on(X.h, M, true, O, n, dense_ops) : 1; },   // t(M) is x
		[&](double *O) { return dense_buffer_route(M, M, true, O); });
}
extern "C" int svt_tcrossprod1_SVT(const svt_view *x, double *out)
{
	return abi_status([&] { return tcrossprod1_SVT_impl(x, out); });
}

static int tcrossprod2_SVT_SVT_impl(const svt_view *x, const svt_view *y, double *out)
{
	if (ensure_init() || check_mult_view(x, "input objects") ||
	    check_mult_view(y, "input objects"))
		return -1;
	if (x->dim[1] != y->dim[1])
		return svt_set_error("input SVT_SparseMatrix objects are non-conformable");
	if (x->Rtype != y->Rtype)
		return svt_set_error("input SVT_SparseMatrix objects must have the "
				     "same type() for now");
	const int out_nrow = x->dim[0], out_ncol = y->dim[0];
	const size_t out_n = (size_t) out_nrow * out_ncol;
	memset(out, 0, out_n * sizeof(double));
	if (out_n == 0)
		return 0;
	const int64_t Lpp_nops = view_nzcount(y) * out_nrow;
	const int64_t Rpp_nops = view_nzcount(x) * out_ncol;
	const double dense_ops = (double) (Lpp_nops < Rpp_nops ? Lpp_nops : Rpp_nops);
	CscGuard X(x), Y(y);
	if (X.h == NULL || Y.h == NULL) return -1;
	const OwnedCsc Ty = transposed_for(Y);
	if (Ty.t == NULL) return -1;
	const bool pays = !x->svt_is_null && !y->svt_is_null && x->dim[1] > 0 &&
			  sparse_route_pays(X.h->nnz, Y.h->nnz, x->dim[1], dense_ops, false);
	return sparse_then_dense(out, out_n,
		[&](double *O) { return pays ? dev_crossprod_sparse_on(X.h, Ty.t, false, O, out_nrow, dense_ops) : 1; },   // t(t(x)) is x
		[&](double *O) {
			const OwnedCsc Tx = transposed_for(X);      // (only now: the sparse-aware route needs none)
			return Tx.t == NULL ? -1 : dense_buffer_route(Tx.t, Ty.t, false, O);
		});
}
extern "C" int svt_tcrossprod2_SVT_SVT(const svt_view *x, const svt_view *y, double *out)
{
	return abi_status([&] { return tcrossprod2_SVT_SVT_impl(x, y, out); });
}

// ==================================================================================
// Host level: stats
// ==================================================================================
static int run_colstats(const svt_dev_csc *A, int opcode, int na_rm, double center,
			int64_t inner, void *out_host, int out_Rtype, int *warn)
{
	const size_t out_bytes = (size_t) (A->ncol / inner) * elt_size(out_Rtype);
	DevBuf O;
	DevFlag W;
	if (O.alloc(out_bytes) || W.init())
		return -1;
	if (svt_dev_colstats(A, opcode, na_rm, center, inner, O.p, W.ptr(), 0))
		return -1;
	HIP_TRY(hipMemcpy(out_host, O.p, out_bytes, hipMemcpyDeviceToHost));
	return W.read(warn);
}

// A leaf-range statistic over the device list: shard s takes the units [u0, u1) -- leaves [u0 * unit, u1 * unit),
// ranges balanced by nonzeros (shard_cuts) -- and runs fn(A, u0, flag) on their upload; fn writes its slice of the
// result.  *flag gets the OR of the shards' flags (warn, overflow).
template <class F> static int run_leaf_shards(const svt_view *x, int64_t unit, int64_t nunits, int *flag, F fn)
{
	const std::vector<int> devs = g_devices;
	const int N = (int) devs.size();
	const std::vector<int64_t> cut = shard_cuts(x, unit, nunits, N);
	std::vector<int> f((size_t) N, 0);
	const int rc = run_shards(devs, [&](int s) -> int {
		const int64_t u0 = cut[(size_t) s], u1 = cut[(size_t) s + 1];
		if (u1 <= u0) return 0;
		SubView sv;
		col_block_view(x, u0 * unit, u1 * unit, sv);
		CscGuard A(svt_upload(&sv.v));
		if (A.h == NULL) return -1;
		return fn(A.h, u0, &f[(size_t) s]);
	});
	for (int s = 0; s < N; s++)
		if (f[(size_t) s]) *flag = 1;
	return rc;
}

// C_colStats_SVT, src/SparseArray_matrixStats.c:234-284
static int colStats_SVT_impl(const svt_view *x, int opcode, int na_rm, double center,
				int dims, void *out, int *warn)
{
	*warn = 0;
	if (ensure_init() || check_view(x) || check_stat_op(opcode, x->Rtype))
		return -1;
	if (dims < 1 || dims > x->ndim)
		return svt_set_error("'dims' must be >= 1 and <= %d", x->ndim);
	if (device_op_supported(opcode))
		return -1;
	int64_t inner, nout;
	split_dims(x, dims, &inner, &nout);
	if (nout == 0)
		return 0;
	const int out_Rtype = svt_colStats_out_Rtype(opcode, x->Rtype);
	if (inner > 0 && shard_applies(x)) {      // shard s: output cells [g0, ...)
		const size_t osz = elt_size(out_Rtype);
		return run_leaf_shards(x, inner, nout, warn, [&](const svt_dev_csc *A, int64_t g0, int *w) {
			return run_colstats(A, opcode, na_rm, center, inner, (char *) out + (size_t) g0 * osz, out_Rtype, w);
		});
	}
	CscGuard A(x);
	if (A.h == NULL) return -1;
	if (inner > 0)
		return run_colstats(A.h, opcode, na_rm, center, inner, out, out_Rtype, warn);
	DevBuf P;       // zero-extent inner dims: every result summarizes an empty vector
	const svt_dev_csc E = empty_segments(A.h, nout, P);
	return E.col_ptr ? run_colstats(&E, opcode, na_rm, center, 1, out, out_Rtype, warn) : -1;
}
extern "C" int svt_colStats_SVT(const svt_view *x, int opcode, int na_rm, double center,
				int dims, void *out, int *warn)
{
	return abi_status([&] { return colStats_SVT_impl(x, opcode, na_rm, center, dims, out, warn); });
}

// colMedians(): .colMedians_SVT_SparseMatrix, R/SparseArray-matrixStats.R:761-784 (pure R in the
// reference, with a TODO asking for a .Call version).  out: ncol(x) doubles.
// colQuantiles(x, probs, na.rm, type = 7): no method in the reference (R/SparseArray-matrixStats.R:5-12); the rule is
// base R's quantile.default type 7 (kernels_median.hip).  out: ncol(x) * nprobs doubles, column-major.
// colMads(x, center, constant, na.rm): no method in the reference either; stats::mad without low / high
// (kernels_median.hip).  vec: the centers, one per result, or NULL for the medians.  out: ncol(x) doubles.
static int order_stat_SVT(const svt_view *x, int what, const double *vec, int nprobs, double constant, int na_rm,
			  int by_row, double *out)
{
	const bool quant = what == ORDER_QUANTILES;
	const double *probs = vec;
	if (ColOperand::check(x, by_row, order_stat_names[what][0], order_stat_names[what][1]))
		return -1;
	if (quant) {
		if (nprobs < 0 || (nprobs > 0 && probs == NULL))
			return svt_set_error("invalid 'probs'");
		for (int q = 0; q < nprobs; q++)        // (before anything is uploaded; NaN fails both comparisons)
			if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
				return svt_set_error("'probs' outside [0,1]");
	}
	const int64_t nout = x->dim[by_row ? 0 : 1];
	if (nout == 0 || (quant && nprobs == 0))
		return 0;
	const ColOperand X(x, by_row);
	const svt_dev_csc *M = X.M;
	if (M == NULL) return -1;
	DevBuf P, O, W;
	const size_t out_bytes = (size_t) nout * (quant ? (size_t) nprobs : 1) * 8;
	const size_t vec_bytes = quant ? (size_t) nprobs * 8 : what == ORDER_MADS && vec ? (size_t) nout * 8 : 0;
	if ((vec_bytes && P.upload(vec, vec_bytes)) || O.alloc(out_bytes) || W.alloc(order_stat_ws_bytes(what, nout)))
		return -1;
	if (launch_order_stat(what, M->col_ptr, M->val, M->Rtype, M->nrow, nout, M->nnz, P.as<double>(), nprobs, constant,
			      na_rm, O.as<double>(), W.p, 0))
		return -1;
	HIP_TRY(hipDeviceSynchronize());
	return staged_download(out, O.p, out_bytes);
}

extern "C" int svt_colMedians_SVT(const svt_view *x, int na_rm, double *out)
{
	return abi_status([&] { return order_stat_SVT(x, ORDER_MEDIANS, NULL, 0, 0.0, na_rm, 0, out); });
}

extern "C" int svt_rowMedians_SVT(const svt_view *x, int na_rm, double *out)
{
	return abi_status([&] { return order_stat_SVT(x, ORDER_MEDIANS, NULL, 0, 0.0, na_rm, 1, out); });
}

extern "C" int svt_colQuantiles_SVT(const svt_view *x, const double *probs, int nprobs, int na_rm, double *out)
{
	return abi_status([&] { return order_stat_SVT(x, ORDER_QUANTILES, probs, nprobs, 0.0, na_rm, 0, out); });
}

extern "C" int svt_rowQuantiles_SVT(const svt_view *x, const double *probs, int nprobs, int na_rm, double *out)
{
	return abi_status([&] { return order_stat_SVT(x, ORDER_QUANTILES, probs, nprobs, 0.0, na_rm, 1, out); });
}

extern "C" int svt_colMads_SVT(const svt_view *x, const double *center, double constant, int na_rm, double *out)
{
	return abi_status([&] { return order_stat_SVT(x, ORDER_MADS, center, 0, constant, na_rm, 0, out); });
}

extern "C" int svt_rowMads_SVT(const svt_view *x, const double *center, double constant, int na_rm, double *out)
{
	return abi_status([&] { return order_stat_SVT(x, ORDER_MADS, center, 0, constant, na_rm, 1, out); });
}

// colRanks(x, ties.method, preserveShape) / rowRanks(x, ties.method): no method in the reference; the rule is
// matrixStats::colRanks (include/svt_hip.h).  The device answers in the compact form (kernels_ranks.hip: a rank per
// stored value, a rank per column for its zeros), which is expanded here: every cell of a column gets the zeros' rank,
// then the stored positions theirs.  M, the operand whose columns are ranked, is x or t(x); transposed != 0 fills
// out[j + i * ncol(M)], else out[i + j * nrow(M)].
template <typename R>
static void expand_ranks(const int64_t *cp, const int32_t *ri, const R *rank_nz, const R *zero_rank, int64_t mrow,
			 int64_t mcol, bool transposed, R *out)
{
	const size_t cells = (size_t) mrow * (size_t) mcol * sizeof(R);
	if (transposed) {
		// a row of the result is the zeros' ranks of all columns, then the stored values of the columns are scattered
		team_run(team_size(cells), [&](int t, int nt) {
			for (int64_t i = mrow * t / nt; i < mrow * (t + 1) / nt; i++)
				memcpy(out + i * mcol, zero_rank, (size_t) mcol * sizeof(R));
		});
		team_run(team_size(cells), [&](int t, int nt) {
			for (int64_t j = mcol * t / nt; j < mcol * (t + 1) / nt; j++)
				for (int64_t k = cp[j]; k < cp[j + 1]; k++)
					out[j + (int64_t) ri[k] * mcol] = rank_nz[k];
		});
		return;
	}
	team_run(team_size(cells), [&](int t, int nt) {
		for (int64_t j = mcol * t / nt; j < mcol * (t + 1) / nt; j++) {
			R *col = out + j * mrow;
			for (int64_t i = 0; i < mrow; i++) col[i] = zero_rank[j];
			for (int64_t k = cp[j]; k < cp[j + 1]; k++) col[ri[k]] = rank_nz[k];
		}
	});
}

static int ranks_SVT(const svt_view *x, int ties, int preserve_shape, int by_row, void *out)
{
	if (ColOperand::check(x, by_row, "colRanks", "rowRanks"))
		return -1;
	if (check_ties(ties))
		return -1;
	if (x->dim[0] == 0 || x->dim[1] == 0)
		return 0;                                       // zero extents: no cell to write
	const ColOperand X(x, by_row);
	const svt_dev_csc *M = X.M;
	if (M == NULL) return -1;
	const int64_t mrow = M->nrow, mcol = M->ncol, nnz = M->nnz;
	if (mcol > 0x7FFFFFFFLL)
		return svt_set_unsupported("colRanks: more than 2^31-1 columns");
	// the structure comes back for the expansion; the column lengths also say how much the long columns hold
	std::vector<int64_t> cp((size_t) mcol + 1);
	std::vector<int32_t> ri((size_t) nnz);
	HIP_TRY(hipMemcpy(cp.data(), M->col_ptr, cp.size() * 8, hipMemcpyDeviceToHost));
	if (nnz > 0 && staged_download(ri.data(), M->row_idx, (size_t) nnz * 4))
		return -1;
	int64_t long_nnz = 0;
	for (int64_t j = 0; j < mcol; j++)
		if (ranks_form(cp[(size_t) j + 1] - cp[(size_t) j]) == 2) long_nnz += cp[(size_t) j + 1] - cp[(size_t) j];
	if (long_nnz > 0xFFFFFFFFLL)
		return svt_set_unsupported("colRanks: 2^32 or more stored values in the columns sorted in the workspace");
	const size_t esz = ties == SVT_TIES_AVERAGE ? 8 : 4;
	const size_t wsb = ranks_ws_bytes(mcol, long_nnz);
	DevBuf RN, RZ, W;
	DevFlag F;
	if (RN.alloc((size_t) nnz * esz) || RZ.alloc((size_t) mcol * esz) || F.init() || W.alloc(wsb))
		return -1;
	if (launch_ranks(M->col_ptr, M->val, M->Rtype, mrow, mcol, nnz, ties, RN.p, RZ.p, F.ptr(), W.p, wsb, 0))
		return -1;
	HIP_TRY(hipDeviceSynchronize());
	int flag = 0;
	if (F.read(&flag)) return -1;
	if (flag)
		return svt_set_error("colRanks: the workspace did not hold the long columns");
	std::vector<char> rn((size_t) nnz * esz), rz((size_t) mcol * esz);
	if ((nnz > 0 && staged_download(rn.data(), RN.p, rn.size())) || staged_download(rz.data(), RZ.p, rz.size()))
		return -1;
	const bool transposed = by_row || !preserve_shape;
	if (esz == 8)
		expand_ranks<double>(cp.data(), ri.data(), (const double *) rn.data(), (const double *) rz.data(), mrow, mcol,
				     transposed, (double *) out);
	else
		expand_ranks<int32_t>(cp.data(), ri.data(), (const int32_t *) rn.data(), (const int32_t *) rz.data(), mrow, mcol,
				      transposed, (int32_t *) out);
	return 0;
}

extern "C" int svt_colRanks_SVT(const svt_view *x, int ties, int preserve_shape, void *out)
{
	return abi_status([&] { return ranks_SVT(x, ties, preserve_shape, 0, out); });
}

extern "C" int svt_rowRanks_SVT(const svt_view *x, int ties, void *out)
{
	return abi_status([&] { return ranks_SVT(x, ties, 0, 1, out); });
}

// C_summarize_SVT, src/SparseArray_summarization.c:112-142
static int summarize_SVT_impl(const svt_view *x, int opcode, int na_rm, double center,
				 double *out_d, int *out_i, int *out_Rtype, int *warn)
{
	*warn = 0;
	if (ensure_init() || check_view(x) || check_stat_op(opcode, x->Rtype))
		return -1;
	if (opcode == SVT_OP_SUM_X_X2 || opcode == SVT_OP_VAR2 || opcode == SVT_OP_SD2)
		return device_op_supported(opcode);
	const int rt = svt_colStats_out_Rtype(opcode, x->Rtype);
	*out_Rtype = rt;
	out_d[0] = out_d[1] = 0.0;
	out_i[0] = out_i[1] = 0;
	CscGuard A(x);
	if (A.h == NULL) return -1;
	svt_dev_csc V = *A.h;      // the whole array as one generalized column
	V.owned = 0;
	DevBuf P;
	if (V.ncol == 0) {         // some outer dim is 0: one empty segment
		V = empty_segments(A.h, 1, P);
		if (V.col_ptr == NULL) return -1;
	}
	const int64_t inner = V.ncol;
	const int ops[2] = { opcode == SVT_OP_RANGE ? SVT_OP_MIN : opcode, SVT_OP_MAX };
	const int nops = opcode == SVT_OP_RANGE ? 2 : 1;
	for (int t = 0; t < nops; t++) {
		double d = 0.0;
		int i = 0;
		void *dst = rt == SVT_REALSXP ? (void *) &d : (void *) &i;
		if (run_colstats(&V, ops[t], na_rm, center, inner, dst, rt, warn))
			return -1;
		out_d[t] = d;
		out_i[t] = i;
	}
	return 0;
}
extern "C" int svt_summarize_SVT(const svt_view *x, int opcode, int na_rm, double center,
				 double *out_d, int *out_i, int *out_Rtype, int *warn)
{
	return abi_status([&] { return summarize_SVT_impl(x, opcode, na_rm, center, out_d, out_i, out_Rtype, warn); });
}

// C_rowStats_SVT, src/SparseArray_matrixStats.c:1121-1205 (six_only: its six operations), and every row statistic
// the R API offers in one call (svt_rowStatsFull_SVT: thirteen).  The checks and the constant fill, one operand on the
// device (the resident cache applies), dev_rowstats_impl, one download.  Not sharded over the device list.
static int rowStats_SVT_impl(const svt_view *x, int opcode, int na_rm, const double *center, int dims, bool six_only,
			     void *out, int *warn)
{
	*warn = 0;
	if (ensure_init() || check_view(x) || check_stat_op(opcode, x->Rtype))
		return -1;
	if (dims < 1 || dims > x->ndim - 1)
		return svt_set_error("'dims' must be >= 1 and <= %d", x->ndim - 1);
	if (six_only && !rowstats_reference_op(opcode))
		return svt_set_error("SparseArray internal error in C_rowStats_SVT():\n"
				     "    operation not supported");
	if (check_rowstats_op(opcode, x->Rtype, x->na_background))       // (the NaArray rules, :639-642)
		return -1;
	const bool range = opcode == SVT_OP_RANGE;
	const int out_Rtype = svt_colStats_out_Rtype(opcode, x->Rtype);
	int64_t inner, nstrata;
	split_dims(x, dims, &inner, &nstrata);
	const int64_t out_len = inner * x->dim[0], nout = out_len * (range ? 2 : 1);
	if (out_len == 0)
		return 0;
	if ((opcode == SVT_OP_MIN || opcode == SVT_OP_MAX || range) && nstrata == 0) {
		// constant fill, :970-982 (range: the minima, then the maxima)
		for (int64_t i = 0; i < nout; i++) {
			if (out_Rtype == SVT_REALSXP)
				((double *) out)[i] = (range ? i < out_len : opcode == SVT_OP_MIN) ? INFINITY : -INFINITY;
			else
				((int *) out)[i] = NA_INT;
		}
		if (out_Rtype != SVT_REALSXP) *warn = 1;
		return 0;
	}
	// (what dev_rowstats_impl refuses, before the operand is uploaded)
	if (nstrata > 0xFFFFFFFFLL)
		return svt_set_unsupported("too many strata for the device coverage counters");
	if (inner > 65535 && x->na_background)
		return svt_set_unsupported("row statistics of NaArray objects: more than 65535 output columns");
	if (inner > 65535 && !rowstats_reference_op(opcode))
		return svt_set_unsupported("row statistics: this operation is not served with more than 65535 output columns");
	CscGuard A(x);
	if (A.h == NULL) return -1;
	const size_t out_bytes = (size_t) nout * elt_size(out_Rtype), ws_bytes = svt_dev_rowstats_ws_bytes_op(A.h, opcode, inner);
	DevBuf O, C, T;
	DevFlag W;
	if (O.alloc(out_bytes) || W.init() || T.alloc(ws_bytes))
		return -1;
	if (center != NULL && C.upload(center, (size_t) out_len * 8))
		return -1;
	if (dev_rowstats_impl(A.h, opcode, na_rm, center ? C.as<double>() : NULL, inner, O.p, W.ptr(), T.p, ws_bytes, 0))
		return -1;
	HIP_TRY(hipDeviceSynchronize());
	if (staged_download(out, O.p, out_bytes)) return -1;
	return W.read(warn);
}
extern "C" int svt_rowStats_SVT(const svt_view *x, int opcode, int na_rm,
				const double *center, int dims, void *out, int *warn)
{
	return abi_status([&] { return rowStats_SVT_impl(x, opcode, na_rm, center, dims, true, out, warn); });
}
extern "C" int svt_rowStatsFull_SVT(const svt_view *x, int opcode, int na_rm,
				    const double *center, int dims, void *out, int *warn)
{
	return abi_status([&] { return rowStats_SVT_impl(x, opcode, na_rm, center, dims, false, out, warn); });
}

// ==================================================================================
// Host level: rowsum / colsum
// ==================================================================================
static int check_group(const int *group, int n, int ngroup)   // rowsum_methods.c:15-37
{
	for (int i = 0; i < n; i++) {
		const int g = group[i];
		if (g == NA_INT) {
			if (ngroup < 1)
				return svt_set_error("'ngroup' must be >= 1 when 'group' "
						     "contains missing values");
		} else if (g < 1 || g > ngroup) {
			return svt_set_error("all non-NA values in 'group' must "
					     "be >= 1 and <= 'ngroup'");
		}
	}
	return 0;
}

static int groupsum_host(const svt_dev_csc *A, const int32_t *col_ptr32,
			 const int *group, int ngroup, int na_rm, bool colsum,
			 void *out, int *ovflow)
{
	const int64_t glen = colsum ? A->ncol : A->nrow;
	const int64_t out_len = colsum ? A->nrow * (int64_t) ngroup
				       : (int64_t) ngroup * A->ncol;
	if (out_len > 0x7FFFFFFFLL)   // safe_int_mult() guard, :296-301
		return svt_set_error("too many groups (matrix of sums will be too big)");
	const size_t osz = elt_size(A->Rtype);
	if (out_len == 0)
		return 0;
	DevBuf G, O, S;
	DevFlag W;
	if (G.upload(group, (size_t) glen * 4) || O.alloc((size_t) out_len * osz) ||
	    S.alloc(groupsum_scratch_bytes(A->Rtype, out_len)) || W.init())
		return -1;
	GroupSumArgs a = groupsum_args(A, col_ptr32, G.as<int>(), ngroup, na_rm, O.p);
	a.scratch = S.p; a.ovflow_flag = W.ptr();
	if (colsum ? launch_colsum(a, 0) : launch_rowsum(a, 0)) return -1;
	if (staged_download(out, O.p, (size_t) out_len * osz)) return -1;
	return W.read(ovflow);
}

static int xsum_SVT(const svt_view *x, const int *group, int ngroup, int na_rm,
		    bool colsum, void *out, int *ovflow)
{
	*ovflow = 0;
	if (ensure_init() || check_view(x))
		return -1;
	if (x->ndim != 2)
		return svt_set_error("input object must have 2 dimensions");
	if (x->na_background)      // rowsum()/colsum() have no NaArray methods (R/rowsum-methods.R)
		return svt_set_error("NaArray objects are not supported by this operation");
	if (x->Rtype != SVT_REALSXP && x->Rtype != SVT_INTSXP)
		return svt_set_error("rowsum() and colsum() do not support "
				     "SVT_SparseMatrix objects of this type at the moment");
	if (check_group(group, colsum ? x->dim[1] : x->dim[0], ngroup))
		return -1;
	if (!colsum && shard_applies(x)) {
		// shard s: the leaves [c0, c1); its ngroup x (c1 - c0) block of the column-major result is contiguous in `out`
		const int64_t ncol = x->dim[1];
		if ((int64_t) ngroup * ncol > 0x7FFFFFFFLL)   // safe_int_mult() guard, src/rowsum_methods.c:296-301
			return svt_set_error("too many groups (matrix of sums will be too big)");
		const size_t osz = elt_size(x->Rtype);
		return run_leaf_shards(x, 1, ncol, ovflow, [&](const svt_dev_csc *A, int64_t c0, int *ov) {
			return groupsum_host(A, NULL, group, ngroup, na_rm, false, (char *) out + (size_t) ngroup * c0 * osz, ov);
		});
	}
	CscGuard A(x);
	if (A.h == NULL) return -1;
	return groupsum_host(A.h, NULL, group, ngroup, na_rm, colsum, out, ovflow);
}

// C_rowsum_SVT, src/rowsum_methods.c:281-325
extern "C" int svt_rowsum_SVT(const svt_view *x, const int *group, int ngroup,
			      int na_rm, void *out, int *ovflow)
{
	return abi_status([&] { return xsum_SVT(x, group, ngroup, na_rm, false, out, ovflow); });
}

// C_colsum_SVT, src/rowsum_methods.c:363-401
extern "C" int svt_colsum_SVT(const svt_view *x, const int *group, int ngroup,
			      int na_rm, void *out, int *ovflow)
{
	return abi_status([&] { return xsum_SVT(x, group, ngroup, na_rm, true, out, ovflow); });
}

static int xsum_dgC(int nrow, int ncol, const double *xx, const int *xi, const int *xp,
		    const int *group, int ngroup, int na_rm, bool colsum, double *out)
{
	if (ensure_init() || check_group(group, colsum ? ncol : nrow, ngroup))
		return -1;
	const int64_t nnz = ncol > 0 ? xp[ncol] : 0;
	DevBuf P, I, X;
	if (P.upload(xp, (size_t) (ncol + 1) * 4) || I.upload(xi, (size_t) nnz * 4) ||
	    X.upload(xx, (size_t) nnz * 8))
		return -1;
	svt_dev_csc D;                      // (the int32 'p' slot goes beside it: the atomic kernels read either flavour)
	memset(&D, 0, sizeof(D));
	D.Rtype = SVT_REALSXP; D.nrow = nrow; D.ncol = ncol; D.nnz = nnz;
	D.row_idx = I.as<int32_t>(); D.val = X.p;
	int ovflow = 0;                     // (doubles: never raised)
	return groupsum_host(&D, P.as<int32_t>(), group, ngroup, na_rm, colsum, out, &ovflow);
}

// C_rowsum_dgCMatrix / C_colsum_dgCMatrix, src/rowsum_methods.c:328-356, 404-439
extern "C" int svt_rowsum_dgCMatrix(int nrow, int ncol, const double *xx, const int *xi,
				    const int *xp, const int *group, int ngroup,
				    int na_rm, double *out)
{
	return abi_status([&] { return xsum_dgC(nrow, ncol, xx, xi, xp, group, ngroup, na_rm, false, out); });
}
extern "C" int svt_colsum_dgCMatrix(int nrow, int ncol, const double *xx, const int *xi,
				    const int *xp, const int *group, int ngroup,
				    int na_rm, double *out)
{
	return abi_status([&] { return xsum_dgC(nrow, ncol, xx, xi, xp, group, ngroup, na_rm, true, out); });
}

// ==================================================================================
// Host level: column statistics of a dgCMatrix (src/sparseMatrix_utils.c:106-223)
// ==================================================================================
// The (x, p) slots of a dgCMatrix are the CSC layout itself (the 'i' slot is not read, as in
// the reference: :115-116, :152-153, :213-214).  which: 0 = colMins, 1 = colMaxs,
// 2 = colRanges (out: ncol x 2, mins then maxs, :155), 3 = colVars.  The extrema follow the
// SVT rules for doubles (NA wins, then NaN, one implicit zero when nzcount < nrow:
// min_double/max_double/minmax_double, :15-103); colVars is col_var() (:173-203): plain IEEE
// arithmetic, no NA rule and no "NA when fewer than two values" rule.
static int colstat_dgC(int nrow, int ncol, const double *xx, const int *xp, int na_rm,
		       int which, double *out)
{
	if (ensure_init())
		return -1;
	if (nrow < 0 || ncol < 0 || xp == NULL)
		return svt_set_error("invalid dgCMatrix slots");
	if (ncol == 0)
		return 0;
	std::vector<int64_t> cp((size_t) ncol + 1);
	for (int j = 0; j <= ncol; j++) {
		if (xp[j] < 0 || (j > 0 && (xp[j] < xp[j - 1] || xp[j] - xp[j - 1] > nrow)))
			return svt_set_error("invalid dgCMatrix 'p' slot");
		cp[(size_t) j] = xp[j];
	}
	const int64_t nnz = cp[(size_t) ncol];
	if (nnz > 0 && xx == NULL)
		return svt_set_error("invalid dgCMatrix slots");
	DevBuf P, X, O;
	if (P.upload(cp.data(), cp.size() * 8) || X.upload(xx, (size_t) nnz * 8) ||
	    O.alloc((size_t) ncol * 8 * (which == 2 ? 2 : 1)))
		return -1;
	svt_dev_csc A;
	memset(&A, 0, sizeof(A));
	A.Rtype = SVT_REALSXP; A.nrow = nrow; A.ncol = ncol; A.nnz = nnz;
	A.col_ptr = P.as<int64_t>(); A.val = X.p;
	static const int ops[4][2] = { { SVT_OP_MIN, -1 }, { SVT_OP_MAX, -1 }, { SVT_OP_MIN, SVT_OP_MAX }, { SVT_OP_VAR1, -1 } };
	for (int t = 0; t < 2 && ops[which][t] >= 0; t++)
		if (dev_colstats_ex(&A, ops[which][t], na_rm, svt_na_real(), 1, O.as<double>() + (size_t) t * ncol, NULL, 0, 1))
			return -1;
	HIP_TRY(hipDeviceSynchronize());
	return staged_download(out, O.p, (size_t) ncol * 8 * (which == 2 ? 2 : 1));
}

// C_colMins_dgCMatrix / C_colMaxs_dgCMatrix, src/sparseMatrix_utils.c:128-138
extern "C" int svt_colMins_dgCMatrix(int nrow, int ncol, const double *xx, const int *xp,
				     int na_rm, double *out)
{
	return abi_status([&] { return colstat_dgC(nrow, ncol, xx, xp, na_rm, 0, out); });
}
extern "C" int svt_colMaxs_dgCMatrix(int nrow, int ncol, const double *xx, const int *xp,
				     int na_rm, double *out)
{
	return abi_status([&] { return colstat_dgC(nrow, ncol, xx, xp, na_rm, 1, out); });
}
// C_colRanges_dgCMatrix, src/sparseMatrix_utils.c:143-166
extern "C" int svt_colRanges_dgCMatrix(int nrow, int ncol, const double *xx, const int *xp,
				       int na_rm, double *out)
{
	return abi_status([&] { return colstat_dgC(nrow, ncol, xx, xp, na_rm, 2, out); });
}
// C_colVars_dgCMatrix, src/sparseMatrix_utils.c:205-223
extern "C" int svt_colVars_dgCMatrix(int nrow, int ncol, const double *xx, const int *xp,
				     int na_rm, double *out)
{
	return abi_status([&] { return colstat_dgC(nrow, ncol, xx, xp, na_rm, 3, out); });
}
