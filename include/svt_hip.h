/*
 * svt_hip.h -- C ABI of libsvt_hip.so, the MI355X (gfx950) backend for
 * SparseArray's SVT compute hot path.
 *
 * Plain C: pointers and sizes only, no R types, no torch types.  There are
 * two levels:
 *
 *   1. Host level -- one function per `.Call` entry point of the reference
 *      (src/R_init_SparseArray.c:94,121-134).  Arguments are host pointers.
 *      The function marshals the SVT leaves into the CSC device layout,
 *      runs the HIP kernels and copies the result back into the caller's
 *      buffer.  This is what the R package's C glue binds.
 *
 *   2. Device level -- operands already resident in HBM (uploaded once with
 *      svt_upload(), or wrapped around existing device buffers), kernels
 *      launched asynchronously on a caller-supplied HIP stream, no
 *      allocation and no synchronisation inside.  This is what bench.py and
 *      the multi-GPU driver use.
 *
 * Return convention (all int-returning functions):
 *     0   success
 *   < 0   (-1) error; message in svt_last_error().  The R glue turns it into
 *         error(), like the reference's own error() calls
 *         (e.g. src/SparseMatrix_mult.c:943-966).
 *   > 0   (SVT_UNSUPPORTED = 1) not supported HERE: the device kernels do not take
 *         this operand or operation -- 2^31 nonzeros or more in the second operand of
 *         the row-panel product (an SVT's total count is unbounded,
 *         R/SVT_SparseArray-class.R:13-23; the host entry points fall back to the
 *         transposition route inside the library), a permuted array of 2^31 - 1 leaves or
 *         more in an aperm of 2^31 nonzeros or more (no aperm is refused for the operand's
 *         nonzero count alone: t() and the permutations that move the rows take the boxed
 *         drivers, the leaf-preserving ones count in 64 bits), too many strata
 *         for the row-statistics counters, an opcode the R API never sends
 *         (RANGE, SUM_X_X2, VAR2, SD2 for col / row statistics).  The reason is in
 *         svt_last_error(); nothing the caller relies on has been written.  The R glue
 *         answers it with the reference's own CPU body for that call
 *         (integration/svt_hip_glue.c, HIP_STATUS) -- the same thing it does when the
 *         library or the GPU is absent.  Inside the library a route that is refused
 *         falls back to another one where there is one (the sparse-aware crossprod to
 *         the dense-buffer route, the row-panel product to the transposition route);
 *         only what no device route takes surfaces as > 0.
 * Warning conditions ("NAs introduced by coercion of infinite values to
 * integers", src/SparseArray_matrixStats.c:278-280; "NAs produced by integer
 * overflow", src/rowsum_methods.c:122-123) are reported through the
 * `warn` / `ovflow` out-parameters so that the caller raises them on the R
 * thread after the call.
 *
 * Element types use R's SEXPTYPE codes.  Dense matrices are column-major
 * (R layout).  Missing values: NA_integer_ = INT_MIN, NA_real_ = the NaN with
 * low word 1954.
 */
#ifndef SVT_HIP_H
#define SVT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_UNSUPPORTED 1

#define SVT_LGLSXP 10
#define SVT_INTSXP 13
#define SVT_REALSXP 14

/* Opcodes of src/Rvector_summarization.h:12-34 */
#define SVT_OP_ANYNA            1
#define SVT_OP_COUNTNAS         2
#define SVT_OP_ANY              3
#define SVT_OP_ALL              4
#define SVT_OP_MIN              5
#define SVT_OP_MAX              6
#define SVT_OP_RANGE            7
#define SVT_OP_SUM              8
#define SVT_OP_PROD             9
#define SVT_OP_MEAN            10
#define SVT_OP_CENTERED_X2_SUM 11
#define SVT_OP_SUM_X_X2        12
#define SVT_OP_VAR1            13
#define SVT_OP_VAR2            14
#define SVT_OP_SD1             15
#define SVT_OP_SD2             16

/*
 * Host view of an SVT (Sparse Vector Tree, src/leaf_utils.h:10-31): the
 * tree flattened to its prod(dim[1..ndim-1]) leaves in depth-first order
 * (outermost dim slowest).  nzcount[j] == 0 is a NULL leaf / NULL subtree;
 * nzvals[j] == NULL with nzcount[j] > 0 is a lacunar leaf (all ones).
 * Replaces the (x_dim, x_type, x_SVT) argument triple of the .Call entry
 * points (src/SparseMatrix_mult.h:6-43, src/SparseArray_matrixStats.h:6-28,
 * src/rowsum_methods.h:6-36).
 */
typedef struct svt_view {
	int32_t Rtype;
	int32_t ndim;
	const int32_t *dim;
	int32_t svt_is_null;          /* x@SVT is NULL */
	int64_t nleaves;
	const int32_t *nzcount;
	const int32_t *const *nzoffs;
	const void *const *nzvals;
	int32_t na_background;        /* NaArray: the implicit value is NA, not zero (R/NaArray-class.R) */
} svt_view;

/* ---------------------------------------------------------------------- */
/* Library state                                                          */
/* ---------------------------------------------------------------------- */

/* Selects the HIP device for the calling process (one process per GPU).
   Returns 0, or -1 when no gfx950 device is usable.  Called implicitly with
   device 0 by the first host-level call.  Sets the device list below to {device}. */
int svt_init(int device);
const char *svt_last_error(void);
/* "gfx950" etc. of the selected device, or "" before svt_init(). */
const char *svt_device_arch(void);

/*
 * Device list of the host-level entry points (one process, several GPUs).  With more than one entry, four entry
 * points split an operand of at least svt_set_shard_min_nnz() nonzeros over the listed devices, one host thread,
 * pinned staging buffer pair and set of device buffers per entry:
 *   svt_crossprod2_SVT_mat  row blocks of x and y (boundaries at multiples of 128 rows); every shard forms a whole
 *                           ncol(x) x K partial, then a reduce-scatter: shard s fetches slice s of every partial,
 *                           adds them in list order ((p0 + p1) + p2) + ..., and copies the slice into `out`.  The
 *                           sums depend on the list's length and the row blocks only: {0,1} gives the bits of {0,0}.
 *   svt_matmul_SVT_mat      the same row blocks of x, y replicated; each shard writes its rows of `out`.
 *   svt_colStats_SVT        ranges of output cells balanced by nonzeros; each shard writes its slice; warn ORed.
 *   svt_rowsum_SVT          leaf ranges balanced by nonzeros; each shard writes its columns; ovflow ORed.
 * Every other entry point, and these below the threshold, run on the first entry as with one device.  A shard that
 * fails makes the call fail with its message; else a shard that answers > 0 makes the call answer > 0.  Sharded
 * calls do not use the resident cache (svt_resident_set_limit): they upload their parts and free them.  With a
 * one-entry list the entry points run exactly the one-device code.  The marshalling threads of svt_set_max_threads()
 * are divided among the shards (at least one each); the 96 MB of pinned staging buffers of the sharded path are
 * divided too (48 MB / N per buffer, two per shard), next to the 96 MB of the one-device path.
 * Ordinals may repeat ({0,0,0,0}: four shards on device 0).  Peer access is enabled between distinct ordinals.
 * No run on more than one physical device exists yet.
 */
/* 0, or -1 (svt_last_error()) when an ordinal is out of range or not gfx950, or n > 16: the previous list stays.
   n == 0: back to {the device of the last svt_init()}.  The first entry becomes the calling thread's device. */
int svt_set_devices(const int *ordinals, int n);
/* Length of the list (0 before svt_init()); fills up to cap entries of ordinals. */
int svt_get_devices(int *ordinals, int cap);
/* Operands with fewer nonzeros stay on the first device (default 2^24, an unmeasured guess); 0 = always shard. */
void svt_set_shard_min_nnz(int64_t nnz);

/*
 * Resident operands (off by default).  R code calls the entry points below over and over
 * on the same object, and each call marshals and uploads the whole tree again.  With a
 * byte limit > 0 the host-level entry points keep the device copy of every SVT operand
 * (plus what they derive from it: the panel-blocked layout, t(x)) up to that many bytes,
 * least recently used first out, and recognise the operand of a later call by a
 * fingerprint of its view: dims, type, and per leaf the host pointers, the count and
 * eight sampled (offset, value) pairs.  R vectors are not modified once shared; callers
 * that overwrite leaves in place must call svt_resident_clear().  This is the device-side
 * counterpart of the reference operating in place on host memory
 * (src/SVT_SparseArray_class.c:598-633 walks the leaves on every call, at no cost).
 */
int svt_resident_set_limit(size_t bytes);          /* 0 = off, frees everything */
void svt_resident_clear(void);
void svt_resident_stats(size_t *bytes, int64_t *entries, int64_t *hits, int64_t *misses);

/* ---------------------------------------------------------------------- */
/* 1. Host level: the .Call entry points                                   */
/* ---------------------------------------------------------------------- */

/* C_crossprod2_SVT_mat, src/SparseMatrix_mult.c:931-982.
   out: ncol(x) x (tr_y ? y_nrow : y_ncol) doubles.
   Types: the reference's entry point requires type(x) == typeof(y) and its R method coerces the
   integer operand of a mixed pair on the host first; svt_crossprod2_SVT_mat, _mat_SVT and
   svt_matmul_SVT_mat also take an integer operand next to a double one and widen it on the device
   (NA_integer_ -> NA_real_, as as.double() does). */
int svt_crossprod2_SVT_mat(const svt_view *x, const void *y, int y_nrow,
			   int y_ncol, int y_Rtype, int tr_y, double *out);
/* C_crossprod2_mat_SVT, src/SparseMatrix_mult.c:985-1034.
   out: (tr_x ? x_nrow : x_ncol) x ncol(y) doubles. */
int svt_crossprod2_mat_SVT(const void *x, int x_nrow, int x_ncol, int x_Rtype,
			   const svt_view *y, int tr_x, double *out);
/* C_crossprod2_SVT_SVT, src/SparseMatrix_mult.c:1037-1101. */
int svt_crossprod2_SVT_SVT(const svt_view *x, const svt_view *y, double *out);
/* C_crossprod1_SVT, src/SparseMatrix_mult.c:1104-1140. */
int svt_crossprod1_SVT(const svt_view *x, double *out);
/* x %*% y in one call (R/SparseMatrix-mult.R:195-215: the R methods transpose x on the host
   with C_transpose_2D_SVT, src/SparseArray_aperm.c:348-423, then call C_crossprod2_SVT_mat /
   C_crossprod2_SVT_SVT).  Here x is uploaded once and transposed on the device.
   out: nrow(x) x ncol(y) doubles, column-major.  Same checks and messages as the
   crossprod2 entry points. */
int svt_matmul_SVT_mat(const svt_view *x, const void *y, int y_nrow, int y_ncol,
		       int y_Rtype, double *out);
int svt_matmul_SVT_SVT(const svt_view *x, const svt_view *y, double *out);

/* tcrossprod(x) and tcrossprod(x, y) of SVT_SparseMatrix objects in one call (round 6).  The R methods
   (R/SparseMatrix-mult.R:165-193) are crossprod(t(x)) / crossprod(t(x), t(y)) with t() on the host
   (C_transpose_2D_SVT, then a second marshalling of the transposed trees); here x (and y) are uploaded as they are and
   transposed on the device -- and the sparse-aware kernel of svt_dev_crossprod_csc_csc wants the ROWS of t(x), i.e. x
   itself, so its side needs no transposition at all.  Same checks, messages, route choice and NA / NaN rules as
   svt_crossprod1_SVT / svt_crossprod2_SVT_SVT on the transposed operands.
   out: nrow(x) x nrow(x) resp. nrow(x) x nrow(y) doubles, column-major. */
int svt_tcrossprod1_SVT(const svt_view *x, double *out);
int svt_tcrossprod2_SVT_SVT(const svt_view *x, const svt_view *y, double *out);

/* colMedians(x, na.rm) of a 2-D SVT: .colMedians_SVT_SparseMatrix / .padded_median,
   R/SparseArray-matrixStats.R:690-784 -- pure R in the reference (one sort per leaf; its TODO
   at :690-691 asks for a .Call version).  Median of each column's nrow values, the implicit
   zeros included; any NA/NaN among the nonzeros gives NA_real_ unless na_rm, an empty column
   of a 0-row matrix NA_real_.  out: ncol(x) doubles.  rowMedians(x) is colMedians(t(x)) as
   in the reference (:802-815). */
int svt_colMedians_SVT(const svt_view *x, int na_rm, double *out);
/* rowMedians(x): the same on t(x), transposed on the device.  out: nrow(x) doubles. */
int svt_rowMedians_SVT(const svt_view *x, int na_rm, double *out);

/* colQuantiles(x, probs, na.rm, type = 7) of a 2-D SVT.  The reference has no method (colQuantiles and colIQRs are in
   its list of statistics to add, R/SparseArray-matrixStats.R:5-12); the rule is matrixStats::colQuantiles(type = 7),
   i.e. base R's quantile.default type 7, on each column's nrow values, the implicit zeros included.  With the n values
   left after the NA rule sorted ascending as x[1..n], in IEEE double exactly as written (no fused multiply-add):
       index = 1 + (n - 1) * p;  lo = floor(index);  hi = ceiling(index);  q = x[lo]
       if (index > lo && x[hi] != x[lo]) { h = index - lo;  q = (1 - h) * x[lo] + h * x[hi] }
   -Inf and +Inf as neighbours give NaN (not NA), two equal neighbours that value.  NA rule as svt_colMedians_SVT:
   na_rm drops NA/NaN from the stored values; otherwise any NA/NaN makes every quantile of the column NA_real_; n == 0
   gives NA_real_.  Stored zeros count among the zeros.  Integer / logical values are read as doubles.
   probs: nprobs >= 0 doubles (host), each finite and in [0, 1] (else error "'probs' outside [0,1]", raised before
   anything is uploaded); unsorted and repeated entries are allowed and the output keeps their order.
   out: ncol(x) * nprobs doubles (rowQuantiles: nrow(x) * nprobs), column-major: out[j + q * ncol].  A 0-column operand
   or nprobs == 0 writes nothing.  Errors: not 2-D, NaArray ("colQuantiles() is not supported on NaArray objects").
   Status > 0 only for more than 2^31-1 columns; the operand's nonzero count is not limited.
   rowQuantiles(x) is colQuantiles(t(x)) with t() on the device (boxed past 2^31 nonzeros, as for rowMedians).
   colIQRs / rowIQRs are this call with probs = (0.25, 0.75) and Q3 - Q1 on the host.
   These calls are not sharded over the device list of svt_set_devices(): they run on the first entry.
   Not offered: colOrderStats, quantile types other than 7, N-d operands, NaArray operands. */
int svt_colQuantiles_SVT(const svt_view *x, const double *probs, int nprobs, int na_rm, double *out);
int svt_rowQuantiles_SVT(const svt_view *x, const double *probs, int nprobs, int na_rm, double *out);

/* colMads(x, center, constant, na.rm) of a 2-D SVT: stats::mad without low / high on each column's nrow values, the
   implicit zeros included (colMads is in the reference's list of statistics to add, R/SparseArray-matrixStats.R:5-12,
   rowMads in its TODO).  Every operation is IEEE double, each rounded on its own.  Per column, with stored values x
   (NA / NaN = missing):
     1. the NA rule of svt_colMedians_SVT: a missing value without na_rm gives NA_real_; na_rm drops the missing stored
        values and the padding keeps its size; n values remain, n == 0 gives NA_real_;
     2. c = center[j], or with center == NULL the column's median by the median's own rule (the middle value, or
        (lo + hi) * 0.5 -- not the 0.5 quantile);
     3. c NA or NaN (the median of -Inf and +Inf is NaN) gives NA_real_;
     4. t_i = fabs(x_i - c), one subtraction; every zero, stored or implicit, becomes fabs(0.0 - c).  A t_i that is NaN
        (x_i and c the same infinity) gives NA_real_, also under na_rm: stats::mad takes the median of the deviations
        without na.rm;
     5. M = the median of the n values t by the median's rule; the result is constant * M, one product.  `constant` is
        not checked (stats::mad's default is 1.4826).
   center: NULL or ncol(x) doubles on the host (rowMads: nrow(x)).  out: ncol(x) doubles (rowMads: nrow(x)).
   rowMads(x) is colMads(t(x)) with t() on the device, as for rowMedians.  Limits and errors are svt_colMedians_SVT's:
   2-D operands, double / integer / logical values, at most 2^31-1 columns (status > 0 beyond), any number of nonzeros;
   NaArray operands are an error ("colMads() is not supported on NaArray objects"); not sharded over the device list. */
int svt_colMads_SVT(const svt_view *x, const double *center /* NULL or ncol(x) */, double constant, int na_rm,
		    double *out);
int svt_rowMads_SVT(const svt_view *x, const double *center /* NULL or nrow(x) */, double constant, int na_rm,
		    double *out);

/* colRanks(x, ties.method, preserveShape) of a 2-D SVT: rank(na.last = "keep", ties.method) of each column's nrow
   values, the implicit zeros included (matrixStats::colRanks; the reference has no method).  Per column, with the
   missing stored values (NaN / NA for doubles, NA_integer_ for integers and logicals) left out, and for a non-missing
   value v:
     L = the non-missing values < v (the implicit zeros count when 0 < v);
     E = the values == v under IEEE == (-0.0, a stored 0.0 and the implicit zeros are one tie group; v counts);
     SVT_TIES_MAX L + E (matrixStats' default), SVT_TIES_MIN L + 1, SVT_TIES_AVERAGE (double) (2L + E + 1) * 0.5,
     SVT_TIES_DENSE 1 + the distinct values < v (the zeros are one distinct value if the column holds any).
   +-Inf are ordinary values.  A missing value gets NA and is counted in nobody's L or E; there is no na.rm.
   out: nrow(x) * ncol(x) cells, int32 (NA_integer_) for max / min / dense, double (NA_real_ for NaN and NA alike) for
   average.  colRanks with preserve_shape == 0 (matrixStats' default) fills the TRANSPOSED shape, out[j + i * ncol],
   ncol x nrow; with preserve_shape != 0 out[i + j * nrow].  rowRanks(x) is colRanks(t(x), preserveShape = FALSE):
   out[i + j * nrow], nrow x ncol, t() on the device (boxed past 2^31 nonzeros).  Cell indices are 64-bit; zero extents
   write nothing.  The device computes the compact form of svt_dev_colranks; it is expanded on the host.
   Errors: not 2-D ("the colRanks() method for SparseArray objects only supports 2D objects ..."; rowRanks() in the row
   form), NaArray operands ("colRanks() is not supported on NaArray objects"), another `ties` ("'ties.method' must be
   "max", "average", "min" or "dense""); double / integer / logical values.  Status > 0: more than 2^31-1 columns, or
   2^32 or more stored values in columns too long to be sorted in LDS.  Not sharded over the device list.
   Not offered: ties.method "first", "last" and "random" (every implicit zero would need a rank of its own). */
#define SVT_TIES_MAX 0
#define SVT_TIES_AVERAGE 1
#define SVT_TIES_MIN 2
#define SVT_TIES_DENSE 3
int svt_colRanks_SVT(const svt_view *x, int ties, int preserve_shape, void *out);
int svt_rowRanks_SVT(const svt_view *x, int ties, void *out);

/* C_summarize_SVT, src/SparseArray_summarization.c:112-142.  The result is
   left in out_d[0..1] or out_i[0..1] according to *out_Rtype. */
int svt_summarize_SVT(const svt_view *x, int opcode, int na_rm, double center,
		      double *out_d, int *out_i, int *out_Rtype, int *warn);

/* Result element type of a col/row stat (src/Rvector_summarization.c:97-165):
   SVT_LGLSXP/SVT_INTSXP -> int32 buffer, SVT_REALSXP -> double buffer. */
int svt_colStats_out_Rtype(int opcode, int in_Rtype);
/* C_colStats_SVT, src/SparseArray_matrixStats.c:234-284.
   out: prod(dim[dims..]) elements. */
int svt_colStats_SVT(const svt_view *x, int opcode, int na_rm, double center,
		     int dims, void *out, int *warn);
/* C_rowStats_SVT, src/SparseArray_matrixStats.c:1121-1205.
   center: NULL or prod(dim[0..dims-1]) doubles.  out: same length. */
int svt_rowStats_SVT(const svt_view *x, int opcode, int na_rm,
		     const double *center, int dims, void *out, int *warn);
/* Every row statistic of the R API in one call.  C_rowStats_SVT (above) mirrors the reference and takes six
   operations; rowAnys / rowAlls / rowProds go through a transposition and the column statistics there
   (.OLD_rowStats_SparseArray, R/SparseArray-matrixStats.R:122-190, with the TODO of :109-121), and rowMeans /
   rowVars / rowSds / rowRanges are composed of two to four calls (:440, :457: "do all this in a single pass").
   This entry point takes those six plus SVT_OP_ANY, _ALL, _PROD, _RANGE, _MEAN, _VAR1 and _SD1: one operand on the
   device (the resident cache applies), svt_dev_rowstats(), one download.  Same checks, messages, zero-extent
   handling and constant fills as svt_rowStats_SVT.  mean / var1 / sd1 are the plain IEEE expressions of the R
   methods (:511-516, :645-660): sum / nvals, centered_X2_sum / (nvals - 1) and its square root, nvals = the number
   of strata, less the NAs when na_rm; there is no "fewer than two values" rule here.  prod multiplies in no fixed
   order: results are not bit-reproducible.
   center (var1 / sd1 / centered_X2_sum): NULL or prod(dim[0..dims-1]) doubles.  out: prod(dim[0..dims-1]) elements
   of svt_colStats_out_Rtype(); SVT_OP_RANGE: twice that, the minima, then the maxima.
   Status: > 0 for more than 65535 output columns with one of the seven added operations; < 0 ("operation not yet
   supported on NaArray objects") for an added operation other than SVT_OP_RANGE on a NaArray.
   This call is not sharded over the device list of svt_set_devices(): it runs on the first entry. */
int svt_rowStatsFull_SVT(const svt_view *x, int opcode, int na_rm,
			 const double *center, int dims, void *out, int *warn);

/* C_rowsum_SVT / C_colsum_SVT, src/rowsum_methods.c:281-325, 363-401.
   group: 1-based, NA allowed.  out: ngroup x ncol (rowsum) or nrow x ngroup
   (colsum); int32 for SVT_INTSXP input, else double. */
int svt_rowsum_SVT(const svt_view *x, const int *group, int ngroup, int na_rm,
		   void *out, int *ovflow);
int svt_colsum_SVT(const svt_view *x, const int *group, int ngroup, int na_rm,
		   void *out, int *ovflow);
/* C_rowsum_dgCMatrix / C_colsum_dgCMatrix, src/rowsum_methods.c:328-356,
   404-439: the (x, i, p) slots of a dgCMatrix. */
int svt_rowsum_dgCMatrix(int nrow, int ncol, const double *xx, const int *xi,
			 const int *xp, const int *group, int ngroup,
			 int na_rm, double *out);
int svt_colsum_dgCMatrix(int nrow, int ncol, const double *xx, const int *xi,
			 const int *xp, const int *group, int ngroup,
			 int na_rm, double *out);

/* C_colMins_dgCMatrix / C_colMaxs_dgCMatrix / C_colRanges_dgCMatrix / C_colVars_dgCMatrix,
   src/sparseMatrix_utils.c:128-166, 205-223 (registered at src/R_init_SparseArray.c:49-52;
   R wrappers R/sparseMatrix-utils.R:300-330): column statistics of a dgCMatrix from its
   Dim, x and p slots (the i slot is not read).  out: ncol doubles; colRanges: ncol x 2
   column-major (mins, then maxs).  NA / NaN rules of min_double() etc. (:15-103): an NA gives
   NA_real_ unless na_rm, else a NaN gives NaN; a column with fewer than nrow stored entries
   starts from 0.  colVars is col_var() (:173-203): IEEE arithmetic throughout. */
int svt_colMins_dgCMatrix(int nrow, int ncol, const double *xx, const int *xp,
			  int na_rm, double *out);
int svt_colMaxs_dgCMatrix(int nrow, int ncol, const double *xx, const int *xp,
			  int na_rm, double *out);
int svt_colRanges_dgCMatrix(int nrow, int ncol, const double *xx, const int *xp,
			    int na_rm, double *out);
int svt_colVars_dgCMatrix(int nrow, int ncol, const double *xx, const int *xp,
			  int na_rm, double *out);

/* ---------------------------------------------------------------------- */
/* 2. Device level                                                         */
/* ---------------------------------------------------------------------- */

/*
 * CSC-like device layout of an SVT (the device-side analogue of
 * dump_SVT_to_CsparseMatrix_slots(), src/SVT_SparseArray_class.c:598-633):
 *   col_ptr int64[ncol+1], row_idx int32[nnz], val f64|i32[nnz]
 * with ncol = number of leaves, nrow = dim[0]; lacunar leaves are expanded
 * to explicit ones.  All pointers are device pointers.
 */
typedef struct svt_dev_csc {
	int32_t Rtype;
	int32_t owned;        /* buffers were allocated by svt_upload() */
	int64_t nrow;
	int64_t ncol;
	int64_t nnz;
	int64_t *col_ptr;
	int32_t *row_idx;
	void *val;
	int32_t na_background; /* NaArray operand: implicit entries are NA (col stats / summarization
	                          only; set by svt_upload(), 0 for wrapped buffers) */
} svt_dev_csc;

/*
 * Workspaces.  One contract for every device-level entry point that takes `ws` (or the `gid` buffer of
 * svt_dev_rowsum_prepare), stated here once; the comments below point to it:
 *   - the caller aligns `ws` and the output arrays to 256 bytes (what a device allocation has; `ws` is carved into
 *     arrays at multiples of 256 bytes from its start) and passes at least the bytes the matching `_ws_bytes()` /
 *     `_gid_bytes()` query advertises.  A smaller `ws_bytes` is an error ("... workspace too small", "... id buffer
 *     too small"), answered before anything is launched or written -- by the `_prepared` calls too;
 *   - the call writes nothing outside [ws, ws + the advertised size) and its outputs at the sizes their comments give;
 *   - every cell of every output is written, the not-finite flag of the sparse x sparse products included (also when
 *     the result has no cells), unless the comment of the call says which cells it leaves alone and when;
 *   - the result does not depend on what `ws` holds on entry: a call clears what it needs cleared.  A `_prepared`
 *     call reads what its `_prepare` call left, and nothing else of the workspace's past.
 * Tested in an arena of 0xA5 bytes with guard bands: tests/test_hip_ws_discipline.py for the products, the row
 * statistics, colMedians and the prepared rowsum; the test files of the other families for theirs.
 */

/* Marshal + H2D.  Returns NULL on error. */
svt_dev_csc *svt_upload(const svt_view *x);
/* Wrap device buffers owned by the caller (e.g. a torch allocation). */
svt_dev_csc *svt_wrap_device_csc(int Rtype, int64_t nrow, int64_t ncol,
				 int64_t nnz, int64_t *col_ptr,
				 int32_t *row_idx, void *val);
void svt_release(svt_dev_csc *h);

/*
 * crossprod(A, Y): out[c, k] = sum_r A[r, c] * Y[r, k], the kernel family
 * K1-K8 of the reference (src/SparseMatrix_mult.c:131-239) for all K dense
 * columns in one pass over A.
 *   Y      in_nrow x K, column-major with leading dimension ldY (doubles for
 *          a REALSXP A, int32 for an INTSXP A); or, with tr_y != 0, K x
 *          in_nrow column-major (ldY >= K), i.e. rows of Y are contiguous.
 *   out    element (c, k) is written at out[c * out_stride_c + k *
 *          out_stride_k]: (1, ncol) gives the column-major ncol x K result
 *          of C_crossprod2_SVT_mat, (K, 1) gives the K x ncol result of
 *          C_crossprod2_mat_SVT.
 *   ws     workspace of at least svt_dev_crossprod_ws_bytes() bytes ("Workspaces" above).
 * Asynchronous on `stream` (a hipStream_t).
 */
size_t svt_dev_crossprod_ws_bytes(int64_t nrow, int64_t ncol, int K);
/* The two phases of svt_dev_crossprod_csc_dense(), callable separately so a
   dense operand can be prepared once and multiplied several times (and so
   that each phase can be timed): (1) stage Y into `ws` and evaluate the
   reference's per-column prescan predicates (src/SparseMatrix_mult.c:23-36);
   (2) the sparse x dense product proper, reading `ws`. */
int svt_dev_dense_prepare(const void *Y, int64_t ldY, int64_t nrow, int K,
			  int tr_y, int Rtype, void *ws, size_t ws_bytes,
			  void *stream);
int svt_dev_crossprod_prepared(const svt_dev_csc *A, const void *ws, int K,
			       double *out, int64_t out_stride_c,
			       int64_t out_stride_k, void *stream);
int svt_dev_crossprod_csc_dense(const svt_dev_csc *A, const void *Y,
				int64_t ldY, int K, int tr_y, double *out,
				int64_t out_stride_c, int64_t out_stride_k,
				void *ws, size_t ws_bytes, void *stream);

/*
 * Fast path of crossprod(A, Y) for f64 operands: a panel-blocked copy of A
 * ("PBC", see sparsearray_amd/csrc/kernels_mult_pbc.hip) built once per
 * sparse operand -- the device analogue of the reference's per-call leaf
 * "preprocessing" (src/SparseMatrix_mult.c:632-724) -- and a kernel that keeps
 * row panels of Y in LDS and per-column partial sums in registers.
 *   CBW   columns per wavefront, WPB wavefronts per workgroup, logR = log2(rows per panel).
 *         Two families, both with 1 <= CBW <= 40: (CBW, 16, 7), the LDS-DMA kernel, and
 *         (CBW, 4, 9 .. 15), the gather kernels (rows of Y straight from L2).  (0, 0, 0) = chosen
 *         by the operand's density: (40, 16, 7), or, below ~0.25 % density, (40, 4, 9 .. 11).
 *         Any other layout is refused (NULL, svt_last_error()).  An LDS-DMA layout of an operand
 *         with fewer than 256 (or 2^28 and more) rows is built without records: its products run
 *         the general kernels of svt_dev_crossprod_csc_dense(), with their results.
 * svt_dev_pbc_build() allocates and synchronises (not for the launch path).
 * svt_dev_crossprod_pbc() has the semantics and the out-indexing of
 * svt_dev_crossprod_csc_dense() (A is needed for the general path that
 * takes over when Y holds NaN/Inf/NA); Y is f64.  ws: svt_dev_crossprod_pbc_ws_bytes() bytes ("Workspaces" above).
 */
typedef struct svt_dev_pbc svt_dev_pbc;
svt_dev_pbc *svt_dev_pbc_build(const svt_dev_csc *A, int CBW, int WPB, int logR);
void svt_dev_pbc_release(svt_dev_pbc *P);
/* Layout buffers come from a stream-ordered pool of the library's own (one per device) that keeps up to 3 GiB of
   released memory for the next build; svt_dev_pbc_release() frees behind the work of every stream that has run a
   product with the layout (an event recorded on each of them at release time: no device-wide synchronisation, and
   nothing put on the stream per product; a stream destroyed before the handle is released makes the release
   synchronise the device instead -- a stream that has run a product with a layout should outlive the layout's
   handle, or the handle be released first: the release records on every stream it noted, and a stale
   hipStream_t is only as safe as the runtime's validation of it).  svt_dev_pbc_trim() hands everything the pools hold
   but no layout uses back to the driver -- e.g. before another allocator of the process needs the memory. */
void svt_dev_pbc_trim(void);
/* Device bytes held by a layout (records + tile table + flags). */
size_t svt_dev_pbc_bytes(const svt_dev_pbc *P);
size_t svt_dev_crossprod_pbc_ws_bytes(const svt_dev_pbc *P, int K);
int svt_dev_crossprod_pbc(const svt_dev_pbc *P, const svt_dev_csc *A,
			  const double *Y, int64_t ldY, int K, int tr_y,
			  double *out, int64_t out_stride_c,
			  int64_t out_stride_k, void *ws, size_t ws_bytes,
			  void *stream);

/* CUs the LDS-DMA product kernel leaves idle (default 0).  Its workgroups take a whole CU each, so a
   collective's kernels cannot start beside it; with n > 0 (a multiple of 8: n / 8 per XCD) the row splits are
   chosen so that at most 256 - n workgroups run -- for the multi-GPU driver, whose all-reduce of step i
   runs beside the product of step i + 1 (the reference has no counterpart: its OpenMP loop,
   src/SparseMatrix_mult.c:253-258, owns the cores it is given).  Process-wide; takes effect at the next
   product (a workspace sized by svt_dev_crossprod_pbc_ws_bytes() fits either setting). */
void svt_dev_pbc_set_spare_cus(int n);
int svt_dev_pbc_spare_cus(void);

/* Pacing of the gather product (very sparse operands, K a multiple of 128, >= 64 row panels): its grid is
   persistent, every XCD owns a range of rows, and a wavefront runs at most `dsync` row panels ahead of the
   slowest wavefront of its XCD that has started, so that the rows of the dense operand the XCD gathers stay
   in its L2; `spin` = polls after which a wavefront that waits in vain stops pacing itself (results never
   depend on the pacing).  Defaults (1, 256).  dsync < 0:
   the unpaced kernels (one launch per chunk of rows) run instead.  Process-wide; no reference counterpart
   (src/SparseMatrix_mult.c:131-152 walks leaf by leaf on the host). */
void svt_dev_pbc_set_gather_pacing(int dsync, int spin);

/* Products with many column blocks and no row split (A %*% Y on the layout of t(A)) are launched one round of
   workgroups at a time, so that every round starts aligned and the dense tile its workgroups stage streams
   through the XCDs' L2 once per round, and the last, partly filled round (54 of 256 CUs at BASELINE config 2b) is cut by
   rows into 256 / its size splits whose partial sums are added in split order (round 5); on = 2: per round, the last round
   whole; on = 0: one launch.  Default 1.  Process-wide, tuning / measurement. */
void svt_dev_pbc_set_round_launches(int on);

/* The same, restricted to the leaves from `first_col` on (rounded down to the kernel's block of
   16 * CBW columns): cells of earlier leaves are not written.  What the unary crossprod(x) needs:
   of dense column k only the leaves c >= k (compute_sym_dotprods_*, src/SparseMatrix_mult.c:
   263-296, computes ncol^2 / 2 dot products and mirrors them). */
int svt_dev_crossprod_pbc_from(const svt_dev_pbc *P, const svt_dev_csc *A,
			       const double *Y, int64_t ldY, int K, int tr_y,
			       double *out, int64_t out_stride_c,
			       int64_t out_stride_k, void *ws, size_t ws_bytes,
			       void *stream, int64_t first_col);

/* What svt_dev_crossprod_pbc_from() with the same (P, K, tr_y, output strides, first_col) launches under the present
   settings of the knobs (spare CUs, gather pacing, round launches): a pure host query that calls the functions the
   launch calls and enqueues nothing; for tests and fuzzers that must know which kernel, split count and launch count
   they exercise.  The device's CU count enters as in the launch.
     kind              0 none (no records: the general kernels answer in phase 2), 1 LDS-DMA, 2 gather
     kernel            SVT_PBC_KERNEL_*: the product kernel of phase 1
     NV                accumulator vectors per lane, (CBW + 15) / 16   (0 for the general kernels)
     nsplit            row splits whose partial sums the reduce kernel adds (gatherx: one per XCD with rows)
     panels_per_split  row panels per split (gather / gather2: over the whole operand, not per row chunk)
     direct            1: the product kernel writes `out` itself, no partials
     launches          launches of the product kernel: rounds of column blocks plus the cut last round (LDS-DMA),
                       row chunks (gather, gather2), 1 (gatherx), 0 (general)
     tail_splits       row splits of the cut last round (1: no such round), tail_blocks its column blocks */
enum { SVT_PBC_KERNEL_GENERAL = 0, SVT_PBC_KERNEL_DMA = 1, SVT_PBC_KERNEL_GATHER = 2, SVT_PBC_KERNEL_GATHER2 = 3,
       SVT_PBC_KERNEL_GATHERX = 4 };
typedef struct svt_pbc_plan {
	int kind, kernel, NV, nsplit;
	int64_t panels_per_split;
	int direct, launches, tail_splits, tail_blocks;
} svt_pbc_plan;
int svt_dev_crossprod_pbc_plan(const svt_dev_pbc *P, int K, int tr_y, int64_t out_stride_c,
			       int64_t out_stride_k, int64_t first_col, svt_pbc_plan *plan);

/* The two phases of svt_dev_crossprod_pbc() separately (so that each can be
   timed): phase 1 = the LDS-panel product kernel (partial sums into ws),
   phase 2 = deterministic sum of the partials into `out` + the general path
   when Y is not finite. */
int svt_dev_crossprod_pbc_phase(const svt_dev_pbc *P, const svt_dev_csc *A,
				const double *Y, int64_t ldY, int K, int tr_y,
				double *out, int64_t out_stride_c,
				int64_t out_stride_k, void *ws, size_t ws_bytes,
				void *stream, int phase);

/* col stats over segments of `inner` consecutive leaves each
   (dims > 1 => inner = prod(dim[1..dims-1])); out has ncol/inner elements of
   svt_colStats_out_Rtype().  warn_flag: device int, set to 1 on the
   "NAs introduced" condition (may be NULL). */
int svt_dev_colstats(const svt_dev_csc *A, int opcode, int na_rm,
		     double center, int64_t inner, void *out, int *warn_flag,
		     void *stream);

/* Which launch form svt_dev_colstats() -- and every host entry point that ends in it: svt_colStats_SVT,
   svt_summarize_SVT, the dgCMatrix column statistics -- takes for `nseg` generalized columns holding `nnz` nonzeros in
   all.  A pure host query (no device, no handle), the same function the launcher calls; for tests and fuzzers that
   must know which kernel they exercise.  The form follows from nseg and the AVERAGE length nnz / nseg alone:
     0  one thread per column            (average < 4, at least 4096 columns)
     1  16 lanes per column              (average < 160)
     2  one wavefront per column         (160 <= average < 1024)
     3  one workgroup per column, the column kept in registers for the centred pass   (1024 <= average <= 10240)
     4  one workgroup per column, streaming   (average > 10240)
     5  split: *nchunk workgroups per column, partial states combined in chunk order   (fewer than 512 columns,
        average >= 65536)
   Forms 1, 2 and 3 keep a column of at most 256, 1024 and 12288 nonzeros in registers and read a longer one
   twice (var1, sd1, centered_X2_sum); that choice is made per column, inside the launch.
   *nchunk (may be NULL): chunks per column for form 5, else 1. */
int svt_dev_colstats_form(int64_t nseg, int64_t nnz, int *nchunk);

/* colMedians on the device (see svt_colMedians_SVT): out = ncol doubles (device);
   ws: svt_dev_colmedians_ws_bytes() bytes (two f64 key arrays + the sort's scratch; "Workspaces" above). */
size_t svt_dev_colmedians_ws_bytes(int64_t nnz, int64_t ncol);
int svt_dev_colmedians(const svt_dev_csc *A, int na_rm, double *out, void *ws, size_t ws_bytes,
		       void *stream);

/* colQuantiles on the device (see svt_colQuantiles_SVT): probs (nprobs doubles, already validated by the caller) and
   out (ncol * nprobs doubles, out[j + q * ncol]) are device pointers; ws: svt_dev_colquantiles_ws_bytes() bytes (a
   too small one is an error).  Asynchronous on `stream`, allocates nothing, does not synchronise: one counting
   launch whatever nprobs is, one select launch for the (column, prob) pairs it could not decide. */
size_t svt_dev_colquantiles_ws_bytes(int64_t nnz, int64_t ncol, int nprobs);
int svt_dev_colquantiles(const svt_dev_csc *A, const double *probs, int nprobs, int na_rm,
			 double *out, void *ws, size_t ws_bytes, void *stream);

/* colMads on the device (see svt_colMads_SVT): center (NULL = the medians, else ncol doubles) and out (ncol doubles)
   are device pointers.  Asynchronous on `stream`, allocates nothing, reads nothing back: without a center the median's
   two launches into a center array inside ws, then one counting launch over the deviations (which answers a column whose
   median is 0 and more than half of whose values are zeros from the median's counts, without reading it again) and one
   select launch for the columns it could not decide.
   ws: svt_dev_colmads_ws_bytes(nnz, ncol) = max(ncol, 1) * 64 + 1024 bytes: the per-column arrays of the two counting
   passes (28 bytes a column each), the centers (8), and room to align the three to 256 bytes.  A smaller one is an
   error ("svt_dev_colmads: workspace too small"). */
size_t svt_dev_colmads_ws_bytes(int64_t nnz, int64_t ncol);
int svt_dev_colmads(const svt_dev_csc *A, const double *center /* device, NULL = medians */, double constant,
		    int na_rm, double *out, void *ws, size_t ws_bytes, void *stream);

/* colRanks on the device in the compact form a sparse matrix allows (the rule: svt_colRanks_SVT): all zeros of a
   column tie, so the result is rank_nz[k], one rank for every stored position k of the CSC (64-bit positions), and
   zero_rank[j], the rank of column j's zeros -- 4 or 8 bytes per nonzero instead of nrow * ncol cells.  Both are int32
   for SVT_TIES_MAX / MIN / DENSE and double for SVT_TIES_AVERAGE.  A stored 0.0 or -0.0 gets zero_rank[j]; zero_rank[j]
   is NA when the column holds no zero at all, stored or implicit.
   Columns are served by their stored length, inside one call: svt_dev_colranks_form(col_nnz), a pure host query,
   answers 0 (short: a wavefront per column, counted in LDS), 1 (a workgroup per column, sorted in LDS) or 2 (long:
   gathered and sorted in the workspace).  ws: svt_dev_colranks_ws_bytes(ncol, long_nnz), long_nnz = the sum of the
   stored lengths of the columns of form 2 (0 is returned for 2^32 or more: not offered).  A workspace below
   svt_dev_colranks_ws_bytes(ncol, 0) is an error ("svt_dev_colranks: workspace too small"); if it was made for fewer
   long nonzeros than the operand holds, nothing is written for the long columns and *flag, a device word that every
   call clears first, is set to 1.  The sort of the long columns runs over the long nonzeros the workspace has room
   for (at most nnz), so a workspace made for the exact long_nnz costs least.
   Asynchronous on `stream`, allocates nothing, reads nothing back. */
int svt_dev_colranks_form(int64_t col_nnz);
size_t svt_dev_colranks_ws_bytes(int64_t ncol, int64_t long_nnz);
int svt_dev_colranks(const svt_dev_csc *A, int ties, void *rank_nz, void *zero_rank, int *flag, void *ws,
		     size_t ws_bytes, void *stream);

/* row sums: out[(j % inner) * nrow + r] = sum over the leaves j that map to
   that cell.  Every output cell is owned by one workgroup (LDS row panels, no
   memory atomics); ws: svt_dev_rowstats_ws_bytes() bytes ("Workspaces" above). */
size_t svt_dev_rowstats_ws_bytes(int64_t nrow, int64_t ncol);
int svt_dev_rowsums(const svt_dev_csc *A, int na_rm, int64_t inner,
		    double *out, void *ws, size_t ws_bytes, void *stream);
/* The table of run bounds per row panel that svt_dev_rowsums() derives from the operand's offsets (a quarter
   of its time at BASELINE config 2) depends on the operand and `inner` only: svt_dev_rowsums_prepare() leaves
   it in `ws` once, svt_dev_rowsums_prepared() -- same operand, same `inner`, same `ws` -- uses it as it is. */
int svt_dev_rowsums_prepare(const svt_dev_csc *A, int64_t inner, void *ws, size_t ws_bytes, void *stream);
int svt_dev_rowsums_prepared(const svt_dev_csc *A, int na_rm, int64_t inner,
			     double *out, void *ws, size_t ws_bytes, void *stream);

/* Any row statistic of a resident operand: the six operations of svt_rowStats_SVT plus SVT_OP_ANY, _ALL, _PROD,
   _RANGE, _MEAN, _VAR1 and _SD1 (see svt_rowStatsFull_SVT for their rules).  out[(j % inner) * nrow + r], inner * nrow
   elements of svt_colStats_out_Rtype(); SVT_OP_RANGE: twice that, the minima, then the maxima.  center: device,
   inner * nrow doubles or NULL (centered_X2_sum, var1, sd1).  warn_flag: device int, set to 1 when an integer min /
   max / range cell had nothing to look at (may be NULL).
   Asynchronous on `stream`; allocates nothing and does not synchronise.  ws: svt_dev_rowstats_ws_bytes_op() bytes
   for this (operand, opcode, inner): the table of run bounds, which mean / var1 / sd1 build once for their two or
   three passes, plus their sums, NA counts and center, which never leave the device ("Workspaces" above).
   Status: > 0 for more than 65535 output columns with an added operation or a NaArray operand; < 0 for an added
   operation other than SVT_OP_RANGE on a NaArray operand and for any / all on doubles.
   One device: the caller shards. */
size_t svt_dev_rowstats_ws_bytes_op(const svt_dev_csc *A, int opcode, int64_t inner);
int svt_dev_rowstats(const svt_dev_csc *A, int opcode, int na_rm, const double *center, int64_t inner,
		     void *out, int *warn_flag, void *ws, size_t ws_bytes, void *stream);

/* Which form one pass of svt_dev_rowstats() / svt_dev_rowsums() takes for an operand of nrow x ncol leaves with `nnz`
   nonzeros (what svt_dev_csc says of it).  A pure host query, the function the launchers call:
     0  pipelined whole-column kernel over (output column, chunk of 64 leaves) units
     1  pipelined whole-column kernel, one output column at a time
     2  whole-column kernel (all rows of an output column in LDS)
     3  row panels in LDS behind the table of run bounds; *panel_shift = log2 of the rows per panel, *nsplit = the
        ranges the strata are cut into (cells then added to a zeroed `out`)
     4  memory atomics (more than 65535 output columns)
   opcode: an operation served in one pass.  SVT_OP_MEAN, _VAR1 and _SD1 queue the passes SVT_OP_COUNTNAS (na_rm),
   SVT_OP_SUM and SVT_OP_CENTERED_X2_SUM: ask for those.  panel_shift and nsplit may be NULL; they are 0 and 1 for
   the other forms. */
int svt_dev_rowstats_form(int64_t nrow, int64_t ncol, int64_t nnz, int na_background, int opcode, int64_t inner,
			  int *panel_shift, int64_t *nsplit);

/* rowsum(): out (ngroup x ncol, zeroed by the callee); group is a device
   array of nrow 1-based group ids (NA -> last group).  f64 input only at
   this level. */
int svt_dev_rowsum(const svt_dev_csc *A, const int *group, int ngroup,
		   int na_rm, double *out, void *stream);
/* The same for an (operand, grouping) pair used more than once: svt_dev_rowsum_prepare() writes the group of
   every nonzero -- a 16-bit 0-based id, NA -> the last group (src/rowsum_methods.c:51-54) -- into `gid`
   (svt_dev_rowsum_gid_bytes(A) bytes, device memory); svt_dev_rowsum_prepared() then streams 10 bytes per
   nonzero (value + id) and looks nothing up.  1 <= ngroup <= 20480 (a column's sums live in LDS).  `gid` is a
   workspace in the sense of "Workspaces" above; svt_dev_rowsum_prepared() is not told its size. */
size_t svt_dev_rowsum_gid_bytes(const svt_dev_csc *A);
int svt_dev_rowsum_prepare(const svt_dev_csc *A, const int *group, int ngroup, void *gid, size_t gid_bytes,
			   void *stream);
int svt_dev_rowsum_prepared(const svt_dev_csc *A, const void *gid, int ngroup, int na_rm, double *out,
			    void *stream);

/* Which kernels the three calls above launch.  Pure host queries (no device, no handle), the functions the launchers
   call; for tests and fuzzers that must know which kernel they exercise.
   svt_dev_rowsum_form(): the form of svt_dev_rowsum() -- and of svt_rowsum_SVT and svt_rowsum_dgCMatrix, which end in
   the same launcher -- for an nrow x ncol operand of `nnz` nonzeros and values of type Rtype; col_ptr32 != 0: the
   offsets are the int32 'p' slot of a dgCMatrix.
     0  memory atomics, a wavefront per column: integers, int32 offsets, more than 8192 groups, or columns shorter
        than a quarter of the groups on average (nnz / ncol < ngroup / 4, both quotients truncated)
     1  a workgroup per column, sums in LDS, the int group table                       (fewer than 65536 rows)
     2  the same behind a 16-bit copy of the table          (fewer than 64 columns, or more than 5120 groups)
     3  windowed: *cols_per_wg columns (a wavefront each) per workgroup walk the rows *window_rows at a time, their
        sums -- cols_per_wg * ngroup * 8 bytes, at most 160 KiB -- in LDS
   *cols_per_wg is 0 for the forms 0 to 2; *window_rows is the same for every operand.  Both may be NULL.
   svt_dev_rowsum_prepare_form(): 0 two ids per thread (fewer than 65536 rows or 64 columns, 65535 groups), 1 the walk
   of form 3 above with *cols_per_wg (8 to 16) columns per workgroup.
   svt_dev_rowsum_prepared_form(): 0 and *cols_per_wg (1 to 16; 1 to 3 for more than 5120 groups), or 1 for a shape
   svt_dev_rowsum_prepared() refuses (more than 20480 groups). */
int svt_dev_rowsum_form(int64_t nrow, int64_t ncol, int64_t nnz, int ngroup, int Rtype, int col_ptr32,
			int *cols_per_wg, int64_t *window_rows);
int svt_dev_rowsum_prepare_form(int64_t nrow, int64_t ncol, int64_t nnz, int ngroup, int *cols_per_wg);
int svt_dev_rowsum_prepared_form(int64_t ncol, int ngroup, int *cols_per_wg);

/* Thread control (C_get_num_procs / C_get_max_threads / C_set_max_threads,
   src/thread_control.c:47-66; R/thread-control.R sets the team size around every
   .Call and restores it).  The device kernels have no thread team to size: the
   library reports the host's processor count, remembers the value it is given
   and returns the previous one, so SparseArray.Call() keeps working unchanged.
   No HIP call is made. */
int svt_get_num_procs(void);
int svt_get_max_threads(void);
int svt_set_max_threads(int nthread);

/* t(A) for a 2-d operand, CSC -> CSC (device counterpart of transpose_2D_SVT,
   src/SparseArray_aperm.c:148-423; every `%*%` / tcrossprod starts with it,
   R/SparseMatrix-mult.R:165-206).  The caller provides the output arrays
   (out_col_ptr int64[nrow+1], out_row_idx int32[nnz], out_val like A's) and
   svt_dev_transpose_ws_bytes() bytes of workspace; entries of every output leaf
   come out in ascending offset order.
   Operands of 2^31 nonzeros or more take the boxed driver: runs of consecutive columns of at
   most 2^30 nonzeros (or one column) are transposed one after the other by the routes below the
   limit and copied to their place -- bit for bit the result of the unboxed routes.  The cuts
   between boxes are found by a search over the offsets and read back: such a call synchronises
   the stream once.  Its workspace grows with nrow and the box size, not with nnz. */
size_t svt_dev_transpose_ws_bytes(int64_t nrow, int64_t nnz);
int svt_dev_transpose(const svt_dev_csc *A, int64_t *out_col_ptr, int32_t *out_row_idx,
		      void *out_val, void *ws, size_t ws_bytes, void *stream);
/* Alignment and workspace, for svt_dev_transpose() and svt_dev_aperm() alike: "Workspaces" above; the outputs are the
   three arrays at the sizes given above. */
/* Which form svt_dev_transpose() takes for an nrow x ncol operand of nnz nonzeros (nslab = 1), or the step "first
   two axes change places" of svt_dev_aperm() for nslab matrices of nrow x ncol holding nnz nonzeros in all
   (nslab > 1) -- the decision of the launch itself, by the same functions.  Host only: no launch, no device needed.
     out[0]  1: the bucketed form (count, scatter, finish); 0: the key sort (t()) / another route (aperm)
     out[1]  fbits: a fine bucket is 2^fbits rows (0 .. 6)        out[2]  cbits: 2^cbits fine buckets per coarse one (4, 5)
     out[3]  nfb: fine buckets per matrix                          out[4]  ncoarse: coarse buckets per matrix
     out[5]  ngroups: groups of 256 columns per matrix
     out[6]  8-bit passes of the key sort over the row index, ceil(bits(nrow) / 8)
     out[7]  why not: 0 taken; 1 the shape rule refuses (out[1..5] are then -1, -1, 0, 0, 0); 2 the shape rule
             accepts, but the tables of the form need more than the workspace of t() sets aside for them
   Returns 0, or -1 for a NULL `out` or nslab < 1. */
int svt_dev_transpose_plan(int64_t nrow, int64_t ncol, int64_t nnz, int64_t nslab, int64_t out[8]);
/* Box limit of the transposition and of the aperm that moves the rows, process-wide (tests, timing):
   n > 0 sends every such operand of more than n nonzeros through the boxed driver with boxes of at
   most n nonzeros (or one column / one index of the axis that becomes the rows); n <= 0 restores the
   default (boxes only from 2^31 nonzeros on, of at most 2^30 for t(), 2^28 for aperm).
   Leaf-preserving permutations are never boxed.  Every call reads it once; a workspace sized under
   another setting may be too small (the call says so). */
void svt_dev_set_box_nnz(int64_t n);
/* Calls of this process that took a boxed driver (t(), and through it rowMedians, tcrossprod,
   %*% ...; aperm: once per call); reset != 0 zeroes the count and returns the count before. */
int64_t svt_dev_boxed_calls(int reset);

/* x %*% y for two sparse operands, y much sparser than a dense matrix (the `svt %*% svt2` of BASELINE config 3):
   out[r + k * ldo] = sum over the nonzeros (j, b) of column k of B of b * A[r, j] -- for finite operands the sum
   the reference forms per cell (C_crossprod2_SVT_SVT on t(x), src/SparseMatrix_mult.c:1037-1101: one operand's
   leaves expanded, the other's walked over them, :728-820), without the order of its additions (the same
   products, added as the lane groups get to them; exact for integer operands below 2^53).  A non-finite
   value or an NA in either operand changes what the reference computes (its dirty-leaf loops multiply the
   implicit zeros too): then `*not_finite` (device int, may be NULL; the second int of `ws` holds the same flag)
   is set and `out` must be recomputed by the dense route (svt_matmul_SVT_SVT does; a launch that finds the flag
   up already leaves `out` alone).  Otherwise every cell of the A->nrow x B->ncol result is written; ws:
   svt_dev_matmul_csc_csc_ws_bytes(A) bytes ("Workspaces" above).  A result without cells has a flag of 0.  Asynchronous.
   What depends on A alone -- the table of run bounds and a look at all its values, one pass over the operand --
   can be done once per operand: svt_dev_matmul_csc_csc_prepare(A, ws) fills `ws`, which
   svt_dev_matmul_csc_csc_prepared() then only reads (plus its second int, the flag of the last product), as the
   panel-blocked layout serves crossprod(A, Y).  svt_dev_matmul_csc_csc() does the same work for ONE product and
   less of it: its table pass looks only at the leaves of A that no column of B refers to, the product kernel at
   every value it reads (all of B, the other leaves of A); the `ws` it leaves is not a prepared one. */
size_t svt_dev_matmul_csc_csc_ws_bytes(const svt_dev_csc *A);
int svt_dev_matmul_csc_csc(const svt_dev_csc *A, const svt_dev_csc *B, double *out, int64_t ldo,
			   void *ws, size_t ws_bytes, int *not_finite, void *stream);
int svt_dev_matmul_csc_csc_prepare(const svt_dev_csc *A, void *ws, size_t ws_bytes, void *stream);
int svt_dev_matmul_csc_csc_prepared(const svt_dev_csc *A, const svt_dev_csc *B, double *out, int64_t ldo,
				    void *ws, size_t ws_bytes, int *not_finite, void *stream);

/* crossprod(X, Y) for two sparse operands without a dense buffer (round 6; kernels_gram.hip):
   out[c + j * ldo] = sum over the rows r where X[r, c] and Y[r, j] are both nonzero of X[r, c] * Y[r, j] -- for
   finite operands the cell C_crossprod2_SVT_SVT / C_crossprod1_SVT form (src/SparseMatrix_mult.c:1037-1140: one
   operand's leaves expanded into a dense buffer, ALL leaves of the other walked over it, :728-887; K11-K13
   :263-296), without the multiply-adds against the buffer's zeros and without the order of its additions
   (exact for integer operands below 2^53).
     Xt    t(X) in the device layout (svt_dev_transpose): Xt->nrow = ncol(X), Xt->ncol = nrow(X) leaves.
     Y     nrow(X) x ncol(Y).
     sym   != 0: Y is X (Xt = t(Y)), the unary crossprod(x): the cells c <= j are formed and mirrored
           (compute_sym_dotprods_*, :827-873, writes out[k] and out[k * ncol] from one dot product).
   A non-finite value or an NA anywhere in either operand changes what the reference computes (its dirty-leaf
   loops multiply the implicit zeros too): `*not_finite` (device int, may be NULL; the first int of `ws` holds
   the same flag) is set and `out` must come from the dense-buffer route (svt_crossprod2_SVT_SVT /
   svt_crossprod1_SVT do that; a launch that finds the flag up leaves `out` alone).  A result without cells
   (ncol(X) or ncol(Y) == 0) has a flag of 0.  ws: svt_dev_crossprod_csc_csc_ws_bytes(Xt) bytes ("Workspaces" above),
   sized under the panel setting of the call.  Asynchronous. */
size_t svt_dev_crossprod_csc_csc_ws_bytes(const svt_dev_csc *Xt);
int svt_dev_crossprod_csc_csc(const svt_dev_csc *Xt, const svt_dev_csc *Y, int sym, double *out, int64_t ldo,
			      void *ws, size_t ws_bytes, int *not_finite, void *stream);
/* Results up to `one_block_max` cells tall (<= 20400, the default: 160 KB of LDS; two workgroups per CU up to 10200
   cells; the symmetric form stops at 16384) keep a whole result column in one workgroup's LDS; taller ones are
   cut into panels of 2^log2_panel (<= 14; default 13) cells.  Negative / out-of-range arguments restore the
   defaults.  Process-wide; tests and tuning (workspaces sized before a change may be too small after it). */
void svt_dev_crossprod_csc_csc_set_panel(int one_block_max, int log2_panel);

/* The dense-buffer route of the same product on resident operands -- the reference's own form (one operand
   densified 128 or more columns at a time, the panel / general product kernels against each chunk; the Lpp / Rpp
   choice of src/SparseMatrix_mult.c:1077-1097; Y == X, the same handle: the unary form, ncol^2 / 2 dot products
   + mirror): what the host entry points fall back to when an operand is not finite, and the yardstick the
   sparse-aware kernel is measured against.  out: ncol(X) x ncol(Y) doubles, column-major (device).  Allocates
   its buffers and synchronises the device: not for a launch path. */
int svt_dev_crossprod_csc_csc_dense_buffer(const svt_dev_csc *X, const svt_dev_csc *Y, double *out);

/* Route choice of svt_crossprod2_SVT_SVT / svt_crossprod1_SVT: the sparse-aware kernel above is taken when its
   estimated time -- pairs of nonzeros that meet in a row (nnz(x) * nnz(y) / nrow, half of it for the unary form)
   at the measured gather rate, plus t(x) -- times `factor` is below that of the dense-buffer route (the reference's
   own Lpp_nops / Rpp_nops count of multiply-adds, src/SparseMatrix_mult.c:1077-1078, at the measured rate of the
   panel kernels).  factor < 0: never; 0: always; default 1.  Process-wide. */
void svt_sparse_crossprod_set_cost(double factor);

/* aperm(x, perm) for an N-d operand (C_aperm_SVT, src/SparseArray_aperm.c:935-970;
   R/SparseArray-aperm.R).  `dim` are the array's ndim extents (dim[0] = A->nrow,
   prod(dim[1..]) = A->ncol), `perm` is 1-based as in R.  Output: the CSC layout of
   the permuted array, prod(dim[perm[1..]]) + 1 column pointers and A->nnz entries
   (caller-allocated); 1 <= ndim <= 8.  Asynchronous on `stream`, except for permutations whose new
   leading axis is an old outer axis and whose second axis is the old rows (aperm(x, c(3, 1, 2))): the
   choice between the per-slab kernel and the key sort reads one counter back and synchronises the
   stream once.
   Every permutation is taken at every nonzero count.  Leaf-preserving permutations (perm[1] == 1) count
   positions in 64 bits.  The others, on an operand of 2^31 nonzeros or more (or past svt_dev_set_box_nnz),
   take the boxed driver: with q = perm[1] the old axis that becomes the rows, ranges of indices of axis q of
   at most 2^28 nonzeros (or one index) are gathered, permuted one after the other by the routes below the
   limit and copied to their place -- bit for bit the result of the unboxed routes (perm = c(2, 1): the boxed
   t()).  Such a call synchronises the stream once for its cuts, and wherever a box's own route does (the
   slab form).  It answers > 0 only when the permuted array has 2^31 - 1 leaves or more.
   Workspace: svt_dev_aperm_perm_ws_bytes() is the need of one permutation (what svt_dev_aperm() checks);
   svt_dev_aperm_ws_bytes() is at least the need of every permutation of `dim`, and the same value for both
   whenever the boxed driver is not taken.  Past the limit the boxed need does not grow with nnz (route area at
   the box size, two box-sized temporaries, O(leaves of the result + dim[q] + nnz / box)), and that of a
   leaf-preserving permutation is the scratch of one scan over the leaf counts. */
size_t svt_dev_aperm_ws_bytes(int64_t nnz, int ndim, const int64_t *dim);
size_t svt_dev_aperm_perm_ws_bytes(int64_t nnz, int ndim, const int64_t *dim, const int *perm);
int svt_dev_aperm(const svt_dev_csc *A, int ndim, const int64_t *dim, const int *perm,
		  int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val,
		  void *ws, size_t ws_bytes, void *stream);
/* How many transpositions / permutations of this process took which route (diagnostics; the differential fuzzers
   print it): counts[0] t() bucketed, [1] t() by the key sort, [2] aperm leaf-preserving, [3] first two axes swapped,
   [4] slab form, [5] 3-d through an intermediate, [6] general (composed), [7] key sort with 32-bit keys, [8] key sort
   with 64-bit keys, [9] slab form refused at run time.  Steps of composed routes count too.  reset != 0 zeroes them. */
void svt_dev_aperm_route_counts(int64_t counts[10], int reset);

/* Host level: same, on host buffers (x->nleaves leaves in, out_* as above with
   nnz = sum of x->nzcount). */
int svt_aperm_SVT(const svt_view *x, const int *perm, int64_t *out_col_ptr,
		  int32_t *out_row_idx, void *out_val);
/* C_transpose_2D_SVT, src/SparseArray_aperm.c:395-423 (t() of an SVT_SparseMatrix,
   R/SparseArray-aperm.R:11-20; every tcrossprod() and the non-native row*() statistics start
   with it, R/SparseMatrix-mult.R:165-206, R/SparseArray-matrixStats.R:140-147): x is uploaded,
   transposed on the device (svt_dev_transpose) and t(x) comes back as its CSC layout --
   x->dim[0] + 1 column pointers and sum(x->nzcount) entries, ascending offsets inside every
   leaf.  The glue rebuilds the R leaves from it (integration/svt_hip_glue.c). */
int svt_transpose_2D_SVT(const svt_view *x, int64_t *out_col_ptr,
			 int32_t *out_row_idx, void *out_val);

/* x[i, j] of a 2-D operand by an N-index (C_subset_SVT_by_Nindex, src/SparseArray_subsetting.c:223-297, 759-843):
   result cell (p, q) is x[i[p], j[q]]; indices in any order, any number of times; an entry is stored in the result
   exactly when its source entry is stored, and its value is copied bit for bit; offsets ascend inside every result
   column; Rtype and na_background pass through.  Not offered: N-d operands.  (Subassignment x[i, j] <- value, and
   subsetting and subassignment by an L-index or M-index: at the end of this header.)

   Device level, two primitives over tiles of svt_dev_subset_tile() nonzeros (kernels_subset.hip), each a `_count`
   call that writes the result's column pointers and returns its nonzero count, and a `_fill` call into arrays the
   caller sized from it.  Subscripts are device arrays of 0-based int32.
     column gather  out column q = column cols[q] of A.  out_col_ptr int64[ncols_sel + 1]; out_row_idx int32[*out_nnz],
                    out_val like A's.  ncols_sel <= 2^31 - 2; *out_nnz may exceed 2^31 (repeats) and A->nnz.
     row filter     `rows` strictly increasing: the entries of those rows, row rows[p] renumbered p.  out_col_ptr
                    int64[A->ncol + 1].  The fill call reads the workspace as the count call left it (the same A).
   A `_count` call launches on `stream` and synchronises it once, to return *out_nnz and read the validation flag; a
   `_fill` call is asynchronous.  `_count` answers 0; < 0 for an index outside [0, extent) or a workspace below
   svt_dev_subset_*_ws_bytes(); > 0 (rows) for a subscript in range that is not strictly increasing -- the caller
   then takes t(), the column gather with the row subscript, t().  Every index is checked before it is used as an
   address; on < 0 and > 0 nothing is written outside `ws` (out_col_ptr and *out_nnz keep their contents).
   ncols_sel == 0 writes out_col_ptr[0] = 0 without a launch or a synchronisation; an operand without nonzeros has its
   subscripts checked all the same.  Alignment and workspace: "Workspaces" above. */
int svt_dev_subset_tile(void);
size_t svt_dev_subset_cols_ws_bytes(int64_t ncols_sel);
int svt_dev_subset_cols_count(const svt_dev_csc *A, const int32_t *cols, int64_t ncols_sel, int64_t *out_col_ptr,
			      int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream);
int svt_dev_subset_cols_fill(const svt_dev_csc *A, const int32_t *cols, int64_t ncols_sel, const int64_t *out_col_ptr,
			     int32_t *out_row_idx, void *out_val, void *stream);
size_t svt_dev_subset_rows_ws_bytes(int64_t nrow, int64_t ncol, int64_t nnz);
int svt_dev_subset_rows_count(const svt_dev_csc *A, const int32_t *rows, int64_t nrows_sel, int64_t *out_col_ptr,
			      int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream);
int svt_dev_subset_rows_fill(const svt_dev_csc *A, const int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val,
			     const void *ws, size_t ws_bytes, void *stream);
/* The composition x[rows, cols] (the one statement of it; svt_subset_SVT_begin and DeviceCSC.subset both call it):
   the column gather first, then the rows by the filter, or, when the filter answers > 0, by t() -> gather -> t()
   (svt_dev_transpose as it is).  nrows_sel / ncols_sel < 0: the whole axis (the pointer is not read); both < 0: a copy.
   Results, intermediates and workspaces come from `alloc(bytes, ctx)` -- device memory aligned to 256 bytes, NULL on
   failure -- and go back through `release(p, ctx)`, which may be called while work on `stream` that uses the block is
   still queued (a stream-ordered allocator, or one that waits like hipFree).  The three result arrays (*out_col_ptr
   int64[ncol' + 1]; *out_row_idx, *out_val of at least one element) are the caller's to release.  Synchronises
   `stream` once per count call; the last fill / transposition is still queued on return.  < 0: a bad index. */
typedef void *(*svt_dev_alloc_fn)(size_t bytes, void *ctx);
typedef void (*svt_dev_free_fn)(void *p, void *ctx);
int svt_dev_subset(const svt_dev_csc *A, const int32_t *rows, int64_t nrows_sel, const int32_t *cols, int64_t ncols_sel,
		   svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int64_t *out_nnz,
		   int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val, void *stream);
/* counts[0] column gathers, [1] row filters, [2] general-row compositions (each also counts its one gather) of this
   process, counted where the work is launched (the fill calls); reset != 0 zeroes them. */
void svt_dev_subset_route_counts(int64_t counts[3], int reset);

/* Host level.  `rows` / `cols`: 1-based as an N-index arrives, or NULL for the whole axis.  begin checks the
   subscripts on the host (NA_INTEGER or an index outside 1..extent: < 0, before anything is uploaded), uploads x
   (through the resident cache when it is on), runs svt_dev_subset and leaves the result on the device: *out_nnz is
   its nonzero count, its extents are the subscripts' lengths.  end copies it into out_col_ptr int64[ncol' + 1],
   out_row_idx int32[nnz], out_val (x's type) and releases it; all three NULL: release only.  NaArray operands are
   taken; ndim != 2 answers > 0.  Runs on the first device of the list (not sharded). */
typedef struct svt_subset_result svt_subset_result;
int svt_subset_SVT_begin(const svt_view *x, const int *rows, int64_t nrows_sel, const int *cols, int64_t ncols_sel,
			 svt_subset_result **res, int64_t *out_nnz);
int svt_subset_SVT_end(svt_subset_result *res, int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val);

/* Arith and Math on SVT operands (C_Arith_SVT1_SVT2, C_Arith_SVT1_v2, C_unary_minus_SVT, C_Math_SVT;
   R/SparseArray-Arith-methods.R, R/SparseArray-Math-methods.R; the element rules of src/SparseVec_Arith.c and
   src/SparseVec_Math.c): the result is a new sparse operand in the device layout.  Two families (kernels_arith.hip):

     merge  x op y, op one of SVT_ARITH_ADD / _SUB / _MULT, for two operands of the same nrow and the same number of
            leaves (N-d operands are leaves x rows), each REALSXP or INTSXP.  At every position stored in x or in y the
            value is op(x or 0, y or 0) in the result's type, and it is stored unless it == 0 (-0.0 and integer 0 too;
            NaN, NA and +-Inf stay -- which is what `*` against an implicit zero keeps).  A stored zero of an operand is
            an ordinary value.  int op int is int: computed in double, a result <= INT_MIN or > INT_MAX is NA_integer_
            and raises the overflow flag, NA_integer_ propagates.  With a double side the result is double and
            NA_integer_ becomes NA_real_.
     map    f(v) on the stored values of one operand, stored unless f(v) == 0.  kind SVT_ARITH_SCALAR: x op s, op one of
            _MULT _DIV _POW _MOD _IDIV with the scalar s of type s_Rtype (an INTSXP s is passed as its double value);
            / and ^ give double, an INTSXP x with an INTSXP s stays int (overflow as above; %% takes the sign of the
            divisor, %/% floors), anything else is computed in double by R's rules for the operators.  kind
            SVT_ARITH_NEG: -x, the type kept.  kind SVT_ARITH_MATH: one of SVT_MATH_ABS .. SVT_MATH_EXPM1 on a REALSXP
            operand; SVT_MATH_SIN .. SVT_MATH_SIGNIF (the rest of the reference's list) answer > 0.

   Both cut their work into tiles of svt_dev_arith_tile() entries (of x for the map, of the merged sequence of
   x->nnz + y->nnz entries for the merge), place every result entry by 64-bit prefix sums, keep the rows ascending
   inside every result column and give the same bits on every run.  `_count` writes out_col_ptr int64[ncol + 1], returns
   *out_nnz and synchronises `stream` once; `_fill` is asynchronous, reads the workspace as the count call left it
   (same operands, same operation), writes out_row_idx int32[*out_nnz] and out_val (svt_dev_arith_out_Rtype()), and ORs
   1 into the device word `ovflow` (may be NULL) when an integer result overflowed.  Status: < 0 for extents that
   differ, a workspace below svt_dev_arith_*_ws_bytes(), an unknown kind or opcode or one the family does not take, an
   LGLSXP operand, a Math operation on an INTSXP operand; > 0 for an operand with na_background (the reference has
   separate NaArray methods) and for the Math operations listed above.  On a non-zero status nothing is written outside
   `ws`.  Alignment and workspace: "Workspaces" above. */
enum { SVT_ARITH_ADD = 1, SVT_ARITH_SUB = 2, SVT_ARITH_MULT = 3, SVT_ARITH_DIV = 4, SVT_ARITH_POW = 5, SVT_ARITH_MOD = 6,
       SVT_ARITH_IDIV = 7 };
enum { SVT_MATH_ABS = 1, SVT_MATH_SIGN = 2, SVT_MATH_SQRT = 3, SVT_MATH_FLOOR = 4, SVT_MATH_CEILING = 5, SVT_MATH_TRUNC = 6,
       SVT_MATH_LOG1P = 7, SVT_MATH_EXPM1 = 8,
       SVT_MATH_SIN = 9, SVT_MATH_ASIN = 10, SVT_MATH_SINH = 11, SVT_MATH_ASINH = 12, SVT_MATH_SINPI = 13, SVT_MATH_TAN = 14,
       SVT_MATH_ATAN = 15, SVT_MATH_TANH = 16, SVT_MATH_ATANH = 17, SVT_MATH_TANPI = 18, SVT_MATH_ROUND = 19,
       SVT_MATH_SIGNIF = 20 };
enum { SVT_ARITH_MERGE = 0, SVT_ARITH_SCALAR = 1, SVT_ARITH_NEG = 2, SVT_ARITH_MATH = 3 };
int svt_dev_arith_tile(void);
/* SVT_INTSXP or SVT_REALSXP: the type of the result; 0 for a combination no family takes.  y_Rtype: the second
   operand's or the scalar's type (not read for _NEG and _MATH).  Needs no GPU. */
int svt_dev_arith_out_Rtype(int kind, int op, int x_Rtype, int y_Rtype);
size_t svt_dev_arith_merge_ws_bytes(int64_t ncol, int64_t x_nnz, int64_t y_nnz);
int svt_dev_arith_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int op, int64_t *out_col_ptr, int64_t *out_nnz,
			      void *ws, size_t ws_bytes, void *stream);
int svt_dev_arith_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, int op, const int64_t *out_col_ptr,
			     int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, size_t ws_bytes, void *stream);
size_t svt_dev_arith_map_ws_bytes(int64_t ncol, int64_t nnz);
int svt_dev_arith_map_count(const svt_dev_csc *x, int kind, int op, double s, int s_Rtype, int64_t *out_col_ptr,
			    int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream);
int svt_dev_arith_map_fill(const svt_dev_csc *x, int kind, int op, double s, int s_Rtype, const int64_t *out_col_ptr,
			   int32_t *out_row_idx, void *out_val, int *ovflow, const void *ws, size_t ws_bytes, void *stream);
/* The compositions count -> allocate -> fill, one per family, over the allocator of svt_dev_subset(): the workspace
   comes from `alloc` and goes back through `release`; the three result arrays (*out_col_ptr int64[ncol + 1];
   *out_row_idx, *out_val of at least one element, *out_Rtype their type) are the caller's to release.  `ovflow`: a
   device word the caller zeroed, or NULL.  Synchronise `stream` once; the fill is still queued on return. */
int svt_dev_arith_merge(const svt_dev_csc *x, const svt_dev_csc *y, int op, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
			void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx,
			void **out_val, int *ovflow, void *stream);
int svt_dev_arith_map(const svt_dev_csc *x, int kind, int op, double s, int s_Rtype, svt_dev_alloc_fn alloc,
		      svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr,
		      int32_t **out_row_idx, void **out_val, int *ovflow, void *stream);

/* Host level.  begin uploads the operand(s) (through the resident cache when it is on), runs the composition on the
   first device of the list (not sharded) and leaves the result on the device: *out_Rtype its type, *out_nnz its
   nonzero count, *ovflow set to 1 when an integer result overflowed ("NAs produced by integer overflow": the caller
   warns); its extents are x's.  svt_Arith_SVT_end copies it into out_col_ptr int64[nleaves + 1], out_row_idx
   int32[nnz], out_val and releases it; all three NULL: release only.  The dims of x and y must be identical (< 0:
   "non-conformable arrays").  What the R methods check before the call (the operations that would not stay sparse, the
   scalar's value) is the caller's business: the library computes what it is asked.  `digits` of svt_Math_SVT_begin is
   read by SVT_MATH_ROUND / _SIGNIF only, which answer > 0. */
typedef struct svt_arith_result svt_arith_result;
int svt_Arith_SVT_SVT_begin(const svt_view *x, const svt_view *y, int op, svt_arith_result **res, int *out_Rtype,
			    int64_t *out_nnz, int *ovflow);
int svt_Arith_SVT_scalar_begin(const svt_view *x, int op, double s, int s_Rtype, svt_arith_result **res, int *out_Rtype,
			       int64_t *out_nnz, int *ovflow);
int svt_unary_minus_SVT_begin(const svt_view *x, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz);
int svt_Math_SVT_begin(const svt_view *x, int op, double digits, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz);
int svt_Arith_SVT_end(svt_arith_result *res, int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val);

/* Sparse x sparse products with a SPARSE result (kernels_spgemm.hip): C = A %*% B, A m x n and B n x K resident 2-D
   operands of REALSXP or INTSXP, C an m x K operand of REALSXP in the device layout.  svt_dev_matmul_csc_csc() is the
   same product with a dense result; this one serves the product whose dense form cannot exist (1e6 x 1e4 at 1 % times
   a 1e4 x 1e4 matrix with a few nonzeros per column: 80 GB dense, a few GB sparse) and the chain that stays on the
   device (product -> sweep -> log1p -> colVars without a densification).

   The rule.  For every cell (i, k) the value is the sum, in ASCENDING ORDER OF THE INNER INDEX j, of
   (double) A[i, j] * (double) B[j, k] over the j where A stores an entry at (i, j) AND B stores one at (j, k); the
   accumulator starts from +0.0, each product is rounded and then added (no fused multiply-add), an integer value is
   converted as Arith converts it (NA_integer_ becomes NA_real_).  A cell is stored exactly when at least one such pair
   meets in it and the sum is not == 0: -0.0 and a sum that cancels are dropped, a NaN stays, a stored zero of an operand
   is an ordinary value (the rule of Arith above).  For finite operands the result is the dense product made sparse;
   two runs give the same bits; the count pass and the fill pass form the same sums, so a cancellation cannot make
   them disagree about the number of nonzeros.

   `*not_finite` (device int32, may be NULL) is set to 1 when ANY stored value of A or of B is NaN, +-Inf, NA_real_ or
   NA_integer_ -- all stored values, not only those a pair reads: there the reference's %*% multiplies the implicit
   zeros too -- and to 0 otherwise.  The result is written completely under the rule either way; with the flag up its
   dense form may differ from the reference's answer, with the flag down the two agree cell for cell.

   The work is cut into items (result column, panel of svt_dev_spgemm_panel(nrow) rows of A); result positions are
   64-bit prefix sums over the items, nnz(C) may exceed 2^31, rows ascend inside every result column.  `_count` writes
   out_col_ptr int64[K + 1] (all zeros for an empty result) and *not_finite, returns *out_nnz and synchronises `stream`
   once; `_fill` is asynchronous, takes the same operands on the workspace the count call left and writes out_row_idx
   int32[*out_nnz] and out_val double[*out_nnz].  Status, each answered before anything is written: < 0 for extents that
   do not conform ("non-conformable arguments"), a workspace below svt_dev_spgemm_ws_bytes() ("workspace too small"),
   an LGLSXP operand or any other type; > 0 for an operand with na_background, for B with 2^31 - 1 nonzeros or more
   (the limit of svt_dev_matmul_csc_csc), for more items than one launch takes and for an LDS request the device
   refuses.  Alignment and workspace: "Workspaces" above.  svt_dev_spgemm() is the composition count -> allocate -> fill
   over the allocator of svt_dev_subset(), like svt_dev_arith_merge: the workspace comes from `alloc` and goes back
   through `release`, the three result arrays (*out_col_ptr int64[K + 1]; *out_row_idx, *out_val of at least one
   element) are the caller's to release; one synchronisation of `stream`, the fill still queued on return. */
int svt_dev_spgemm_panel(int64_t nrow);
size_t svt_dev_spgemm_ws_bytes(const svt_dev_csc *A, int64_t K);
int svt_dev_spgemm_count(const svt_dev_csc *A, const svt_dev_csc *B, int64_t *out_col_ptr, int64_t *out_nnz, void *ws,
			 size_t ws_bytes, int *not_finite, void *stream);
int svt_dev_spgemm_fill(const svt_dev_csc *A, const svt_dev_csc *B, const int64_t *out_col_ptr, int32_t *out_row_idx,
			double *out_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_spgemm(const svt_dev_csc *A, const svt_dev_csc *B, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx,
		   int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, double **out_val, int *not_finite,
		   void *stream);
/* Host level: x %*% y (tr_x = tr_y = 0), crossprod(x, y) (tr_x != 0: t(x) %*% y) and tcrossprod(x, y) (tr_y != 0:
   x %*% t(y)) of two 2-D operands of REALSXP or INTSXP, each with its own type.  begin uploads the operands (through the
   resident cache when it is on), transposes on the device where asked, runs svt_dev_spgemm on the first device of the
   list (not sharded) and leaves the REALSXP result on the device: *out_nnz its nonzero count, *not_finite (host) the
   flag above; its extents are those of the product.  svt_Arith_SVT_end copies it out and releases it.  < 0: an operand
   that is not 2-D ("input objects must have 2 dimensions"), of another type or a NaArray, extents that do not conform
   ("non-conformable arguments"); > 0: what the device call refuses. */
int svt_matmul_SVT_SVT_sparse_begin(const svt_view *x, const svt_view *y, int tr_x, int tr_y, svt_arith_result **res,
				    int64_t *out_nnz, int *not_finite);

/* Compare and Logic on SVT operands (C_Compare_SVT1_SVT2, C_Compare_SVT1_v2, C_Logic_SVT1_SVT2;
   R/SparseArray-Compare-methods.R, R/SparseArray-Logic-methods.R; the element rules of src/SparseVec_Compare.c and
   src/SparseVec_Logic.c): the result is a new LGLSXP operand in the device layout, its values int32 1 or NA_integer_.
   They are further rules on the two kernel families of Arith (kernels_arith.hip), with the same tiles, the same
   placement and the same workspaces: svt_dev_arith_merge_ws_bytes() sizes the workspace of the two merges,
   svt_dev_arith_map_ws_bytes() that of the map.

     compare merge  x op y, op one of SVT_COMPARE_NE / _LT / _GT (the three that are FALSE where both sides are zero),
                    each operand LGLSXP, INTSXP or REALSXP (an LGLSXP operand is an int32 operand).  Both sides are
                    taken as doubles, NA_integer_ as NA_real_; a NaN or NA on either side gives NA, which is stored.
     compare map    x op s for any of the six operators and a scalar s of type s_Rtype (LGLSXP, INTSXP, REALSXP; an
                    integer or logical s is passed as its double value, INT_MIN standing for NA), provided 0 op s is
                    FALSE: x == 0, x >= 0, x < 1, a NaN or NA s and the like answer < 0, because the result would not
                    be sparse and computing the stored positions alone would be silently wrong.
     logic merge    x & y, x | y for two LGLSXP operands, by the three-valued tables.

   At every position stored in x or in y the value is rule(x or 0, y or 0); it is stored unless it is 0 (FALSE).  A
   stored zero of an operand is an ordinary value.  The count / fill contract is that of svt_dev_arith_*: `_count`
   writes out_col_ptr int64[ncol + 1] and *out_nnz and synchronises `stream` once; `_fill` is asynchronous, reads the
   workspace as the count call left it and writes out_row_idx int32[*out_nnz] and out_val int32[*out_nnz]; rows ascend
   in every result column; two runs give the same bits; there is no overflow word.  Status: < 0 for extents that
   differ, a workspace too small, an unknown opcode, a merge Compare with an op other than != < >, a map Compare whose
   scalar makes 0 op s anything but FALSE, Logic with an operand that is not LGLSXP, an operand or scalar type outside
   logical / integer / double; > 0 for an operand with na_background.  On a non-zero status nothing is written outside
   `ws`: out_col_ptr and *out_nnz keep their contents.  Alignment and workspace: "Workspaces" above. */
enum { SVT_COMPARE_EQ = 1, SVT_COMPARE_NE = 2, SVT_COMPARE_LE = 3, SVT_COMPARE_GE = 4, SVT_COMPARE_LT = 5,
       SVT_COMPARE_GT = 6 };
enum { SVT_LOGIC_AND = 1, SVT_LOGIC_OR = 2 };
int svt_dev_compare_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int op, int64_t *out_col_ptr, int64_t *out_nnz,
				void *ws, size_t ws_bytes, void *stream);
int svt_dev_compare_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, int op, const int64_t *out_col_ptr,
			       int32_t *out_row_idx, int32_t *out_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_compare_map_count(const svt_dev_csc *x, int op, double s, int s_Rtype, int64_t *out_col_ptr, int64_t *out_nnz,
			      void *ws, size_t ws_bytes, void *stream);
int svt_dev_compare_map_fill(const svt_dev_csc *x, int op, double s, int s_Rtype, const int64_t *out_col_ptr,
			     int32_t *out_row_idx, int32_t *out_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_logic_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int op, int64_t *out_col_ptr, int64_t *out_nnz,
			      void *ws, size_t ws_bytes, void *stream);
int svt_dev_logic_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, int op, const int64_t *out_col_ptr,
			     int32_t *out_row_idx, int32_t *out_val, const void *ws, size_t ws_bytes, void *stream);
/* The compositions count -> allocate -> fill over the allocator of svt_dev_subset(), like svt_dev_arith_merge: the
   result arrays (*out_col_ptr int64[ncol + 1]; *out_row_idx, *out_val int32 of at least one element) are the caller's
   to release.  Synchronise `stream` once; the fill is still queued on return. */
int svt_dev_compare_merge(const svt_dev_csc *x, const svt_dev_csc *y, int op, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
			  void *ctx, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, int32_t **out_val,
			  void *stream);
int svt_dev_compare_map(const svt_dev_csc *x, int op, double s, int s_Rtype, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
			void *ctx, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, int32_t **out_val,
			void *stream);
int svt_dev_logic_merge(const svt_dev_csc *x, const svt_dev_csc *y, int op, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
			void *ctx, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, int32_t **out_val,
			void *stream);

/* Host level, like svt_Arith_*_begin: the operands go up (through the resident cache when it is on), the composition
   runs on the first device of the list, the result (LGLSXP, the extents of x) stays on the device and *out_nnz is its
   nonzero count.  The existing svt_Arith_SVT_end ends it, with int32 values.  The dims of x and y must be identical
   (< 0: "non-conformable arrays").  Not offered: NaArray operands (> 0), character / raw / complex operands, == <= >=
   between two arrays, dense-array operands. */
int svt_Compare_SVT_SVT_begin(const svt_view *x, const svt_view *y, int op, svt_arith_result **res, int64_t *out_nnz);
int svt_Compare_SVT_scalar_begin(const svt_view *x, int op, double s, int s_Rtype, svt_arith_result **res, int64_t *out_nnz);
int svt_Logic_SVT_SVT_begin(const svt_view *x, const svt_view *y, int op, svt_arith_result **res, int64_t *out_nnz);

/* sweep(x, MARGIN, STATS, op): Arith and Compare between a sparse operand and a device vector that holds one element
   per row, per leaf, or per row of a group of leaves -- t(t(x) / colSums(x)), x * gene_weights (R's recycling of a
   vector of length nrow), sweep(x, 1, q, ">").  The reference has no method: it refuses every vector of length != 1.  A
   third kernel family next to the map and the merge (kernels_arith.hip):

     sweep  f(v, stats[k]) on the stored values of x, stored unless the result == 0, where for an entry of row r in
            leaf q   k = (with_rows ? r : 0) + (with_rows ? nrow : 1) * ((q / stride) % len).
            with_rows 1, stride 1, len 1: one element per row.  with_rows 0, stride 1, len ncol: one per leaf (the
            columns of a matrix, and what colSums(x, dims = 1) of an N-d array returns).  For the N-d array of extents
            dim[] (dim[0] == nrow) and a run of consecutive dimensions a..b (1-based): with_rows = (a == 1),
            stride = prod(dim[1 .. a-2]) (0-based; 1 when a <= 2), len = prod of the run's extents without dimension 1;
            `stats` is then the column-major array of the run's extents.  stats_len must be (with_rows ? nrow : 1) * len.

   Arith takes op one of SVT_ARITH_MULT / _DIV / _POW / _MOD / _IDIV (_ADD and _SUB answer < 0: the result wouldn't be
   sparse in general), x INTSXP or REALSXP, stats INTSXP or REALSXP (device int32 / double); the result's type is
   svt_dev_arith_out_Rtype(SVT_ARITH_SCALAR, op, x->Rtype, stats_Rtype), integer overflow gives NA_integer_ and ORs 1
   into `ovflow`.  Compare takes the six operators, x and stats LGLSXP, INTSXP or REALSXP, and gives int32 1 /
   NA_integer_.  Both evaluate the element rules of the maps.

   Every element of `stats` must keep the result sparse, and the count call checks that on the device before anything
   else runs: for * not NA / NaN and finite; for / %% %/% not NA / NaN and != 0; for ^ not NA / NaN and > 0; for Compare
   not NA / NaN and 0 op s FALSE.  On an element that does not, the call answers < 0, *bad_index is the smallest such
   index (0-based; -1 otherwise; bad_index may be NULL) and nothing is written outside `ws`.

   Apart from that the contract is that of svt_dev_arith_map* / svt_dev_compare_map*: `_count` writes out_col_ptr
   int64[ncol + 1] and *out_nnz and synchronises `stream` once (the refused element is read in that same
   synchronisation); `_fill` is asynchronous and reads the workspace as the count call left it; rows ascend in every
   result column; no atomic decides a position; two runs give the same bits.  Status: < 0 for a vector whose length
   does not match the three integers, integers that do not divide the operand's leaves, a workspace below
   svt_dev_sweep_ws_bytes(), an unknown opcode, a type outside the above; > 0 for an operand with na_background.  On a
   non-zero status nothing is written outside `ws`.  Alignment and workspace: "Workspaces" above. */
size_t svt_dev_sweep_ws_bytes(int64_t ncol, int64_t nnz);
int svt_dev_arith_sweep_count(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
			      int with_rows, int64_t stride, int64_t len, int64_t *out_col_ptr, int64_t *out_nnz,
			      int64_t *bad_index, void *ws, size_t ws_bytes, void *stream);
int svt_dev_arith_sweep_fill(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
			     int with_rows, int64_t stride, int64_t len, const int64_t *out_col_ptr, int32_t *out_row_idx,
			     void *out_val, int *ovflow, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_compare_sweep_count(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
				int with_rows, int64_t stride, int64_t len, int64_t *out_col_ptr, int64_t *out_nnz,
				int64_t *bad_index, void *ws, size_t ws_bytes, void *stream);
int svt_dev_compare_sweep_fill(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
			       int with_rows, int64_t stride, int64_t len, const int64_t *out_col_ptr, int32_t *out_row_idx,
			       int32_t *out_val, const void *ws, size_t ws_bytes, void *stream);
/* The compositions count -> allocate -> fill over the allocator of svt_dev_subset(), like svt_dev_arith_map and
   svt_dev_compare_map. */
int svt_dev_arith_sweep(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len, int with_rows,
			int64_t stride, int64_t len, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx,
			int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val,
			int *ovflow, int64_t *bad_index, void *stream);
int svt_dev_compare_sweep(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len, int with_rows,
			  int64_t stride, int64_t len, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx,
			  int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, int32_t **out_val,
			  int64_t *bad_index, void *stream);
/* Host level, like svt_Arith_SVT_scalar_begin / svt_Compare_SVT_scalar_begin: `stats` is a host vector of stats_len
   elements of stats_Rtype, `margin` names nmargin dimensions of x (1-based, a strictly increasing run of consecutive
   dimensions; anything else answers < 0) and the three integers are derived from x->dim.  The result stays on the
   device and svt_Arith_SVT_end ends it.  First device of the list; not sharded.  NaArray operands answer > 0. */
int svt_Arith_SVT_vector_begin(const svt_view *x, int op, const void *stats, int64_t stats_len, int stats_Rtype,
			       const int *margin, int nmargin, int64_t *bad_index, svt_arith_result **res, int *out_Rtype,
			       int64_t *out_nnz, int *ovflow);
int svt_Compare_SVT_vector_begin(const svt_view *x, int op, const void *stats, int64_t stats_len, int stats_Rtype,
				 const int *margin, int nmargin, int64_t *bad_index, svt_arith_result **res, int64_t *out_nnz);

/* pmin() / pmax() and is.na() / is.nan() / is.infinite() on SVT operands (.pminmax2 and .isFUN_SVT,
   R/SparseArray-misc-methods.R; C_SVT_apply_isFUN): further rules on the three kernel families of Arith
   (kernels_arith.hip; the element rules svt_rule_pminmax and svt_rule_isfun of svt_arith_rules.h), with the same tiles,
   the same 64-bit placement and the same workspaces: svt_dev_arith_merge_ws_bytes() sizes the workspace of the merge,
   svt_dev_arith_map_ws_bytes() that of the two maps, svt_dev_sweep_ws_bytes() that of the sweep.

   `op` of the pminmax calls is SVT_PMINMAX_MIN or SVT_PMINMAX_MAX, ORed with SVT_PMINMAX_NA_RM for na.rm = TRUE; any
   other value answers < 0.  Both sides are widened to the result's type svt_dev_pminmax_out_Rtype() -- the wider of
   logical < integer < double; NA_integer_ becomes NA_real_ -- and the result is, without na.rm,
   isna(x) ? x : isna(y) ? y : (y < x ? y : x) (pmax: y > x), with it isna(y) ? x : isna(x) ? y : the same; isna is NaN
   or NA_real_ for a double, NA_integer_ else; ties take x; the chosen side's bits are returned unchanged.

     pminmax merge  two operands of the same nrow and the same number of leaves, each LGLSXP, INTSXP or REALSXP.  At
                    every position stored in x or in y the value is rule(x or 0, y or 0); it is stored unless it == 0
                    (-0.0 and integer 0 too; a NaN or NA stays).  A stored zero of an operand is an ordinary value.
     pminmax map    pmin(x, s) / pmax(x, s) for a scalar s of type s_Rtype (an integer or logical s is passed as its
                    double value, INT_MIN standing for NA), provided pmin(0, s) == 0: s not NA / NaN, and >= 0 for pmin,
                    <= 0 for pmax; any other s answers < 0.  With na.rm an NA entry of x becomes s.
     pminmax sweep  the same rule as f(v, stats[k]), the vector and its geometry as in svt_dev_arith_sweep; every
                    element must satisfy the scalar's condition, the first that does not is named in *bad_index and
                    nothing is written outside `ws`.
     isfun map      op SVT_IS_NA, SVT_IS_NAN or SVT_IS_INFINITE on the stored values of an LGLSXP, INTSXP or REALSXP
                    operand: a new LGLSXP operand that stores int32 1 where the function is TRUE.  is.na is ISNAN for a
                    double and NA_integer_ else; is.nan a NaN that is not NA_real_; is.infinite +-Inf; the last two are
                    FALSE everywhere on an integer or logical operand (base R's answer).

   The count / fill / composition contract is that of svt_dev_arith_* and svt_dev_compare_*: `_count` writes out_col_ptr
   int64[ncol + 1] and *out_nnz and synchronises `stream` once; `_fill` is asynchronous, reads the workspace as the
   count call left it (same operands, same operation) and writes out_row_idx int32[*out_nnz] and out_val; rows ascend in
   every result column; no atomic decides a position; two runs give the same bits; there is no overflow word.  Status:
   < 0 for extents that differ, a workspace too small, an unknown opcode, a type outside logical / integer / double, a
   scalar or vector element that does not keep the result sparse; > 0 for an operand with na_background.  On a non-zero
   status nothing is written outside `ws`.  Alignment and workspace: "Workspaces" above. */
enum { SVT_PMINMAX_MIN = 1, SVT_PMINMAX_MAX = 2, SVT_PMINMAX_NA_RM = 4 };
enum { SVT_IS_NA = 1, SVT_IS_NAN = 2, SVT_IS_INFINITE = 3 };
/* SVT_LGLSXP, SVT_INTSXP or SVT_REALSXP: the wider of the two types; 0 when either is none of them.  Needs no GPU. */
int svt_dev_pminmax_out_Rtype(int x_Rtype, int y_Rtype);
int svt_dev_pminmax_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int op, int64_t *out_col_ptr, int64_t *out_nnz,
				void *ws, size_t ws_bytes, void *stream);
int svt_dev_pminmax_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, int op, const int64_t *out_col_ptr,
			       int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_pminmax_map_count(const svt_dev_csc *x, int op, double s, int s_Rtype, int64_t *out_col_ptr, int64_t *out_nnz,
			      void *ws, size_t ws_bytes, void *stream);
int svt_dev_pminmax_map_fill(const svt_dev_csc *x, int op, double s, int s_Rtype, const int64_t *out_col_ptr,
			     int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_pminmax_sweep_count(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
				int with_rows, int64_t stride, int64_t len, int64_t *out_col_ptr, int64_t *out_nnz,
				int64_t *bad_index, void *ws, size_t ws_bytes, void *stream);
int svt_dev_pminmax_sweep_fill(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len,
			       int with_rows, int64_t stride, int64_t len, const int64_t *out_col_ptr, int32_t *out_row_idx,
			       void *out_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_isfun_map_count(const svt_dev_csc *x, int op, int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes,
			    void *stream);
int svt_dev_isfun_map_fill(const svt_dev_csc *x, int op, const int64_t *out_col_ptr, int32_t *out_row_idx, int32_t *out_val,
			   const void *ws, size_t ws_bytes, void *stream);
/* The compositions count -> allocate -> fill over the allocator of svt_dev_subset(), like svt_dev_arith_merge and
   svt_dev_compare_map: the result arrays are the caller's to release, *out_Rtype is the type of *out_val.  Synchronise
   `stream` once; the fill is still queued on return. */
int svt_dev_pminmax_merge(const svt_dev_csc *x, const svt_dev_csc *y, int op, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
			  void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx,
			  void **out_val, void *stream);
int svt_dev_pminmax_map(const svt_dev_csc *x, int op, double s, int s_Rtype, svt_dev_alloc_fn alloc, svt_dev_free_fn release,
			void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx,
			void **out_val, void *stream);
int svt_dev_pminmax_sweep(const svt_dev_csc *x, int op, const void *stats, int stats_Rtype, int64_t stats_len, int with_rows,
			  int64_t stride, int64_t len, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx,
			  int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val,
			  int64_t *bad_index, void *stream);
int svt_dev_isfun_map(const svt_dev_csc *x, int op, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx,
		      int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, int32_t **out_val, void *stream);
/* Host level, like svt_Arith_*_begin and svt_Compare_*_begin: the operands go up (through the resident cache when it is
   on), the composition runs on the first device of the list (not sharded), the result (the extents of x) stays on the
   device: *out_Rtype its type (LGLSXP for svt_isFUN_SVT_begin), *out_nnz its nonzero count.  svt_Arith_SVT_end ends
   it.  The dims of x and y must be identical (< 0: "non-conformable arrays"); NaArray operands answer > 0.  `margin` of
   the vector form as in svt_Arith_SVT_vector_begin.  The vector form has no counterpart in the reference and is one more
   than the two-operand, the scalar and the isFUN forms need: it is what a host-level sweep(x, MARGIN, STATS, pmin) calls,
   as svt_Arith_SVT_vector_begin is for the Arith operators. */
int svt_pminmax_SVT_SVT_begin(const svt_view *x, const svt_view *y, int op, svt_arith_result **res, int *out_Rtype,
			      int64_t *out_nnz);
int svt_pminmax_SVT_scalar_begin(const svt_view *x, int op, double s, int s_Rtype, svt_arith_result **res, int *out_Rtype,
				 int64_t *out_nnz);
int svt_pminmax_SVT_vector_begin(const svt_view *x, int op, const void *stats, int64_t stats_len, int stats_Rtype,
				 const int *margin, int nmargin, int64_t *bad_index, svt_arith_result **res, int *out_Rtype,
				 int64_t *out_nnz);
int svt_isFUN_SVT_begin(const svt_view *x, int op, svt_arith_result **res, int64_t *out_nnz);

/* abind(), cbind() and rbind() of SVT operands (C_abind_SVT_SparseArray_objects, src/SparseArray_abind.c;
   R/SparseArray-abind.R, R/NaArray-abind.R): nobj >= 1 objects bound along dimension `along` (1-based) into a new
   operand in the device layout, leaves x rows with the outermost dimension slowest.  A pure copy (kernels_abind.hip).

     along the rows (along == 1; concatenate_leaves, :129-181)  every object has the same number of leaves; result leaf L
            is leaf L of object 0, then of object 1, ...; the rows of object n are shifted by off[n] = the nrow of the
            objects before it, so rows stay ascending; the result's nrow is the sum, at most 2^31 - 1.
     along a leaf dimension (along >= 2; concatenate_SVTs and the recursion, :94-125, 186-230)  every object has the same
            nrow.  inner = prod(dim[1 .. along-2]), ext[n] = object n's extent along the binding dimension, start[n] = the
            ext of the objects before it, D = their sum, outer = the product of the dimensions after it (the same for
            every object: ncol_n == inner * ext[n] * outer).  Result leaf q = a + inner * (j + D * c) is leaf
            a + inner * ((j - start[n]) + ext[n] * c) of the object n whose [start[n], start[n] + ext[n]) holds j.
            cbind of matrices is inner == outer == 1; a new trailing dimension is ext[n] == 1 with outer == 1.

   In both forms an entry is stored in the result exactly when its source entry is stored (a stored zero stays
   stored), in the source's order.  ans_Rtype, the result's type, is at least the widest of logical < integer < double
   over the objects (the R method coerces every object to it before the call; here the copy widens): a value whose
   object has the result's type is copied bit for bit, logical -> integer leaves the bits as they are, integer or
   logical -> double converts the value and NA_integer_ becomes NA_real_.  NaArray operands (na_background) are taken
   when ALL objects have it, and the result has it.  Allowed, and never a launch over an empty range: nobj == 1 (a copy
   that may widen), objects without nonzeros, objects of extent 0 along the binding dimension, a result without leaves.
   Not offered: COO objects, binding with a dense array, deparse.level, sharding over the device list, an entry in the
   R glue (integration/svt_hip_glue.c binds neither this nor subset nor Arith; INTEGRATION.md describes the call).

   Device level.  `objs`: a host array of nobj handles.  `ext`: a host array of the nobj extents along the binding
   dimension, or NULL for the rows form (`inner` is then not read).  The result is cut into pieces, each a whole leaf
   of one object (out_nleaves * nobj of them in the rows form, out_nleaves else); svt_dev_abind_count writes
   out_col_ptr int64[out_nleaves + 1] and *out_nnz and synchronises `stream` once; svt_dev_abind_fill is asynchronous,
   takes the same operands, reads the workspace as the count call left it and writes out_row_idx int32[*out_nnz] and
   out_val (ans_Rtype) in tiles of svt_dev_abind_tile() result entries; two runs give the same bits.  Status < 0,
   answered on the host before anything is launched or written: nobj < 1, a NULL object, an ans_Rtype that is not
   logical / integer / double or is narrower than an object's type, objects with and without na_background, leaf
   counts that differ (rows form), nrow that differ or an ncol_n that is not inner * ext[n] * outer for one outer (leaf
   form), rows that sum past 2^31 - 1, more than 2^31 - 2 pieces, a workspace below svt_dev_abind_ws_bytes(nobj,
   out_nleaves, rows_form).  Also < 0, found by the count kernels: an object whose col_ptr descends or passes its nnz
   (nothing is read through it).  On a non-zero status nothing is written outside `ws`: out_col_ptr and *out_nnz keep
   their contents.  Alignment and workspace: "Workspaces" above. */
int svt_dev_abind_tile(void);
size_t svt_dev_abind_ws_bytes(int nobj, int64_t out_nleaves, int rows_form);
int svt_dev_abind_count(const svt_dev_csc *const *objs, int nobj, int64_t inner, const int64_t *ext, int ans_Rtype,
			int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream);
int svt_dev_abind_fill(const svt_dev_csc *const *objs, int nobj, int64_t inner, const int64_t *ext, int ans_Rtype,
		       const int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes,
		       void *stream);
/* The composition count -> allocate -> fill over the allocator of svt_dev_subset(): the workspace comes from `alloc`
   and goes back through `release`; *out_nrow and *out_nleaves are the result's extents, its type is ans_Rtype, and the
   three result arrays (*out_col_ptr int64[*out_nleaves + 1]; *out_row_idx, *out_val of at least one element) are the
   caller's to release.  Synchronises `stream` once (not at all for a result without leaves); the fill is still queued
   on return. */
int svt_dev_abind(const svt_dev_csc *const *objs, int nobj, int64_t inner, const int64_t *ext, int ans_Rtype,
		  svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int64_t *out_nrow, int64_t *out_nleaves,
		  int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val, void *stream);

/* Host level.  `objs`: nobj views of the same number of dimensions.  begin checks `along` and the dims on the host, with
   the messages of the C entry point ("'along' must be >= 1 and <= the number of dimensions of the objects to bind",
   "all the objects to bind must have the same number of dimensions") and, for extents that differ off the binding
   dimension, "all the objects to bind must have the same extent along dimension <k> (they are bound along dimension
   <along>)"; uploads the objects (through the resident cache when it is on), runs svt_dev_abind on the first device of
   the list (not sharded) and leaves the result on the device: *out_nnz is its nonzero count, its type is ans_Rtype,
   its dims are those of the objects with the extents summed along `along`.  The existing svt_Arith_SVT_end copies it
   into out_col_ptr int64[nleaves + 1], out_row_idx int32[nnz], out_val and releases it. */
int svt_abind_SVT_begin(const svt_view *const *objs, int nobj, int along, int ans_Rtype, svt_arith_result **res,
			int64_t *out_nnz);

/* Coercion between a dense array and a resident operand, and nzwhich() (as(a, "SVT_SparseArray") =
   C_build_SVT_from_Rarray, as.array(x) = C_from_SVT_SparseArray_to_Rarray, nzwhich(x, arr.ind=) = C_nzwhich_SVT,
   src/SVT_SparseArray_class.c; kernels_coerce.hip).  The dense array is a device buffer in R's layout: column-major,
   nrow = dim[0] rows, nleaves = prod(dim[1:]) leaves, no padding between the leaves; its type is double, integer or
   logical (logical is int32).  In this layout CSC order is flat cell order, so the three are streaming passes over
   tiles of svt_dev_coerce_tile() cells or entries, and what a workgroup does does not depend on how the cells are cut
   into leaves.  The element rules are stated once, in sparsearray_amd/csrc/svt_coerce_rules.h.

     keep rule (collect_offsets_of_nonzero_* / collect_offsets_of_nonNA_*, src/Rvector_utils.c:556-594)  a cell is stored
            when it is != 0: -0.0 and integer 0 are dropped; a NaN, NA_real_, +-Inf, a subnormal and NA_integer_ are
            stored.  Under na_background a cell is stored when it is not NA: R_IsNA for a double (the NaN whose low word
            is 1954; a plain NaN is stored), NA_integer_ for an integer or a logical; zeros are stored.
     type   the result's type is the source's or a wider one, logical < integer < double: the same type moves bit for
            bit, logical -> integer leaves the bits as they are, integer or logical -> double converts the value and
            NA_integer_ becomes NA_real_ (the rule of abind).  A narrower type answers > 0: the reference coerces with
            warnings, this library does not.

   Dense -> sparse is a stream compaction over the flat cell index: the position of a kept cell is its rank among the
   kept cells, out_col_ptr[q] the rank at cell q * nrow.  svt_dev_from_dense_count writes out_col_ptr int64[nleaves + 1]
   and *out_nnz and synchronises `stream` once; it leaves in `ws` the tile bases and one bit per cell.
   svt_dev_from_dense_fill is asynchronous, takes the same operands, reads the workspace as the count call left it (the
   array is not tested again) and writes out_row_idx int32[*out_nnz] and out_val (ans_Rtype).  Every position is a 64-bit
   prefix sum, none is decided by an atomic, two runs give the same bits.  Status < 0, answered on the host before
   anything is launched or written (out_col_ptr and *out_nnz keep their contents): a type that is not logical / integer
   / double, nrow < 0 or nleaves < 0, nrow > 2^31 - 1, nrow * nleaves past int64, a workspace below
   svt_dev_from_dense_ws_bytes(nrow * nleaves).  Allowed, and never a launch over an empty range: nrow == 0 (every
   pointer is 0) and nleaves == 0 (out_col_ptr[0] = 0); neither synchronises.  Alignment and workspace: "Workspaces"
   above.

   svt_dev_from_dense is the composition count -> allocate -> fill over the allocator of svt_dev_subset(): the workspace
   comes from `alloc` and goes back through `release`; the three result arrays (*out_col_ptr int64[nleaves + 1];
   *out_row_idx, *out_val of at least one element) are the caller's to release.  Synchronises `stream` once; the fill is
   still queued on return.

   Sparse -> dense.  svt_dev_to_dense writes EVERY cell of out[A->nrow * A->ncol] (out_Rtype, column-major, aligned to 16
   bytes): the background -- zero, or NA of out_Rtype when na_background != 0; a parameter, because a wrapped operand
   carries none -- and the stored values, by the type rule, at q * nrow + row_idx.  Asynchronous, no workspace, no launch
   when the output has no cells.  A workgroup owns consecutive tiles of output cells, builds each in LDS and writes it
   out once.  The operand is not trusted: the col_ptr of the leaves a tile touches are checked before any is followed
   (one that descends or passes A->nnz: the tile gets the background alone), and an entry whose row is outside [0, nrow)
   or whose cell lies before its tile is never used as an address; either raises the device word *bad (int32, only ever
   set to nonzero, like `ovflow` of Arith; may be NULL), which stays on the device so that the call remains
   asynchronous.  (Rows are looked at where the walk over a leaf's entries meets them; with the rows of every leaf
   ascending, which the layout promises, that is every entry.)

   svt_dev_nzwhich.  `dim`: a host array of ndim (1 .. 8) extents with dim[0] == nrow and prod(dim[1:]) == ncol (< 0
   otherwise, on the host) and at most 2^31 - 1 leaves (< 0 past that, on the host: a tile numbers the leaves it touches
   in 32 bits; the entries and the linear indices are 64-bit).  arr_ind == 0: out int64[nnz], the 0-based linear index leaf * nrow + row of every stored
   entry in storage order (nzwhich_SVT_as_Lindex less the + 1; 64-bit where the reference switches to doubles past
   INT_MAX).  arr_ind != 0: out int32[nnz * ndim], column-major, the 0-based coordinate tuples of
   extract_nzcoo_and_nzvals_from_SVT; with nnz > INT_MAX < 0, "too many nonzero elements in SVT_SparseArray object to
   return their "array coordinates" (n-tuples) in a matrix".  Asynchronous, no launch for nnz == 0.  A stored zero is an
   entry like any other.  nzvals is the val array and nzcount is nnz: neither needs a call.

   Not offered: host-level entry points and R glue (uploading a dense array costs more than the reference's loop over
   it: the value is on resident data), narrowing coercions, type<- (C_set_SVT_type), COO -> SVT (it needs a sort),
   dgCMatrix / CSC conversions, float32, character / raw / complex types, sharding over the device list, a dense array
   with a leading dimension larger than nrow. */
int svt_dev_coerce_tile(void);
size_t svt_dev_from_dense_ws_bytes(int64_t ncells);
int svt_dev_from_dense_count(const void *x, int x_Rtype, int64_t nrow, int64_t nleaves, int ans_Rtype, int na_background,
			     int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream);
int svt_dev_from_dense_fill(const void *x, int x_Rtype, int64_t nrow, int64_t nleaves, int ans_Rtype, int na_background,
			    const int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val, const void *ws, size_t ws_bytes,
			    void *stream);
int svt_dev_from_dense(const void *x, int x_Rtype, int64_t nrow, int64_t nleaves, int ans_Rtype, int na_background,
		       svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int64_t *out_nnz, int64_t **out_col_ptr,
		       int32_t **out_row_idx, void **out_val, void *stream);
int svt_dev_to_dense(const svt_dev_csc *A, int na_background, int out_Rtype, void *out, int *bad, void *stream);
int svt_dev_nzwhich(const svt_dev_csc *A, int ndim, const int64_t *dim, int arr_ind, void *out, void *stream);

/* Random count arrays: poissonSparseArray(dim, lambda) and simple_rpois(n, lambda) (C_poissonSparseArray and
   C_simple_rpois, src/randomSparseArray.c; kernels_coerce.hip).  Every cell of the array is drawn from Poisson(lambda)
   and the nonzeros are kept, as an integer operand.  On the device this is the compaction of svt_dev_from_dense_* with a
   generated cell in place of a loaded one: the same masks, tile bases, publish pass and workspace; the array of the
   cells never exists.  The rules are stated once, in sparsearray_amd/csrc/svt_random_rules.h.

     generator  Philox4x32-10 (Salmon et al., SC 2011).  cell = leaf * nrow + row, in 64 bits, counted in the WHOLE
            array; block = cell >> 1; counter = (lo32(block), hi32(block), 0, 0); key = (lo32(seed), hi32(seed)).  The
            even cell of a block takes the output words (w0, w1), the odd cell (w2, w3); x = w_hi << 32 | w_lo and
            u = (x >> 11) * 2^-53, in [0, 1).  Counter words 2 and 3 are reserved.
     value  find_interval of the reference: the first k with u < ticks[k], or the number of ticks when there is none.
     ticks  compute_cumsum_dpois of the reference, on the host in long double: at most 32 doubles, the cumulated
            probabilities, ascending.  Their NUMBER is the reference's for every lambda (its stopping rule on its own
            arithmetic, a double exp() and double quotients lambda / n: 18 ticks at lambda = 1, 31 at 4); their VALUES
            come from the same sum with both in long double, the true CDF rounded once, where the reference's own are
            up to 2 ulp off.  svt_poisson_ticks writes them to ticks32 (32 doubles; may be NULL) and returns their number:
            0 when every cell is 0 (lambda == 0, or exp(-lambda) rounds to 1); -1 when lambda is negative, NaN or
            infinite or when 32 ticks are not enough ("'lambda' too big?": every lambda of 4.5 and above, none up to 4).
            Needs no GPU.  The kernels get the table by value and call no exp.
     seed   `seed` carries the 64 bits of an unsigned seed (0 .. 2^64 - 1; a seed of 2^63 and above arrives as the
            negative int64_t of the same bits).  It stands in for R's global RNG state; R's streams are not reproduced.

   A cell is a pure function of (seed, cell), so the array does not depend on the tiling or the grid, two runs give the
   same bits, and `first_leaf` makes a call produce the leaves [first_leaf, first_leaf + nleaves) of a larger array of
   nrow rows: the windows of an array bound with svt_dev_abind ARE the array.

   The contract is that of svt_dev_from_dense_*.  svt_dev_poisson_count writes out_col_ptr int64[nleaves + 1] and
   *out_nnz and synchronises `stream` once; svt_dev_poisson_fill is asynchronous, takes the same operands, reads the
   workspace as the count call left it and writes out_row_idx int32[*out_nnz] and out_val int32[*out_nnz] (the value is
   made again only where the mask has a bit).  Every position is a 64-bit prefix sum and none is decided by an atomic.
   Status < 0, answered on the host before anything is launched or written: nrow, first_leaf or nleaves < 0, nrow >
   2^31 - 1, (first_leaf + nleaves) * nrow past int64, a workspace below svt_dev_poisson_ws_bytes(nrow * nleaves), a
   lambda for which svt_poisson_ticks answers -1.  Allowed, and never a launch over an empty range: nrow == 0 and
   nleaves == 0, as for svt_dev_from_dense_count.  svt_dev_poisson is the composition over the allocator of
   svt_dev_subset().  svt_dev_rpois writes out[i] = the value of cell first + i, i < n, int32: the dense form, asynchronous,
   no workspace; < 0 for n < 0 ("'n' cannot be negative"), first < 0, first + n past int64, a bad lambda.

   Host level.  svt_poissonSparseArray_begin runs svt_dev_poisson with first_leaf = 0 on the first device of the list
   (not sharded) and leaves the result on the device: *out_nnz is its nonzero count, its type is integer.  The existing
   svt_Arith_SVT_end copies it out and releases it.  svt_simple_rpois writes out[n] on the host.

   Not offered: randomSparseArray() (exactly floor(n * density) positions without replacement is a selection over all
   cells), a lambda per row or per column, a lambda above what 32 ticks resolve, sharding over the device list, an entry
   in the R glue. */
int svt_poisson_ticks(double lambda, double *ticks32);
size_t svt_dev_poisson_ws_bytes(int64_t ncells);
int svt_dev_poisson_count(double lambda, int64_t seed, int64_t nrow, int64_t first_leaf, int64_t nleaves, int64_t *out_col_ptr,
			  int64_t *out_nnz, void *ws, size_t ws_bytes, void *stream);
int svt_dev_poisson_fill(double lambda, int64_t seed, int64_t nrow, int64_t first_leaf, int64_t nleaves,
			 const int64_t *out_col_ptr, int32_t *out_row_idx, int32_t *out_val, const void *ws, size_t ws_bytes,
			 void *stream);
int svt_dev_poisson(double lambda, int64_t seed, int64_t nrow, int64_t first_leaf, int64_t nleaves, svt_dev_alloc_fn alloc,
		    svt_dev_free_fn release, void *ctx, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx,
		    void **out_val, void *stream);
int svt_dev_rpois(double lambda, int64_t seed, int64_t first, int64_t n, int32_t *out, void *stream);
int svt_poissonSparseArray_begin(int64_t nrow, int64_t nleaves, double lambda, int64_t seed, svt_arith_result **res,
				 int64_t *out_nnz);
int svt_simple_rpois(int64_t n, double lambda, int64_t seed, int32_t *out);

/* Subassignment x[i, j, ...] <- value by an N-index (.subassign_SVT_by_Nindex, R/SparseArray-subassignment.R:114-170;
   C_subassign_SVT_with_short_Rvector, src/SparseArray_subassignment.c:1005-1230): the result is a new operand in the
   device layout with x's extents.  Its type is the wider of x's and the value's, logical < integer < double; a value
   of that type moves bit for bit, integer or logical -> double converts and NA_integer_ becomes NA_real_.  A leaf is
   SELECTED when all its coordinates along dims 2..N are in the subscripts; a selected leaf is rebuilt from its dense
   form, so an entry is stored in it exactly when the final value is not zero (-0.0 and integer 0 count as zero, a NaN
   or NA does not, and a stored zero of x in it disappears even on a row outside i); every other leaf comes back
   untouched, stored zeros included.  An empty selection is a copy of x in the result's type.

     vector form  `vals`: nvals >= 1 values of v_Rtype.  The value of row subscript position p is vals[p % nvals], the
                  same in every selected leaf; positions apply in order, so the last occurrence of a row wins; repeats
                  among the leaves repeat the same assignment.  (The R method takes this form when length(value) <=
                  length(i) and length(i) %% length(value) == 0; the library recycles whatever it is given.)
     SVT form     `v`: an operand with the selection's extents (the reference's C_subassign_SVT_with_SVT is a stub).
                  `rows` strictly increasing or the whole axis, `leaves` without repeats, in any order: leaf leaves[q]
                  of the selection becomes leaf q of v with row r renamed rows[r].

   On the device layout this is a merge (kernels_subassign.hip, kernels_arith.hip).  A PLACEMENT builds an operand Y
   with x's extents that holds the new values which may have to be stored -- the non-zero values of the vector form,
   every stored entry of v -- and two COVER TABLES, one byte per row and one per leaf, non-zero where the subscripts
   reach.  The ASSIGN MERGE is one more rule on the merge kernels of Arith: at a place stored in Y the result is Y's
   value; at a place stored in x alone it is dropped when its row and its leaf are both covered, x's value otherwise;
   an entry is kept unless its leaf is covered and its value == 0.  So x[i, j] <- 0 builds an empty Y and costs one
   pass over nnz(x), whatever the size of the selection.

   Device level.  Subscripts are device arrays of 0-based int32, in any order and with repeats (vector form); a length
   < 0 stands for the whole axis and the pointer is not read.  svt_dev_subassign_place_*_count writes y_col_ptr
   int64[ncol + 1], cover_row uint8[nrow] and cover_leaf uint8[ncol] (a table may be NULL when its axis is whole: it is
   then not written, and NULL is what the merge takes for "the whole axis"), returns *y_nnz and synchronises `stream`
   once; svt_dev_subassign_place_*_fill is asynchronous, takes the same operands, reads the workspace as the count call
   left it and writes y_row_idx int32[y_nnz] and y_val (the value's type) in tiles of svt_dev_subassign_tile() entries.
   svt_dev_assign_merge_count / _fill follow svt_dev_arith_merge_count / _fill, with the workspace of
   svt_dev_arith_merge_ws_bytes(ncol, x->nnz, y->nnz); the result's type is the wider of x's and y's and there is no
   overflow word.  Every position is a 64-bit prefix sum and two runs give the same bits.  Status: < 0 for an index
   outside [0, extent) (every index is checked before it is used as an address), a workspace below
   svt_dev_subassign_place_ws_bytes(nrow, ncol) / svt_dev_arith_merge_ws_bytes(), nvals < 1 ("replacement has length
   zero"), a type outside logical / integer / double, extents of v that differ from the selection's ("the selection and
   supplied value must have the same dimensions"), extents of y that differ from x's; > 0 for an operand with
   na_background and, SVT form, for rows in range that are not strictly increasing or a repeated leaf.  On a non-zero
   status nothing is written outside `ws`.  Alignment and workspace: "Workspaces" above.

   Not offered: a dense array value, NaArray operands, the SVT form with rows out of
   order or repeated leaves, character / raw / complex types, sharding over the device list, an entry in the R glue
   (INTEGRATION.md describes the call). */
int svt_dev_subassign_tile(void);
size_t svt_dev_subassign_place_ws_bytes(int64_t nrow, int64_t ncol);
int svt_dev_subassign_place_vector_count(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel,
					 const int32_t *leaves, int64_t nleaves_sel, const void *vals, int64_t nvals, int v_Rtype,
					 int64_t *y_col_ptr, unsigned char *cover_row, unsigned char *cover_leaf, int64_t *y_nnz,
					 void *ws, size_t ws_bytes, void *stream);
int svt_dev_subassign_place_vector_fill(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel,
					const int32_t *leaves, int64_t nleaves_sel, const void *vals, int64_t nvals, int v_Rtype,
					const int64_t *y_col_ptr, int64_t y_nnz, int32_t *y_row_idx, void *y_val, const void *ws,
					size_t ws_bytes, void *stream);
int svt_dev_subassign_place_svt_count(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel,
				      const int32_t *leaves, int64_t nleaves_sel, const svt_dev_csc *v, int64_t *y_col_ptr,
				      unsigned char *cover_row, unsigned char *cover_leaf, int64_t *y_nnz, void *ws, size_t ws_bytes,
				      void *stream);
int svt_dev_subassign_place_svt_fill(int64_t nrow, int64_t ncol, const int32_t *rows, int64_t nrows_sel,
				     const int32_t *leaves, int64_t nleaves_sel, const svt_dev_csc *v, const int64_t *y_col_ptr,
				     int64_t y_nnz, int32_t *y_row_idx, void *y_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_assign_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, const unsigned char *cover_row,
			       const unsigned char *cover_leaf, int64_t *out_col_ptr, int64_t *out_nnz, void *ws, size_t ws_bytes,
			       void *stream);
int svt_dev_assign_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, const unsigned char *cover_row,
			      const unsigned char *cover_leaf, const int64_t *out_col_ptr, int32_t *out_row_idx, void *out_val,
			      const void *ws, size_t ws_bytes, void *stream);
/* The compositions place -> merge over the allocator of svt_dev_subset(): Y, the tables and the workspaces come from
   `alloc` and go back through `release`; the three result arrays (*out_col_ptr int64[ncol + 1]; *out_row_idx, *out_val
   of at least one element, *out_Rtype their type) are the caller's to release.  Synchronise `stream` twice (the two
   count calls), once for an empty selection (the one-object case of svt_dev_abind: a copy that may widen); the last
   fill is still queued on return. */
int svt_dev_subassign_vector(const svt_dev_csc *x, const int32_t *rows, int64_t nrows_sel, const int32_t *leaves,
			     int64_t nleaves_sel, const void *vals, int64_t nvals, int v_Rtype, svt_dev_alloc_fn alloc,
			     svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr,
			     int32_t **out_row_idx, void **out_val, void *stream);
int svt_dev_subassign_svt(const svt_dev_csc *x, const int32_t *rows, int64_t nrows_sel, const int32_t *leaves,
			  int64_t nleaves_sel, const svt_dev_csc *v, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx,
			  int *out_Rtype, int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val,
			  void *stream);

/* Host level.  `index`: x->ndim subscripts, 1-based as an N-index arrives, index[a] == NULL (or index == NULL) for the
   whole axis, index_len[a] their lengths.  begin checks them on the host (NA_INTEGER or an index outside 1..extent: < 0,
   "subscript contains out-of-bound indices or NAs", before anything is uploaded), expands those of dims 2..N into the
   leaf list (the outermost dimension slowest; at most 2^31 - 2 leaves), uploads x and the value (through the resident
   cache when it is on), runs the composition on the first device of the list (not sharded) and leaves the result on
   the device: *out_Rtype its type, *out_nnz its nonzero count, its dims are x's.  The existing svt_Arith_SVT_end copies
   it out and releases it.  `vals` is a host array of nvals values of v_Rtype; the dims of `v` must be the selection's.
   What the R method checks before the call (the value's class, its length against the selection) is the caller's. */
int svt_subassign_SVT_vector_begin(const svt_view *x, const int *const *index, const int64_t *index_len, const void *vals,
				   int64_t nvals, int v_Rtype, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz);
int svt_subassign_SVT_SVT_begin(const svt_view *x, const int *const *index, const int64_t *index_len, const svt_view *v,
				svt_arith_result **res, int *out_Rtype, int64_t *out_nnz);

/* Subsetting and subassignment by a linear index (L-index) or a matrix subscript (M-index): x[which(...)],
   x[cbind(i, j)], x[x > 10] <- 10 (.subset_SVT_by_Lindex / _by_Mindex, R/SparseArray-subsetting.R;
   .subassign_SVT_by_Lindex / _by_Mindex, R/SparseArray-subassignment.R; C_subset_SVT_by_Lindex,
   C_subassign_SVT_by_Lindex and subassign_leaf_by_OPBuf in the reference's src/).  An L-index over an N-d array is an
   L-index over the (nrow x nleaves) device layout: cell L is row L % nrow of leaf L / nrow; an M-index row is the cell
   sum(m_a * prod(dim[0 .. a-1])).  One device function turns either form into a checked cell number; no index is used as
   an address before that (kernels_lindex.hip).

   Device level.  An L-index is a device int64[K], 0-based, INT64_MIN for NA -- what svt_dev_nzwhich writes.  An M-index
   is a device int32[K * ndim], column-major and 0-based -- what svt_dev_nzwhich writes with arr_ind -- with `dim` a host
   array of ndim (1 .. 8) extents, dim[0] == nrow and prod(dim[1:]) == ncol (< 0 otherwise, on the host).  Where one
   function takes both forms, ndim == 0 says L-index (`dim` is then not read).

   Gather.  svt_dev_subset_lindex / _mindex write out[K] of A's type, one value per index in index order: the stored
   value bit for bit (a stored zero, -0.0 or a NaN payload as it is), else the background (0, or NA when
   A->na_background), and NA for an NA L-index.  One lookup per index: two col_ptr reads, then a binary search of row_idx
   between them.  Asynchronous, no workspace, nothing launched for K == 0.  `bad` is a device int32 word the caller
   zeroed, in the convention of svt_dev_to_dense: a first kernel checks every index and raises bit 1 for one outside the
   array (an NA_integer_ coordinate of an M-index included), and the gather, which reads the word, then writes nothing;
   bit 2: a col_ptr pair that descends or leaves [0, nnz] was not followed (that index reads the background).

   Subassignment.  The value is brought to the wider type of the two (logical < integer < double, NA_integer_ becomes
   NA_real_); positions apply in order, so the LAST occurrence of a cell wins; a cell whose final value is zero (-0.0 and
   integer 0 too; a NaN or NA is stored) has no entry afterwards; a cell that no index reaches keeps x's entry bit for
   bit, a stored zero included (the N-index form above rebuilds a selected leaf; this form does not).  It is a merge:
     placement  svt_dev_subassign_place_lindex_count / _fill build the placed operand Y with x's extents: one entry per
                DISTINCT assigned cell holding the cell's last value vals[p % nvals], zeros included -- a zero in Y is the
                deletion mark.  The count call checks every index (one outside the array, an NA included: < 0, and nothing
                was written outside `ws`), notes whether the cells are strictly increasing (the output of nzwhich() /
                which() always is) and synchronises `stream` once to learn both.  Sorted route: position p is entry p of
                Y, no sort, no de-duplication, *y_nnz = K without a second synchronisation.  Unsorted route: (cell, p)
                through the library's stable radix sort on the bits of nrow * ncol - 1 (svt_dev_lindex_sort_passes()
                passes of 8 bits), a flag per run end, a 64-bit scan; one more synchronisation for *y_nnz.  Either way
                y_col_ptr int64[ncol + 1] comes from one binary search per leaf.  The fill call is asynchronous and
                reads `ws` as the count call left it.  No atomic decides a position; two runs give the same bits.
                ws: svt_dev_subassign_place_lindex_ws_bytes(K, ncol), 44 bytes per index plus the sort's tables.
     merge      svt_dev_assign_cells_merge_count / _fill: the merge of svt_dev_arith_merge_* under the rule
                svt_rule_assign_cells -- at a place stored in y the result is y's value widened, kept iff it is not zero;
                at a place stored in x alone x's value widened, always kept.  No cover tables.  ws:
                svt_dev_arith_merge_ws_bytes(ncol, nnz(x), nnz(y)).
   svt_dev_subassign_lindex / _mindex are the composition over the allocator of svt_dev_subset(), like
   svt_dev_subassign_vector; K == 0 is the widening copy of x.  Status < 0: an index outside the array or NA, nvals < 1
   ("replacement has length zero"), a workspace smaller than its _ws_bytes, a type outside logical / integer / double;
   > 0: an operand with na_background, K > 2^31 - 1 (the sort's payload is 32 bits).  On a non-zero status nothing is
   written outside `ws`.  svt_dev_lindex_route_counts: counts[0] sorted, [1] unsorted placements of this process, counted
   in the count call; reset != 0 zeroes them.

   Not offered: NaArray subassignment, COO operands, character / raw / complex types, K >= 2^31 for the subassignment,
   sharding over the device list, an entry in the R glue. */
int svt_dev_subset_lindex(const svt_dev_csc *A, const int64_t *lindex, int64_t K, void *out, int *bad, void *stream);
int svt_dev_subset_mindex(const svt_dev_csc *A, const int32_t *mindex, int64_t K, int ndim, const int64_t *dim, void *out, int *bad,
			  void *stream);
size_t svt_dev_subassign_place_lindex_ws_bytes(int64_t K, int64_t ncol);
int svt_dev_lindex_sort_passes(int64_t nrow, int64_t ncol);
int svt_dev_subassign_place_lindex_count(int64_t nrow, int64_t ncol, const void *index, int64_t K, int ndim, const int64_t *dim,
					 const void *vals, int64_t nvals, int v_Rtype, int64_t *y_col_ptr, int64_t *y_nnz, void *ws,
					 size_t ws_bytes, void *stream);
int svt_dev_subassign_place_lindex_fill(int64_t nrow, int64_t ncol, const void *index, int64_t K, int ndim, const int64_t *dim,
					const void *vals, int64_t nvals, int v_Rtype, const int64_t *y_col_ptr, int64_t y_nnz,
					int32_t *y_row_idx, void *y_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_assign_cells_merge_count(const svt_dev_csc *x, const svt_dev_csc *y, int64_t *out_col_ptr, int64_t *out_nnz, void *ws,
				     size_t ws_bytes, void *stream);
int svt_dev_assign_cells_merge_fill(const svt_dev_csc *x, const svt_dev_csc *y, const int64_t *out_col_ptr, int32_t *out_row_idx,
				    void *out_val, const void *ws, size_t ws_bytes, void *stream);
int svt_dev_subassign_lindex(const svt_dev_csc *x, const int64_t *lindex, int64_t K, const void *vals, int64_t nvals, int v_Rtype,
			     svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int *out_Rtype, int64_t *out_nnz,
			     int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val, void *stream);
int svt_dev_subassign_mindex(const svt_dev_csc *x, const int32_t *mindex, int64_t K, int ndim, const int64_t *dim, const void *vals,
			     int64_t nvals, int v_Rtype, svt_dev_alloc_fn alloc, svt_dev_free_fn release, void *ctx, int *out_Rtype,
			     int64_t *out_nnz, int64_t **out_col_ptr, int32_t **out_row_idx, void **out_val, void *stream);
void svt_dev_lindex_route_counts(int64_t counts[2], int reset);

/* Host level.  `lindex`: K 1-based int64 cell numbers, INT64_MIN for NA; `mindex`: a K x x->ndim int matrix,
   column-major, 1-based, NA_INTEGER for NA.  Every index is checked on the host before anything is uploaded (< 0:
   "linear index (L-index) contains out-of-bound indices", "linear index (L-index) contains NAs" -- subassignment only; in
   a subsetting L-index an NA gives NA --, "matrix subscript (M-index) contains out-of-bound indices", "matrix subscript
   (M-index) contains NAs").  The subsetting calls upload x (through the resident cache when it is on), gather and
   download `out`: K values of x's type.  The subassignment calls leave the result on the device like
   svt_subassign_SVT_vector_begin, and svt_Arith_SVT_end ends them.  First device of the list; not sharded.  NaArray
   subassignment and character / raw / complex operands: > 0. */
int svt_subset_SVT_by_Lindex(const svt_view *x, const int64_t *lindex, int64_t K, void *out);
int svt_subset_SVT_by_Mindex(const svt_view *x, const int *mindex, int64_t K, void *out);
int svt_subassign_SVT_by_Lindex_begin(const svt_view *x, const int64_t *lindex, int64_t K, const void *vals, int64_t nvals,
				      int v_Rtype, svt_arith_result **res, int *out_Rtype, int64_t *out_nnz);
int svt_subassign_SVT_by_Mindex_begin(const svt_view *x, const int *mindex, int64_t K, const void *vals, int64_t nvals, int v_Rtype,
				      svt_arith_result **res, int *out_Rtype, int64_t *out_nnz);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_H */
