/*
 * gdhip.h -- C ABI of libgdhip.so: the MI355X (gfx950) implementation of GetDist's weighted-sample
 * statistics + 1D/2D kernel-density hot path.
 *
 * The reference (GetDist 1.7.7) is pure Python and has NO FFI seam for this path: every
 * entry point below replaces a span of numpy/scipy calls inside the reference's Python methods; the
 * span is cited as file:line under /root/reference/getdist/.  The binding a maintainer would add is a
 * ctypes stub (getdist_amd/_lib.py, and INTEGRATION.md).
 *
 * Conventions: all entry points are extern "C", return 0 on success or a negative gd_status; no C++
 * exception crosses the ABI; sizes are int64_t; floating point is IEEE fp64 throughout; "d_" pointers
 * are DEVICE pointers obtained from gd_dev_alloc (opaque to the caller), everything else is host
 * memory owned by the caller.  A gd_ctx is bound to one device and one stream and is not thread-safe;
 * use one ctx per thread/GPU.  gd_last_error(ctx) returns a static/ctx-owned message for the last
 * failing call.
 */
#ifndef GDHIP_H
#define GDHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gd_ctx gd_ctx;

typedef enum gd_status {
    GD_OK = 0,
    GD_ERR_BADARG = -1,    /* -> ValueError / SettingError in the Python layer */
    GD_ERR_NOMEM = -2,     /* -> MemoryError */
    GD_ERR_HIP = -3,       /* -> RuntimeError (message holds hipGetErrorString) */
    GD_ERR_EMPTY = -4,     /* "no samples in bin" -> DensitiesError (densities.py:83-84) */
    GD_ERR_SOLVER = -5,    /* bandwidth root-find failed -> fallback / BandwidthError (mcsamples.py:1258-1268) */
    GD_ERR_FFT = -6,       /* rocFFT failure */
    GD_ERR_NODEVICE = -7,  /* no HIP device visible */
    GD_ERR_TIMEOUT = -8    /* a collective / communicator set-up gave up waiting for a peer (the communicator was aborted and
                              dropped: renegotiate over the host application's own channel) -> parallel.CommTimeout */
} gd_status;

/* ---------------------------------------------------------------- context / memory ------------- */
int gd_device_count(void);
int gd_create(int device, gd_ctx** out);
void gd_destroy(gd_ctx* ctx);
const char* gd_last_error(gd_ctx* ctx);
const char* gd_version(void);
/* info[0]=CU count, [1]=LDS bytes/block, [2]=total HBM bytes, [3]=free HBM bytes, [4]=clock kHz, [5]=warp size */
int gd_device_info(gd_ctx* ctx, int64_t* info6);
int gd_sync(gd_ctx* ctx);
int gd_dev_alloc(gd_ctx* ctx, int64_t bytes, void** d_out);
int gd_dev_free(gd_ctx* ctx, void* d_ptr);
int gd_memcpy_h2d(gd_ctx* ctx, void* d_dst, const void* src, int64_t bytes);
int gd_memcpy_d2h(gd_ctx* ctx, void* dst, const void* d_src, int64_t bytes);
/* D2H on a second stream, ordered after the work queued so far on the compute stream; dst should be page-locked
 * (gd_host_alloc).  gd_copy_sync waits for all such copies. */
int gd_memcpy_d2h_async(gd_ctx* ctx, void* dst, const void* d_src, int64_t bytes);
int gd_copy_sync(gd_ctx* ctx);
/* gd_copy_mark: a point on the copy stream after every copy (and all compute-stream work) issued so far;
 * gd_copy_wait blocks until that point has been reached -- the caller's own result copies, not later ones (a batch
 * of results can be delivered while the next batch already computes).  16 marks are kept; an older token waits for
 * the newer mark that replaced it. */
int gd_copy_mark(gd_ctx* ctx, int32_t* token_out);
int gd_copy_wait(gd_ctx* ctx, int32_t token);
int gd_memcpy_d2d(gd_ctx* ctx, void* d_dst, const void* d_src, int64_t bytes);
int gd_memset(gd_ctx* ctx, void* d_dst, int value, int64_t bytes);
/* d_dst[k] = d_src[index[k]] for `count` items of item_bytes each (item_bytes % 16 == 0), one kernel launch;
 * stream-ordered (returns once enqueued; `index` may be released on return) */
int gd_gather_items(gd_ctx* ctx, void* d_dst, const void* d_src, const int32_t* index, int32_t count, int64_t item_bytes);
/* page-locked host memory for fast, asynchronous D2H of result grids.  Blocks of 32 MB and more are anonymous memory on
 * transparent huge pages (MADV_HUGEPAGE, the device's NUMA node preferred) registered with the runtime -- result copies into
 * 4-KB-page blocks allocated late in a process ran measurably slower --, smaller ones hipHostMalloc;
 * free with gd_host_free only. */
int gd_host_alloc(gd_ctx* ctx, int64_t bytes, void** out);
int gd_host_free(gd_ctx* ctx, void* ptr);
/* HIP-event timing on the ctx stream (bench.py measures kernels with these, not torch events) */
int gd_timer_start(gd_ctx* ctx);
int gd_timer_stop_ms(gd_ctx* ctx, double* ms_out);

/* ---------------------------------------------------------------- sample set -------------------
 * Replaces WeightedSamples.setSamples/_weightsChanged (chains.py:276-323): the library keeps its own
 * column-major (SoA) fp64 copy of the N x n sample array and of the weights in HBM.
 * X[i*row_stride + j*col_stride] is sample i of parameter j (strides in elements); weights may be
 * NULL (unit weights: chains.py:313-315).  Re-uploading replaces the previous set. */
int gd_upload(gd_ctx* ctx, const double* X, int64_t N, int64_t n, int64_t row_stride, int64_t col_stride,
              const double* weights);
int gd_num_rows(gd_ctx* ctx, int64_t* N, int64_t* n);
/* device pointer to column j (N doubles) / weights (NULL if unit) -- for tests and zero-copy users; an ALIAS of the resident
 * set that dies with the next upload or mutator (gd_export_device hands out copies that do not) */
int gd_column_ptr(gd_ctx* ctx, int64_t j, void** d_out);
/* gd_clone_samples: the device half of MCSamples.copy (mcsamples.py:308-322, copy.deepcopy of a sample set): dst receives
 *   allocations of its OWN holding src's N x n columns and sample weights (none for a unit-weight set), filled by
 *   device-to-device copies on dst's stream behind an event recorded on src's stream; the call returns when the copies are
 *   complete.  dst is then in the state gd_upload of the same data leaves it in (row / column counts, the integral-weights
 *   flag and the weights' total, no cached prefix sums, bucket or index columns); the spare columns
 *   (gd_set_extra_column) are NOT copied, and while src has auxiliary weights selected it is src's sample weights that
 *   are copied.  Nothing is borrowed (unlike gd_attach_samples): src may be re-uploaded or destroyed afterwards.
 *   GD_ERR_BADARG: dst == src, src without a sample set, contexts on different devices, src borrowing dst's set. */
int gd_clone_samples(gd_ctx* dst, gd_ctx* src);

/* ---------------------------------------------------------------- sample set from device memory
 * gd_upload_device: install a sample set of the context's own from arrays that already live in DEVICE memory of the
 *   context's device (a sampler's torch / CuPy output), without a host round trip.  The source is copied, never adopted; the
 *   resident state afterwards is the one gd_upload leaves for the same values converted to fp64 on the host (columns
 *   bit-equal: the conversions from fp32 / fp16 / bf16 are exact; spare columns zeroed; weights, byte multiplicities,
 *   integral flag and weight total computed by the same code).
 *   parts: `nparts` blocks of rows (one per chain), stacked in the order given.  Element (i, j) of a part is
 *     base[i * row_stride + j * col_stride] (strides in ELEMENTS of `dtype`, >= 0), i < rows, j < cols; `cols` must be the
 *     same in every part.  weights (NULL in every part, or in none): rows elements of `w_dtype`, w_stride apart.
 *   keep / m: the source columns that become resident columns 0..m-1, in that order (NULL: all of them, m ignored).
 *   producer_streams / nstreams: the streams that wrote the sources (none: the caller has synchronised already).  An entry
 *     (void*)1 / (void*)2 is the legacy / per-thread default stream, anything else a hipStream_t.  An event is recorded on
 *     each and the context's stream waits for those events; the host does not wait for a producer.  The call returns when
 *     the copy is complete.
 *   Everything is validated BEFORE the previous sample set is released or a kernel launched; a refusal leaves the previous
 *   set resident.  GD_ERR_BADARG: nparts <= 0, a NULL base or negative row count, differing column counts, no rows at
 *   all, an unknown dtype, a keep[] entry out of range, weights in some parts only, or a span (from shape and strides) that
 *   leaves its allocation.  A valid description this call does not serve comes back with a status of its own:
 *   GD_ERR_DECLINED for memory the HOST can read as well (page-locked, managed) and for negative strides -- the caller takes
 *   the host route (gd_upload); GD_ERR_OTHER_DEVICE for device memory of another device than the context's (make the context
 *   on that device); GD_ERR_NOT_DEVICE for a pointer the runtime does not know.
 * gd_fetch_device_array: the rows x cols array described the same way, converted to fp64, into the row-major HOST array
 *   `out` (the fixed-parameter probe's first / last row and candidate columns, device weights and loglikes).  Same
 *   validation and statuses; producer_stream is one entry of the kind above, or NULL.
 * gd_download_samples: the resident columns as a row-major N x n fp64 HOST array (the inverse of gd_upload; `out` should
 *   be page-locked, gd_host_alloc): blocks of rows are transposed on the device into scratch and copied out. */
typedef enum gd_dtype { GD_DT_F64 = 0, GD_DT_F32 = 1, GD_DT_F16 = 2, GD_DT_BF16 = 3 } gd_dtype;
#define GD_ERR_DECLINED (-24)
#define GD_ERR_OTHER_DEVICE (-25)
#define GD_ERR_NOT_DEVICE (-26)
typedef struct gd_dev_part {
    const void* base;
    int64_t rows, cols;
    int64_t row_stride, col_stride;
    const void* weights; /* may be NULL */
    int64_t w_stride;
} gd_dev_part;
int gd_upload_device(gd_ctx* ctx, const gd_dev_part* parts, int32_t nparts, int32_t dtype, int32_t w_dtype,
                     const int32_t* keep, int32_t m, void* const* producer_streams, int32_t nstreams);
int gd_fetch_device_array(gd_ctx* ctx, const void* base, int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride,
                          int32_t dtype, void* producer_stream, double* out);
int gd_download_samples(gd_ctx* ctx, double* out);
/* what the runtime says about a pointer: kind GD_PTR_*, and for device memory the device it lives on (else -1) */
enum { GD_PTR_DEVICE = 0, GD_PTR_PINNED = 1, GD_PTR_MANAGED = 2, GD_PTR_UNKNOWN = 3 };
int gd_pointer_info(gd_ctx* ctx, const void* ptr, int32_t* kind_out, int32_t* device_out);

/* ---------------------------------------------------------------- editing the resident sample set
 * gd_select_samples: replace the context's OWN resident sample set by a selection of itself, device to device: the rows a
 *   mutator keeps (filter, thin, removeBurn: chains.py:941-1061), the columns it keeps (deleteFixedParams) and at most one
 *   appended column (addDerived).  The resident state afterwards is the one gd_upload leaves for the same selection made
 *   with numpy on the host (columns and weights bit-equal, spare columns zeroed, integral flag, weight total and byte
 *   multiplicities computed by the same code, no cached prefix sums, bucket or index columns, no auxiliary weights).
 *   Rows (row_kind):
 *     GD_SEL_ALL        every row.
 *     GD_SEL_RANGE      rows [lo, hi).
 *     GD_SEL_MASK_U8    `rows` is N bytes; the rows whose byte != 0, in ascending order.
 *     GD_SEL_WEIGHT_GT  the rows whose sample weight > thr (evaluated on the resident weight column; a unit-weight set
 *                       has weight 1 in every row), in ascending order.
 *     GD_SEL_ROWS_I32   `rows` is a list of K int32 row numbers: any order, repeats allowed, K may exceed N (what
 *                       gd_thin_rows writes).
 *     flags & GD_SEL_ROWS_ON_DEVICE: `rows` (mask or list) is device memory of the context's device, else host memory.  A
 *     host list is checked against [0, N); a device list is trusted, as gd_gather_rows trusts it.
 *   Columns: keep[m] are the resident columns that stay, ascending (NULL: all n, m ignored).  append_kind
 *     GD_SEL_APPEND_HOST puts the host vector append_host (N doubles, one per row of the CURRENT set) behind them,
 *     GD_SEL_APPEND_SLOT the spare column append_slot (where gd_expr_eval(..., GD_EX_TO_COLUMN, slot) leaves an
 *     expression); the appended column goes through the same row selection.
 *   Weights (weight_kind): GD_SEL_W_KEEP selects the weight column like a sample column (none stays none);
 *     GD_SEL_W_UNIT leaves the new set without weights; GD_SEL_W_REPLACE takes new_weights, one double per SELECTED row
 *     (K must then state their number for every row kind, and is checked against the count selected).
 *   Ordered selections (mask, weight threshold) become a device int32 row list first -- a count per tile of 1024 rows, an
 *   exclusive scan of the tile counts, an ordered placement by wave ballot -- and one gather kernel moves the data;
 *   GD_SEL_ALL / GD_SEL_RANGE are device-to-device copies per column.  The new set is built beside the old one and installed
 *   when complete; the call returns when it is.  *count_out (may be NULL) receives the new row count.
 *   Refusals leave the previous set resident and untouched.  GD_ERR_BADARG: no resident set, a borrowed one
 *   (gd_attach_samples), auxiliary weights selected, N >= 2^31, lo / hi outside [0, N] or lo >= hi, a keep[] entry out of
 *   range or not ascending, no column left (m + appended == 0), an unknown kind, a missing pointer, GD_SEL_W_REPLACE
 *   without a vector or with a K that is not the count selected, a host row number outside [0, N), and no row selected
 *   ("no rows selected").  GD_ERR_NOMEM when the second set does not fit beside the first.
 * gd_set_weights: replace only the SAMPLE WEIGHT column of the context's own resident set by the N host doubles w_host
 *   (NULL: unit weights, no weight column).  Integral flag, total and byte multiplicities are recomputed as by an upload;
 *   everything cached that depends on the weights goes (cumulative weights, auxiliary / like weights, the batched call's
 *   index columns, the bucket columns -- their bucket count follows the weight mode); the sample columns are not touched.
 *   GD_ERR_BADARG for no resident set, a borrowed one, or while auxiliary weights are selected. */
enum { GD_SEL_ALL = 0, GD_SEL_RANGE = 1, GD_SEL_MASK_U8 = 2, GD_SEL_WEIGHT_GT = 3, GD_SEL_ROWS_I32 = 4 };
enum { GD_SEL_W_KEEP = 0, GD_SEL_W_UNIT = 1, GD_SEL_W_REPLACE = 2 };
enum { GD_SEL_APPEND_NONE = 0, GD_SEL_APPEND_HOST = 1, GD_SEL_APPEND_SLOT = 2 };
#define GD_SEL_ROWS_ON_DEVICE 1
#define GD_SEL_TILE 1024 /* rows per tile of the count / placement passes */
typedef struct gd_selection {
    int32_t row_kind, flags;
    int64_t lo, hi;      /* GD_SEL_RANGE */
    const void* rows;    /* GD_SEL_MASK_U8: N bytes; GD_SEL_ROWS_I32: K int32 */
    int64_t K;           /* GD_SEL_ROWS_I32: the list's length; with GD_SEL_W_REPLACE: the number of new weights */
    double thr;          /* GD_SEL_WEIGHT_GT */
    const int32_t* keep; /* may be NULL */
    int32_t m;
    int32_t append_kind, append_slot;
    int32_t weight_kind;
    const double* append_host;
    const double* new_weights;
} gd_selection;
int gd_select_samples(gd_ctx* ctx, const gd_selection* sel, int64_t* count_out);
int gd_set_weights(gd_ctx* ctx, const double* w_host);

/* ---------------------------------------------------------------- the resident samples as device arrays
 * gd_export_device: the mirror image of gd_upload_device.  Selected rows of selected resident columns (or of the sample
 *   weights) are written into a DEVICE array of the caller's, in the element type and with the strides it states.  The
 *   result is a SNAPSHOT, a copy device to device into memory the sample set does not own: every mutator and re-upload may
 *   replace the resident set afterwards.  The call only reads the set, so a borrowed one (gd_attach_samples) may be exported.
 *   Rows: row_kind, flags, lo, hi, rows, K, thr exactly as in gd_selection (GD_SEL_ALL / RANGE / MASK_U8 / WEIGHT_GT /
 *     ROWS_I32, GD_SEL_ROWS_ON_DEVICE; masks and thresholds become an ascending row list by the same compaction; a host list
 *     is checked against [0, N), a device list is trusted; a list may be in any order, with repeats), and one kind more:
 *     GD_EXP_ROWS_COLUMN_NZ, the rows whose value in resident column mask_col (a spare column, where
 *     gd_expr_eval(..., GD_EX_TO_COLUMN, slot) leaves a boolean expression as 0.0 / 1.0) is != 0: the mask never leaves the
 *     device.  Unlike gd_select_samples a selection may be EMPTY (lo == hi, K == 0, nothing kept).
 *   Columns: cols[m] are resident column indices in any order, repeats allowed, the spare columns n .. n + 3 included,
 *     1 <= m <= 65535.  cols == NULL: the sample weight column (m is ignored and taken as 1); a unit-weight set writes 1.
 *   Destination: element (k, c) of the result -- k-th selected row, c-th listed column -- goes to
 *     base[k * row_stride + c * col_stride] (strides in ELEMENTS of `dtype`, >= 0), converted from fp64 with IEEE
 *     round-to-nearest-even in ONE step (csrc/cvtfloat.hpp; overflow gives inf, subnormal results are kept).  Only these
 *     elements are written: nothing between or behind them.  rows_capacity is the number of rows the destination has room for.
 *   consumer_stream: the caller's stream that used the destination last and will use it next: NULL none, (void*)1 the legacy
 *     default stream, (void*)2 the per-thread default stream, else a hipStream_t.  The library's stream waits (an event) for
 *     the work that stream has been given before the first store, and that stream waits (an event) for the export's kernels;
 *     the host waits for neither.  With NULL the call returns once the destination is written.
 *   *count_out (required) receives K, the number of rows selected.  K > rows_capacity: nothing is written and the call
 *     returns GD_DRAW_MORE_ROWS -- a first call with rows_capacity 0 (base is then not looked at) is how a caller learns K for
 *     a mask before it allocates.  K == 0 launches nothing and returns GD_OK.
 *   Kernels, one per call, chosen from the strides and the alignment as on the way in: slab (contiguous rows into a
 *     row-major destination, col_stride 1: a block takes R rows, reads each column's run with 16-byte loads into LDS and
 *     writes converted rows, 16-byte stores when row_stride == m), column (row_stride 1 or a single column: a converting
 *     copy, two rows per lane), tile (any other strides: 32 x 32), gathered (any row list).
 *   Every check passes BEFORE anything is launched; a refusal writes nothing.  With rows_capacity > 0 the destination must
 *     be what gd_upload_device accepts as a source, with the same statuses (GD_ERR_DECLINED for page-locked / managed memory
 *     and negative strides, GD_ERR_OTHER_DEVICE, GD_ERR_NOT_DEVICE, GD_ERR_BADARG for a misaligned pointer or a span that
 *     leaves its allocation), and GD_ERR_BADARG when two of its rows_capacity x m elements share an address (a zero stride
 *     with extent > 1, row_stride < m with col_stride 1).  GD_ERR_BADARG also: no resident set, N >= 2^31 with a row list,
 *     a range outside [0, N] or lo > hi, a missing pointer, an unknown kind or dtype, a column out of range, m outside
 *     1 .. 65535, a host row number outside [0, N), negative rows_capacity.
 * gd_export_alloc / gd_export_free / gd_export_fetch: device memory for a result that must outlive every context
 *   (devarray.DeviceArray): allocated on `device` with no context, so that it neither comes from nor returns to a context's
 *   block cache and stays valid across mutators, re-uploads and gd_destroy; freed, and read back to the host, with the
 *   device index alone.  They return GD_OK, GD_ERR_NOMEM or GD_ERR_HIP (no context: no error text). */
#define GD_EXP_ROWS_COLUMN_NZ 5
typedef struct gd_export {
    int32_t row_kind, flags; /* a GD_SEL_* row kind or GD_EXP_ROWS_COLUMN_NZ; GD_SEL_ROWS_ON_DEVICE */
    int64_t lo, hi;          /* GD_SEL_RANGE */
    const void* rows;        /* GD_SEL_MASK_U8: N bytes; GD_SEL_ROWS_I32: K int32 */
    int64_t K;               /* GD_SEL_ROWS_I32: the list's length */
    double thr;              /* GD_SEL_WEIGHT_GT */
    int32_t mask_col;        /* GD_EXP_ROWS_COLUMN_NZ */
    int32_t m;
    const int32_t* cols;     /* NULL: the sample weights */
    void* base;
    int64_t rows_capacity, row_stride, col_stride;
    int32_t dtype, reserved; /* GD_DT_* */
    void* consumer_stream;
} gd_export;
int gd_export_device(gd_ctx* ctx, const gd_export* ex, int64_t* count_out);
int gd_export_alloc(int32_t device, int64_t bytes, void** d_out);
int gd_export_free(int32_t device, void* d_ptr);
int gd_export_fetch(int32_t device, void* dst, const void* d_src, int64_t bytes);

/* ---------------------------------------------------------------- weighted moments -------------
 * gd_weight_stats: norm=sum w (chains.py:312), max w (chains.py:1349), sum w^2 (chains.py:499,536),
 *   count of w > thresh (mcsamples.py:559-560).   out4 = {norm, max_w, sum_w2, n_above}
 * gd_col_stats: per column over rows [row_lo,row_hi): min, max (mcsamples.py:1434-1435), weighted mean
 *   (chains.py:379), weighted variance about that mean (chains.py:409-410). out = n x 4 {min,max,mean,var}
 * gd_cov: weighted means and covariance of the listed columns over rows [row_lo,row_hi)
 *   (chains.py:373-384 setMeans, :709-733 cov + mean_diffs :763-780); means_out m, cov_out m x m, norm_out 1; minmax_out
 *   (may be NULL) m x 2 = the columns' min / max over the range -- updateBaseStatistics then needs no separate
 *   gd_col_stats call (the variances are the diagonal).  Up to 207 columns in ONE read of the samples (round 6): deviations
 *   are taken from a provisional shift s (the mean of 256 strided rows), a column of ones rides in the slab, and
 *   mean = s + sum w (x - s) / sum w,  cov_ij = sum w (x_i - s_i)(x_j - s_j) / sum w - (mean_i - s_i)(mean_j - s_j):
 *   the reference's two passes (means, then deviations from the means) to rounding -- (mean - s)^2 is ~1e-3 of the
 *   variance, so the subtraction costs no digits.  208 columns and above: two passes as before. */
int gd_weight_stats(gd_ctx* ctx, int64_t row_lo, int64_t row_hi, double thresh, double* out4);
int gd_col_stats(gd_ctx* ctx, int64_t row_lo, int64_t row_hi, double* out);
int gd_cov(gd_ctx* ctx, const int32_t* cols, int32_t m, int64_t row_lo, int64_t row_hi, double* means_out,
           double* cov_out, double* norm_out, double* minmax_out);

/* ---------------------------------------------------------------- weighted quantiles -----------
 * Replaces initParamConfidenceData + confidence (chains.py:793-838: argsort, cumsum(w[idx]),
 * searchsorted(cumsum, target), x[idx[min(ix,N-1)]]) by a sort-free MSB radix select.
 * targets are cumulative-weight targets (norm*limfrac, computed by the caller exactly as the
 * reference does); out[c*k + t] = smallest sample value v of column cols[c] whose cumulative weight
 * sum_{x<=v} w reaches targets[c*k+t] (the maximum if none does). */
int gd_quantiles(gd_ctx* ctx, const int32_t* cols, int32_t ncols, int64_t row_lo, int64_t row_hi,
                 const double* targets, int32_t k, double* out);

/* gd_quantiles_mm: the same selection when the caller knows each column's minimum and maximum over (a superset of) the
 * row range -- minmax[2c], minmax[2c+1]; the base statistics have them (gd_cov's minmax_out).  Then ONE counting pass
 * over the monotone linear bucket index (int)((x - min) * nbuckets / (max - min)) in 32768 (unit weights) or 16384
 * (fp64 weights) LDS buckets narrows every target to a few hundred rows, which one collect pass gathers and a sorted walk
 * of the cumulative weight finishes exactly as above: two reads of the columns instead of four.  Taken for unit weights
 * and integer multiplicities (whose bucket sums are exact in any order of addition); minmax == NULL, real weights, a
 * degenerate range, more rows than the bucket lists can hold, or a list overflow (heavily tied data) take the radix
 * path of gd_quantiles; the result is the same sample value either way. */
int gd_quantiles_mm(gd_ctx* ctx, const int32_t* cols, int32_t ncols, int64_t row_lo, int64_t row_hi,
                    const double* targets, int32_t k, const double* minmax, double* out);

/* gd_quantiles_mm_probe: gd_quantiles_mm whose counting pass -- when it walks WHOLE columns of the sample set (row_lo = 0,
 * row_hi = N, the linear path) -- also serves two other consumers of the same read (round 6):
 *   - the first 8 autocovariance lag sums of getCorrelationLength's probe (chains.py:423-466, what gd_autocov_lags_batch(cols,
 *     probe_means, 0, 8) returns: sum_i d_i d_{i+l}, d = (x - mean) w) into probe_out[c * 8 + l]; *probe_done = 1 when they
 *     were computed (0: the select took another path -- call gd_autocov_lags_batch);
 *   - the columns' 16-bit bucket indices are kept on the device: the select's own collect pass, and later gd_prebin8_batch /
 *     gd_prebin8_hist2d / gd_prebin_batch of the same columns, read those 2 bytes per sample instead of the 8-byte value
 *     (a bucket that lies inside one bin maps through a table; the ~1 % that straddle a bin edge re-read the sample and
 *     take the exact fp64 route of mcsamples.py:1497 -- the indices are bit-equal either way).
 * probe_means / probe_out / probe_done may be NULL (then this is gd_quantiles_mm). */
int gd_quantiles_mm_probe(gd_ctx* ctx, const int32_t* cols, int32_t ncols, int64_t row_lo, int64_t row_hi,
                          const double* targets, int32_t k, const double* minmax, double* out, const double* probe_means,
                          double* probe_out, int32_t* probe_done);

/* ---------------------------------------------------------------- autocorrelation / N_eff ------
 * gd_autocov_lags: out[l] = sum_{i} d_i d_{i+k0+l}, d=(x-mean)*w, l<nlags -- the un-normalised lag
 *   sums convolve.autoConvolve (convolve.py:458-478) obtains by FFT for chains.py:441.
 * gd_kde_lag_sums: out[l] = sum_i exp(-(x_i-x_{i+k_l})^2 * inv4s2) w_i w_{i+k_l}
 *   (corr_k and the uncorrelated-term loop of getEffectiveSamplesGaussianKDE, chains.py:514-540). */
int gd_autocov_lags(gd_ctx* ctx, int32_t col, double mean, int64_t k0, int32_t nlags, double* out);
int gd_kde_lag_sums(gd_ctx* ctx, int32_t col, double inv4s2, const int64_t* lags, int32_t nlags, double* out);
/* 2D variant (getEffectiveSamplesGaussianKDE_2d, chains.py:576-635): out[l] = sum_i exp(-(d^T K d)/4) w_i w_{i+k_l},
 * d = (x_i - x_{i+k}, y_i - y_{i+k}), kinv3 = {K00, K01+K10, K11} with K = inv(cov)/h^2 */
int gd_kde_lag_sums_2d(gd_ctx* ctx, int32_t coli, int32_t colj, const double* kinv3, const int64_t* lags, int32_t nlags,
                       double* out);
/* batched over columns in one launch: out is ncols x nlags (per-column mean / inv4s2, shared lag list) */
int gd_autocov_lags_batch(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* means, int64_t k0,
                          int32_t nlags, double* out);
int gd_kde_lag_sums_batch(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* inv4s2, const int64_t* lags,
                          int32_t nlags, double* out);
/* the same lag sums restricted to rows [row_lo,row_hi) (one chain of a multi-chain set, mcsamples.py:941-962) */
int gd_autocov_lags_range_batch(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* means, int64_t row_lo,
                                int64_t row_hi, int64_t k0, int32_t nlags, double* out);

/* ---------------------------------------------------------------- binning ----------------------
 * Index rule (mcsamples.py:1497): ix = (int)((x - binmin)/fine_width + 0.5), IEEE fp64, no FMA
 * contraction, true division.  Truncating rule (kde_bandwidth.py:86-87): (int)((x - range_min)/dx).
 * gd_hist1d: fused index + weighted bincount (mcsamples.py:1554) for ncols columns -> out ncols x F.
 * gd_bin_indices: writes the int32 indices (tests: bit-exact index parity; n_out_of_range counts
 *   indices outside [0,F)).
 * gd_prebin: u16 bin-index columns kept on the device for the batched 2D path; d_idx is N u16.
 * gd_hist2d: weighted 2D histogram hist[iy*F+ix] (mcsamples.py:1724-1728) for B pairs, direct from the
 *   fp64 columns (x index from colx with rule `round`, y from coly) -> d_hist B x F x F (device).
 * gd_hist2d_prebinned: same from u16 index columns produced by gd_prebin.  LDS counters: fp64 for real weights,
 *   u32 for unit or integral weights (exact), 16-bit packed for large unit-weight batches with exact overflow
 *   detection and a u32 redo of the affected pairs -- the result is always the exact weighted count.
 * gd_minmax_affine: min/max over samples of a*x_i + b*x_j (the sheared coordinate p2,
 *   mcsamples.py:1373 + kde_bandwidth.py:77-78); out 2*B.
 * gd_hist2d_sheared: rotated histogram of mcsamples.py:1372-1378: x index = trunc((x_i - xmin)/dx),
 *   y index = trunc(((r0*x_i + r1*x_j) - ymin)/dy). */
int gd_hist1d(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* binmin, const double* width,
              int32_t F, double* out);
/* the same with the histograms left in device memory (d_out: ncols x F doubles from gd_dev_alloc); returns when the
 * kernels are enqueued on the context's stream */
int gd_hist1d_dev(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* binmin, const double* width,
                  int32_t F, void* d_out);
int gd_bin_indices(gd_ctx* ctx, int32_t col, double binmin, double width, int32_t round_half, int32_t F,
                   int32_t* idx_out, int64_t* n_out_of_range);
int gd_prebin(gd_ctx* ctx, int32_t col, double binmin, double width, int32_t F, void* d_idx_u16);
/* Byte-index variant of the batched triangle binning (unit weights, fine_bins_2D = 256, the base grid of 98 % of a
 * triangle's pairs): gd_prebin8_batch writes (unsigned char)((x - binmin)/width + 0.5) for ncols columns in one launch
 * (d_idx_out[c]: device buffers of N bytes, 16-byte aligned) and reports in bad_out[c] how many samples fell outside
 * [0, F) -- zero by construction of the bin range (mcsamples.py:1486-1498), and required to be zero by
 * gd_hist2d_prebinned8, which builds B 256 x 256 histograms (device, B x 256 x 256 fp64, [y][x]) from pairs of those
 * columns: one block per pair, 16-bit counters packed two per LDS word, two bin addresses per v_perm_b32.  A wrapped
 * counter (more than 65535 samples in one bin) is detected exactly and reported as GD_ERR_SOLVER; the caller then uses
 * gd_prebin_batch + gd_hist2d_prebinned for that batch. */
int gd_prebin8_batch(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* binmin, const double* width, int32_t F,
                     void* const* d_idx_out, int64_t* bad_out);
int gd_hist2d_prebinned8(gd_ctx* ctx, int32_t B, const void* const* d_idx_x, const void* const* d_idx_y, void* d_hist);
/* gd_prebin8_hist2d: both of the above enqueued back to back with ONE wait: first the `ncols` byte index columns that have
 * to be (re)made (ncols may be 0), then the B histograms over index columns d_idx_x / d_idx_y (which may be among the
 * columns just made).  bad_out as gd_prebin8_batch; GD_ERR_SOLVER when any sample fell outside the grid or a counter
 * wrapped -- the histograms are then invalid and the caller takes gd_prebin_batch + gd_hist2d_prebinned. */
int gd_prebin8_hist2d(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* binmin, const double* width,
                      void* const* d_idx_out, int64_t* bad_out, int32_t B, const void* const* d_idx_x,
                      const void* const* d_idx_y, void* d_hist);

/* several index columns in one launch (d_idx_u16[c] receives column cols[c] binned with binmin[c], width[c]) */
int gd_prebin_batch(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* binmin, const double* width, int32_t F,
                    void* const* d_idx_u16);
int gd_hist2d(gd_ctx* ctx, int32_t B, const int32_t* colx, const int32_t* coly, const double* binminx,
              const double* widthx, const double* binminy, const double* widthy, int32_t F, void* d_hist);
int gd_hist2d_prebinned(gd_ctx* ctx, int32_t B, const void* const* d_idx_x, const void* const* d_idx_y, int32_t F,
                        void* d_hist);
int gd_minmax_affine(gd_ctx* ctx, int32_t B, const int32_t* coli, const int32_t* colj, const double* a,
                     const double* b, double* out);
int gd_hist2d_sheared(gd_ctx* ctx, int32_t B, const int32_t* coli, const int32_t* colj, const double* r0,
                      const double* r1, const double* xmin, const double* dx, const double* ymin, const double* dy,
                      int32_t F, void* d_hist);

/* gd_isj1d: kde_bandwidth.py:102-135 gaussian_kde_bandwidth_binned for B histograms (host, B x F) with effective
 *   sample numbers neff[b]: DCT-II of hist/sum, the Botev improved-Sheather-Jones fixed point (:59-73) solved by
 *   MINPACK hybrd for one unknown as scipy.optimize.fsolve(x0 = 0.53 N^-1/5, xtol = x0/20, factor = 1) runs it, then
 *   the brentq re-check on [0.019 N^-1/5, 0.5] when the root is below 0.019 N^-1/5 -- all inside one kernel.
 *   hfrac_out[b] = bandwidth in units of the bin range; status_out[b] = GD_OK, or GD_ERR_SOLVER where the
 *   reference returns None ("1D auto bandwidth failed": zero functional). */
int gd_isj1d(gd_ctx* ctx, int32_t B, int32_t F, const double* hist, const double* neff, double* hfrac_out,
             int32_t* status_out);
/* the same reading the histograms in device memory (gd_hist1d_dev) */
int gd_isj1d_dev(gd_ctx* ctx, int32_t B, int32_t F, const void* d_hist, const double* neff, double* hfrac_out,
                 int32_t* status_out);

/* ---------------------------------------------------------------- 1D density -------------------
 * gd_dct1d: a = DCT-II(data/sum(data)) (scipy.fftpack.dct type 2, unnormalised), for the Botev ISJ
 *   fixed point (kde_bandwidth.py:113-117).  in/out host arrays B x F.
 * gd_density1d: everything after the bandwidth for B parameters (mcsamples.py:1588-1668): Gaussian
 *   taps (Kernel1D :129-135), 'same' convolution (convolve.py:196-202), boundary correction of order
 *   bco (0,1,2; mcsamples.py:1600-1647), mbc rounds of multiplicative bias correction (:1649-1666),
 *   normalize("max") (densities.py:71-92).  hist: B x F (host); smooth[b] in fine-bin units, winw[b];
 *   flags[b] bit0=has_limits_bot bit1=has_limits_top bit2=periodic.  P_out: B x F.
 *   status_out[b] = GD_OK or GD_ERR_EMPTY. */
int gd_dct1d(gd_ctx* ctx, int32_t B, int32_t F, const double* hist, double* a_out);
int gd_density1d(gd_ctx* ctx, int32_t B, int32_t F, const double* hist, const double* smooth, const int32_t* winw,
                 const int32_t* flags, int32_t bco, int32_t mbc, double* P_out, int32_t* status_out);
/* the same reading the histograms in device memory (gd_hist1d_dev); P_out is on the host */
int gd_density1d_dev(gd_ctx* ctx, int32_t B, int32_t F, const void* d_hist, const double* smooth, const int32_t* winw,
                     const int32_t* flags, int32_t bco, int32_t mbc, double* P_out, int32_t* status_out);

/* ---------------------------------------------------------------- 2D bandwidth -----------------
 * gd_kopt2d: KernelOptimizer2D.__init__ + the psi functionals get_h needs (kde_bandwidth.py:146-270)
 *   for B square histograms (device, B x F x F): a2 = dct2d(data/sum)[1:,1:]^2 (:151), t* by Brent's
 *   method on the 2D fixed point over [0,0.1] with xtol=1e-6 (:162,177-196; scipy brentq semantics:
 *   rtol=4eps, maxiter=100), the fallback_t rules (:164-175; fallback_t<=0 means None),
 *   psi_02, psi_20, psi_11 = func2d at t* (:245-247), and when do_corr[b]: psi_00 (:267) and the odd
 *   functionals psi_13, psi_31 from |fft2|^2 (:156-157,198-214,269-270).
 *   Then KernelOptimizer2D.get_h (:234-306) on the device, one wavefront per pair: the closed-form bandwidths
 *   (:245-252) and, when do_corr[b], the two TNC minimisations of the AMISE (:276-302) started from corr[b]
 *   (scipy.optimize.minimize(method="TNC") ported evaluation-faithfully, csrc/solvers.hpp), with the reference's
 *   acceptance rules.
 *   out: B x 12 = {t_star, p02, p20, p11, p00, p13, p31, status(0 ok, <0 gd_status), hx, hy, corr,
 *   get_h status (0 ok, GD_ERR_BADARG = "bias not positive definite", GD_ERR_SOLVER = no functionals)};
 *   hx, hy are fractions of the histogram's bin range. */
int gd_kopt2d(gd_ctx* ctx, int32_t B, int32_t F, const void* d_hist, const double* neff, const int32_t* do_corr,
              const double* fallback_t, const double* corr, double* out);
/* The same work in two stream-ordered stages, for callers that keep several launches in flight:
 *   gd_kopt2d_enqueue: everything up to the functionals (sums, DCT, power spectra, the fixed point) on ctx's stream; returns
 *     at once.  d_rows: device block of B x GD_KOPT_BLOCK_DOUBLES doubles: the B x 12 result rows
 *     {t_star, p02, p20, p11, p00, p13, p31, status, ...} followed by get_h's per-pair inputs, which this call uploads.
 *     *ticket_out identifies the point on ctx's stream behind those kernels (32 tickets are kept).
 *   gd_kopt2d_finish: get_h (the closed forms and the TNC minimisations) for those rows on `ctx`'s stream -- which may be
 *     ANOTHER context of the same device than stage_a_ctx: its stream waits for the ticket, so the serial TNC stage of one
 *     launch runs beside the next launch's DCT / fixed point -- and the finished B x 12 rows in `out` (host).  Blocks
 *     until they are there. */
#define GD_KOPT_BLOCK_DOUBLES 15
int gd_kopt2d_enqueue(gd_ctx* ctx, int32_t B, int32_t F, const void* d_hist, const double* neff, const int32_t* do_corr,
                      const double* fallback_t, const double* corr, void* d_rows, int32_t* ticket_out);
int gd_kopt2d_finish(gd_ctx* ctx, gd_ctx* stage_a_ctx, int32_t ticket, int32_t B, void* d_rows, double* out);
/* gd_get_h: the get_h stage alone, from host arrays: psi is B x 6 = {p02, p20, p11, p00, p13, p31};
 *   out: B x 4 = {hx, hy, corr, status}. */
int gd_get_h(gd_ctx* ctx, int32_t B, const double* psi, const double* neff, const double* corr, const int32_t* do_corr,
             double* out);

/* ---------------------------------------------------------------- 2D density -------------------
 * gd_density2d: everything after the bandwidth for B pairs sharing F (mcsamples.py:1857-1990):
 *   window synthesis from (rx, ry, corr, winw) (:1863-1867), zero-padded linear FFT convolution via
 *   rocFFT (convolve.py:405-436), linear boundary correction of order bco (0/1) where a parameter has a
 *   limit (:1905-1961), mbc rounds of multiplicative bias correction (:1963-1976), normalize("max") (:1990).
 *   flags[b]: bit0/1 = x has_limits_bot/top, bit2/3 = y bot/top (non-periodic axes only, :1688-1703);
 *   bit4/5 = x/y periodic (circular convolution on the folded grid, convolve.py:215-323; must be equal for the
 *   whole batch); bit6 = has_prior, i.e. the boundary-correction block applies (defaults to "any of bits 0-3").
 *   d_hist: B x F x F (device, [y][x]); d_P_out: B x F x F (device).  status_out[b] as gd_density1d. */
int gd_density2d(gd_ctx* ctx, int32_t B, int32_t F, const void* d_hist, const double* rx, const double* ry,
                 const double* corr, const int32_t* winw, const int32_t* flags, int32_t bco, int32_t mbc,
                 void* d_P_out, int32_t* status_out);
/* gd_density2d_enqueue: the same work, but the call returns as soon as it is enqueued on the context's stream, so
 *   the host prepares the next batch (and builds result objects) while this one computes.  The per-pair table is
 *   staged through page-locked memory owned by the context; `status_pinned` must be page-locked (gd_host_alloc) and
 *   is valid after gd_sync, or after gd_copy_sync of a gd_memcpy_d2h_async issued after this call.  d_hist and
 *   d_P_out must stay allocated until then. */
int gd_density2d_enqueue(gd_ctx* ctx, int32_t B, int32_t F, const void* d_hist, const double* rx, const double* ry,
                         const double* corr, const int32_t* winw, const int32_t* flags, int32_t bco, int32_t mbc,
                         void* d_P_out, int32_t* status_pinned);

/* gd_density2d_enqueue_indexed: the same for a batch that is NOT contiguous in d_hist: pair b convolves the histogram
 *   hist_index[b] of the block (B_src x F x F) -- the pairs of one frame-size class picked out of a grid-size class, without
 *   copying their histograms together first. */
int gd_density2d_enqueue_indexed(gd_ctx* ctx, int32_t B, int32_t F, const void* d_hist, const int32_t* hist_index,
                                 const double* rx, const double* ry, const double* corr, const int32_t* winw,
                                 const int32_t* flags, int32_t bco, int32_t mbc, void* d_P_out, int32_t* status_pinned);

/* ---------------------------------------------------------------- second lane -----------------
 * A context is one stream; a second context on the same device gives a second, concurrent lane of work over the
 * SAME resident sample set (independent pairs of a triangle are dealt to two lanes so that one lane's host-side
 * scalar work and result copies hide behind the other lane's kernels).
 * gd_attach_samples: ctx borrows owner's device columns / weights (no copy); owner must outlive ctx or be
 *   re-uploaded only after ctx is destroyed or re-attached.  The extra columns (gd_set_extra_column) are shared too.
 * gd_bind_thread: make ctx's device current for the calling host thread (HIP's current device is per thread);
 *   call once from every additional thread that uses ctx. */
int gd_attach_samples(gd_ctx* ctx, gd_ctx* owner);
int gd_bind_thread(gd_ctx* ctx);

/* ---------------------------------------------------------------- contour levels ---------------
 * gd_contour_levels: densities.py:19-56 getContourLevels(P, contours, half_edge=True) for B grids
 *   (device, B x F x F): out[b*nc + c] = the density level enclosing contours[c] of the half-edge-weighted
 *   mass (argsort of the un-halved grid, cumulative half-weighted mass, linear interpolation between the two
 *   bracketing sorted entries).  status_out[b]: GD_OK; GD_ERR_EMPTY = "Contour level outside plotted ranges"
 *   (:51-52); GD_ERR_SOLVER = more than 1024 exactly equal values at the level (do that grid on the host). */
int gd_contour_levels(gd_ctx* ctx, int32_t B, int32_t F, const void* d_P, const double* contours, int32_t nc, double* out,
                      int32_t* status_out);

/* ---------------------------------------------------------------- contour paths ----------------
 * gd_contour_paths: the contour geometry of B grids at nc levels each (1..8), what a plotter otherwise gets from a
 *   host contouring library grid by grid.  Grid b is ny[b] x nx[b] doubles (sides 2..4096, row-major, P[iy][ix]) at
 *   d_grids + grid_off[b] (device, offsets in doubles); its axes are the nx[b] entries of x_axes from x_off[b] on and the
 *   ny[b] of y_axes from y_off[b] on (host arrays of x_count / y_count doubles, increasing, used as given; grids may share
 *   an axis -- the pairs of a triangle do); its levels are levels[b*nc ..].  Task t = b*nc + c is (grid b, level c).
 * Semantics per task: a node is above iff P > level (a node at the level is below).  One ring of virtual nodes that
 *   are always below surrounds the grid, at the positions of the edge nodes, so the result is the boundary of
 *   {P > level} as closed loops that run along the domain edge where the set touches it.  Edges of the padded
 *   (ny+2) x (nx+2) lattice are numbered: horizontal (j,i)-(j,i+1) is j*(nx+1)+i, vertical (j,i)-(j+1,i) is
 *   (ny+2)*(nx+1) + j*(nx+2)+i.  A crossed edge (exactly one end above) between real nodes a (lower index) and b
 *   carries the vertex pa*(1-f) + pb*f, f = (level - za)/(zb - za), on the varying coordinate (no fused multiply-add);
 *   a crossed edge to the ring carries the real node's own position with flag 1 ("on the domain boundary").  Walking
 *   a cell's corners counter-clockwise -- (j,i), (j,i+1), (j+1,i+1), (j+1,i) -- a segment starts on the edge where the
 *   walk goes above -> below and ends where it goes below -> above: the above side is on the left, peaks run
 *   counter-clockwise and holes clockwise.  In a saddle cell the centre is above iff all four corners are real and
 *   0.25*(z0+z1+z2+z3) > level; then a start on edge k ends on edge k+1, otherwise on edge k-1.  Loops are listed by
 *   increasing smallest edge id, each from that edge on in segment direction.  A grid entirely above gives one loop,
 *   the domain rectangle (all flagged); a grid entirely below gives none.
 * Results (host): task_vert_off[T+1] and task_loop_off[T+1] (T = B*nc) are the offsets of every task in the vertex
 *   and loop arrays, which the call asks `alloc(user, which, count)` for once their sizes are known -- GD_PATHS_XY:
 *   count x 2 doubles, GD_PATHS_FLAG: count bytes, GD_PATHS_LOOPS: count int32, the first vertex of every loop relative
 *   to its task's first vertex.  `alloc` returns the storage (page-locked for a fast copy) or NULL to fail the call with
 *   GD_ERR_NOMEM; it is not called when there is no vertex at all.  status_out[b] != 0: grid b holds a non-finite value;
 *   then nothing is traced, all offsets are 0 and the call still returns GD_OK.
 * One workgroup per task: a count pass, a device scan of the counts (only the totals come back: results and scratch
 *   are sized exactly), then compaction of the crossed edges in id order and ordering of the cycles by pointer jumping
 *   (csrc/contourpaths.hip).  GD_ERR_BADARG before any launch for nc outside 1..8, a side outside 2..4096, an axis
 *   offset outside its array, a non-finite level.  Blocks until the results are complete. */
#define GD_PATHS_XY 0
#define GD_PATHS_FLAG 1
#define GD_PATHS_LOOPS 2
typedef void* (*gd_paths_alloc_fn)(void* user, int32_t which, int64_t count);
int gd_contour_paths(gd_ctx* ctx, int32_t B, const void* d_grids, const int64_t* grid_off, const int32_t* ny, const int32_t* nx,
                     const double* x_axes, const int64_t* x_off, int64_t x_count, const double* y_axes, const int64_t* y_off,
                     int64_t y_count, const double* levels, int32_t nc, gd_paths_alloc_fn alloc, void* user,
                     int64_t* task_vert_off, int64_t* task_loop_off, int32_t* status_out);

/* ---------------------------------------------------------------- credible limits 1D -----------
 * gd_limits1d: densities.py:186-248 Density1D.initLimitGrids + getLimits for B densities on regular grids
 *   (host arrays: P is B x F, x0[b] the first grid abscissa, spacing[b] the grid step).  Each density is refined
 *   `factor` times (<= 0: the reference default max(2, 20000 / F)) with the not-a-knot cubic spline through its F
 *   values; per contour c the density level below which (1 - contours[c]) of the refined mass lies is read off the
 *   ranked refined values (interpolating towards the NEXT ranked value, :227), and the outermost crossings of that
 *   level are located.  out[(b*nc + c)*4 ..] = {lower, upper, has_min, has_top} with has_* = 1.0 where the density at
 *   that end of the grid is still >= the level (no crossing: the limit is the grid end).  status_out[b]: GD_OK or
 *   GD_ERR_SOLVER (level beyond the ranked values / no crossing found, where the reference raises IndexError). */
int gd_limits1d(gd_ctx* ctx, int32_t B, int32_t F, const double* P, const double* x0, const double* spacing,
                const double* contours, int32_t nc, int32_t factor, double* out, int32_t* status_out);

/* ---------------------------------------------------------------- auxiliary vectors ------------
 * The reference lets most statistics take an arbitrary vector instead of a column index (`_makeParamvec`,
 * chains.py:325-337), a row filter `where=` (chains.py:666-780) or alternative weights (chains.py:793-838).
 * gd_set_extra_column: copy a host vector (N rows) into spare column `slot` (0..3); it is then addressed as
 *   column index  n + slot  by every entry point that takes column indices.
 * gd_aux_weights: copy a host weight vector (N rows, e.g. weights*where) into the auxiliary weight buffer
 *   (shared with gd_like_weights); gd_select_weights(ctx, 1) makes every weighted entry point use it.
 * gd_col_minmax: out[2c], out[2c+1] = min, max of column cols[c] over the rows of [lo,hi) whose value in
 *   column cond_col is < cond_below (cond_col < 0: all rows; +inf / -inf when no row qualifies) -- the
 *   N-dimensional confidence-region limits of _setLikeStats (mcsamples.py:2263-2274) with cond_col = the
 *   loglikes column and cond_below = its weighted quantile from gd_quantiles. */
int gd_set_extra_column(gd_ctx* ctx, int32_t slot, const double* x);
int gd_aux_weights(gd_ctx* ctx, const double* w);
int gd_col_minmax(gd_ctx* ctx, const int32_t* cols, int32_t ncols, int64_t lo, int64_t hi, int32_t cond_col,
                  double cond_below, double* out);

/* ---------------------------------------------------------------- thinned chains ---------------
 * Raftery-Lewis and CorrSteps (mcsamples.py:1039-1221) work on weight-one thinnings of integer-weight chains
 * (chains.py:878-916 thin_indices_single_samples).
 * gd_weights_integral: *out = 1 when every sample weight is a non-negative integer (or weights are absent).
 * gd_thin_rows: the thinned row list of chain rows [lo,hi) for `factor`, as int32 global row indices into
 *   d_rows (device, `capacity` entries).  unique_mode = 1 is the reference's branch for factor >= max weight
 *   (np.unique(cumsum // factor) first indices, :889-892), 0 its sequential loop (:894-914: row i once per
 *   multiple of factor in (C_{i-1}, C_i]).  Both come from one cached prefix sum of the weights.
 * gd_binary_transitions: for each column c and threshold t (thresholds: ncols x nthr, nthr <= 4), with
 *   b[k] = (x[rows[k]] >= u ? 0 : 1): counts_out[(c*nthr+t)*12 + 0..7] = np.bincount(4 b[k-2] + 2 b[k-1] + b[k])
 *   (:1065-1066) and [8..11] = np.bincount(2 b[k-1] + b[k]) (:1120-1122).
 * gd_thinned_lag_sums: out[c*maxoff + off-1] = sum_k (x[rows[k+off]]-means[c]) (x[rows[k]]-means[c])  (:1204-1206). */
int gd_weights_integral(gd_ctx* ctx, int32_t* out);
int gd_thin_rows(gd_ctx* ctx, int64_t lo, int64_t hi, int64_t factor, int32_t unique_mode, void* d_rows, int64_t capacity,
                 int64_t* count_out);
int gd_binary_transitions(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const void* d_rows, int64_t K,
                          const double* thresholds, int32_t nthr, int64_t* counts_out);
int gd_thinned_lag_sums(gd_ctx* ctx, const int32_t* cols, int32_t ncols, const double* means, const void* d_rows, int64_t K,
                        int32_t maxoff, double* out);

/* ---------------------------------------------------------------- mean likelihoods -------------
 * The optional `meanlikes` branches of get1DDensityGridData / get2DDensityGridData.
 * gd_like_weights: build the device vector  weights*exp(mean_loglike - loglikes)  (mode 0; mcsamples.py:1560,
 *   1830)  or  weights*loglikes  (mode 1, shade_likes_is_mean_loglikes; :1558) from the host column
 *   loglikes (N rows); *sum_out (optional) = the sum of the vector, so that mode 1 with sum_out gives
 *   mean_loglike = sum/norm (chains.py:380-383).  loglikes == NULL drops the vector.
 * gd_select_weights: which = 1 makes every histogram entry point (gd_hist1d, gd_hist2d, gd_hist2d_prebinned)
 *   accumulate the like weights instead of the sample weights (the `np.bincount(..., weights=w)` of
 *   :1561,1831); which = 0 restores the sample weights.  Must be 0 for everything else.
 * gd_likes1d: mcsamples.py:1672-1682 for B parameters: rawbins = conv(hist, Win); likehist/P where P>0,
 *   smoothed, times P/rawbins; the exp(-(l - min l)) transform when shade_mean_loglikes; / max.
 *   hist, likehist, P (the finished density of gd_density1d), likes_out: host B x F; smooth/winw/flags as
 *   gd_density1d.
 * gd_likes2d: mcsamples.py:1886-1903,2004-2006 for B pairs: bin2Dlikes = conv(likehist, Win) [with the
 *   mbc re-smoothing of :1890-1897 when mbc != 0], divided by the uncorrected conv(hist, Win) where that
 *   exceeds 1e-4 of its maximum (0 elsewhere), / max.  d_hist, d_likehist, d_likes_out: device B x F x F;
 *   rx/ry/corr/winw/flags as gd_density2d (only the periodic bits matter).  The convolutions are evaluated
 *   by direct summation, not FFTs: the same linear maps, but free of the cancellation noise whose sign decides
 *   the reference's `bin2Dlikes > 0` mask at low-likelihood pixels ("mean likelihoods"). */
int gd_like_weights(gd_ctx* ctx, const double* loglikes, int32_t mode, double mean_loglike, double* sum_out);
int gd_select_weights(gd_ctx* ctx, int32_t which);
int gd_likes1d(gd_ctx* ctx, int32_t B, int32_t F, const double* hist, const double* likehist, const double* P,
               const double* smooth, const int32_t* winw, const int32_t* flags, int32_t shade_mean_loglikes,
               double* likes_out, int32_t* status_out);
int gd_likes2d(gd_ctx* ctx, int32_t B, int32_t F, const void* d_hist, const void* d_likehist, const double* rx,
               const double* ry, const double* corr, const int32_t* winw, const int32_t* flags, int32_t mbc,
               void* d_likes_out, int32_t* status_out);

/* gd_density2d_masked: gd_density2d for ONE pair whose prior mask was edited by a user callback
 *   (mask_function, mcsamples.py:1767-1770,1907-1919): mask_bc = the (F+2 winw)^2 mask after _setEdgeMask2D
 *   (host, row-major; NULL when no boundary correction), mask_mbc = the same after _setAllEdgeMask2D (NULL when
 *   mbc == 0), zero_mask = F^2 bytes, 1 where mask < 1e-8 (bool_mask: the bias correction does not divide there and
 *   the density is zeroed at the end, :1973-1979).  The mask moments are summed directly.  Non-periodic axes only. */
int gd_density2d_masked(gd_ctx* ctx, int32_t F, const void* d_hist, double rx, double ry, double corr, int32_t winw,
                        int32_t flags, int32_t bco, int32_t mbc, const double* mask_bc, const double* mask_mbc,
                        const unsigned char* zero_mask, void* d_P_out, int32_t* status_out);

/* ---------------------------------------------------------------- raw N-D histograms -----------
 * gd_histnd_batch: the binning of getRawNDDensityGridData (mcsamples.py:2121-2171) for B densities in one call.
 *   Density b has dims[b] parameters: columns cols[o_b .. o_b + dims[b] - 1] (o_b = dims[0] + ... + dims[b-1], axis 0
 *   first) with per-axis bin origins binmin[] and widths width[] laid out like cols.  Every axis has nb bins; the
 *   index of sample i on an axis is (int)((x_i - binmin)/width + 0.5), bit-exact with the reference (the index
 *   columns of gd_prebin8_batch for nb <= 256, of gd_prebin_batch above; each distinct (column, binmin, width) is
 *   binned once per call), and the flat bin is q = ix_0 + nb ix_1 + nb^2 ix_2 + ... (_flattenValues).  Density b has
 *   M_b = nb^dims[b] <= GD_HISTND_MAX_BINS bins; its grids start at element M_0 + ... + M_{b-1} of each output (host
 *   fp64), so a grid read as a C array of shape (nb,)*d is indexed [ix_{d-1}, ..., ix_0].  flags select the outputs:
 *     GD_HISTND_H      H_out[q]    = sum of the currently selected weights (unit when none) over the samples in q;
 *     GD_HISTND_LIKES  HL_out[q]   = sum of the like-weight vector of gd_like_weights (build it in mode 0:
 *                                    w exp(mean_loglike - L), mcsamples.py:2158);
 *     GD_HISTND_LMIN   Lmin_out[q] = min of column loglike_col over the samples in q, +inf for an empty bin.
 *   Deterministic: unit weights and integral multiplicities add integer counts (exactly np.bincount); real weights add
 *   round(w 2^k) in 64-bit fixed point (2^k N max(w) < 2^61), so reruns are bit-equal; the min is an integer min of
 *   an order-preserving encoding.  Tiers: a density whose counters (4 bytes per bin for counts, 8 for fixed point and
 *   for each of HL / Lmin) fit 128 KB is binned in LDS per (density, chunk of rows) and flushed with integer atomics;
 *   larger grids take global integer atomics.  Returns GD_ERR_BADARG for a grid above GD_HISTND_MAX_BINS, a dimension
 *   outside 1..GD_HISTND_MAXD, missing like weights, or any sample whose index falls outside [0, nb) (checked before
 *   it is counted: nothing is written out of bounds).  Blocks until the grids are in the host arrays. */
#define GD_HISTND_MAXD 25
#define GD_HISTND_MAX_BINS (1 << 25)
#define GD_HISTND_H 1
#define GD_HISTND_LIKES 2
#define GD_HISTND_LMIN 4
int gd_histnd_batch(gd_ctx* ctx, int32_t B, const int32_t* dims, const int32_t* cols, const double* binmin,
                    const double* width, int32_t nb, int32_t flags, int32_t loglike_col, double* H_out, double* HL_out,
                    double* Lmin_out);

/* ---------------------------------------------------------------- principal components --------
 * The O(N) passes of MCSamples.PCA (mcsamples.py:682-885) over resident columns.  Per column a map is applied in registers:
 * maps[c] = 0 (N: x), 1 (L: log x), 2 (M: log -x); a non-positive argument of a log gives -inf / NaN, which propagates.
 * Both entries use the SAMPLE weights (unit when there are none), also while gd_select_weights(ctx, 1) has auxiliary
 * weights selected, and norm = sum of those weights.  Two passes each, every sum taken as fixed-order block partials of
 * v_mfma_f64_16x16x4_f64 tile products added in a fixed order (no floating-point atomics): reruns are bit-identical.
 * No N x n scratch: maps, projection and exp are recomputed from the resident columns in each pass.  Returns
 * GD_ERR_BADARG, before any launch, when no samples are uploaded, n (np) is outside 1..uploaded columns, a column index
 * or map is out of range, or (gd_pca_project) np > GD_PCA_MAX_PROJ or n_all is outside 1..uploaded columns.  Both block
 * until the results are in the host arrays.
 *
 * gd_pca_corr: steps 1-2.  y_c = map_c(x_{cols[c]}), c < n.  mean_out[c] = sum w y_c / norm (pass 1);
 *   sd_out[c] = sqrt(sum w (y_c - mean_c)^2 / norm) and corr_out[i n + j] = sum w d_i d_j / norm / (sd'_i sd'_j) with
 *   d = y - mean and sd' = sd where sd != 0, else 1 (pass 2).  The diagonal of corr_out is 1 by construction.
 * gd_pca_project: steps 4-5 for the np analysed columns.  Per row z_k = (map_k(x_{cols[k]}) - mean[k]) / sd'_k,
 *   p_i = sum_k U[i np + k] z_k, then exp(p_i) when doexp.  newmean_out[i] = sum w p_i / norm (pass 1);
 *   newsd_out[i] = sqrt(sum w (p_i - newmean_i)^2 / norm), and with q_i = (p_i - newmean_i) / newsd_i
 *   pcpc_out[i np + j] = sum w q_i q_j / norm and pcpar_out[i n_all + j] = sum w q_i (x_j - all_means[j]) / all_sd[j] / norm
 *   over resident columns j < n_all (pass 2). */
#define GD_PCA_MAX_PROJ 448
int gd_pca_corr(gd_ctx* ctx, const int32_t* cols, int32_t n, const int32_t* maps, double* mean_out, double* sd_out,
                double* corr_out);
int gd_pca_project(gd_ctx* ctx, const int32_t* cols, int32_t np, const int32_t* maps, const double* mean, const double* sd,
                   const double* U, int32_t doexp, int32_t n_all, const double* all_means, const double* all_sd,
                   double* newmean_out, double* newsd_out, double* pcpc_out, double* pcpar_out);

/* ---------------------------------------------------------------- Gaussian mixtures -------------
 * gd_mixture_nll: minus the log of a K-component, d-dimensional Gaussian-mixture density at every resident sample row of
 *   [row_lo, row_hi) (gaussian_mixtures.MixtureND.logLikes, MixtureND.MCSamples(logLikes=True); the reference forms
 *   -log(pdf) with one einsum per component, gaussian_mixtures.py:135-155):
 *     out[r - row_lo] = -log sum_k exp(logcoef[k] - 1/2 |W_k (x_r - mu_k)|^2),   x_r = the columns cols[0..d) of row r,
 *   mu_k = means[k d ..], W_k = whiten[k d d ..] row-major LOWER-TRIANGULAR (entries above the diagonal are not read) with
 *   W_k = L_k^-1 for cov_k = L_k L_k^T, logcoef[k] = log(weight_k) - log(norm_k).  The sum over components is a max-shifted
 *   log-sum-exp: the result stays finite where exp(-chi^2 / 2) underflows (chi^2 above ~1490).  Sample weights are not
 *   involved.  The selected columns are read from HBM once for all K components (a block stages its rows' columns in LDS),
 *   there is no N x d temporary, W and mu are read through the scalar cache, fp64 throughout with a summation order fixed
 *   by (d, K): reruns are bit-identical.  `out` is host memory (page-locked for a full-rate copy).  Returns GD_ERR_BADARG,
 *   before any launch, when no samples are uploaded, d is outside 1..uploaded columns (or above 1280: one 16-row tile of
 *   d columns must fit in LDS), K < 1, a column index is out of range or the row range is empty or outside the sample set.
 *   Blocks until the result is in `out`. */
int gd_mixture_nll(gd_ctx* ctx, const int32_t* cols, int32_t d, int32_t K, const double* means, const double* whiten,
                   const double* logcoef, int64_t row_lo, int64_t row_hi, double* out);

/* ---------------------------------------------------------------- weight-one sample draws -------
 * gd_draw_single_rows: the rows that makeSingleSamples (mcsamples.py:578-606) and random_single_samples_indices
 *   (chains.py:918-939) keep: row i of the resident sample set is kept when  rand_i <= threshold_i,  with the sample weight
 *   w_i (1 when the set is unweighted; the sample weights also while auxiliary weights are selected) and
 *     mode 0: threshold_i = w_i / (a * b)     (the array branch, mcsamples.py:606, and chains.py:939)
 *     mode 1: threshold_i = (w_i / a) / b     (the file branch, mcsamples.py:600)
 *   in IEEE fp64 with exactly these operations (the two orders round differently, and both are the reference's).
 *   rand is np.random.default_rng(random_state).random(N): either pcg_state = {state_hi, state_lo, inc_hi, inc_lo}, the two
 *   128-bit words of a PCG64 bit_generator.state["state"], from which every thread regenerates its rows' variates bit for bit
 *   (csrc/pcg64.hpp; the generator itself is then N steps further: bit_generator.advance(N)), or d_rand, a device vector
 *   of N doubles drawn on the host by any other bit generator -- exactly one of the two is given.
 *   d_rows (device, `capacity` int32 entries) receives the kept row numbers in ascending order and *count_out their count
 *   K.  Nothing is written at or beyond `capacity`: when K > capacity the call writes no row, sets *count_out = K and
 *   returns GD_DRAW_MORE_ROWS; call again with room for K.  GD_ERR_BADARG when no samples are uploaded, both or neither
 *   source of variates is given, the mode is unknown, or the set has 2^31 rows or more (row numbers are int32).  Two reads
 *   of the weights, no N-sized temporary.  Blocks until the list is complete.
 * gd_gather_rows: d_out (device, K x m fp64, row-major) = the resident columns cols[0..m) (any order, repeats allowed;
 *   spare columns included) at the rows of the device list d_rows (K int32); a row number outside the sample set gives NaN.
 *   K = 0 does nothing.  Blocks until d_out is written. */
#define GD_DRAW_MORE_ROWS (-21)
int gd_draw_single_rows(gd_ctx* ctx, const uint64_t* pcg_state, const void* d_rand, double a, double b, int32_t mode,
                        void* d_rows, int64_t capacity, int64_t* count_out);
int gd_gather_rows(gd_ctx* ctx, const void* d_rows, int64_t K, const int32_t* cols, int32_t m, void* d_out);

/* ---------------------------------------------------------------- chain export: text on the device -------
 * The text that np.savetxt(fmt="%W.Pe") makes of sample rows (chains.py:1063-1085 saveAsText, mcsamples.py:596-601 the file
 * branch of makeSingleSamples) or of a matrix, formatted on the device: every value is Python's "%W.Pe" % x byte for
 * byte (csrc/fmtdouble.hpp: correctly rounded from the exact binary value, ties to even, at least two exponent digits,
 * "inf" / "-inf" / "nan" without a sign on NaN, upper case for `upper`), right-justified to `width`; with sep = 1 one
 * space separates the fields of a row (np.savetxt), with sep = 0 nothing does ("%16.7E" rows); every row ends with '\n'.
 * prec is 0..17, width 0..32; a field takes at most max(width, prec + 8) + 1 bytes, separator or newline included, so
 * rows * m * that many bytes always fit.
 * gd_format_rows: field j of a row is srcs[j]: a resident column (spare columns included: gd_set_extra_column is how a
 *   loglike vector gets there), GD_FMT_SRC_WEIGHT = the sample weights (1.0 when the set is unweighted; the sample weights
 *   also while auxiliary weights are selected), or the constants GD_FMT_SRC_ZERO = 0.0 / GD_FMT_SRC_ONE = 1.0.  The rows are
 *   either the contiguous range [row_lo, row_hi) (d_rows NULL) or the K rows of the device int32 list d_rows, in list order
 *   (row_lo = row_hi = 0); a listed row number outside the sample set formats every field as NaN, as gd_gather_rows does.
 * gd_format_matrix: the K x m fp64 matrix at d_x (device), element (r, c) at d_x[r * row_stride + c * col_stride].
 * d_out (device, `capacity` bytes) receives the text and *bytes_out its size.  Nothing is written at or beyond `capacity`:
 *   when the text is longer the call writes nothing, sets *bytes_out to the size needed and returns GD_FORMAT_MORE_BYTES.
 * GD_ERR_BADARG, before any launch: no samples uploaded, a column or code out of range, an empty or out-of-range row
 *   interval, both or neither row selector, prec or width out of range, m < 1, or so many fields that one row of them
 *   does not fit in LDS (about 900 at the widest format).  A list or matrix with K = 0 gives 0 bytes.
 * A block owns a tile of rows and transposes through LDS (column-major loads, row-major text); a first pass counts the
 *   bytes of every tile, one block scans them, a second pass formats again and writes.  Blocks until the text is complete. */
#define GD_FORMAT_MORE_BYTES (-22)
#define GD_FMT_SRC_WEIGHT (-1)
#define GD_FMT_SRC_ZERO (-2)
#define GD_FMT_SRC_ONE (-3)
int gd_format_rows(gd_ctx* ctx, const int32_t* srcs, int32_t m, int64_t row_lo, int64_t row_hi, const void* d_rows, int64_t K,
                   int32_t width, int32_t prec, int32_t upper, int32_t sep, void* d_out, int64_t capacity, int64_t* bytes_out);
int gd_format_matrix(gd_ctx* ctx, const void* d_x, int64_t K, int32_t m, int64_t row_stride, int64_t col_stride,
                     int32_t width, int32_t prec, int32_t upper, int32_t sep, void* d_out, int64_t capacity, int64_t* bytes_out);

/* ---------------------------------------------------------------- chain ingestion: text parsed on the device -------
 * The doubles that np.loadtxt (chains.py:115-125 loadNumpyTxt) makes of whitespace-separated decimal text, parsed from a
 * block of text resident on the device: every value is correctly rounded (ties to even; overflow gives +-inf, underflow
 * +-0, "-0" keeps its sign, "nan" / "inf" / "infinity" in any letter case) by integer arithmetic only (csrc/parsedouble.hpp).
 * Separators are space, '\t', '\v', '\f' and a '\r' directly before '\n'; '#' opens a comment that runs to the end of the
 * line; a line without a token is skipped.  A text is NOT PLAIN, and both calls then return GD_PARSE_NOT_PLAIN with
 * nothing written, when rows differ in their number of fields, a '\r' is not followed by '\n', a byte is NUL or >= 0x80,
 * a token is outside np.loadtxt's grammar for a float field ("1_0", hex, "1d5", "1e", ...) or a line is longer than
 * GD_PARSE_MAX_LINE bytes, its '\n' included (a block stages the lines it owns through LDS): the caller then parses the file
 * on the host.
 * gd_parse_scan: scans d_text[0, nbytes) from its start up to its last '\n'; with last != 0 the text ends the file and a
 *   final line without '\n' is included.  *rows_out = data rows, *fields_out = fields per row (0 when there is no row),
 *   *consumed_out = bytes consumed (nbytes with `last`; otherwise the offset behind the last '\n', from where the caller
 *   continues once more text has arrived; 0 when there is no '\n').
 * gd_parse_rows: parses the same block again -- nbytes is what the scan consumed, rows and m what it reported -- and stores
 *   field j of data row r at d_out[j * ld + row_offset + r] (fp64, the column-major layout of the context and of the
 *   binary cache).  A token the 128-bit fast path cannot decide (about one in 2^73 of random text, but every exact tie
 *   scaled by a negative power of ten, a token of more than 19 digits at or next to a tie -- where its first 19 digits and
 *   their successor round apart, about one long token in a thousand -- and whatever lies outside 1e-310 .. 1e345) is
 *   stored as NaN and listed: entry k of d_fix (device, fix_capacity entries of four int64) = {row_offset + r, j, byte
 *   offset of the token in d_text, its length}, in no particular order.  *fix_count_out counts them all, also beyond
 *   fix_capacity -- the list is then short and the caller knows.  The call scans first, so a text that is not plain leaves
 *   d_out untouched.
 * GD_ERR_BADARG before any launch: null pointers, negative sizes, ld < row_offset + rows; after the scan: rows, m or nbytes
 *   that are not what the scan of this block reports.  Neither call needs an uploaded sample set.  nbytes = 0 does nothing.
 * Tiles of 24 KiB of text; a first pass counts the rows of every tile, one block scans the counts, a second pass parses
 *   and stores with lanes running along rows.  Both calls block until their results are complete. */
#define GD_PARSE_NOT_PLAIN (-23)
#define GD_PARSE_MAX_LINE 8192
int gd_parse_scan(gd_ctx* ctx, const void* d_text, int64_t nbytes, int32_t last, int64_t* rows_out, int32_t* fields_out,
                  int64_t* consumed_out);
int gd_parse_rows(gd_ctx* ctx, const void* d_text, int64_t nbytes, int32_t last, int64_t rows, int32_t m, void* d_out, int64_t ld,
                  int64_t row_offset, void* d_fix, int64_t fix_capacity, int64_t* fix_count_out);

/* ---------------------------------------------------------------- column expressions ------------
 * gd_expr_eval: one fused pass that evaluates a postfix program per sample row over resident columns (colexpr.ColumnExpr:
 * the derived vector  p.sigma8 * np.sqrt(p.omegam / 0.3)  and the mask  p.H0 > 70  of the GetDist idiom, without host
 * arithmetic and without an N-vector crossing PCIe).  Not in the reference, which forms such vectors with numpy.
 * `code` holds ncode (op, arg) pairs of int32; `consts` the nconst doubles GD_EX_CONST refers to.
 *   GD_EX_COL    pushes column `arg` of the row: a resident column, spare columns n + slot included, or GD_EX_WEIGHT = the
 *                sample weights (1.0 for a unit-weight set; the sample weights also while auxiliary weights are selected,
 *                as in gd_format_rows).
 *   GD_EX_CONST  pushes consts[arg].
 *   unary ops    replace the top:  NEG (flips the sign bit), ABS (clears it), SQRT, SQUARE (x * x), RECIP (1 / x), EXP, LOG,
 *                LOG10, LOG2, SIN, COS, TAN, ATAN, TANH, NOT (x == 0 ? 1 : 0).
 *   binary ops   pop b, then a, and push:  ADD SUB MUL DIV POW ATAN2(a, b), MIN / MAX (a NaN operand gives NaN: numpy's
 *                minimum / maximum, not fmin / fmax), LT LE GT GE EQ NE (1.0 / 0.0; with a NaN operand false, NE true),
 *                AND / OR of (a != 0), (b != 0).
 *   GD_EX_WHERE  pops b, a, c and pushes c != 0 ? a : b.
 * + - * / sqrt are the IEEE operations (the library is built with -ffp-contract=off: nothing is fused), so programs of
 * the ops up to MAX, the comparisons, logic and WHERE give numpy's values bit for bit; the transcendental ops are the
 * device library's.  Division by zero and invalid operands give inf / NaN silently (no warning channel).
 * Limits: ncode <= GD_EX_MAX_CODE, stack depth <= GD_EX_MAX_STACK, nconst <= GD_EX_MAX_CONST, and at most GD_EX_MAX_COLS
 * distinct GD_EX_COL arguments (GD_EX_WEIGHT counts as one).
 * Destination `dst`:
 *   GD_EX_TO_COLUMN    spare column slot dst_arg (addressed as column n + dst_arg afterwards); may be a slot the program
 *                      reads (rows are independent).
 *   GD_EX_TO_AUXW      the auxiliary weight buffer receives sample weight * value -- what gd_aux_weights takes from the
 *                      host; created and zeroed as there, refused while gd_select_weights(ctx, 1) is in force.
 *   GD_EX_TO_HOST_F64  host_out receives the hi - lo values as doubles.
 *   GD_EX_TO_HOST_U8   host_out receives one byte per row, value != 0.
 * The device destinations cover every row: they need lo = 0, hi = N, write only rows < N (the zero padding up to the
 * leading dimension stays zero) and return once the kernel has run; the host ones take any [lo, hi) and block until
 * host_out is filled (page-locked memory for a full-rate copy).
 * stats_out (may be NULL) receives {minimum, maximum, number of non-zero values, number of NaNs} of the evaluated rows;
 * minimum and maximum are NaN when a value is NaN (np.min / np.max).  Per-block partials added on the host in block
 * order, no floating-point atomics: reruns are bit-identical.
 * GD_ERR_BADARG before any launch: a null argument, no samples uploaded, an empty or out-of-range row range (or one that
 * is not [0, N) for a device destination), ncode or nconst out of range, an unknown op, a column, constant or slot out
 * of range, too many distinct columns, stack underflow, depth above GD_EX_MAX_STACK, or a final depth other than 1.
 * One kernel: 256 threads, two rows per lane (16-byte loads), the program in the kernel arguments (scalar instruction
 * fetch, wave-uniform dispatch), the columns it reads staged per block in LDS, the evaluation stack with its top in
 * registers and the rest in LDS as [depth][thread]; grid-stride over at most 2048 blocks. */
#define GD_EX_MAX_CODE 128
#define GD_EX_MAX_STACK 16
#define GD_EX_MAX_CONST 32
#define GD_EX_MAX_COLS 16
#define GD_EX_WEIGHT (-1)
#define GD_EX_COL 0
#define GD_EX_CONST 1
#define GD_EX_NEG 2
#define GD_EX_ABS 3
#define GD_EX_SQRT 4
#define GD_EX_SQUARE 5
#define GD_EX_RECIP 6
#define GD_EX_EXP 7
#define GD_EX_LOG 8
#define GD_EX_LOG10 9
#define GD_EX_LOG2 10
#define GD_EX_SIN 11
#define GD_EX_COS 12
#define GD_EX_TAN 13
#define GD_EX_ATAN 14
#define GD_EX_TANH 15
#define GD_EX_NOT 16
#define GD_EX_ADD 17
#define GD_EX_SUB 18
#define GD_EX_MUL 19
#define GD_EX_DIV 20
#define GD_EX_POW 21
#define GD_EX_ATAN2 22
#define GD_EX_MIN 23
#define GD_EX_MAX 24
#define GD_EX_LT 25
#define GD_EX_LE 26
#define GD_EX_GT 27
#define GD_EX_GE 28
#define GD_EX_EQ 29
#define GD_EX_NE 30
#define GD_EX_AND 31
#define GD_EX_OR 32
#define GD_EX_WHERE 33
#define GD_EX_NUM_OPS 34
#define GD_EX_TO_COLUMN 0
#define GD_EX_TO_AUXW 1
#define GD_EX_TO_HOST_F64 2
#define GD_EX_TO_HOST_U8 3
int gd_expr_eval(gd_ctx* ctx, const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int32_t dst,
                 int32_t dst_arg, int64_t lo, int64_t hi, void* host_out, double* stats_out);

/* gd_expr_eval_tab: gd_expr_eval with table look-ups -- np.interp(expr, xp, fp), Density1D.Prob(expr) and
 * Density2D.Prob(ex, ey) of colexpr.py.  Same arguments, destinations, tallies and errors, plus `ntab` tables of host
 * doubles and three more ops whose argument is the table slot (their codes and these limits are NOT part of the GD_EX_
 * set: gd_expr_eval keeps refusing them as unknown ops):
 *   GD_TAB_INTERP   pops x, pushes np.interp(x, p0, p1, left, right): p0 = the nx knots (non-decreasing), p1 = the nx
 *                   values.  numpy's arr_interp step for step: NaN gives NaN (nx == 1: p1[0], as numpy does), x below
 *                   / above the knots gives left / right, the interval is the largest j with p0[j] <= x, x equal to a
 *                   knot (and the last knot) gives p1[j] without arithmetic, else slope * (x - p0[j]) + p1[j] with
 *                   numpy's retry from the right-hand knot when that is NaN.
 *   GD_TAB_SPLINE1  pops x, pushes derivative `deriv` (0 .. 3) of the piecewise cubic with the nx knots p0 and the
 *                   4 (nx - 1) coefficients p1 = {y, c1, c2, c3} per interval: with k = the interval of x and
 *                   t = x - p0[k], y + t (c1 + t (c2 + t c3)); 0.0 outside [p0[0], p0[nx - 1]], NaN for NaN
 *                   (densities.NotAKnotSpline, whose host evaluation is the same expression).
 *   GD_TAB_SPLINE2  pops y, then x, pushes the bicubic tensor-product B-spline with knots p0 (nx of them), p1 (ny) and
 *                   the (nx - 4) (ny - 4) coefficients p2 at (x, y), as FITPACK's fpbisp evaluates one point
 *                   (scipy's RectBivariateSpline.ev): arguments clamped to the knot range, fpbspl's recursion with its
 *                   equal-knot guard, the 16 terms summed as sp = sp + (c hx) hy in fpbisp's loop order.
 * Nothing is contracted into an fma, so all three equal numpy / scipy bit for bit.  `kind` of a table is the op that
 * may refer to it.  The tables are copied into the context's scratch on its stream ahead of the launch and are not kept.
 * GD_ERR_BADARG before any launch, in addition to gd_expr_eval's: ntab outside 0 .. GD_TAB_MAX_TABLES, tables NULL with
 * ntab > 0, a table slot out of range, a table whose kind is not the op's, a null table pointer, nx < 1 (INTERP), nx < 4
 * (SPLINE1), nx or ny < 8 (SPLINE2), a table of more than GD_TAB_MAX_DOUBLES doubles in all, deriv outside 0 .. 3, knots
 * that are not finite or not non-decreasing.  With ntab == 0 the call IS gd_expr_eval: the same kernel runs. */
#define GD_TAB_INTERP 34
#define GD_TAB_SPLINE1 35
#define GD_TAB_SPLINE2 36
#define GD_TAB_MAX_TABLES 4
#define GD_TAB_MAX_DOUBLES 4194304
typedef struct gd_expr_table {
    int32_t kind;  /* GD_TAB_INTERP / GD_TAB_SPLINE1 / GD_TAB_SPLINE2 */
    int32_t deriv; /* SPLINE1: the derivative order; else 0 */
    int32_t nx, ny;
    const double* p0; /* host pointers, see above; unused ones may be NULL */
    const double* p1;
    const double* p2;
    double left, right; /* INTERP: the values below p0[0] / above p0[nx - 1] */
} gd_expr_table;
int gd_expr_eval_tab(gd_ctx* ctx, const int32_t* code, int32_t ncode, const double* consts, int32_t nconst, int32_t dst,
                     int32_t dst_arg, int64_t lo, int64_t hi, void* host_out, double* stats_out, const gd_expr_table* tables,
                     int32_t ntab);

/* ---------------------------------------------------------------- stand-alone convolutions -------
 * The device-backed forms of getdist/convolve.py's public functions (host arrays in and out; the Python module
 * getdist_amd/convolve.py does the padding, the centring roll and the mode slices exactly as convolve.py:196-444).
 * gd_circ_convolve: out = irfft(rfft(a) * rfft(b)) for two real frames of n0 x n1 doubles (n0 == 1: one dimension,
 *   any n1 >= 2) -- the transform pair behind convolveFFT / convolveFFTn / convolve1D_periodic / convolve2D_periodic
 *   (convolve.py:371-436, 215-367), through rocFFT.
 * gd_convolve1d_direct: out_full[i] = sum_j x[j] y[i-j], i < nx + ny - 1: what np.convolve evaluates when an operand
 *   is shorter than 1000 samples (convolve.py:199-202).
 * gd_autoconvolve: autoConvolve(x, n, normalize) (convolve.py:458-478): result[k] = sum_i x_i x_{i+k} [/ (N - k)],
 *   k < n, through a real FFT of length s = nearestFFTnumber(2 N) (passed in: the table lives in the Python module).
 *   x_host != NULL: that vector of nx values; else the resident column `col` as (x - mean) * w (use_weights != 0) --
 *   the vector getAutocorrelation builds (chains.py:439-441) -- without it ever existing on the host. */
int gd_circ_convolve(gd_ctx* ctx, int32_t n0, int32_t n1, const double* a, const double* b, double* out);
int gd_convolve1d_direct(gd_ctx* ctx, const double* x, int64_t nx, const double* y, int64_t ny, double* out_full);
int gd_autoconvolve(gd_ctx* ctx, int32_t col, double mean, int32_t use_weights, const double* x_host, int64_t nx, int64_t s,
                    int64_t n, int32_t normalize, double* out);

/* gd_like_stats: the sample-likelihood numbers of MCSamples._setLikeStats (mcsamples.py:2216-2243) from the column
 *   `col` holding loglikes (an extra column, gd_set_extra_column) and the selected weights, in two passes:
 *   out8 = {min L, max L, sum w, sum w L, sum w L^2, sum w exp(L - min L), sum w exp(-(L - min L)),
 *           first row index attaining min L (np.argmin)}. */
int gd_like_stats(gd_ctx* ctx, int32_t col, double* out8);


/* ---------------------------------------------------------------- one native entry for a batch of pairs ----------
 * gd_density2d_batch: MCSamples.get2DDensityGridData (mcsamples.py:1748-2010) for P parameter pairs in ONE call, with
 * every host decision of the reference made inside the library (csrc/batch2d.hpp):
 *   - the per-pair correlation handling, angle_scale and the up-scaling of the fine grid (mcsamples.py:1796-1816),
 *   - the bin edges of _binSamples (mcsamples.py:1486-1498) and the 2D histograms (:1724-1728), index columns cached
 *     per (parameter, grid size) and shared by the pairs of a triangle,
 *   - the effective sample numbers of the parameters that have none yet (_get1DNeff -> getEffectiveSamplesGaussianKDE,
 *     chains.py:477-574, mcsamples.py:1230-1235), on the first stream BESIDE the binning on the second,
 *   - getAutoBandwidth2D (mcsamples.py:1285-1419): branch A (sheared re-binning + Cholesky de-rotation), B (rule of
 *     thumb), C (KernelOptimizer2D on the pair's own grid), the fallback widths and the higher-order widening,
 *   - window half-widths and frame sizes, batches of equal frame size, the convolution / boundary correction /
 *     multiplicative bias correction / normalisation of gd_density2d_enqueue (mcsamples.py:1857-1990) on two streams,
 *     the optimiser's launch cut in two so that the first half is convolved while the second is optimised,
 *   - the D2H copies of the finished grids into ONE page-locked block of the caller, batch by batch on the copy streams.
 * The call returns when everything is enqueued; the grids are complete after gd_copy_wait(ctx, tokens_out[0]) and, when
 * `twin` was given, gd_copy_wait(twin, tokens_out[1]).
 *
 * ctx    : the context holding the samples.  twin: a second context on the same device attached to it
 *          (gd_attach_samples) = the second stream; NULL runs everything on one stream.
 * params : n records, index = column number; only the columns that occur in `pairs` are read.  `neff` is in/out: NaN on
 *          entry = not known yet, computed here when the bandwidth is automatic (smooth_scale_2D < 0).  `owned` != 0
 *          marks the parameters whose N_eff THIS rank computes in a multi-rank job; the others arrive through `exchange`.
 * corr / cov : the n x n correlation and covariance matrices of the columns (chains.py:155-169, 709-733), row-major.
 * lag_probe  : optional n x 8 autocovariance lag sums (gd_autocov_lags_batch of all columns, lags 0..7) a caller may have
 *          prefetched beside its quantile select; NULL = computed here.
 * pairs  : P x 2 column indices (x, y).
 * exchange : optional; called exactly once per call, on the calling thread, after this rank's own N_eff kernels are
 *          through: it receives the n-vector of N_eff values (NaN = unknown here) and fills in the other ranks' values
 *          (an all-gather); return non-zero to abort.  NULL with settings->comm_exchange and a communicator on the context
 *          (gd_comm_init): the library exchanges them itself (ncclAllReduce on the context's stream).
 * grids_pinned : page-locked block of >= sum F_k^2 doubles (F_k from gd_batch2d_grid_sizes); pair k's grid lands at
 *          meta[k][1] doubles from its start, F x F row-major, [y][x].
 * status_pinned : P int32, page-locked; after the copies have landed status_pinned[(int)meta[k][30]] is GD_OK or
 *          GD_ERR_EMPTY ("no samples in bin", densities.py:83-84) for pair k.  Until a batch of convolutions has run its
 *          words hold 0x7fffffff: the call pre-sets them and the batch's last launch overwrites them -- the library's own
 *          threads read the words of the first batches to learn that those batches have RUN (the deferred shear chain starts
 *          then), so the block has to be host-visible while the call runs, as page-locked memory is.
 * meta   : P x GD_BATCH2D_META doubles:
 *          [0] F  [1] offset of the grid  [2..4] (hx, hy, corr) of the kernel in parameter units (NaN when the scale is fixed)
 *          [5] bandwidth branch 0/1/2 = A/B/C (-1: fixed scale)  [6..17] the optimiser's record as gd_kopt2d writes it
 *          [18..20] window scales rx, ry in fine-bin units and the window's correlation  [21] window half-width
 *          [22] bits: 1 = "Parameters are 100% correlated", 2 = "fine_bins_2D not large enough", 4 = fallback widths used
 *          [23..26] xbinmin, xbinmax, ybinmin, ybinmax  [27] the pair's correlation as used for the grid  [28] nbin2D
 *          [29] 0 / 1 = the grid's copy runs on ctx's / twin's copy stream  [30] index into status_pinned  [31] N_eff used
 * levels / level_status : when settings->want_levels, P x ncontours contour levels (gd_contour_levels) and P states.
 * Errors: GD_ERR_BADARG "bias not positive definite" (kde_bandwidth.py:229-230) and setting errors; GD_ERR_SOLVER when
 *   raise_on_bandwidth_errors and the optimiser found no root; GD_ERR_FFT + 1000 * ... never; a parameter whose chain
 *   correlation outlasts the 8-lag probe returns GD_BATCH2D_NEED_NEFF with its column in gd_last_error -- the caller
 *   computes that N_eff (getCorrelationLength's long route) and calls again. */
#define GD_BATCH2D_META 32
#define GD_BATCH2D_NEED_NEFF (-20)

typedef struct gd_param2d {
    double range_min, range_max; /* par.range_min / range_max after _initParam (mcsamples.py:1421-1484) */
    double param_min, param_max; /* column extrema */
    double sigma_range, err;     /* par.sigma_range, par.err */
    double mean, var;            /* weighted mean and variance of the column (the N_eff probe) */
    double neff;                 /* par.N_eff_kde; NaN = unknown (in/out) */
    int32_t has_limits_bot, has_limits_top, periodic;
    int32_t owned; /* bit 0: this rank computes the parameter's N_eff; bit 1: no bandwidth warning / error for it (1D) */
} gd_param2d;

typedef struct gd_batch2d_settings {
    int32_t fine_bins_2D, boundary_correction_order, mult_bias_correction_order, num_bins_2D;
    double smooth_scale_2D, max_corr_2D;
    double norm, sum_w2;                /* sum w, sum w^2 of the sample weights (chains.py:312,499) */
    int32_t uncorrelated_sampler;       /* sampler in ("nested", "uncorrelated"): N_eff = norm^2 / sum_w2 (chains.py:507-508) */
    int32_t raise_on_bandwidth_errors;
    int32_t want_levels, ncontours;     /* contour levels on the device instead of lazily delivered grids */
    const double* contours;
    /* choreography (defaults in parentheses; 0 = default) */
    int32_t two_streams_min;            /* (64)  pairs from which the convolution uses both streams */
    int32_t two_streams_split;          /* (400) pairs above which the optimiser's launch is cut in two */
    int32_t kopt_split_min;             /* (256) ... when the base grid's launch has at least this many pairs */
    double kopt_first_fraction;         /* (0.5) */
    int32_t first_batch, max_batch;     /* (128, 320) grids in the first / in every further convolution batch */
    double max_batch_bytes;             /* (24e9) device scratch a batch may take */
    int32_t comm_exchange;              /* 1: exchange the N_eff values over the context's communicator (gd_comm_init): one
                                           sum all-reduce of n doubles, every rank contributing the parameters it owns */
    int32_t bandwidths_only;            /* 1: stop when the bandwidths are known -- meta[2..5], [18..22], [31] are filled, nothing is
                                           convolved or copied (a caller that edits each pair's prior mask, mcsamples.py:1767-1770,
                                           needs the window half-widths first and then convolves through gd_density2d_masked) */
    /* optional per-pair inputs (NULL = none); with smooth_scale_2D < 0 only */
    const double* pair_neff;            /* P effective sample numbers instead of min(N_eff x, N_eff y): the caller's 2D estimate
                                           under use_effective_samples_2D (mcsamples.py:1322-1328, chains.py:576-635) */
    const double* bandwidths;           /* P x 3 (hx, hy, corr) in parameter units instead of getAutoBandwidth2D */
    int32_t results_in_flight;          /* 1: the caller has not waited for the PREVIOUS batched call's result copies (a stream of
                                           calls): this call's first grids queue behind those copies anyway, so the deferred
                                           shear chain starts when the first part's convolution is enqueued (throughput) instead
                                           of when it has run (0: the first grids of THIS call are what its delivery waits for) */
} gd_batch2d_settings;

typedef int (*gd_neff_exchange_fn)(void* user, double* neff_n, int32_t n);

/* F_out[k] = the fine grid size pair k will get (mcsamples.py:1796-1816: 256, or 192 * (3 / angle_scale) // 3 for
 * strongly correlated pairs); host only. */
int gd_batch2d_grid_sizes(const gd_batch2d_settings* settings, int32_t n, const double* corr, const int32_t* pairs,
                          int32_t P, int32_t* F_out);
int gd_density2d_batch(gd_ctx* ctx, gd_ctx* twin, const gd_batch2d_settings* settings, gd_param2d* params, int32_t n,
                       const double* corr, const double* cov, const double* lag_probe, const int32_t* pairs, int32_t P,
                       gd_neff_exchange_fn exchange, void* exchange_user, void* grids_pinned, int64_t grids_doubles,
                       int32_t* status_pinned, double* meta, double* levels, int32_t* level_status, int32_t* tokens_out2);
/* ---------------------------------------------------------------- one native entry for a batch of 1D densities ----
 * gd_density1d_batch: MCSamples.get1DDensityGridData (mcsamples.py:1500-1686) for B parameters in ONE call, the host
 * decisions of the reference made inside the library (csrc/batch1d.hpp):
 *   - the bin edges of _binSamples (mcsamples.py:1486-1496) and the fused index + weighted bincount (:1554),
 *   - with smooth_scale_1D <= 0: the effective sample numbers of the parameters that have none yet (as gd_density2d_batch
 *     computes them), the Botev ISJ bandwidth (gd_isj1d) and the scalar tail of getAutoBandwidth1D (:1256-1283: the rule
 *     of thumb when the solver fails or the width is very small, the higher-order rescaling); otherwise the fixed scales
 *     of :1572-1582,
 *   - the smoothing scale in fine-bin units, the window half-width, and everything of gd_density1d (:1588-1668).
 * The histograms stay in device memory between the three stages.  Blocking: P_out is complete on return.
 *
 * params : n records as for gd_density2d_batch, index = column number; only the listed columns are read.  `neff` is in/out
 *          (NaN = not known; computed here when the bandwidth is automatic; GD_BATCH2D_NEED_NEFF as for the 2D entry).
 * cols   : B column indices (a parameter may be listed once).  P_out : B x F doubles (host), normalised to max = 1.
 * hist_out : optional B x F doubles (host): the histograms (the mean-likelihood profiles of gd_likes1d need them).
 * meta   : B x GD_BATCH1D_META doubles: [0] binmin [1] binmax [2] the bandwidth h in units of the bin range (par.kde_h;
 *          NaN when the scale is fixed) [3] smooth_1D in fine-bin units [4] window half-width
 *          [5] bits: 1 = "1D auto bandwidth failed" (solver returned None), 2 = very small or failed: rule-of-thumb
 *          fallback used, 4 = "fine_bins not large enough to well sample smoothing scale"
 *          [6] N_eff used (NaN when the scale is fixed) [7] GD_OK or GD_ERR_EMPTY ("no samples in bin") for the density
 *          [8] with bit 2: the solver's own width that the fallback replaced (NaN = it returned None) -- the "h=" of the
 *          reference's message "auto bandwidth for X very small or failed (h=..,N_eff=..). Using fallback (h=..)" (:1262).
 *          A parameter whose record has (owned & 2) set is one the caller lists in no_warning_params (or a chi2 parameter
 *          under no_warning_chi2_params, :1259-1261): the fallback is then taken without bit 2 and without an error.
 * Errors: GD_ERR_BADARG for setting errors ("Parameter range is <= 0", an unknown boundary_correction_order); GD_ERR_SOLVER
 *   when raise_on_bandwidth_errors is set and the fallback would have been used. */
#define GD_BATCH1D_META 9

typedef struct gd_density1d_settings {
    int32_t fine_bins, num_bins, boundary_correction_order, mult_bias_correction_order;
    double smooth_scale_1D;
    double norm, sum_w2;           /* sum w, sum w^2 of the sample weights (N_eff of parameters that have none yet) */
    int32_t uncorrelated_sampler;  /* as gd_batch2d_settings */
    int32_t raise_on_bandwidth_errors;
} gd_density1d_settings;

int gd_density1d_batch(gd_ctx* ctx, const gd_density1d_settings* settings, gd_param2d* params, int32_t n, const int32_t* cols,
                       int32_t B, double* P_out, double* hist_out, double* meta);

/* Completes the last batched call(s) of the context (waits for their result copies, hands their device blocks back to
 * the library's pool); gd_batch2d_invalidate additionally marks every cached index column stale (the next call bins
 * again -- what a benchmark does between steps, and what gd_upload does by itself). */
int gd_batch2d_finish(gd_ctx* ctx);
int gd_batch2d_invalidate(gd_ctx* ctx);
/* How many times gd_density2d_batch has ENTERED its own N_eff collective (settings->comm_exchange) on this context, counted
 * when the all-reduce is issued -- i.e. also for a call that failed afterwards (a matrix that is not positive definite, a
 * bandwidth error, GD_BATCH2D_NEED_NEFF from the columns nobody owned).  A multi-rank caller reads it around a call to
 * learn whether this rank has already taken part in the step's collective, so that its error path neither skips nor
 * repeats it ("exactly once per rank and step"; the reference has no such exchange: mcsamples.py:1230-1235 is per process). */
int gd_batch2d_exchanges(gd_ctx* ctx, int64_t* count_out);

/* The per-parameter preparation of the densities (MCSamples._initParam for a list of whole sample columns) in one call:
 * the quantile select with the autocovariance probe riding on it (exactly gd_quantiles_mm_probe with 11 targets per column:
 * the range_confidence quantile, its mirror, the deciles 0.1 .. 0.9), then the scalar tail in fp64 with Python's own
 * operations in Python's order: spans of four deciles, scale / 1.049, the flat test, sigma_range, the limit decisions
 * against smooth_1D, the widened ranges.  recs[c] arrives with has_limits_bot / has_limits_top as the prior ranges set them
 * (limits: ncols x 2, the prior bounds where the flags are set) and leaves final.
 *
 * With settings->ahead the entry then ENQUEUES, without waiting, what the next gd_density2d_batch over these columns starts
 * with, because it needs nothing but what is known here:
 *   - the byte-index columns of the base grid (fine_bins_2D = 256, enough columns for the 64 pairs of the byte-index route;
 *     unit weights only -- a sample set with real weights, which the batched call also bins from byte indices, gets the lag
 *     sums alone) on `twin`'s stream, into the index-column cache of ctx's batched calls;
 *   - behind them, on ctx's own stream, the first launch of the N_eff lag sums (automatic bandwidths, a correlated sampler,
 *     probe delivered, no chain that outlasts it), partial sums copied to page-locked memory by a kernel behind the launch.
 * gd_density2d_batch uses a piece when its own arguments are the same to the bit (the columns -- in any order --, their
 * kernel widths, the lags, N; bin minimum and width per column) -- results are those of a call without the pieces, bit for
 * bit: the partial sums are added per column in the same block order -- and otherwise waits for the
 * piece's event, discards it and proceeds as it would have.  Every replacement of the samples or weights and gd_destroy drop
 * pending pieces after their events.  GDHIP_PREPARE_AHEAD=0 in the environment: nothing is enqueued ahead. */
typedef struct gd_prepared_param {
    double range_min, range_max, sigma_range;
    int32_t has_limits_bot, has_limits_top;
} gd_prepared_param;

typedef struct gd_prepare_settings {
    int32_t fine_bins_2D;
    int32_t auto_bandwidth;       /* smooth_scale_2D < 0 and nothing injected: the batched call will want N_eff */
    int32_t uncorrelated_sampler; /* sampler "nested" / "uncorrelated": N_eff needs no lag sums */
    int32_t ahead;                /* bit 0: the N_eff lag sums, bit 1: the index columns */
} gd_prepare_settings;

int gd_prepare_params(gd_ctx* ctx, gd_ctx* twin, const gd_prepare_settings* settings, const int32_t* cols, int32_t ncols,
                      const double* targets, const double* minmax, const double* means, const double* vars, const double* err,
                      const double* limits, double* quantiles_out, double* probe_out, int32_t* probe_done,
                      gd_prepared_param* recs);
/* out3 = pieces enqueued ahead, consumed by a batched call, discarded (mismatch, edit, teardown) on this context so far */
int gd_prepare_ahead_counts(gd_ctx* ctx, int64_t* out3);


/* ---------------------------------------------------------------- multi-GPU: RCCL over xGMI ------------------------
 * One process per GPU.  The path has no data-path collective: pairs are partitioned and every rank copies
 * its own grids to its host.  What is exchanged are small per-rank vectors -- the partial moments of a row share
 * (chains.py:709-733 pooled over ranks), the per-parameter state _initParam leaves (mcsamples.py:1421-1484; ~12 doubles
 * per parameter) and the N_eff values (one double per parameter) -- by ALL-GATHER, and additive partial tables
 * (histograms, bucket counts: chains.py:793-838, mcsamples.py:1486-1498,1724-1728) by SUM ALL-REDUCE.
 * gd_comm_unique_id: rank 0 obtains the 128-byte RCCL id and hands it to the other ranks by whatever means the host
 *   application has (torch.distributed's store, MPI, a file); gd_comm_init: every rank then joins with it (collective).
 * gd_comm_allgather: recv[r * count ..] = rank r's `send` (host vectors; staged through the context's device block, the
 *   collective itself runs on device memory on the context's stream: ncclAllGather).  gd_comm_allreduce_sum likewise.
 * The *_dev forms take device pointers and return once enqueued on the context's stream.
 * With a communicator on the context gd_density2d_batch exchanges the N_eff values itself when `exchange` is NULL. */
/* gd_comm_rccl_path: the file the collectives resolve to and whether it was already mapped by the process (the host
 *   application's RCCL, e.g. PyTorch's bundled copy: the library never maps a second RCCL beside it).
 * gd_comm_init runs ncclCommInitRank under a watchdog and the host-vector collectives poll the stream and the
 *   communicator's asynchronous error state instead of blocking: a rank that never arrives or dies is an error return
 *   (GD_ERR_HIP, after GDHIP_COMM_TIMEOUT_S seconds, default 120; the communicator is aborted and dropped), not a hang.
 * gd_upload_shard + gd_comm_share_columns: sample distribution over xGMI -- rank r uploads only its block of columns
 *   [first[r], first[r+1]) (column-major, column stride col_stride >= N; weights by every rank), then every rank
 *   broadcasts its block to the others (W ncclBroadcast in one group).  After gd_comm_share_columns the context holds the
 *   full set exactly as after gd_upload of the whole array (chains.py:276-300: one sample array per process). */
int gd_comm_rccl_path(char* buf, int32_t len, int32_t* preloaded_out);
int gd_upload_shard(gd_ctx* ctx, const double* X_cols, int64_t N, int64_t n, int64_t col_first, int64_t col_count,
                    int64_t col_stride, const double* weights);
int gd_comm_share_columns(gd_ctx* ctx, const int64_t* first_by_rank /* world + 1 entries */);
int gd_comm_unique_id(void* id128_out);
int gd_comm_init(gd_ctx* ctx, int32_t world, int32_t rank, const void* id128);
int gd_comm_info(gd_ctx* ctx, int32_t* world_out, int32_t* rank_out);
/* gd_comm_abandon: the one entry point that may be called from ANOTHER thread while a gd_comm_* call of this context has not
 * returned (a binding-side watchdog giving up on gd_comm_init): the stuck call, should it come back, installs no communicator
 * and returns GD_ERR_TIMEOUT.  (The reference has no multi-process path; this belongs to the build's RCCL seam) */
int gd_comm_abandon(gd_ctx* ctx);
int gd_comm_destroy(gd_ctx* ctx);
int gd_comm_allgather(gd_ctx* ctx, const double* send, int64_t count, double* recv);
int gd_comm_allreduce_sum(gd_ctx* ctx, double* inout, int64_t count);
int gd_comm_allgather_dev(gd_ctx* ctx, const void* d_send, int64_t count, void* d_recv);
int gd_comm_allreduce_sum_dev(gd_ctx* ctx, const void* d_send, int64_t count, void* d_recv);

#ifdef __cplusplus
}
#endif
#endif /* GDHIP_H */
