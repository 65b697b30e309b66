/*
 * dkm.h -- C ABI of libdkm.so, the MI355X (gfx950) k-means Lloyd hot path.
 *
 * Drop-in boundary for dislib's k-means (reference: /root/reference,
 * dislib v0.2.0).  The reference is pure Python over PyCOMPSs tasks; the
 * functions below replace its per-Subset task bodies and its reduction tree.
 * Each entry cites the reference function it replaces.
 *
 * Conventions
 *  - All array pointers are DEVICE pointers (hipMalloc / torch CUDA tensors)
 *    unless documented otherwise.  The caller owns every buffer; the library
 *    never allocates or frees caller memory.  A scratch area ("workspace") of
 *    dkm_workspace_bytes() bytes is provided by the caller.
 *  - Every call is asynchronous and stream-ordered on `stream` (a
 *    hipStream_t passed as void*; NULL = the legacy default stream).
 *  - Every call returns 0 on success, or a nonzero DKM_E_* / hipError_t code;
 *    dkm_last_error() returns a thread-local message for the last failure.
 *    No C++ exception ever crosses this boundary.
 *  - Matrices are row-major with a leading dimension (elements) `ld`.
 */
#ifndef DKM_H
#define DKM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DKM_ABI_VERSION 9

/* error codes (besides hipError_t values passed through) */
#define DKM_OK 0
#define DKM_E_ARG 10001       /* invalid argument / shape                    */
#define DKM_E_WORKSPACE 10002 /* workspace too small                         */
#define DKM_E_LAUNCH 10003    /* kernel launch failed                        */
#define DKM_E_PARSE 10004     /* malformed input text (loaders)              */
#define DKM_E_COMM 10005      /* RCCL missing or an RCCL call failed         */

/* assignment modes (flags) */
#define DKM_MODE_AUTO 0     /* library picks: SCREEN32 when profitable       */
#define DKM_MODE_EXACT 1    /* direct ||x-c||^2 in numpy's pairwise order for
                               every (sample, centre): reference arithmetic   */
#define DKM_MODE_SCREEN32 2 /* fp32 ||c||^2-2x.c screen with a rigorous error
                               bound; ambiguous samples re-checked with the
                               EXACT arithmetic.  Labels identical to EXACT. */
#define DKM_MODE_SCREEN_BF16X3 3 /* same, x.c from bf16 hi/lo splits on the
                               bf16 MFMA (hi*hi + hi*lo + lo*hi); its own
                               bound; labels identical to EXACT.            */
#define DKM_MODE_SCREEN_BF16 4 /* same, one bf16 product per term (hi*hi):
                               a third of the matrix work, a looser bound;
                               the candidates it leaves are re-checked with
                               the EXACT arithmetic.  Labels identical.     */
#define DKM_MODE_MASK 0xff  /* the arithmetic; flags may be OR'ed above it:  */
#define DKM_MODE_NOHINT 0x100 /* the incoming labels of dkm_partial_sum /
                               dkm_assign_delta are not used as hints (the
                               caller knows them to be poor, e.g. labels of
                               the initial centres): no threshold pass    */
#define DKM_MODE_B1 0x200   /* the single-product screen in its
                               centres-on-rows form (k_screen_b1, the
                               fallback when k_screen_b2's LDS image does
                               not fit) for every shape; identical labels */
#define DKM_MODE_TRANSLATE 0x400 /* with DKM_MODE_SCREEN_BF16 (or the AUTO
                               choice of it), no sorted image: the centres-
                               on-lanes screen scores ||c||^2 - 2 x.(c - m)
                               with m the centres' mean (the same order of
                               the centres for every sample; x.m is common to
                               all of them), so its bf16 rounding error
                               scales with max ||c - m|| instead of
                               max ||c||: crowded centres (the reference's
                               U[0, 1) initial centres) leave far fewer
                               samples to the re-checks.  Labels identical */

/* sum-dtype flags for dkm_update_centers (reference keeps X's dtype for the
 * partial sums; base.py:178 and :147) */
#define DKM_SUMS_F64 0
#define DKM_SUMS_F32 1  /* fp32 samples: centre = fl32(fl32(sum)/fl32(count)) */
#define DKM_SUMS_RECIP 2 /* sparse: centre = sum * (1.0/count) (scipy divide) */

int dkm_abi_version(void);

/* Load every kernel's code object now instead of at its first launch (the
 * runtime loads a source file's kernels lazily, several ms per file: the
 * first Lloyd iterations paid it inside the fit).  Optional; idempotent.
 * Replaces nothing in the reference (PyCOMPSs workers import their
 * libraries before the first task). */
int dkm_preload(void);
const char *dkm_last_error(void);

/* Workspace needed for k centres of d features and up to n_queue re-check
 * slots (n_queue = 0 lets the library pick).  Host function. */
size_t dkm_workspace_bytes(int64_t k, int64_t d, int64_t n_queue);

/* prepare flags */
#define DKM_PREP_CSR 1 /* prepare for the CSR kernels only: the transposed
                          centres C^T (fp64 and fp32, d rows, stride k
                          rounded up to 16) and |c|^2, without the dense
                          screens' centre tiles                            */

/* Derive per-iteration centre data (fp32 copy, |c|^2 in sklearn's sequential
 * order, error-bound scalars, optionally C^T) into the workspace and ZERO the
 * accumulator acc[k*(d+1)] ([sums | counts]) when acc != NULL.  Replaces the
 * implicit per-task centre broadcast of base.py:110,114 (and sklearn's
 * row_norms of the centres, recomputed per sample by the reference).
 * For dkm_bounds_ok(k, d) shapes it also computes every centre's drift
 * since the last dkm_assign_delta_bounds_* call on this workspace.        */
int dkm_prepare_centers(const double *C, int64_t k, int64_t d, int flags,
                        void *ws, size_t ws_bytes, double *acc, void *stream);

/* Fused assignment + per-cluster sum/count for dense samples.
 * Replaces `_partial_sum` (cluster/kmeans/base.py:166-181), including
 * `_vec_matrix_euclid` (:204-205), `np.argmin` (:173) and `set_label` (:176).
 * Accumulates into acc = [sums k*d | counts k] (fp64, += semantics; call
 * dkm_prepare_centers first in an iteration).  labels (int32[n]) may be NULL
 * when not wanted.  X is fp64 (…_f64) or fp32 (…_f32); C is always fp64.  */
int dkm_partial_sum_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                        const double *C, int64_t k, const void *ws,
                        size_t ws_bytes, int32_t *labels, double *acc,
                        int mode, void *stream);
int dkm_partial_sum_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                        const double *C, int64_t k, const void *ws,
                        size_t ws_bytes, int32_t *labels, double *acc,
                        int mode, void *stream);

/* Incremental form of dkm_partial_sum for the Lloyd loop.  labels (int32[n],
 * in/out) holds each sample's previous label (-1 = none); on return it holds
 * the new labels (identical to dkm_partial_sum's) and delta (k*(d+1), +=)
 * has received +x / +1 for every sample that joined a cluster and -x / -1
 * for every sample that left one, so acc_new = acc_old + delta is the
 * [sums | counts] of the new assignment (up to fp64 rounding order).  After
 * the first iterations few labels change, so almost no sample is added
 * anywhere; the caller refreshes acc from scratch periodically.           */
int dkm_assign_delta_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                         const double *C, int64_t k, const void *ws,
                         size_t ws_bytes, int32_t *labels, double *delta,
                         int mode, void *stream);
int dkm_assign_delta_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                         const double *C, int64_t k, const void *ws,
                         size_t ws_bytes, int32_t *labels, double *delta,
                         int mode, void *stream);

/* The sample image: a resident bf16 copy of X in the operand order of the
 * screen that reads it, plus fp32 |x|^2 per row.  Built once per dataset
 * (it depends only on X): the screen then streams 2 or 4 B per feature
 * instead of sizeof(X) and skips the conversion.  Labels, sums and
 * re-checks still come from X itself, so results are identical with or
 * without it.  An image is valid only for the exact X, n and d (and kind)
 * it was built from; rebuild it if X changes.
 *   kind DKM_IMAGE_SINGLE: bf16(fl32(x)) for the label-hinted
 *     single-product screen (MODE_SCREEN_BF16 or the AUTO choice when the
 *     sums exceed LDS; d <= 128);
 *   kind DKM_IMAGE_SPLIT: bf16 hi and lo of fl32(x) for the d <= 32
 *     bf16x3 screen (MODE_SCREEN_BF16X3 or the AUTO choice), read by its
 *     delta / labels-only launches;
 *   kind DKM_IMAGE_GEMM: bf16(fl32(x)) in the 256-row tiles of the
 *     single-product GEMM screen (d > 128: MODE_SCREEN_BF16 or AUTO), plus
 *     an fp32 upper bound of ||x|| per row (2 B per feature + 4 B per row;
 *     10M x 1024: 20.5 GB).
 * dkm_x_image_kind(k, d, mode) says which kind the selected screen reads
 * (DKM_IMAGE_NONE: building one would be wasted).  The _img forms of
 * dkm_partial_sum / dkm_assign_delta take it (image NULL = none); every
 * other argument is theirs.  Same interface as base.py:166-181.
 * image_kind | DKM_IMAGE_BUILD: the image memory is allocated but not built
 * yet; the call builds it (the d <= 32 bf16x3 screen's full-sums pass writes
 * the split image while it converts X anyway -- no separate pass over X --
 * any other call builds it first with dkm_x_image_*), after which the
 * caller passes the kind without the flag.                                */
#define DKM_IMAGE_NONE 0
#define DKM_IMAGE_SINGLE 1
#define DKM_IMAGE_SPLIT 2
#define DKM_IMAGE_SORTED 3
#define DKM_IMAGE_GEMM 4
#define DKM_IMAGE_BUILD 0x100
int dkm_x_image_kind(int64_t k, int64_t d, int mode);
size_t dkm_x_image_bytes(int64_t n, int64_t d, int kind);
int dkm_x_image_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                    int kind, void *image, size_t image_bytes, void *stream);
int dkm_x_image_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                    int kind, void *image, size_t image_bytes, void *stream);
/* The label-sorted image (DKM_IMAGE_SORTED, dkm_x_image_bytes(n, d, 3)
 * bytes): the DKM_IMAGE_SINGLE image of X with its rows grouped by
 * `labels` (a counting sort in the workspace, which needs n label slots:
 * dkm_workspace_bytes(k, d, n_queue >= n)), plus the row order and a copy of
 * the labels in that order.  The single-product screen then screens 32-row
 * tiles of (mostly) one label and skips every 32-centre block the triangle
 * inequality proves farther than that label's centre.  The labels never
 * depend on the grouping.  The image's label copy is maintained by the
 * calls that take the image: once built, pass it to EVERY call that updates
 * those labels (MODE_SCREEN_BF16 or AUTO; other modes refuse it), or build
 * it again.  dkm_x_image_sorted_ok(k, d): whether (k, d) takes it.        */
int dkm_x_image_sorted_ok(int64_t k, int64_t d);
int dkm_x_image_sorted_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                           const int32_t *labels, int64_t k, const void *ws,
                           size_t ws_bytes, void *image, size_t image_bytes,
                           void *stream);
int dkm_x_image_sorted_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                           const int32_t *labels, int64_t k, const void *ws,
                           size_t ws_bytes, void *image, size_t image_bytes,
                           void *stream);
/* The same image, and acc += the full [sums | counts] of X by `labels` (the
 * dkm_label_sums_* result) in the same pass over X: a fit that builds the
 * image from an iteration's labels gets that iteration's sums without a
 * second read of X (predict, then this call, instead of partial_sum, then
 * dkm_x_image_sorted_*).  Sums are fp64 atomics: equal to dkm_label_sums_*
 * up to the order of the additions.                                        */
int dkm_x_image_sorted_sums_f64(const double *X, int64_t n, int64_t d,
                                int64_t ldx, const int32_t *labels, int64_t k,
                                const void *ws, size_t ws_bytes, void *image,
                                size_t image_bytes, double *acc, void *stream);
int dkm_x_image_sorted_sums_f32(const float *X, int64_t n, int64_t d,
                                int64_t ldx, const int32_t *labels, int64_t k,
                                const void *ws, size_t ws_bytes, void *image,
                                size_t image_bytes, double *acc, void *stream);
/* image_bytes: the image buffer's size, checked against
 * dkm_x_image_bytes(n, d, image_kind) (an image built for other n or d is
 * refused instead of read out of bounds).                                 */
int dkm_partial_sum_img_f64(const double *X, const void *image, int image_kind,
                            size_t image_bytes, int64_t n, int64_t d,
                            int64_t ldx, const double *C, int64_t k,
                            const void *ws, size_t ws_bytes, int32_t *labels,
                            double *acc, int mode, void *stream);
int dkm_partial_sum_img_f32(const float *X, const void *image, int image_kind,
                            size_t image_bytes, int64_t n, int64_t d,
                            int64_t ldx, const double *C, int64_t k,
                            const void *ws, size_t ws_bytes, int32_t *labels,
                            double *acc, int mode, void *stream);
int dkm_assign_delta_img_f64(const double *X, const void *image,
                             int image_kind, size_t image_bytes, int64_t n,
                             int64_t d, int64_t ldx, const double *C,
                             int64_t k, const void *ws, size_t ws_bytes,
                             int32_t *labels, double *delta, int mode,
                             void *stream);
int dkm_assign_delta_img_f32(const float *X, const void *image, int image_kind,
                             size_t image_bytes, int64_t n, int64_t d,
                             int64_t ldx, const double *C, int64_t k,
                             const void *ws, size_t ws_bytes, int32_t *labels,
                             double *delta, int mode, void *stream);

/* dkm_assign_delta_img_* with per-row distance bounds (Hamerly's pair) kept
 * by the caller between the calls of one Lloyd loop: ub[i] >= the distance
 * of row i to its label's centre, lb[i] <= its distance to every other
 * centre (fp32[n] each, 16-B aligned like labels; rank-local).  A row with
 * ub < lb provably keeps its label and is neither read nor scored; every
 * other row goes through the screen and the exact re-check as in
 * dkm_assign_delta_img_*, so labels and delta are identical to that call's.
 *   bounds_flags = DKM_BOUNDS_INIT: ub / lb hold nothing yet (first call, or
 *     the labels were written by any other call since the last one): every
 *     row is screened from the image and gets its bounds.
 *   bounds_flags = 0: the previous call on (ws, labels, ub, lb) was a bounds
 *     call.  The drift of every centre since that call is computed by
 *     dkm_prepare_centers from the centres the workspace kept (never taken
 *     from the caller: any centre set is covered; a drift that is not
 *     finite makes every row active), the bounds pass moves ub / lb by it
 *     and lists the rows with !(ub < lb), and the list is screened from X.
 *     When more than 45 % of the rows are active (the measured crossover;
 *     DKM_BOUNDS_LIST_FRAC in the environment overrides it), the image
 *     screen over all rows runs instead; the choice is made on the device.
 *     DKM_BOUNDS_INIT calls run no bounds pass and are not counted by
 *     dkm_bounds_counters.
 * Shapes: dkm_bounds_ok(k, d) (d <= 32, 2 <= k <= 256 and [sums | counts]
 * that fit LDS beside the centres: k <= 192 at d = 32; any ldx), mode
 * AUTO or SCREEN_BF16X3 without flags, a built DKM_IMAGE_SPLIT image, a
 * workspace with n label slots (dkm_workspace_bytes(k, d, n_queue >= n));
 * anything else is refused with DKM_E_ARG.  Replaces the same reference
 * code as dkm_assign_delta_* (base.py:166-181).
 * dkm_bounds_counters (host, syncs `stream`): over the workspace's life,
 * out[0] calls that ran the bounds pass, out[1] rows it left active, out[2]
 * rows it skipped, out[3] calls whose active rows were screened as a list
 * (out has 4 entries).
 * A row the screen cannot decide goes to the exact re-check.  When the
 * re-check's fp32 stage decides it (its two best fp32 scores over all k
 * centres lie more than twice the fp32 bound apart), that stage writes the
 * row's ub / lb from those scores; only a row left to the reference
 * arithmetic (a tie or near-tie under fp32, a non-finite value) keeps
 * (+inf, 0) and is screened again at the next call.  DKM_BOUNDS_SETTLE=0 in
 * the environment (read at every call) leaves every re-checked row at
 * (+inf, 0).  dkm_bounds_settled (host, syncs `stream`): the rows the
 * re-check gave bounds to, over the workspace's life.                       */
#define DKM_BOUNDS_INIT 1
int dkm_bounds_ok(int64_t k, int64_t d);
int dkm_assign_delta_bounds_f64(const double *X, const void *image,
                                int image_kind, size_t image_bytes, int64_t n,
                                int64_t d, int64_t ldx, const double *C,
                                int64_t k, const void *ws, size_t ws_bytes,
                                int32_t *labels, double *delta, int mode,
                                float *ub, float *lb, int bounds_flags,
                                void *stream);
int dkm_assign_delta_bounds_f32(const float *X, const void *image,
                                int image_kind, size_t image_bytes, int64_t n,
                                int64_t d, int64_t ldx, const double *C,
                                int64_t k, const void *ws, size_t ws_bytes,
                                int32_t *labels, double *delta, int mode,
                                float *ub, float *lb, int bounds_flags,
                                void *stream);
int dkm_bounds_counters(const void *ws, int64_t *out, void *stream);
int dkm_bounds_settled(const void *ws, int64_t *n_settled, void *stream);

/* acc[k*(d+1)] += [sums | counts] of the rows of X by labels (label < 0 or
 * >= k: skipped): the sums half of dkm_partial_sum for known labels.       */
int dkm_label_sums_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                       const int32_t *labels, int64_t k, const void *ws,
                       size_t ws_bytes, double *acc, void *stream);
int dkm_label_sums_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                       const int32_t *labels, int64_t k, const void *ws,
                       size_t ws_bytes, double *acc, void *stream);

/* -----------------------------------------------------------------------
 * The reference's own summation order (KMeans sums="reference"): centres
 * bit-identical to dislib's, from run to run and for any number of ranks.
 * No floating-point atomic; no result depends on a grid or block size.
 *
 * dkm_ordered_sums_*: the sums half of `_partial_sum` (base.py:166-181:
 * `partials[label][0] += sample`, `partials[label][1] += 1`) for every
 * Subset at once.  subset_off (device int64[n_subsets + 1], ascending,
 * subset_off[0] = 0, subset_off[n_subsets] = n) cuts the rows of X into
 * Subsets.  For Subset s, cluster c and column j the rows of s with label c
 * are added in ascending row order in ONE sequential chain that starts from
 * +0.0 (the reference's integer 0 placeholder adds like +0.0, so no partial
 * holds -0.0): an fp64 chain for fp64 rows; for fp32 rows a true fp32 chain
 * (every add rounded to fp32, subnormals kept), stored widened, which is
 * exact.  Integer samples uploaded as fp64 are exact while |sum| < 2^53.
 * partials (n_subsets x k (d + 1) fp64, every element written): Subset s at
 * partials + s k (d + 1), laid out [sums k x d | counts k] like `acc`; the
 * counts are integers.  Labels outside [0, k) are skipped, as in
 * dkm_label_sums_*.  ws: dkm_ordered_workspace_bytes(n, n_subsets, k, d)
 * bytes (0: shape refused -- n < 2^31 - 1, k <= 8191); after the call its
 * first n int32 hold the row indices grouped stably by (Subset, label)
 * (labels outside [0, k) last in their Subset).  Cost: one more read of X,
 * and the parallelism is n_subsets x k x d chains -- one Subset is slow by
 * definition of the order.                                                */
size_t dkm_ordered_workspace_bytes(int64_t n, int64_t n_subsets, int64_t k,
                                   int64_t d);
int dkm_ordered_sums_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                         const int32_t *labels, int64_t k,
                         const int64_t *subset_off, int64_t n_subsets,
                         void *ws, size_t ws_bytes, double *partials,
                         void *stream);
int dkm_ordered_sums_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                         const int32_t *labels, int64_t k,
                         const int64_t *subset_off, int64_t n_subsets,
                         void *ws, size_t ws_bytes, double *partials,
                         void *stream);
/* The reduction loop of `_recompute_centers` with `_merge` (base.py:137-141,
 * 184-191): acc[len] <- the root of the arity tree over the n_partials
 * buffers of `len` fp64 each; one thread per element walks the tree.
 * `schedule` (device int32) is the tree, flattened on the host: n_ops ops
 * [dst, count, src_0 .. src_{count-1}], each folding its sources left to
 * right (acc = src_0; acc += src_1; ...).  A source i < n_partials is
 * partials[i], else slot i - n_partials of `scratch` (slots of `len` fp64);
 * dst is a scratch slot, or -1 for `acc` (the last op).  n_ops = 0 (one
 * partial): acc <- partials[0].  sums_f32: the leading elements of every
 * buffer that fold in fp32 (k d for fp32 samples -- the reference's fp32
 * sums merge in fp32 --, 0 otherwise); the rest (the integer counts) fold
 * in fp64.  The schedule is trusted: its indices are not checked.          */
int dkm_merge_tree(const double *partials, int64_t n_partials, int64_t len,
                   const int32_t *schedule, int64_t n_ops, int64_t sums_f32,
                   double *scratch, double *acc, void *stream);

/* -----------------------------------------------------------------------
 * StandardScaler on resident samples (reference
 * dislib/preprocessing/classes.py).  X is fp64 (..._f64) or fp32 (..._f32),
 * row-major with any ldx >= d; three pure streams over X, no floating-point
 * atomic.  Compiled without fast-math and with IEEE fp32 divide and sqrt.
 *
 * dkm_col_stats_*: the fast column statistics.  out[d] (fp64) <- the column
 * sums of x (mean = NULL: `_partial_sum`, classes.py:114-116, summed over
 * all Subsets at once, which also replaces `_merge_sums`, :119-123) or of
 * (x - mean[j])^2 (mean: device fp64[d]; `_partial_var` and `_merge_vars`,
 * :126-134), accumulated in fp64 whatever X's dtype (fp32 samples are
 * widened, which is exact; the mean stays fp64).  Every block writes its
 * partial sums into ws (dkm_scale_workspace_bytes(n, d) bytes) and a second
 * kernel adds them in a fixed order; the grid is a function of (n, d) only,
 * so the same call gives the same bits every time.  The order is not the
 * reference's: results agree with it to rounding, not bit for bit.  n = 0
 * gives zeros.                                                            */
size_t dkm_scale_workspace_bytes(int64_t n, int64_t d);
int dkm_col_stats_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                      const double *mean, void *ws, size_t ws_bytes,
                      double *out, void *stream);
int dkm_col_stats_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                      const double *mean, void *ws, size_t ws_bytes,
                      double *out, void *stream);
/* dkm_col_chain_*: the same statistics in the reference's order, for every
 * Subset at once: `np.sum(subset.samples, axis=0)` (classes.py:116) when
 * mean = NULL, `np.sum((subset.samples - mean) ** 2, axis=0)` (:129) else.
 * subset_off (device int64[n_subsets + 1]) cuts the rows as in
 * dkm_ordered_sums_*.  Each (Subset, column) is ONE sequential chain in
 * ascending row order from +0.0 (numpy's order for a C-contiguous matrix of
 * two or more columns), in the samples' dtype: fp32 chains round every add
 * to fp32, and the subtraction and the square are each rounded in that
 * dtype before the add (mean: a device vector of X's dtype).  Subset s is
 * written to partials[s * ldp .. s * ldp + d) (fp64; fp32 results are
 * widened, which is exact; ldp >= d, the other elements are untouched), the
 * layout dkm_merge_tree folds (`_merge_sums`, `_merge_vars`, :119-134).  No
 * result depends on a grid or block size.  The parallelism is n_subsets x d
 * chains: few Subsets are slow by definition of the order.                */
int dkm_col_chain_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                      const double *mean, const int64_t *subset_off,
                      int64_t n_subsets, double *partials, int64_t ldp,
                      void *stream);
int dkm_col_chain_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                      const float *mean, const int64_t *subset_off,
                      int64_t n_subsets, double *partials, int64_t ldp,
                      void *stream);
/* dkm_scale_transform_*: Y = (X - mean) / sqrt(var), element by element
 * (`_transform`, classes.py:144-147).  The sqrt is taken once per column in
 * the statistics' dtype, the subtraction and the one divide per element in
 * numpy's promotion of the two dtypes, all IEEE correctly rounded; a zero
 * variance gives numpy's NaN / inf.  _f64: fp64 samples and statistics;
 * _f32: fp32 both, fp32 Y; _f32_f64: fp32 samples, fp64 statistics, fp64 Y;
 * _f64_f32: fp64 samples, fp32 statistics (an fp32 sqrt), fp64 Y.  Y is
 * n x d with leading dimension ldy >= d and may be X itself (same ld).    */
int dkm_scale_transform_f64(const double *X, int64_t n, int64_t d,
                            int64_t ldx, const double *mean,
                            const double *var, double *Y, int64_t ldy,
                            void *stream);
int dkm_scale_transform_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                            const float *mean, const float *var, float *Y,
                            int64_t ldy, void *stream);
int dkm_scale_transform_f32_f64(const float *X, int64_t n, int64_t d,
                                int64_t ldx, const double *mean,
                                const double *var, double *Y, int64_t ldy,
                                void *stream);
int dkm_scale_transform_f64_f32(const double *X, int64_t n, int64_t d,
                                int64_t ldx, const float *mean,
                                const float *var, double *Y, int64_t ldy,
                                void *stream);

/* ------------------------------------------------------------------------
 * GaussianMixture, covariance_type='full' (dislib/cluster/gm/base.py): the
 * three passes of an EM iteration over resident rows, all fp64 on the f64
 * MFMA (fp32 rows are widened in the loads, as numpy promotes them).  No
 * floating-point atomic: partials of fixed row ranges added in a fixed
 * order, grids that depend on (n, d, k) only -- the same input gives the
 * same bits from run to run.  One workspace serves the three.
 * --------------------------------------------------------------------- */
#define DKM_GM_UPPER 1 /* every precisions_chol[c] is upper triangular: the
                          E-step skips the rows below each 16-column panel  */
size_t dkm_gm_workspace_bytes(int64_t n, int64_t d, int64_t k);
/* Replaces _estimate_responsibilities (:201-237) for every row:
 *   y = (x - means[c]) . precisions_chol[c],
 *   wlp[c] = -(d log(2 pi) + sum y^2) / 2 + log_det_w[c]
 *            (log_det_w = log det chol + log weight, k values),
 *   lse = max + log(sum_c exp(wlp[c] - max)), resp[row][c] = exp(wlp[c] - lse)
 * (resp: n x k, row-major), labels[row] = the first maximum of resp[row]
 * (int64, nullable), *log_prob_sum (device) = the sum of the rows' lse.     */
int dkm_gm_estep_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                     const double *means, const double *precisions_chol,
                     const double *log_det_w, int64_t k, int flags, void *ws,
                     size_t ws_bytes, double *resp, int64_t *labels,
                     double *log_prob_sum, void *stream);
int dkm_gm_estep_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                     const double *means, const double *precisions_chol,
                     const double *log_det_w, int64_t k, int flags, void *ws,
                     size_t ws_bytes, double *resp, int64_t *labels,
                     double *log_prob_sum, void *stream);
/* Replaces _estimate_parameters_subset (:19-29) over all rows:
 * out[0 .. k) = the column sums of resp, out[k .. k + k d) = resp^T X.     */
int dkm_gm_mstep_sums_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                          const double *resp, int64_t k, void *ws,
                          size_t ws_bytes, double *out, void *stream);
int dkm_gm_mstep_sums_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                          const double *resp, int64_t k, void *ws,
                          size_t ws_bytes, double *out, void *stream);
/* Replaces _estimate_covariances_full (:103-117) over all rows: cov[c] (k x
 * d x d) = sum_n resp[n][c] (x_n - means[c]) (x_n - means[c])^T, computed
 * on and above the diagonal and mirrored.                                  */
int dkm_gm_mstep_cov_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                         const double *resp, const double *means, int64_t k,
                         void *ws, size_t ws_bytes, double *cov,
                         void *stream);
int dkm_gm_mstep_cov_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                         const double *resp, const double *means, int64_t k,
                         void *ws, size_t ws_bytes, double *cov,
                         void *stream);
/* resp[i][c] = (labels[i] == c) ? 1 : 0 (_resp_subset, :770-776).          */
int dkm_gm_onehot(const int32_t *labels, int64_t n, int64_t k, double *resp,
                  void *stream);

/* y[i] += x[i] (device, fp64): acc_new = acc_old + delta.                  */
int dkm_add_f64(double *y, const double *x, int64_t n, void *stream);
/* The same, and *nonzero (device int32) <- 1 if any x[i] != 0, else 0:
 * a delta of all zeros leaves acc bit-identical, so the caller knows that
 * no sample changed cluster since its last full recomputation (its
 * periodic refresh is then skipped: the sums are exactly those of the
 * current assignment).                                                   */
int dkm_add_f64_nz(double *y, const double *x, int64_t n, int32_t *nonzero,
                   void *stream);
/* The running sums kept compensated: (hi, lo) += x by TwoSum, renormalised
 * so that hi = fl(hi + lo) -- hi is what dkm_update_centers reads.  Each
 * add is exact to ~2^-106 |hi|, so the only drift of a delta-updated state
 * against a fresh recomputation is the rounding of the deltas themselves
 * (<= ~2^-52 of the moved rows' magnitude per iteration), not the
 * |sums| x iterations of a plain fp64 add.  nonzero: as dkm_add_f64_nz
 * (NULL = not wanted).                                                   */
int dkm_add_f64_dd(double *hi, double *lo, const double *x, int64_t n,
                   int32_t *nonzero, void *stream);

/* Assignment only.  Replaces `_predict` (base.py:194-201).  Needs a prepared
 * workspace (dkm_prepare_centers with acc = NULL is allowed).             */
int dkm_predict_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                    const double *C, int64_t k, const void *ws,
                    size_t ws_bytes, int32_t *labels, int mode, void *stream);
int dkm_predict_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                    const double *C, int64_t k, const void *ws,
                    size_t ws_bytes, int32_t *labels, int mode, void *stream);

/* Centre recomputation + convergence criterion.  Replaces
 * `_recompute_centers` (base.py:137-147, the division and empty-cluster
 * rule) and the criterion of `_converged` (:122-135):
 *   C[c] = sums[c] / counts[c] for counts[c] != 0 (else unchanged),
 *   diff[1+c] = ||C_new[c] - C_old[c]||_2, diff[0] = sum over c in index
 *   order (diff: device buffer of k+1 doubles), and
 *   *flag = (diff[0] < tol*tol) ? 1 : 0 (flag nullable).
 * For DKM_SUMS_RECIP (sparse input) the per-centre distance follows
 * sklearn's sqrt(max(0, (-2 a.b + |a|^2) + |b|^2)) with sequential sums, as
 * the reference's sparse criterion does (base.py:123 pairwise_distances).
 * acc is the (all-reduced) [sums | counts] buffer.  sums_mode: DKM_SUMS_*. */
int dkm_update_centers(const double *acc, double *C, int64_t k, int64_t d,
                       int sums_mode, double tol, double *diff,
                       int32_t *flag, void *stream);

/* CSR samples (int64 indptr[n+1], int32 indices, fp64 data; d columns).
 * Replaces the sparse branch of `_partial_sum`/`_predict` (base.py:169,196:
 * sklearn euclidean_distances = sqrt(max(0, (-2 x.c + |x|^2) + |c|^2))).  */
int dkm_partial_sum_csr_f64(const int64_t *indptr, const int32_t *indices,
                            const double *data, int64_t n, int64_t d,
                            const double *C, int64_t k, const void *ws,
                            size_t ws_bytes, int32_t *labels, double *acc,
                            void *stream);
/* Incremental CSR form (the fit loop), same contract as
 * dkm_assign_delta_f64: labels in/out (-1 = none), delta += the rows whose
 * label changed (+x to the new cluster, -x from the previous one).       */
int dkm_assign_delta_csr_f64(const int64_t *indptr, const int32_t *indices,
                             const double *data, int64_t n, int64_t d,
                             const double *C, int64_t k, const void *ws,
                             size_t ws_bytes, int32_t *labels, double *delta,
                             void *stream);
int dkm_predict_csr_f64(const int64_t *indptr, const int32_t *indices,
                        const double *data, int64_t n, int64_t d,
                        const double *C, int64_t k, const void *ws,
                        size_t ws_bytes, int32_t *labels, void *stream);
/* Host query: the number of slices (1, 2, 4 or 8) the CSR screen cuts its
 * bf16 C^T of (k, d) into and, when `width` is not NULL, the centres per
 * slice (a multiple of 64; slice s holds centres [s width, (s + 1) width)
 * below k, so the last slices may hold fewer or none).  0 for k < 1 or
 * d < 1.                                                                   */
int dkm_csr_slices(int64_t k, int64_t d, int64_t *width);

/* ------------------------------------------------------------------------
 * Multi-GPU: the one collective of a Lloyd iteration (SURVEY.md section
 * 8(b,e)).  Replaces the `_merge` arity tree and the `compss_wait_on` gather
 * (cluster/kmeans/base.py:137-143, 184-191): an in-place RCCL sum of every
 * GPU's [sums k*d | counts k] buffer; each rank then runs the same
 * dkm_update_centers.  librccl is loaded at the first call (the instance
 * already in the process if any).  Host functions.
 * --------------------------------------------------------------------- */
#define DKM_COMM_ID_BYTES 128

/* One process per GPU: rank 0 creates the id (DKM_COMM_ID_BYTES bytes),
 * the caller hands it to every rank, every rank joins with its device. */
int dkm_allreduce_unique_id(void *id);
int dkm_allreduce_init_rank(const void *id, int nranks, int rank, int device);
/* One process driving ndev GPUs (ncclCommInitAll over devs[]). */
int dkm_allreduce_init(int ndev, const int *devs);
/* buf[0..count) (device memory of `device`) <- sum over all ranks,
 * stream-ordered on `stream` (a hipStream_t of that device). */
int dkm_allreduce_sum_f64(double *buf, int64_t count, int device,
                          void *stream);
/* Destroy every communicator of this process. */
int dkm_allreduce_finalize(void);
/* Destroy the communicator of `device` only (0 when it has none). */
int dkm_allreduce_finalize_device(int device);
/* 0 when librccl loads and has every entry point used here: a cheap,
 * non-blocking check every rank makes before the collective
 * ncclCommInitRank, so that the ranks agree on a fallback up front. */
int dkm_allreduce_available(void);
/* The communicator of `device`: its rank count (ncclCommCount) and this
 * rank's index in it (ncclCommUserRank).  DKM_E_ARG if it has none. */
int dkm_allreduce_comm_info(int device, int *nranks, int *rank);

/* Synthetic make_blobs rows [row0, row0+n) into X (n x d, ld = d), blob ids
 * into blob (nullable).  Counter-based: any row range regenerates
 * identically.  Bench/test data generator, not part of the reference path. */
int dkm_make_blobs_f64(double *X, int64_t row0, int64_t n, int64_t d,
                       int64_t n_blobs, uint64_t seed, double box, double std,
                       int32_t *blob, void *stream);

/* Diagnostics of the last SCREEN32 call on this workspace (device -> host,
 * synchronous on `stream`): number of samples sent to the exact re-check.  */
int dkm_screen_stats(const void *ws, int64_t *n_rechecked, void *stream);
/* Single-product screen counters over the workspace's life (host, syncs
 * `stream`): out[0] tiles given the threshold pass, out[1] tiles it
 * decided (the rest took the top-3 pass), out[2] 32-centre blocks screened
 * by threshold passes over the label-sorted image (DKM_IMAGE_SORTED),
 * out[3] tiles of that image the steady-state pass handed to the general
 * one (out has 4 entries).                                                 */
int dkm_screen_counters(const void *ws, int64_t *out, void *stream);
/* The lists the last single-product screen launch left (host, syncs
 * `stream`; diagnostics): out[0] samples for the exact re-check list,
 * out[1] two-candidate entries, out[2] 3..6-candidate entries, out[3]
 * samples that overflowed a list (found by the label scan).               */
int dkm_screen_lists(const void *ws, size_t ws_bytes, int64_t *out,
                     void *stream);

/* Build flags of this library: 0 for a product build.  DKM_BUILD_TIMING_ONLY
 * when an object was compiled with an A/B timing probe that invalidates
 * results (DKM_AB_B2_PROBE, DKM_AB_SORTED_BSCALE != 1, DKM_AB_SORTED_DBG);
 * DKM_BUILD_AB_VARIANT when any
 * object comes from an A/B variant build (csrc/variants*.sh).  bench.py
 * records a non-zero value in its line, and tests/test_isa_guard.py checks
 * that the in-tree library reports 0. */
#define DKM_BUILD_TIMING_ONLY 1
#define DKM_BUILD_AB_VARIANT 2
int dkm_build_flags(void);

/* ------------------------------------------------------------------------
 * Distance-primitive reuse outside the Lloyd loop (SURVEY.md section 8
 * row f4).  fp64 rows, row-major with leading dimensions; device pointers;
 * stream-ordered.
 * --------------------------------------------------------------------- */

/* Workspace bytes of dkm_knn_f64 (0 for invalid sizes). */
size_t dkm_knn_workspace_bytes(int64_t nq, int64_t nx, int64_t kn);
/* Host query (launches nothing): how dkm_knn_f64 / dkm_knn_csr_f64 cut the
 * fit rows for (nq, nx, kn).  Returns 1 when the call runs passes of <= 32
 * columns (kn <= 32 or kn > 2048), 2 when it takes the two-scan path
 * (32 < kn <= 2048), and writes, where not NULL, the rows per partition and
 * the number of partitions of that path (partition p = rows [p plen,
 * (p + 1) plen) below nx).  A two-scan call whose candidate list outgrows
 * 4096 entries for some query reruns in the passes' partitions, which do not
 * depend on kn (ask with kn = 1).  0 for nq < 1, nx < 1, nx > INT32_MAX or
 * kn outside [1, nx].                                                      */
int dkm_knn_plan(int64_t nq, int64_t nx, int64_t kn, int64_t *plen,
                 int32_t *parts);
/* For each query row of Q (nq x d): the kn (1..32, <= nx) rows of X
 * (nx x d) nearest by dist = sqrt(r), r = sum_t (q_t - x_t)^2 summed
 * sequentially from t = 0 (sklearn KD-tree EuclideanDistance.rdist, the
 * regime sklearn picks for d <= 15), ascending (r, index).  out_dist
 * nq x kn fp64, out_idx nq x kn int64 (row indices of X).
 * Replaces NearestNeighbors.kneighbors: _get_neighbors per Subset pair and
 * _merge_queries (dislib/neighbors/base.py:40-111). */
int dkm_knn_f64(const double *Q, int64_t nq, int64_t ldq, const double *X,
                int64_t nx, int64_t ldx, int64_t d, int64_t kn, void *ws,
                size_t ws_bytes, double *out_dist, int64_t *out_idx,
                void *stream);
/* Sparse kNN, replacing the same reference path on CSR Subsets (sklearn
 * fits brute force on CSR and ranks by pairwise_distances_chunked with
 * squared=True): query CSR (q_indptr[nq+1] int64, q_indices int32 sorted
 * and unique within each row, q_data fp64) against the fit CSR (nx rows),
 * both d columns.  r = max(((-2 q.x) + ||q||^2) + ||x||^2, 0) in the
 * arithmetic of dkm_radius_count_csr_f64; neighbours ascending (r, index),
 * out_dist = sqrt(r).  kn in [1, nx] (passes of 32 beyond 32); workspace =
 * dkm_knn_workspace_bytes(nq, nx, kn).  The query and fit matrices may be
 * the same arrays.  out_f32 != 0: the Subsets were float32 (data passed
 * upcast to fp64): sklearn's upcast path rounds r to float32 before the
 * max, ranks by it and takes the float32 sqrt; so do these. */
int dkm_knn_csr_f64(const int64_t *q_indptr, const int32_t *q_indices,
                    const double *q_data, int64_t nq, const int64_t *x_indptr,
                    const int32_t *x_indices, const double *x_data,
                    int64_t nx, int64_t d, int64_t kn, int out_f32, void *ws,
                    size_t ws_bytes, double *out_dist, int64_t *out_idx,
                    void *stream);

/* DBSCAN epsilon query, replacing _compute_neighbours (dense) of
 * dislib/cluster/dbscan/classes.py:124-141: for query row q, the rows j of
 * X with numpy's sqrt(pairwise-sum((q - x_j)^2)) < eps (_vec_matrix_euclid,
 * :153-154).  Step 1: counts[nq] (int64) <- neighbour counts. */
int dkm_radius_count_f64(const double *Q, int64_t nq, int64_t ldq,
                         const double *X, int64_t nx, int64_t ldx, int64_t d,
                         double eps, int64_t *counts, void *stream);
/* Workspace bytes of dkm_radius_fill_f64 for `total` neighbours. */
size_t dkm_radius_workspace_bytes(int64_t nq, int64_t total);
/* Step 2: offsets[nq+1] = exclusive prefix sum of the counts (device);
 * list q goes to out_idx/out_dist[offsets[q] .. offsets[q+1]), ascending
 * (distance, index).  Reads offsets[nq] to the host (synchronises
 * `stream`). */
int dkm_radius_fill_f64(const double *Q, int64_t nq, int64_t ldq,
                        const double *X, int64_t nx, int64_t ldx, int64_t d,
                        double eps, const int64_t *offsets, void *ws,
                        size_t ws_bytes, int64_t *out_idx, double *out_dist,
                        void *stream);
/* Sparse epsilon query, replacing the `pairwise_distances` branch of
 * _compute_neighbours (dislib/cluster/dbscan/classes.py:130, sparse=True):
 * query rows q0 .. q0+nq of the CSR matrix (indptr[n+1] int64, indices
 * int32 sorted within each row, data fp64, n rows, d columns) against all
 * n rows.  Distance = sklearn 1.7 euclidean_distances for fp64 CSR:
 * sqrt(max(((-2 q.x) + ||q||^2) + ||x||^2, 0)), row norms summed in stored
 * order, q.x by scipy csr_matmat order (increasing column of the
 * intersection).  Same two steps, offsets and workspace as the dense pair.
 * out_f32 != 0 (float32 Subsets, data passed upcast to fp64): r rounded to
 * float32, then max, the float32 sqrt and `dist < float32(eps)`, as
 * sklearn's upcast path and numpy's float32 comparison do. */
int dkm_radius_count_csr_f64(const int64_t *indptr, const int32_t *indices,
                             const double *data, int64_t n, int64_t d,
                             int64_t q0, int64_t nq, double eps, int out_f32,
                             int64_t *counts, void *stream);
int dkm_radius_fill_csr_f64(const int64_t *indptr, const int32_t *indices,
                            const double *data, int64_t n, int64_t d,
                            int64_t q0, int64_t nq, double eps, int out_f32,
                            const int64_t *offsets, void *ws, size_t ws_bytes,
                            int64_t *out_idx, double *out_dist, void *stream);

/* ------------------------------------------------------------------------
 * DBSCAN on the epsilon query's arithmetic, replacing
 * _compute_labels (dislib/cluster/dbscan/classes.py:162-191) with one
 * region: nothing n x n and no neighbour list, O(n) memory, the distances
 * recomputed in each pass.  X is n x d fp64 (n <= INT32_MAX - 64) whose rows
 * the caller has ordered so that neighbouring rows lie close together (by
 * grid cell); orig_index[i] = the Dataset row of ordered row i, a
 * permutation of 0 .. n - 1.  Any order gives the same result: tiles of 64
 * consecutive rows carry a bounding box (first min(d, 16) features), and a
 * tile pair whose boxes are more than eps (1 + 2^-40 on the square) apart
 * is skipped.  The three calls share one workspace and run in this order.
 * --------------------------------------------------------------------- */

/* flags of dkm_dbscan_core_f64 / dkm_dbscan_link_f64: scan every tile pair */
#define DKM_DBSCAN_NOPRUNE 1
/* Workspace bytes (<= 64 n + 2^20; 0 for invalid sizes). */
size_t dkm_dbscan_workspace_bytes(int64_t n, int64_t d);
/* core_out[i] (int32) <- 1 when row i has at least min_samples rows j with
 * dist(i, j) < eps (itself included), by dkm_radius_count_f64's predicate;
 * eps <= 0: none. */
int dkm_dbscan_core_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                        double eps, int64_t min_samples, int flags, void *ws,
                        size_t ws_bytes, int32_t *core_out, void *stream);
/* parent[n] <- a union-find forest over the ordered rows in which two core
 * rows within eps share a root (non-core rows stay their own root);
 * attach[i] <- for a non-core row the core row within eps of the smallest
 * (distance, orig_index), or -1 (core rows: -1). */
int dkm_dbscan_link_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                        double eps, int flags, void *ws, size_t ws_bytes,
                        const int32_t *core, const int32_t *orig_index,
                        int32_t *parent, int32_t *attach, void *stream);
/* labels[orig_index[i]] (int32) <- the cluster of row i: components of the
 * forest with their attached rows, those of fewer than min_samples rows
 * dropped (-1), the others numbered from 0 by their smallest orig_index;
 * *n_clusters (device int32) <- their count.  Path halving writes parent. */
int dkm_dbscan_finalize(int64_t n, int64_t min_samples, void *ws,
                        size_t ws_bytes, const int32_t *core,
                        const int32_t *orig_index, int32_t *parent,
                        const int32_t *attach, int32_t *labels,
                        int32_t *n_clusters, void *stream);

/* ------------------------------------------------------------------------
 * ALS, replacing _update_chunk and _get_rmse of
 * dislib/recommendation/als/base.py:225-253.  The ratings are a CSR matrix
 * (indptr[n_rows+1] int64, indices int32, data fp64); stored entries equal
 * to 0 are skipped everywhere but in the row means, as sparse.find skips
 * them.  An entry whose column is outside the factor matrix (index < 0, or
 * >= m in dkm_als_update_*, >= n_items in dkm_als_sse) is skipped too: it
 * adds nothing to the Gram matrix, to v, to n_c or to the squared error and
 * its count, and no factor row is read for it; a row with such entries only
 * is a row without entries.  Factor rows that no counted entry names are
 * never read.  Column indices need not be sorted, and a column stored twice
 * in a row counts as two entries.
 * Every sum has a fixed order: results are identical from run to run.
 * --------------------------------------------------------------------- */

/* Most latent factors (A and the gather tile share the 160 KiB of LDS). */
#define DKM_ALS_MAX_NF 128
/* Factor rows gathered per pass of dkm_als_update_* (tests walk its edges). */
#define DKM_ALS_CHUNK 16
/* Workspace bytes of dkm_als_sse over n_rows rows; 0 for invalid sizes
 * (n_rows < 0 or > INT32_MAX, n_f outside 1 .. DKM_ALS_MAX_NF).  Host-only. */
size_t dkm_als_workspace_bytes(int64_t n_rows, int64_t n_f);
/* One half-step.  For row i with non-zero entries at columns idx (n_c of
 * them, values r): Y[i] (fp32, n_rows x n_f, contiguous) <- the solution y
 * of (X[idx]^T X[idx] + lambda n_c I) y = X[idx]^T r, with the Gram matrix
 * accumulated, factored (Cholesky) and solved in fp64 and y rounded to fp32
 * on store; zeros for a row without a non-zero entry.  X is m x n_f with
 * row stride ldx, 1 <= n_f <= DKM_ALS_MAX_NF. */
int dkm_als_update_f64(const int64_t *indptr, const int32_t *indices,
                       const double *data, int64_t n_rows, const double *X,
                       int64_t m, int64_t n_f, int64_t ldx, double lambda,
                       float *Y, void *stream);
int dkm_als_update_f32(const int64_t *indptr, const int32_t *indices,
                       const double *data, int64_t n_rows, const float *X,
                       int64_t m, int64_t n_f, int64_t ldx, double lambda,
                       float *Y, void *stream);
/* out[0] (device fp64) <- the sum over the non-zero entries (row, col, r) of
 * CSR rows row_begin <= row < row_end of (r - u . i)^2 with u =
 * users[row - row_begin + user_offset] and i = items[col] (both fp32,
 * contiguous rows of n_f; the dot and the sum in fp64); out[1] <- their
 * count.  user_offset = row_begin indexes users by the CSR row; 0 indexes
 * them by the row's number inside the range, which is how the reference
 * scores the Subsets of its transposed Dataset (base.py:123-126).  Needs
 * row_end - row_begin + user_offset <= n_users. */
int dkm_als_sse(const int64_t *indptr, const int32_t *indices,
                const double *data, int64_t row_begin, int64_t row_end,
                int64_t user_offset, const float *users, int64_t n_users,
                const float *items, int64_t n_items, int64_t n_f, void *ws,
                size_t ws_bytes, double *out, void *stream);
/* out[i] (fp64) <- the mean of row i's stored entries, zeros included; NaN
 * for a row that stores none (np.mean(row.data), base.py:162). */
int dkm_als_row_means(const int64_t *indptr, const double *data,
                      int64_t n_rows, double *out, void *stream);

/* ------------------------------------------------------------------------
 * CascadeSVM: what a node of the cascade needs in place of
 * sklearn.svm.SVC (dislib/classification/csvm/base.py:331-346), the decision
 * values of :350-366 and the convergence quantity of :259-274.  Binary
 * C-SVC.  X is the resident n x d sample matrix (row stride ldx >= d); a
 * node is rows[m], int32 indices into X in any order; node vectors (y, alpha,
 * f) are indexed by the position inside the node.  y is +1 / -1 as fp64,
 * f_i = sum_j alpha_j y_j K_ij - y_i (y times the dual gradient; -y with
 * alpha = 0), so libsvm's -y_i G_i is -f_i.  An index outside its range
 * names a row of zeros and is never dereferenced.  Every sum has a fixed
 * order: results are identical from run to run.
 * --------------------------------------------------------------------- */

#define DKM_SVM_LINEAR 0  /* x_i . x_j                                        */
#define DKM_SVM_RBF 1     /* exp(-gamma (|x_i|^2 + |x_j|^2 - 2 x_i . x_j))     */
/* Largest working set: its q x q block of K (128 KiB) and the staging of the
 * other kernels fit the 160 KiB of LDS. */
#define DKM_SVM_QMAX 128
/* out[i] (fp64) <- |x_i|^2 of every row (an fma chain over the row). */
int dkm_svm_norms_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                      double *out, void *stream);
int dkm_svm_norms_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                      double *out, void *stream);
/* K[a * ldk + j] (fp64, q x m, ldk >= m) <- K(x_rows[ws[a]], x_rows[j]) for
 * the working set ws[q] (positions inside the node; a negative entry is an
 * empty slot whose row of K is not meaningful), 1 <= q <= DKM_SVM_QMAX.
 * norms: dkm_svm_norms_* of X (rbf only).  The dot products run on the fp64
 * MFMA. */
int dkm_svm_rows_f64(const double *X, int64_t n, int64_t d, int64_t ldx,
                     const int32_t *rows, int64_t m, const int32_t *ws,
                     int64_t q, const double *norms, int kernel, double gamma,
                     double *K, int64_t ldk, void *stream);
int dkm_svm_rows_f32(const float *X, int64_t n, int64_t d, int64_t ldx,
                     const int32_t *rows, int64_t m, const int32_t *ws,
                     int64_t q, const double *norms, int kernel, double gamma,
                     double *K, int64_t ldk, void *stream);
/* Working-set selection.  I_up = {y = +1, alpha < C} u {y = -1, alpha > 0},
 * I_low = {y = +1, alpha > 0} u {y = -1, alpha < C}.  gap[0] <- m(alpha) -
 * M(alpha) = max_{I_up} -f - min_{I_low} -f (-inf when either set is empty),
 * gap[1] <- m(alpha), gap[2] <- M(alpha).  ws[0 .. q/2) <- the positions of
 * I_up with the largest -f, ws[q/2 .. 2 (q/2)) <- those of I_low with the
 * smallest -f, taken in turns (up, low, up, ...) so that no position is taken
 * twice; ties go to the lower position; -1 where a set ran out and in the
 * last slot of an odd q.  q >= m: ws = 0 .. m-1, then -1.  mark: m int32 of
 * scratch.  2 <= q <= DKM_SVM_QMAX. */
int dkm_svm_select(const double *f, const double *alpha, const double *y,
                   int64_t m, double C, int64_t q, int32_t *ws, double *gap,
                   int32_t *mark, void *stream);
/* SMO on the working set, one workgroup: libsvm's second-order pair choice
 * (WSS2, TAU = 1e-12 where the curvature is not positive) and two-variable
 * update with clipping to [0, C], on the q x q block K[a * ldk + ws[b]] of
 * dkm_svm_rows_*, until the working set's m - M < eps or max_inner steps.
 * alpha[ws[.]] is updated in place, dy[q] <- y o (alpha_new - alpha_old) (0
 * in empty slots), info[0] <- steps taken, info[1] <- 1 if max_inner ended
 * the loop.  f is read, not written: dkm_svm_update applies dy. */
int dkm_svm_local(const double *K, int64_t ldk, const int32_t *ws, int64_t q,
                  const double *y, double *alpha, const double *f, int64_t m,
                  double C, double eps, int64_t max_inner, double *dy,
                  int32_t *info, void *stream);
/* f[j] += sum_t K[t * ldk + j] dy[t] for j < m, t ascending (fma). */
int dkm_svm_update(const double *K, int64_t ldk, int64_t q, const double *dy,
                   double *f, int64_t m, void *stream);
/* out[i] (fp64) <- sum_s coef[s] K(q_i, x_sv[s]) + b for the nq rows of Q
 * (row stride ldq) against the ns support rows sv[] of X (fp32 when x_f32,
 * else fp64).  qnorm / xnorm: dkm_svm_norms_* of Q and X (rbf only).  The
 * products run on the fp64 MFMA; the sum over s has a fixed order. */
int dkm_svm_decision_f64(const double *Q, int64_t nq, int64_t d, int64_t ldq,
                         const void *X, int x_f32, int64_t n, int64_t ldx,
                         const int32_t *sv, int64_t ns, const double *coef,
                         double b, const double *qnorm, const double *xnorm,
                         int kernel, double gamma, double *out, void *stream);
int dkm_svm_decision_f32(const float *Q, int64_t nq, int64_t d, int64_t ldq,
                         const void *X, int x_f32, int64_t n, int64_t ldx,
                         const int32_t *sv, int64_t ns, const double *coef,
                         double b, const double *qnorm, const double *xnorm,
                         int kernel, double gamma, double *out, void *stream);
/* W[0] <- -0.5 sum_ij c_i c_j l_i l_j K'(x_sv[i], x_sv[j]) + sum_i c_i, the
 * reference's _lagrangian_fast: c = coef (the signed dual coefficients), l =
 * lab (its labels), K' the reference's own kernels -- linear, or its
 * _rbf_kernel, which evaluates to exp(+gamma |x_i - x_j|^2).  tmp: ns fp64
 * of scratch. */
int dkm_svm_w(const void *X, int x_f32, int64_t n, int64_t d, int64_t ldx,
              const int32_t *sv, int64_t ns, const double *coef,
              const double *lab, const double *xnorm, int kernel, double gamma,
              double *tmp, double *W, void *stream);

/* ------------------------------------------------------------------------
 * Dataset loaders.  HOST functions: `buf`
 * and every output are host pointers; no GPU is touched.  `buf` holds
 * the whole file (len bytes); lines end at "\n", "\r\n" or "\r" (Python
 * text mode).  nthreads <= 0 = all hardware threads.  Call *_count first
 * to size the outputs.  `row_line[r]` = 0-based raw line of row r, so the
 * caller can cut Subsets every `subset_size` raw lines exactly like
 * `_load_file` (dislib/data/base.py:145-164).
 * --------------------------------------------------------------------- */

/* counts[4] <- {raw lines, rows, stored entries, threads used}.
 * Replaces the tokenizer of sklearn's load_svmlight_file as called by
 * `_read_libsvm` / `_read_file` (dislib/data/base.py:200-238). */
int dkm_libsvm_count(const char *buf, int64_t len, int nthreads,
                     int64_t *counts);
/* indptr[rows+1], indices[nnz] (as written: the caller applies sklearn's
 * zero_based="auto" shift per chunk), data[nnz], y[rows] (targets),
 * row_line[rows].  DKM_E_PARSE with sklearn's message for a bad number,
 * a negative index or indices that are not strictly increasing. */
int dkm_libsvm_parse(const char *buf, int64_t len, int nthreads,
                     int64_t *indptr, int32_t *indices, double *data,
                     double *y, int64_t *row_line);
/* counts[4] <- {raw lines, rows, fields of the first row, threads used}.
 * delimiter: a byte, or 0 for whitespace runs (numpy's delimiter=None).
 * Replaces np.genfromtxt in `_read_lines` / `_read_file`
 * (dislib/data/base.py:188, :212). */
int dkm_txt_count(const char *buf, int64_t len, int delimiter, int nthreads,
                  int64_t *counts);
/* out[rows x n_cols] row-major fp64 (unconvertible/empty field = NaN),
 * row_line[rows].  DKM_E_PARSE if a row has another number of fields. */
int dkm_txt_parse(const char *buf, int64_t len, int delimiter, int64_t n_cols,
                  int nthreads, double *out, int64_t *row_line);

#ifdef __cplusplus
}
#endif
#endif /* DKM_H */
