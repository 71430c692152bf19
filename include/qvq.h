/*
 * qvq.h -- C ABI of the MI355X LBG vector-quantization engine (libqvq.so).
 *
 * This is the drop-in boundary for coodie/quant's hot path.  The reference has no FFI;
 * its plugin interface is C++:
 *
 *   AbstractQuantizer::quantize(const std::vector<Vector>& trainingSet, size_t n, VectorType eps)
 *       -> tuple<codebook, assignedCodeVector, distortion>        include/Quantizer.hpp:10-16
 *   getQuantizer(Quantizers)                                       include/Quantizer.hpp:20,
 *                                                                  src/Quantizer.cpp:146-155
 *   CompressedImage::compress(image, quantizer, colorSpace, w, h, eps, N)
 *       (times getBlocksAsVectorsFromImage + quantize)             src/Compressor.cpp:107-123
 *
 * The C++ layer in include/quant_amd/ (libquant_amd.so) re-exposes exactly that
 * interface on top of these entry points; INTEGRATION.md shows the binding.  Everything
 * here is plain C: pointers, sizes, status codes; no exceptions cross this boundary.
 *
 * Results: code-vector indices are bit-identical to the reference's (src/Quantizer.cpp:24-32:
 * nanoflann's kd-tree answer over the codebook the reference computes, whose centroids are Kahan
 * sums in ascending row order, src/Quantizer.cpp:59-87) on any rank count; the returned codebook
 * is the exact sum of each final cell's members rounded once and multiplied by fl(1/count) (the
 * reference's Kahan sum agrees to <= 1 ulp).
 */
#ifndef QVQ_H
#define QVQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QVQ_API __attribute__((visibility("default")))

typedef struct qvq_ctx qvq_ctx;

typedef enum {
    QVQ_OK = 0,
    QVQ_EINVAL = 1,       /* bad argument (sizes, null pointers, bits out of range) */
    QVQ_ENOMEM = 2,       /* device or host allocation failed */
    QVQ_EDEVICE = 3,      /* HIP runtime error, or no HIP device */
    QVQ_ECOMM = 4,        /* RCCL error */
    QVQ_EUNSUPPORTED = 5, /* training set the engine cannot sum exactly (see qvq_set_vectors) */
    QVQ_ESTATE = 6        /* call order violated (e.g. qvq_lbg before a training set) */
} qvq_status;

/* Colour spaces, numbered as the reference's enum class ColorSpaces
 * (include/ColorSpace.hpp:6).  NORMAL and SCALED map bytes to values the engine can sum
 * exactly: their rasters take the byte path.  CIE1931 values are not byte images: a
 * CIE1931 raster becomes an exact-mode training set (qvq_set_images). */
enum { QVQ_CS_NORMAL = 0, QVQ_CS_SCALED = 1, QVQ_CS_CIE1931 = 2 };

/* Per-level / per-call timings filled by qvq_get_timings (device ms from HIP events
 * recorded around each level's search kernel on the context's stream). */
typedef struct {
    int levels;                 /* split levels run by the last qvq_lbg (or qvq_lbg_lloyd, qvq_median_cut) */
    double total_ms;            /* the whole call, host wall */
    double assign_ms[32];       /* device time of the assignment kernel per level (exact mode: wall time) */
    double update_ms[32];       /* device time of the centroid-sum kernel per level (exact mode: wall time) */
    double other_ms[32];        /* rest of the level: recheck, kd-tree ties, reduce, finalize + tables */
    uint64_t flagged[32];       /* rows re-checked in fp64 per level */
    uint64_t host_ties[32];     /* exact fp64 ties per level, answered by the reference kd-tree
                                   traversal (device kernel; host only for trees too deep) */
    double wait_ms[32];         /* host wall waiting for the level's codebook (previous finalize) */
    double tree_ms[32];         /* host wall building the level's kd-tree image (overlaps the search) */
    int kahan_redo;             /* 1: a level's ties failed the speculative reference-rule check, and the
                                   quantize ran again with synchronous reference-bit levels */
    int tie_overflow;           /* levels whose tie rows exceeded the check's export (each forces the redo) */
    int kahan_relays;           /* several ranks: levels whose tie rows needed cells summed over every
                                   rank's rows (the chained Kahan sums at the end of the call) */
    double mean_ms;             /* device time of the mean kernel (qvq_set_timing(-3) only) */
} qvq_timings;

/* Context: one per GPU per host thread.  Owns device memory and one HIP stream. */
QVQ_API qvq_status qvq_create(int hip_device, qvq_ctx **out);
QVQ_API void qvq_destroy(qvq_ctx *ctx);
QVQ_API const char *qvq_last_error(const qvq_ctx *ctx);
QVQ_API const char *qvq_version(void);

/*
 * Training set, way 1: raw P6 rasters (host pointer, n_images x xSize x ySize x 3 bytes,
 * image-major), tiled on the device exactly as getBlocksAsVectorsFromImage
 * (src/Compressor.cpp:31-62): the raster is read as xSize rows of ySize pixels, columns
 * past ySize wrap into the next row, components past the end of the buffer are 0.
 * Blocks of image i follow all blocks of image i-1.
 *
 * QVQ_CS_NORMAL and QVQ_CS_SCALED give a byte-path set.  QVQ_CS_CIE1931 gives an exact-mode set
 * (qvq_set_vectors_exact: the reference's arithmetic bit for bit, one rank, qvq_refine
 * unsupported): the bytes are uploaded (or generated) as for the other two, then one kernel tiles
 * them and maps each pixel's three signed bytes r, g, b to
 *   X = ((r*0.490 + g*0.310) + b*0.200) / 0.17697
 *   Y = ((r*0.17697 + g*0.81240) + b*0.01063) / 0.17697
 *   Z = ((r*0 + g*0.01) + b*0.99) / 0.17697
 * (the reference's Cie1931::RGBtoColorSpace, src/ColorSpace.cpp:30-33: every product and sum
 * rounded on its own, a true fp64 division; qvq_host_cie1931 is the same function on the host)
 * straight into the fp64 rows [N][3*bw*bh]; an entry past the end of its image's buffer is three
 * +0.0.  After the image arguments' own checks a CIE1931 call fails, in this order and before the
 * resident set is touched, with QVQ_EINVAL for 3*bw*bh > 64, QVQ_EUNSUPPORTED with a communicator
 * joined (exact mode is one rank), QVQ_EINVAL for 2^31 rows or more; the resident set stays usable.
 */
QVQ_API qvq_status qvq_set_images(qvq_ctx *ctx, const uint8_t *rgb, uint32_t n_images, uint32_t xSize,
                                  uint32_t ySize, uint32_t bw, uint32_t bh, int colorspace);
/* Same, but the rasters are already in device memory (e.g. a torch tensor). */
QVQ_API qvq_status qvq_set_images_device(qvq_ctx *ctx, const void *d_rgb, uint32_t n_images, uint32_t xSize,
                                         uint32_t ySize, uint32_t bw, uint32_t bh, int colorspace);
/* Same, with the rasters generated on the device by the synthetic generator of
 * SURVEY.md 8(d) (image i uses seed0 + i); for benchmarks and scale tests. */
QVQ_API qvq_status qvq_set_synthetic(qvq_ctx *ctx, uint32_t S, uint64_t seed0, uint32_t n_images, uint32_t bw,
                                     uint32_t bh, int colorspace);
/*
 * Training set, way 2: flat fp64 N x dim (the AbstractQuantizer path, include/Quantizer.hpp:10-16).
 * When every value is one the NORMAL or SCALED colour space produces from a byte (or 0.0) the
 * fast path applies (exact integer sums: centroids within 1 ulp of the reference's Kahan sums).
 * Any other data (arbitrary finite doubles, CIE1931 values) takes the exact mode of
 * qvq_set_vectors_exact.  The rows are uploaded once and classified and packed on the device
 * (see qvq_set_vectors_device for the rule).
 */
QVQ_API qvq_status qvq_set_vectors(qvq_ctx *ctx, const double *X, uint64_t n, uint32_t dim);
/*
 * Training set in exact mode, any finite fp64 data: the reference's arithmetic bit for bit
 * -- fp64 search in nanoflann's order with kd-tree ties, centroids as the Kahan sum of each
 * cell's rows in ascending order times fl(1/n) (src/Quantizer.cpp:46-87), so codebook and
 * indices equal the reference's exactly.  Sequential Kahan chains make it slower than the
 * byte path; one rank only (QVQ_EUNSUPPORTED with a communicator).  n < 2^31.
 */
QVQ_API qvq_status qvq_set_vectors_exact(qvq_ctx *ctx, const double *X, uint64_t n, uint32_t dim);
/*
 * The same two for rows that are already in device memory (e.g. a float64 torch tensor): d_X is
 * row-major fp64 n x dim on the context's GPU, 8-byte aligned (a null, misaligned or non-device
 * pointer is QVQ_EINVAL).  flags = 0 chooses the mode from the values as qvq_set_vectors does;
 * QVQ_VECTORS_EXACT forces exact mode as qvq_set_vectors_exact.  stream is the hipStream_t whose
 * queued work produces d_X (NULL = the legacy null stream): the engine records an event on it and
 * makes its own stream wait for that event -- the mirror image of qvq_decode_device.  The call
 * returns when the engine has read the rows for the last time: the caller may overwrite or free
 * d_X on return (exact mode keeps a device-to-device copy of its own).  The argument checks of
 * qvq_set_vectors (n == 0, dim == 0, dim > 64, n >= 2^32; n >= 2^31 with QVQ_VECTORS_EXACT) run
 * before any byte of d_X is read; a set that turns out not to be a byte image returns, in this
 * order, QVQ_EUNSUPPORTED with a communicator joined, QVQ_EINVAL for n >= 2^31, QVQ_EINVAL for a
 * value that is not finite.  A call that returns an error leaves the resident training set as it
 * was.  (The host entry points above take the same route: one upload, then the same device pass.)
 *
 * Which values are byte images: those whose bits equal the colour space's own table entry
 * (qvq_host_colorspace_values), and no others -- not -0.0, not a neighbour of a table value.  The
 * SCALED table is the reference's value under -ffast-math, u * fl(1/255), which is NOT u / 255.0:
 * the two differ in the last bit for 24 of the 256 bytes (u = 33, 37, 41, ...).  A caller who
 * builds SCALED rows on the device with a division therefore gets exact mode, not the byte path;
 * gather the rows from the table instead.
 */
enum { QVQ_VECTORS_EXACT = 1 };   /* flags: force exact mode, as qvq_set_vectors_exact */
QVQ_API qvq_status qvq_set_vectors_device(qvq_ctx *ctx, const void *d_X, uint64_t n, uint32_t dim, uint32_t flags,
                                          void *stream);
/* What is resident: the mode the last qvq_set_* call chose, its colour space and shape. */
typedef struct {
    uint32_t mode;        /* 0 none, 1 byte path, 2 exact mode */
    int32_t colorspace;   /* byte path: QVQ_CS_NORMAL / _SCALED; exact mode: QVQ_CS_CIE1931 for a set that
                             came from a CIE1931 raster, -1 for one from qvq_set_vectors*; -1 for none */
    uint64_t n;
    uint32_t dim;
} qvq_training_info;
QVQ_API qvq_status qvq_get_training_info(const qvq_ctx *ctx, qvq_training_info *out);
/* Device ms of the last qvq_set_vectors* call's two passes over the rows, [0] classify and [1] pack
 * (0 in exact mode), from HIP events under qvq_set_timing(-3); 0 otherwise.  After a CIE1931
 * qvq_set_images* / qvq_set_synthetic call: [0] = 0, [1] = the tile-to-fp64 kernel. */
QVQ_API qvq_status qvq_get_ingest_ms(const qvq_ctx *ctx, double ms[2]);
/* Read back the resident training set: rows row0 .. row0 + nrows - 1 as fp64 [nrows][dim] into out
 * (host memory).  Exact mode: the rows themselves.  Byte path: the value of each row's dim real
 * components under the set's colour space (qvq_host_colorspace_values[code]); pad bytes are not
 * returned.  QVQ_ESTATE with no training set; QVQ_EINVAL for nrows == 0, a range that leaves
 * [0, qvq_num_vectors) or a null out.  Copied through the context's stream under the bounded wait
 * (qvq_set_timeout): out is written only after a wait has succeeded.  Changes nothing resident. */
QVQ_API qvq_status qvq_get_vectors(qvq_ctx *ctx, uint64_t row0, uint64_t nrows, double *out);

QVQ_API uint64_t qvq_num_vectors(const qvq_ctx *ctx);
QVQ_API uint32_t qvq_dim(const qvq_ctx *ctx);

/*
 * Full split-LBG (LBGQuantizer::quantize, src/Quantizer.cpp:122-143) over the training
 * set: n = bits levels, K = 2^bits code vectors.  eps is accepted for signature parity;
 * it cannot change the outputs (one Lloyd step per level); qvq_refine
 * continues from this call's result with eps as a real stopping rule.
 * Outputs (caller-owned host memory, any may be NULL):
 *   codebook   : K x dim fp64
 *   assign     : n u32 (this rank's rows)
 *   distortion : mean squared error of the final codebook, as updateDistortion
 * With a communicator (qvq_comm_init) every rank runs this on its own rows -- consecutive ranges
 * of the global rows, rank 0 first -- and all ranks get the same codebook, distortion and indices
 * as one rank over all the rows (the reference's Kahan rule included: cells whose reference bits
 * decide a tie are summed across the ranks in row order).
 */
QVQ_API qvq_status qvq_lbg(qvq_ctx *ctx, uint32_t bits, double eps, double *codebook, uint32_t *assign,
                           double *distortion);
/* Device pointer to the last qvq_lbg's or qvq_refine's assignment (u32, qvq_num_vectors entries). */
QVQ_API const uint32_t *qvq_assign_device(const qvq_ctx *ctx);

/*
 * Lloyd refinement at fixed K, resident on the device: iterate assignment and centroid steps from
 * a codebook until the assignment stops changing, the distortion settles, or max_iters.
 *
 * For t = 1 .. max_iters:
 *   A_t = the assignment qvq_assign gives for C_{t-1} (the reference's kd-tree answer over that
 *         codebook, ties included);
 *   C_t = the centroids qvq_update gives for A_t (exact sums, empty cells 0);
 *   d_t = the mean squared error of (C_t, A_t), as updateDistortion;
 *   changed[t-1] = rows with A_t != A_{t-1};  dist_trace[t-1] = d_t.
 * After iteration t, in this order:
 *   changed == 0                        -> QVQ_STOP_FIXED (C_t = C_{t-1}: a Lloyd fixed point)
 *   |d_{t-1} - d_t| / d_{t-1} <= eps    -> QVQ_STOP_EPS   (the reference's test, src/Quantizer.cpp:105)
 *   t == max_iters                      -> QVQ_STOP_MAXIT
 *
 * C_start == NULL continues from this context's last successful qvq_lbg or qvq_refine on the
 * current training set: A_0, C_0, d_0 are that call's results and K must be its K (QVQ_EINVAL
 * otherwise); QVQ_ESTATE if there is none, or if a qvq_set_*, qvq_assign or qvq_update* call came
 * in between.  C_start != NULL (K x dim, e.g. another image's codebook) is a warm start: C_0 =
 * C_start, there is no A_0, iteration 1 reports changed = N and takes no eps test; every component
 * must lie within the colour space's value range (QVQ_EINVAL otherwise).
 *
 * QVQ_REFINE_FRESH: after the loop one more assignment A* = assign(C_t) is returned in place of
 * A_t, and distortion is that of (C_t, A*) (closed form from A*'s sums: sum ||x||^2 - 2 sum_k
 * c_k.S_k + sum_k n_k ||c_k||^2); the codebook is not updated again.  max_iters = 0 is legal with
 * this flag only (QVQ_EINVAL without): fresh indices for the starting codebook.
 *
 * Outputs (caller-owned host memory, any may be NULL): codebook K x dim, assign n u32, distortion,
 * changed and dist_trace (max_iters entries each, the first info->iters written), info.
 * qvq_assign_device points at the returned assignment.  A later qvq_lbg on the context gives
 * exactly what it gave before.  Exact mode (qvq_set_vectors_exact, its fallback inside
 * qvq_set_vectors, or a CIE1931 raster) returns QVQ_EUNSUPPORTED.
 *
 * With a communicator (qvq_comm_init or qvq_comm_init_host, any nranks >= 1) every rank calls this
 * on its own rows -- consecutive ranges of the global rows, rank 0 first, as for qvq_lbg -- with
 * the same K, max_iters, eps and flags and the same C_start bytes (or NULL on every rank; it then
 * continues from the sharded qvq_lbg or qvq_refine on the same communicator).  Every rank returns
 * the same codebook, distortion, changed[], dist_trace[] and info: the values one rank would return
 * over all the rows, bit for bit.  changed[] counts the rows of every rank (a warm start reports
 * the global N at iteration 1) and the stop rule sees the global count and distortion only, so
 * every rank stops at the same iteration.  assign and qvq_assign_device hold this rank's rows; the
 * ranks' indices concatenate to the one-rank assignment.  Collectives per call: the histogram
 * behind sum ||x||^2, one all-reduce per iteration run (the level's sums with the rows changed
 * behind them) and one more with QVQ_REFINE_FRESH; several ranks first exchange their verdict on
 * the call and a digest of its arguments: if a rank rejects its call (QVQ_ESTATE, QVQ_EINVAL,
 * QVQ_EUNSUPPORTED) it returns that status, the other ranks return QVQ_EINVAL (qvq_last_error: a
 * peer rejected the call), and so does every rank when the arguments differ; no rank's state is
 * touched and none waits for a peer that will not come.  A collective that fails returns QVQ_ECOMM
 * as everywhere (qvq_comm_init).
 *
 * QVQ_REFINE_RESEED: after each iteration's centroid step the empty cells of C_t take rows of the
 * worst cells as their code vectors (without the flag an empty cell is the zero vector and, at a
 * fixed K, never fills again).  From A_t, the centroids C_t as formed above and the cell counts n_k:
 *   per-row error   for each row, k = A_t[row]: e = 0; for d = 0 .. dim-1 ascending: u = x_d -
 *                   C_t[k][d], e = e + u*u; every subtraction, product and sum rounded once to fp64,
 *                   no fused multiply-add; x_d = qvq_host_colorspace_values[code]; pad components
 *                   take no part (qvq_host_row_error);
 *   quantised error q_row = floor(e 2^s) as an unsigned integer, s = 24 for SCALED (e <= 64), s = 8
 *                   for NORMAL (e <= 64 255^2): q_row < 2^31, sums over < 2^32 rows fit u64;
 *   per cell        E_k = the sum of q_row over the rows of cell k (an exact integer: no order);
 *                   far_k = the row of cell k with the largest q_row, on equal q_row the lowest row;
 *   empties         the cells with n_k = 0, in ascending k;
 *   donors          the cells with n_k >= 2 and E_k > 0, by E_k descending, on equal E_k by k
 *                   ascending;
 *   seeds           m = min(empties, donors); for j < m, C_t[empty_j] takes the dim values of row
 *                   far_{donor_j}.  A donor gives one seed per iteration; its own centroid is not
 *                   touched (qvq_host_reseed_select).
 * C_t with its seeds is iteration t's codebook: searched in iteration t + 1, returned as the
 * call's codebook, and the state a later C_start == NULL call continues from.  d_t and
 * changed[t-1] are those of the unseeded step (an empty cell owns no row).  Reseeding runs in every
 * iteration, the last one included.  QVQ_STOP_FIXED then needs changed == 0 and no seed placed in
 * that iteration; the eps and max_iters tests follow in the order above.  With QVQ_REFINE_FRESH
 * A* is the assignment for the seeded C_t and the distortion its closed form.
 * qvq_get_refine_reseeds returns the seeds placed per iteration.  One rank's byte path only: with
 * a communicator joined (any nranks) the flag is QVQ_EUNSUPPORTED, a verdict that goes through
 * the entry vote like any other; so is a training set of 2^32 - 1 rows or more.  Without the flag
 * nothing changes: the launches and the results are those of the call without it.
 */
enum { QVQ_REFINE_FRESH = 1, QVQ_REFINE_RESEED = 2 };   /* flags */
enum { QVQ_STOP_FIXED = 0, QVQ_STOP_EPS = 1, QVQ_STOP_MAXIT = 2 };
typedef struct { uint32_t iters, stop; } qvq_refine_info;
QVQ_API qvq_status qvq_refine(qvq_ctx *ctx, uint32_t K, const double *C_start /* K x dim, or NULL */,
                              uint32_t max_iters, double eps, uint32_t flags,
                              double *codebook, uint32_t *assign, double *distortion,
                              uint64_t *changed /* max_iters, may be NULL */,
                              double *dist_trace /* max_iters, may be NULL */,
                              qvq_refine_info *info /* may be NULL */);
/* The seeds QVQ_REFINE_RESEED placed in each iteration of the last qvq_refine (all 0 without the
 * flag): the first min(cap, iterations) entries of out, *iters = the iterations (either may be
 * NULL / 0).  QVQ_ESTATE before any qvq_refine on the context. */
QVQ_API qvq_status qvq_get_refine_reseeds(qvq_ctx *ctx, uint64_t *out, uint32_t cap, uint32_t *iters);

/*
 * Split-LBG with Lloyd iterations at every level: the textbook schedule the reference's README
 * describes (after every split, iterate until the distortion settles) and its code does not run
 * (qvq_lbg: one assignment per level).  The reference has none to match: this text is the rule.
 *
 * C^(0) = the mean of the rows, as qvq_lbg forms it.  For level l = 1 .. bits, K = 2^l, H = K / 2:
 *   S[k] = C^(l-1)[k] * (double)(1 + 0.2) and S[k + H] = C^(l-1)[k] * (double)(1 - 0.2) for k < H:
 *   fp64 products, qvq_lbg's split.
 *   The level then runs qvq_refine's loop exactly as its contract words it, with C_0 = S, no A_0,
 *   max_iters = iters, this eps, and QVQ_REFINE_RESEED iff QVQ_LLOYD_RESEED.  It is a warm start:
 *   iteration 1 reports changed = N and takes no eps test; the stop order is qvq_refine's
 *   (QVQ_STOP_FIXED, _EPS, _MAXIT).  The range check on C_start does not apply to S: the searches are
 *   specified for |c| <= 1.2 vmax (qvq_assign), which is what qvq_lbg itself searches.
 *   C^(l), A^(l), d^(l) = that loop's codebook (with its seeds, under the flag), assignment and
 *   distortion.
 * levels[l-1] (bits entries, may be NULL): iters and stop of the level's loop; changed, the rows
 * changed in its last iteration; empty, the cells with no row under A^(l); seeds, the seeds placed
 * in all of its iterations (0 without the flag); distortion = d^(l).
 *
 * Outputs (caller-owned host memory, any may be NULL): codebook 2^bits x dim, assign n u32 and
 * distortion are C, A and d of the last level, written only after the bounded wait has succeeded;
 * qvq_assign_device points at that assignment.  bits = 0 gives one cell, the mean, and no levels.
 * A successful call leaves the state a C_start == NULL qvq_refine continues from (K = 2^bits); a
 * later qvq_lbg returns what it returned before.  qvq_get_timings reports levels and total_ms, and
 * 0 for the rest.  With iters = 1 and no flag a level is one assignment and one centroid step of
 * the split codebook: qvq_lbg's level with exact-sum centroids (qvq_lbg's indices wherever the
 * reference's Kahan sums and the exact sums give the same ones).
 *
 * Errors, in this order, each leaving the context as it was: QVQ_ESTATE without a training set;
 * QVQ_EINVAL for bits > 20, for iters == 0, for !(eps >= 0), for an unknown flag; QVQ_EUNSUPPORTED
 * for an exact-mode set, with any communicator joined (a sharded version needs qvq_refine's entry
 * vote), and for the flag with 2^32 - 1 rows or more.
 */
enum { QVQ_LLOYD_RESEED = 1 };   /* flags */
typedef struct {
    uint32_t iters, stop;   /* iterations run at this level; QVQ_STOP_* of its last one */
    uint64_t changed;       /* rows changed in the level's last iteration */
    uint64_t empty;         /* cells with no row under the level's final assignment */
    uint64_t seeds;         /* seeds placed at this level (0 without the flag) */
    double distortion;      /* d of the level's last iteration */
} qvq_lloyd_level;
QVQ_API qvq_status qvq_lbg_lloyd(qvq_ctx *ctx, uint32_t bits, uint32_t iters, double eps, uint32_t flags,
                                 double *codebook, uint32_t *assign, double *distortion,
                                 qvq_lloyd_level *levels /* bits entries, may be NULL */);

/*
 * Median cut on the device: a codebook of K = 2^bits code vectors by cutting boxes of rows at the
 * median of their widest component; with qvq_refine (C_start = this call's codebook) behind it, the
 * textbook alternative to split-LBG.  The reference names the quantizer (MEDIAN_CUT) and has none
 * to match: this text is the rule.  One rank's byte path: N rows of dim real components; pad
 * components take no part.  u[row][d] = (int8)code + 128 is the ordinal of a row's code byte; both
 * byte colour spaces order their values by it.
 *
 * A[row] = 0.  For level l = 1 .. bits, half = 2^(l-1), for every box b < half:
 *   1. n_b = the rows with A = b; lo_d, hi_d = the minimum and maximum of u[.][d] over them;
 *   2. axis = the d with the largest hi_d - lo_d, on equal ranges the lowest d;
 *   3. n_b = 0 or hi_axis = lo_axis (range 0): the box is not cut, its rows keep b and box
 *      b + half stays empty;
 *   4. else h[v] = the box's rows with u[.][axis] = v, cum(v) = sum of h[w] over w <= v; t = the v in
 *      [lo_axis, hi_axis - 1] that minimises |2 cum(v) - n_b|, on ties the lowest.  Rows with
 *      u[.][axis] > t take A = b + half, the others (a row at t included) keep b.  Both children
 *      are non-empty by construction.
 * cuts[l-1] = the boxes cut at level l (bits entries; may be NULL).
 * After the last level: assign = A; codebook[k] = the centroid of box k by qvq_update's exact-sum
 * rule (an empty box: the zero vector); distortion = the mean squared error of (codebook, A), as
 * updateDistortion (closed form from the boxes' sums); qvq_assign_device points at A.  bits = 0 is
 * legal: one box, its centroid the mean.  Everything before the centroids is integer minima,
 * maxima and counts: exact, whatever order the device takes the rows in.
 * (qvq_host_median_cut_axis and qvq_host_median_cut_select are steps 2 and 4 on the host.)
 *
 * Errors, in this order: QVQ_ESTATE without a training set; QVQ_EINVAL for bits > 20;
 * QVQ_EUNSUPPORTED for an exact-mode set; QVQ_EUNSUPPORTED with any communicator joined (a
 * sharded median cut needs the boxes' minima and maxima over every rank's rows, a min/max reduce
 * the host communicator does not have).  An error leaves the context as it was.  Like qvq_assign, a
 * successful call ends qvq_refine's C_start == NULL continuation (QVQ_ESTATE); a later qvq_lbg on
 * the context returns what it returned before.  Outputs (caller-owned host memory, any may be
 * NULL) are written only after the bounded wait has succeeded.  Under qvq_set_timing(-1)
 * qvq_get_timings reports per level the two row passes in assign_ms and the rest in other_ms.
 */
QVQ_API qvq_status qvq_median_cut(qvq_ctx *ctx, uint32_t bits, double *codebook, uint32_t *assign,
                                  double *distortion, uint32_t *cuts);

/*
 * k-means++ seeding on the device (D^2-sampling, Arthur & Vassilvitskii 2007): K training rows as a
 * starting codebook for qvq_refine (C_start = this call's codebook), for any K in 1 .. 2^20.  Every
 * seed is a training row, K distinct seeds give K non-empty cells, and on the byte path the whole
 * rule is integer arithmetic.  The reference has no such quantizer: this text is the rule.  One
 * rank's byte path: N rows of Dp padded components; o[row][d] = (uint8)(code ^ 0x80) is the ordinal
 * of a code byte.  Both byte colour spaces are affine in it (NORMAL o - 128, SCALED o * fl(1/255));
 * pad bytes hold the space's zero code in every row and add 0 to any difference.
 *
 * Weight: w(a, b) = sum over d < Dp of (o[a][d] - o[b][d])^2, an exact integer <= 64 * 255^2 < 2^22:
 *   the squared distance in NORMAL, 255^2 times it in SCALED before rounding.
 * Random numbers (u64, every operation wraps):
 *   mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *           x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31
 *   draw(seed, j, T) = floor(mix(seed + j) * T / 2^64), the high 64 bits of the 128-bit product: in [0, T).
 * Seeding: s_0 = draw(seed, 0, N); m[row] = w(row, s_0); potential[0] = sum of m.  For j = 1 .. K - 1:
 *   T = sum of m over the rows (a u64); T = 0: every row equals a seed, placed = j, stop.  Else
 *   t = draw(seed, j, T); s_j = the lowest row with (sum of m[i] over i <= row) > t.  The comparison is
 *   strict: a row with m = 0 is never drawn, so no two seeds are equal rows.  Then
 *   m[row] = min(m[row], w(row, s_j)) and potential[j] = sum of m.  Without a stop placed = K.
 *
 * Outputs (caller-owned host memory, any may be NULL, written only after the bounded wait has
 * succeeded): codebook (K x dim fp64): entry j < placed the dim values of row s_j, as
 * qvq_get_vectors(s_j) gives them, entry j >= placed the zero vector (the engine's empty-cell
 * convention); rows (K): s_j, 0xFFFFFFFF for j >= placed; potential (K): entries from placed on
 * repeat 0; info->placed.  potential[j] / N is the mean squared error of seeds 0 .. j under
 * nearest-seed assignment per row in squared ordinal units: divide by dim for the per-component
 * figure qvq_lbg's distortion uses, and by 65025 = 255^2 for SCALED values.
 *
 * The call uses device buffers of its own (m, per-segment sums, the seed list) and touches nothing
 * resident: qvq_assign_device, the C_start == NULL continuation of qvq_refine and a later qvq_lbg
 * behave as if it had not happened.  Errors, in this order, each leaving the context as it was:
 * QVQ_ESTATE without a training set; QVQ_EINVAL for K = 0 or K > 2^20 (K > N is legal: then placed
 * <= the number of distinct rows); QVQ_EUNSUPPORTED for an exact-mode set; QVQ_EUNSUPPORTED with any
 * communicator joined (a sharded seeding needs the prefix over the ranks' rows).  qvq_get_timings
 * reports levels = 0 and the call's total_ms.
 * (qvq_host_kmpp_draw and qvq_host_kmpp_weight are draw and w on the host.)
 */
typedef struct { uint32_t placed; } qvq_kmeanspp_info;
QVQ_API qvq_status qvq_kmeanspp(qvq_ctx *ctx, uint32_t K, uint64_t seed, double *codebook, uint32_t *rows,
                                uint64_t *potential, qvq_kmeanspp_info *info);

/*
 * k-means|| seeding on the device (Bahmani, Moseley, Vattani, Kumar, Vassilvitskii, "Scalable
 * K-Means++", VLDB 2012): qvq_kmeanspp's K - 1 dependent passes over the rows become `rounds` passes.
 * In each, every row decides independently whether it becomes a candidate; the candidates are weighted
 * by the rows nearest to them, and a weighted k-means++ over the candidates picks the K seeds.  The
 * reference has no such quantizer: this text is the rule.  One rank's byte path, in qvq_kmeanspp's
 * terms: the ordinals o = (uint8)(code ^ 0x80), the weight w(a, b) = sum over d < Dp of
 * (o[a][d] - o[b][d])^2, an exact integer below 2^22, and mix and draw(seed, j, T) as above.
 * mulhi64(a, b) is the high 64 bits of the 128-bit product.
 *
 * Options (opts may be NULL; a 0 field is its default): rounds = 5, ell = K, round_cap = 2 * ell + 64.
 * 1. Candidate 0: c_0 = draw(seed, 0, N), qvq_kmeanspp's first seed.  m[row] = w(row, c_0),
 *    near[row] = 0, potential[0] = sum of m.  M = 1.
 * 2. Rounds r = 1 .. rounds: phi = sum of m (u64); phi = 0: the rounds end.  key_r = mix(seed + r),
 *    u(r, row) = mix(key_r + row).  Row `row` joins iff mulhi64(u(r, row), phi) < ell * m[row]: strict,
 *    the right side below 2^39; a row with m = 0 never joins.  The joining rows become candidates M,
 *    M + 1, ... in ascending row order; if more than round_cap join, the round_cap lowest rows are
 *    taken and `truncated` counts the round.  Then for every row and every new candidate c in index
 *    order: if w(row, c) < m[row] then m[row] = w, near[row] = c (strict: the lowest index keeps a tie).
 *    potential[r] = sum of m; rounds_run = r; round_candidates[r - 1] = the candidates added.
 * 3. Weights: wt[c] = the rows with near = c; their sum is N.  Two equal rows that join in one round
 *    give a candidate of weight 0: it is legal and is never drawn below.
 * 4. Reduction: weighted k-means++ over the M candidates, draws from the stream seed + 2^32.
 *    s_0 = the lowest c with (sum of wt[i] over i <= c) > draw(seed + 2^32, 0, N); g[c] = w(c, s_0).
 *    For j = 1 .. K - 1: T = sum of wt[c] * g[c] (below 2^54); T = 0: placed = j, stop.  Else
 *    t = draw(seed + 2^32, j, T), s_j = the lowest c whose prefix of wt * g exceeds t, g = min(g, w(., s_j)).
 *    Without a stop placed = K.  K > M is legal and gives placed <= M.
 *
 * Outputs (caller-owned host memory, any may be NULL, written only after the bounded wait has
 * succeeded): rows (K): the training row of s_j, 0xFFFFFFFF from placed on; codebook (K x dim fp64):
 * entry j < placed that row's values as qvq_get_vectors gives them, the zero vector from placed on;
 * cand_rows and cand_weights (1 + rounds * round_cap entries each, qvq_host_kmeans_par_plan's
 * max_candidates): the candidates' rows and wt, entries from M on 0xFFFFFFFF and 0; info: placed,
 * candidates = M, rounds_run, truncated, round_candidates (0 for rounds not run) and potential
 * (entries 0 .. rounds_run; 0 after).
 *
 * The call uses device buffers of its own (m, near, the join bits, per-segment sums and counts, the
 * candidate list) and touches nothing resident: qvq_assign_device, the C_start == NULL continuation
 * of qvq_refine and a later qvq_lbg behave as if it had not happened.  Errors, in this order, each
 * leaving the context as it was: QVQ_ESTATE without a training set; QVQ_EINVAL for K = 0 or K > 2^16,
 * rounds > 16, ell > 2^17, round_cap < 1 or 1 + rounds * round_cap > 2^20 (after the defaults);
 * QVQ_EUNSUPPORTED for an exact-mode set; QVQ_EUNSUPPORTED with any communicator joined.
 * qvq_get_timings reports levels = 0 and the call's total_ms; under qvq_set_timing(-3) also, per round
 * r, other_ms[r - 1] the sample and assign_ms[r - 1] the update, update_ms[0] candidate 0's pass,
 * update_ms[1] the weights and update_ms[2] the reduction (device ms).
 * (qvq_host_kmeans_par_join is the sampling test on the host.)
 */
typedef struct { uint32_t rounds, ell, round_cap; } qvq_kmeans_par_opts;   /* a 0 field = its default */
typedef struct {
    uint32_t placed;               /* seeds placed, <= K */
    uint32_t candidates;           /* M */
    uint32_t rounds_run;           /* rounds that sampled (they stop early when phi = 0) */
    uint32_t truncated;            /* rounds whose sample passed round_cap */
    uint32_t round_candidates[16]; /* candidates added per round */
    uint64_t potential[17];        /* phi after candidate 0, then after each round run */
} qvq_kmeans_par_info;
QVQ_API qvq_status qvq_kmeans_par(qvq_ctx *ctx, uint32_t K, uint64_t seed, const qvq_kmeans_par_opts *opts,
                                  double *codebook, uint32_t *rows, uint32_t *cand_rows, uint64_t *cand_weights,
                                  qvq_kmeans_par_info *info);

/*
 * Greedy k-means++ seeding on the device (Arthur & Vassilvitskii 2007, section 6; scikit-learn's
 * n_local_trials): every round draws L candidate rows by D^2-sampling and keeps the one that lowers
 * the potential most.  The reference has no such quantizer: this text is the rule.  The terms are
 * qvq_kmeanspp's: the ordinals o, the weight w(a, b), mix and draw(seed, j, T); one rank's byte path.
 *
 * Trial count: trials lies in 0 .. 16.  trials = 0: L = 2 + (7 * floor(log2 K)) / 10 in integer
 *   division (2 for K = 1, 9 for K = 1024, 16 for K = 2^20); otherwise L = trials.  info->trials = L.
 * First seed: s_0 = draw(seed, 0, N); m[row] = w(row, s_0); potential[0] = sum of m.
 * Rounds j = 1 .. K - 1: T = sum of m (a u64).  T = 0: placed = j, stop.  Else for l = 0 .. L - 1:
 *   t_l = draw(seed + l * 2^32, j, T), all arithmetic wrapping (l = 0 is qvq_kmeanspp's own stream);
 *   c_l = the lowest row with (sum of m[i] over i <= row) > t_l; the comparison is strict, so a row
 *     with m = 0 is never drawn;
 *   P_l = sum over the rows of min(m[row], w(row, c_l)), a u64 below 2^54.
 *   Two trials may draw the same row; their P are then equal.  The winner is the l with the smallest
 *   P_l, on equal P the lowest l.  s_j = c_winner, m = min(m, w(., s_j)), potential[j] = P_winner,
 *   trial[j] = the winning l.  Without a stop placed = K.
 * With L = 1 the call returns qvq_kmeanspp's rows, potentials, placed and codebook bit for bit.
 *
 * Outputs (caller-owned host memory, any may be NULL, written only after the bounded wait has
 * succeeded): codebook (K x dim fp64), rows (K) and potential (K) as in qvq_kmeanspp; trial (K):
 * trial[0] = 0, 0xFFFFFFFF from placed on; trial_rows and trial_potential (K x 16 each, row-major):
 * entry [j][l] holds c_l and P_l of round j for l < L; row 0 holds s_0 and potential[0] at l = 0;
 * everything else (l >= L, j >= placed, row 0 at l > 0) is 0xFFFFFFFF and 0.
 *
 * Like qvq_kmeanspp the call uses device buffers of its own and touches nothing resident.  Errors,
 * in this order, each leaving the context as it was: QVQ_ESTATE without a training set; QVQ_EINVAL
 * for K = 0, K > 2^20 or trials > 16; QVQ_EUNSUPPORTED for an exact-mode set; QVQ_EUNSUPPORTED with
 * any communicator joined.  qvq_get_timings reports levels = 0 and the call's total_ms.
 * (qvq_host_kmpp_trials is the trial count on the host.)
 */
typedef struct { uint32_t placed, trials; } qvq_kmeanspp_greedy_info;
QVQ_API qvq_status qvq_kmeanspp_greedy(qvq_ctx *ctx, uint32_t K, uint64_t seed, uint32_t trials, double *codebook,
                                       uint32_t *rows, uint64_t *potential, uint32_t *trial, uint32_t *trial_rows,
                                       uint64_t *trial_potential, qvq_kmeanspp_greedy_info *info);

/* Single steps over the current training set, for tests and benchmarks.
 * qvq_assign: nearest code vector of every row for codebook C (K x dim fp64, host),
 *   with the same MFMA/VALU search + fp64 recheck + kd-tree tie resolution as qvq_lbg.
 *   On a byte-image training set every component of C must lie in [cmin, cmax] =
 *   [min(1.2 vmin, 0.8 vmin), max(1.2 vmax, 0.8 vmax)], vmin and vmax the colour space's smallest
 *   and largest value (SCALED: [0, 1.2]; NORMAL: [-153.6, 152.4]) -- every codebook qvq_lbg can
 *   form, centroids and their 1.2 / 0.8 splits.  The searches' near-tie thresholds and their
 *   f16 / fp32 score scale are worked out for that range: outside it a row could keep a wrong
 *   index unflagged, or a score overflow.  A component outside it, NaN included, is QVQ_EINVAL
 *   before anything reaches the device; assign is not written.  (qvq_refine's C_start keeps its
 *   narrower [vmin, vmax].)  An exact-mode training set is not restricted: it runs no
 *   fp32 search.
 * qvq_update: centroids of the rows under assignment A (host, n u32) into C_out
 *   (K x dim fp64) and counts (K u64), the engine's exact-sum rule. */
QVQ_API qvq_status qvq_assign(qvq_ctx *ctx, const double *C, uint32_t K, uint32_t *assign);
QVQ_API qvq_status qvq_update(qvq_ctx *ctx, const uint32_t *assign, uint32_t K, double *C_out, uint64_t *counts);
/* The reference's own centroid bits (Solution::fixCodeVectors, reference src/Quantizer.cpp:59-87:
 * Kahan sums in ascending row order times fl(1/n), empty cells 0) of the resident rows under
 * assignment A, into C_out (K x dim fp64).  With a communicator of several ranks every rank passes
 * its own rows' assignment and gets the centroids of all ranks' rows, each cell's chain running
 * over the ranks' rows in rank order (the ranks must hold consecutive ranges of the global rows,
 * rank 0 first, as qvq_lbg's sharding does). */
QVQ_API qvq_status qvq_update_kahan(qvq_ctx *ctx, const uint32_t *assign, uint32_t K, double *C_out);
/* Test entry: qvq_update_kahan with this context's rows cut into nsplits virtual ranks at
 * splits[0..nsplits] (0 = splits[0] <= ... <= splits[nsplits] = N), the several-rank chained
 * evaluation run rank after rank on one device; equals qvq_update_kahan for any cuts. */
QVQ_API qvq_status qvq_update_kahan_split(qvq_ctx *ctx, const uint32_t *assign, uint32_t K, const uint64_t *splits,
                                          uint32_t nsplits, double *C_out);
/* Both accept any K (qvq_lbg uses up to 2^20): the device's stable sort by cell keeps one counter per key in
 * LDS and takes the keys in windows (qvq_host_kahan_sort_plan), so K is not bound by the LDS.
 *
 * Test entry: what the last qvq_update_kahan / qvq_update_kahan_split call on this context ran.
 * route: the step-by-step kernel (every cell at most QVQ_KAHAN_DIRECT_MAX rows, default 4096), the
 * segment functions, or the chained evaluation (several ranks, and every qvq_update_kahan_split).
 * The counters are the function routes': blocks of 64 segments whose functions did not compose,
 * block functions that did not answer at evaluation, and segments replayed step by step. */
enum { QVQ_KAHAN_ROUTE_DIRECT = 1, QVQ_KAHAN_ROUTE_FUNCTIONS = 2, QVQ_KAHAN_ROUTE_CHAINED = 3 };
typedef struct { uint32_t route, blocks_not_composable, block_misses, replays; } qvq_kahan_stats;
QVQ_API qvq_status qvq_get_kahan_stats(qvq_ctx *ctx, qvq_kahan_stats *out);

/* Decode (replaces CompressedImage::decompress, reference src/Compressor.cpp:156-165, and the
 * getImageFromVectors it calls, src/Compressor.cpp:64-85): raster[x*ySize+y] = the code-vector bytes
 * codebook[assign[block]] laid out as getImageFromVectors does, including the column wrap and
 * "last block wins" order.  codebook: K x (bw*bh*3) bytes; assign: ceil(xSize/bw)*ceil(ySize/bh)
 * u32; rgb: xSize*ySize*3 bytes.  An index >= K returns QVQ_EINVAL (the reference indexes
 * codeVectors with operator[], undefined behaviour).  ySize + bh - 1 and xSize + bw - 1 must be
 * below 2^32.
 * qvq_decode takes host buffers.  qvq_decode_mse also returns the raport's distortion, the mean
 * squared difference of the signed bytes of orig and the decoded raster (src/Compressor.cpp:
 * 133-146), computed in the same device pass (rgb may then be NULL).  qvq_decode_device takes
 * device pointers and a hipStream_t on which it launches (NULL = the legacy null stream, so
 * work the caller queued on blocking streams is ordered before it; the engine's own queued work
 * is ordered before it on any stream) and synchronises that stream before returning.  d_assign
 * must be 4-byte aligned (QVQ_EINVAL otherwise).  The fast row kernels (ySize % 8 == 0) want
 * d_rgb 8-byte and d_assign 16-byte aligned: a pointer without that takes the per-pixel kernel.
 * d_codebook may have any alignment: the 16-bit codebook reads of the block-height 2, 4 and 8 row
 * kernel need an even pointer only when the codebook stays in global memory (K*bw*bh*3 > 48 KB),
 * and an odd one then takes the byte-reading row kernel.  Every route decodes the same bytes
 * (qvq_host_decode_plan names the one taken). */
QVQ_API qvq_status qvq_decode(qvq_ctx *ctx, const uint8_t *codebook, uint32_t K, const uint32_t *assign,
                              uint64_t nblocks, uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh, uint8_t *rgb);
QVQ_API qvq_status qvq_decode_mse(qvq_ctx *ctx, const uint8_t *codebook, uint32_t K, const uint32_t *assign,
                                  uint64_t nblocks, uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh,
                                  uint8_t *rgb, const uint8_t *orig, double *mse);
QVQ_API qvq_status qvq_decode_device(qvq_ctx *ctx, const void *d_codebook, uint32_t K, const void *d_assign,
                                     uint64_t nblocks, uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh,
                                     void *d_rgb, void *stream);

/* Multi-GPU: join an RCCL communicator (unique_id from qvq_comm_unique_id on rank 0,
 * shipped to the other ranks by the caller).  Each level then all-reduces the
 * per-code-vector sums and counts over xGMI.  nranks = 1 creates a real one-rank
 * communicator (the collective path with identical results).  A collective that fails, or
 * a wait that outlasts the timeout (qvq_set_timeout) while a communicator is joined, returns
 * QVQ_ECOMM and aborts the communicator (the context then runs single-rank until the next
 * qvq_comm_init). */
QVQ_API qvq_status qvq_comm_unique_id(uint8_t id[128]);
QVQ_API qvq_status qvq_comm_init(qvq_ctx *ctx, int nranks, int rank, const uint8_t id[128]);
/* Test-only communicator: every per-level exchange (the same buffers the RCCL all-reduce
 * sums: the mean's and the level's per-code-vector sums and counts as u64, dtype 0; the two
 * distortion terms as double, dtype 1) is copied to pinned host memory, fn(buf, count, dtype,
 * user) must replace it in place by the sum over the nranks ranks and return 0, and the
 * result is copied back.  Lets several processes share one GPU (RCCL refuses two ranks on one
 * device) so the sharded schedule runs in tests on a one-GPU box.  Replaces any communicator. */
typedef int (*qvq_allreduce_fn)(void *buf, uint64_t count, int dtype, void *user);
QVQ_API qvq_status qvq_comm_init_host(qvq_ctx *ctx, int nranks, int rank, qvq_allreduce_fn fn, void *user);
/* The joined communicator: ranks, this rank, kind (QVQ_COMM_NONE: single rank). */
enum { QVQ_COMM_NONE = 0, QVQ_COMM_RCCL = 1, QVQ_COMM_HOST = 2 };
QVQ_API qvq_status qvq_comm_info(const qvq_ctx *ctx, int *nranks, int *rank, int *kind);
/* Bound, in seconds, of every host wait on the context's stream (default 120, or the
 * QVQ_TIMEOUT_S environment variable at qvq_create).  A wait that fails while the stream
 * cannot be drained poisons the context: results are never copied into caller memory after
 * the call returned, and every later call but qvq_destroy returns QVQ_ESTATE. */
QVQ_API qvq_status qvq_set_timeout(qvq_ctx *ctx, double seconds);

/* Which levels get HIP events around their search kernel (each event record idles the GPU
 * ~6 us: every level costs ~10 % of a C3 quantize): -1 every level, -2 none (default), -3 the
 * mean kernel only (mean_ms), n >= 0 level n+1 only.  Unmeasured levels report 0 in
 * qvq_get_timings. */
QVQ_API qvq_status qvq_set_timing(qvq_ctx *ctx, int level);
QVQ_API qvq_status qvq_get_timings(const qvq_ctx *ctx, qvq_timings *out);

/* Test entry: the reference kd-tree of C (K x dim fp64) built on the device (the build qvq_lbg
 * uses for its 48-D levels) against the host's RefKDTree, node for node; result 0 equal, 1
 * different (qvq_last_error names the first difference), 2 the device build gave up.  build_ms
 * (4 doubles): the launch, then its phases (big nodes, small subtrees, the images). */
QVQ_API qvq_status qvq_kdtree_device_check(qvq_ctx *ctx, const double *C, uint32_t K, uint32_t dim, double *build_ms,
                                           uint32_t *result);

/* Host-only helpers (no GPU needed), exported for tests of the host logic. */
/* The reference kd-tree's answer for nq queries (nanoflann semantics, see kdtree.hpp). */
QVQ_API qvq_status qvq_host_kdtree_nn(const double *C, uint32_t K, uint32_t dim, const double *Q, uint64_t nq,
                                      uint32_t *out);
/* The host kd-tree build over C (K x dim), as the device build's image (kdtree_dev.hpp
 * kdb_host_layout: header | nodes[2K], breadth first | point boxes [2K][lo D | hi D] | vind[K]);
 * *need = the image's bytes, written when bytes >= *need (QVQ_EINVAL otherwise).  For tests of
 * the build against a restatement, node for node. */
QVQ_API qvq_status qvq_host_kdtree_image(const double *C, uint32_t K, uint32_t dim, void *img, uint64_t bytes,
                                         uint64_t *need);
/* Exact centroid finalisation from reduced sums, as the device does it:
 * C[k][d] = round(R*hi + lo - bias*cnt) * 2^-scale * fl(1/cnt).  For tests. */
QVQ_API qvq_status qvq_host_finalize(const uint64_t *hi, const uint64_t *lo, const uint64_t *cnt, uint32_t K,
                                     uint32_t dim, int colorspace, double *C_out);
/* Per-block exact contributions of one row of codes, as the device sums them: hi/lo
 * (dim entries each) -- for the host-side sharding tests. */
QVQ_API qvq_status qvq_host_row_terms(const uint8_t *codes, uint32_t dim, int colorspace, uint64_t *hi,
                                      uint64_t *lo);
/* The kernels a shape dispatches to: a training set of n rows of dim components and a codebook of K
 * code vectors (qvq_assign, qvq_update, or a qvq_lbg level of that K): the plan the engine makes
 * for such a level and its run_level switches on, field by field, under the same QVQ_SEARCH /
 * QVQ_KDTREE environment.  For tests that want a given path to run (tests/helpers/largek_cases.py). */
enum { QVQ_PLAN_SEARCH_SMALL = 0, QVQ_PLAN_SEARCH_MF32 = 1, QVQ_PLAN_SEARCH_WIDE = 2, QVQ_PLAN_SEARCH_VALU = 3 };
enum { QVQ_PLAN_RECHECK_MF32 = 0, QVQ_PLAN_RECHECK_STAGED = 1, QVQ_PLAN_RECHECK_CHUNKED = 2,
       QVQ_PLAN_RECHECK_GLOBAL = 3 };
enum { QVQ_PLAN_UPDATE_RUNS = 0, QVQ_PLAN_UPDATE_SORTED = 1, QVQ_PLAN_UPDATE_LDS = 2 };
typedef struct {
    uint32_t search;        /* QVQ_PLAN_SEARCH_SMALL | _MF32 | _WIDE | _VALU */
    uint32_t fused;         /* sums fused into the search (qvq_lbg levels only) */
    uint32_t c32_staged;    /* MF32: fp32 codebook in LDS (the unfused, unpruned search of qvq_assign) */
    uint32_t cb_resident;   /* WIDE: whole codebook in LDS (else streamed slices) */
    uint32_t valu_tiles;    /* VALU: codebook tiles, ceil(K / KT) */
    uint32_t recheck;       /* QVQ_PLAN_RECHECK_MF32 | _STAGED | _CHUNKED | _GLOBAL */
    uint32_t update;        /* QVQ_PLAN_UPDATE_RUNS | _SORTED | _LDS */
    uint32_t update_copies; /* RUNS: LDS copies;  LDS: passes */
    uint32_t prune;         /* a qvq_lbg level of this K searches in pruned order */
    uint32_t device_tree;   /* kd-tree of this K can be built on the device (QVQ_KDTREE=device runs
                               that build; QVQ_KDTREE=host builds no tree image: 0) */
} qvq_plan;
QVQ_API qvq_status qvq_host_plan(uint32_t dim, uint32_t K, uint64_t n, qvq_plan *out);
/* The same for an exact-mode training set (qvq_set_vectors_exact) of dim <= 64 components and a codebook
 * of K code vectors, from the constants the exact kernels' launchers use (quant_amd/csrc/exact_plan.hpp).
 * For tests that want a given chunk or tile edge to run (tests/helpers/exact_cases.py). */
typedef struct {
    uint32_t kc;            /* code vectors per LDS chunk of the fp64 search */
    uint32_t chunks;        /* ceil(K / kc); 1: the whole-codebook path (grid-stride over rows) */
    uint32_t last_chunk;    /* code vectors in the last chunk, 1 .. kc */
    uint32_t templated;     /* 1: the row is held in registers (dim 3, 6, 12, 48) */
    uint32_t tile_rows;     /* T: rows per LDS tile of the Kahan chains (centroids and the mean) */
} qvq_exact_plan;
QVQ_API qvq_status qvq_host_exact_plan(uint32_t dim, uint32_t K, qvq_exact_plan *out);
/* The exact kernels' grid caps, in blocks of `block` rows: more than cap * block rows take the
 * kernel's grid-stride loop a second time (the search, the row-number fill of qvq_set_vectors_exact,
 * the distortion). */
typedef struct { uint32_t block, assign_blocks, iota_blocks, dist_blocks; } qvq_exact_grids;
QVQ_API qvq_status qvq_host_exact_grids(qvq_exact_grids *out);
/* The kernel a decode dispatches to (qvq_decode, qvq_decode_mse, qvq_decode_device): the plan
 * launch_decode switches on (quant_amd/csrc/decode_plan.hpp), from the shape, K and what the
 * device pointers lack in alignment (align_flags: 0 for the host entry points, whose staging is
 * aligned).  For tests that want a given instantiation to run (tests/helpers/decode_cases.py). */
enum { QVQ_DECODE_PIXELS = 0, QVQ_DECODE_ROWS = 1, QVQ_DECODE_ROWS_H = 2 };
enum { QVQ_DECODE_RASTER_UNALIGNED = 1,   /* raster % 8 != 0 */
       QVQ_DECODE_ORIG_UNALIGNED = 2,     /* an original is given and original % 8 != 0 */
       QVQ_DECODE_INDEX_UNALIGNED = 4,    /* indices % 16 != 0 */
       QVQ_DECODE_CODEBOOK_ODD = 8 };     /* codebook % 2 != 0 */
typedef struct {
    uint32_t kernel;        /* QVQ_DECODE_PIXELS: one thread per pixel; _ROWS: 8 pixels per thread, any block
                               height; _ROWS_H: 8 pixels per thread, block height H and no overhang */
    uint32_t H;             /* ROWS_H: 1, 2, 4 or 8; else 0 */
    uint32_t lds;           /* ROWS, ROWS_H: the codebook is staged in LDS (K * bw * bh * 3 <= 48 KB) */
    uint32_t coal;          /* ROWS_H: wave-contiguous stores (ySize % 512 == 0) */
    uint32_t grid;          /* blocks of 256 threads */
    uint32_t lds_bytes;     /* dynamic LDS of the launch */
    uint64_t rounds;        /* trips of the grid-stride loop in the busiest block; >= 2 past the grid cap */
} qvq_decode_plan;
QVQ_API qvq_status qvq_host_decode_plan(uint32_t K, uint32_t xSize, uint32_t ySize, uint32_t bw, uint32_t bh,
                                        uint32_t align_flags, qvq_decode_plan *out);
/* The colour space's byte -> value table (Terms::v64, the values the reference computes):
 * out[b] = the value of byte b.  QVQ_EUNSUPPORTED for CIE1931. */
QVQ_API qvq_status qvq_host_colorspace_values(int colorspace, double out[256]);
/* The value -> code rule of qvq_set_vectors on the host (quant_amd/csrc/byte_image.hpp, the
 * function the device pass applies): *colorspace = QVQ_CS_SCALED if every value of X (n x dim) is a
 * SCALED byte image, else QVQ_CS_NORMAL if every value is a NORMAL one, else -1; codes (n x Dp, Dp =
 * dim rounded up to 4, may be NULL) gets a byte image's codes, pad bytes the space's zero code
 * (0x80 SCALED, 0x00 NORMAL), and is left alone for -1. */
QVQ_API qvq_status qvq_host_classify(const double *X, uint64_t n, uint32_t dim, int32_t *colorspace, uint8_t *codes);
/* The device pass's launch shape: one lane per 4-byte code word (Dp / 4 words per row), `block`
 * lanes per block, at most `blocks` blocks: more than block * blocks words take the kernel's
 * grid-stride loop a second time. */
typedef struct { uint32_t block, blocks; } qvq_ingest_grid;
QVQ_API qvq_status qvq_host_ingest_grid(qvq_ingest_grid *out);
/* The CIE1931 map of qvq_set_images on the host (quant_amd/csrc/cie1931.hpp, the function the
 * tile-to-fp64 kernel and the C++ layer's Cie1931 colour space apply): out [npix][3] = X, Y, Z of
 * rgb [npix][3], the bytes read as signed chars. */
QVQ_API qvq_status qvq_host_cie1931(const uint8_t *rgb, uint64_t npix, double *out);
/* The tile-to-fp64 kernel's launch shape: one lane per (row, pixel in block) slot, n * bw * bh slots,
 * `block` lanes per block, at most `blocks` blocks: more than block * blocks slots take the kernel's
 * grid-stride loop a second time.  One kernel serves every block shape. */
typedef struct { uint32_t block, blocks; } qvq_tile64_grid;
QVQ_API qvq_status qvq_host_tile64_grid(qvq_tile64_grid *out);
/* QVQ_REFINE_RESEED's rule on the host (quant_amd/csrc/reseed_rule.hpp, the text the device
 * passes run).  qvq_host_row_error: *q = the quantised error of the dim values x against the code
 * vector c under the colour space's shift.  qvq_host_reseed_far_key: the key whose u64 maximum over
 * a cell's rows names its far row, (q << 32) | (0xFFFFFFFF - row).  qvq_host_reseed_select: from
 * the K cells' summed errors E, row counts n and far-row keys far, the m seeds in order:
 * empties_out[j] takes row rows_out[j] (K entries each, either may be NULL). */
QVQ_API qvq_status qvq_host_row_error(const double *x, const double *c, uint32_t dim, int colorspace, uint32_t *q);
QVQ_API qvq_status qvq_host_reseed_far_key(uint32_t q, uint32_t row, uint64_t *key);
QVQ_API qvq_status qvq_host_reseed_select(const uint64_t *E, const uint64_t *n, const uint64_t *far, uint32_t K,
                                          uint32_t *empties_out, uint32_t *rows_out, uint32_t *m);
/* The reseed's rows pass: one lane per row, `block` lanes per block, at most `blocks` blocks: more
 * than block * blocks rows take the kernel's grid-stride loop a second time. */
typedef struct { uint32_t block, blocks; } qvq_reseed_grid;
QVQ_API qvq_status qvq_host_reseed_grid(qvq_reseed_grid *out);
/* qvq_median_cut's rule on the host (quant_amd/csrc/median_cut_rule.hpp, the text the kernels run).
 * qvq_host_median_cut_axis: the cut axis of a box from its per-component minima lo and maxima hi
 * (dim entries each).  qvq_host_median_cut_select: the cut t of a box of n rows from its 256-bin
 * histogram on the axis, whose ordinals span [lo, hi], lo < hi <= 255 (QVQ_EINVAL otherwise). */
QVQ_API qvq_status qvq_host_median_cut_axis(const uint32_t *lo, const uint32_t *hi, uint32_t dim, uint32_t *axis);
QVQ_API qvq_status qvq_host_median_cut_select(const uint32_t *hist, uint32_t lo, uint32_t hi, uint64_t n, uint32_t *t);
/* One median-cut level of `boxes` boxes (a power of two: level l has 2^(l-1)) over n rows of dim
 * components: the variant each of its two row passes takes and their launch shape
 * (quant_amd/csrc/median_cut_plan.hpp, the function the launchers switch on).  A pass privatises its
 * per-box state in a block's LDS; boxes that do not fit are cut into *_groups groups of
 * *_group_boxes boxes, each group with blocks of its own that read every row's label and take their
 * boxes' rows; past 16 groups the pass goes straight to global memory (*_lds = 0, *_groups = 0).  A
 * lane per row, `block` lanes per block, at most *_cap blocks per group: more than block * cap rows
 * take a pass's grid-stride loop a second time.  The ranges pass also applies the previous level's
 * cuts; the pass after the last level runs the same loop without ranges (one group, cap 768). */
typedef struct {
    uint32_t range_lds;    /* ranges pass: 1 the boxes' minima and maxima (2 * dim words a box) are privatised in LDS */
    uint32_t hist_lds;     /* histogram pass: 1 the boxes' bins (256 words a box) are privatised in LDS */
    uint32_t full_hist;    /* 1: the per-(box, dim) histograms in one pass replace both (never: 0) */
    uint32_t block;
    uint32_t range_cap, hist_cap;     /* blocks per group at most */
    uint32_t range_grid, hist_grid;   /* blocks per group launched for n rows */
    uint32_t lds_words;    /* 32-bit words of LDS a block privatises in */
    uint32_t range_groups, hist_groups;
    uint32_t range_group_boxes, hist_group_boxes;
} qvq_median_cut_plan;
QVQ_API qvq_status qvq_host_median_cut_plan(uint32_t dim, uint32_t boxes, uint64_t n, qvq_median_cut_plan *out);
/* qvq_kmeanspp's rule on the host (quant_amd/csrc/kmeanspp_rule.hpp, the text the kernels run).
 * qvq_host_kmpp_draw: t = draw(seed, j, T), T > 0 (QVQ_EINVAL otherwise).  qvq_host_kmpp_weight: w of
 * two rows given as their Dp code bytes (pad bytes included), Dp a multiple of 4 up to 64. */
QVQ_API qvq_status qvq_host_kmpp_draw(uint64_t seed, uint64_t j, uint64_t T, uint64_t *t);
QVQ_API qvq_status qvq_host_kmpp_weight(const uint8_t *codes_a, const uint8_t *codes_b, uint32_t Dp, uint32_t *w);
/* The launch shape of qvq_kmeanspp's update pass over n rows (quant_amd/csrc/kmeanspp_plan.hpp, the
 * function the launchers switch on): the rows are cut into `segments` contiguous segments of
 * seg_rows rows (a multiple of block, at least one block; the last may be short), one block of
 * `block` lanes per segment, a lane per row.  At most segments_cap segments, so that the select
 * scans their sums in one block: more than segments_cap * block rows make seg_rows grow. */
typedef struct { uint32_t block, segments, seg_rows, segments_cap; } qvq_kmeanspp_plan;
QVQ_API qvq_status qvq_host_kmeanspp_plan(uint64_t n, qvq_kmeanspp_plan *out);
/* qvq_kmeanspp_greedy's trial count on the host (quant_amd/csrc/kmeanspp_greedy_plan.hpp, the function
 * the call runs): *L = trials, or the default for trials = 0.  QVQ_EINVAL where the call gives it
 * (K = 0, K > 2^20, trials > 16). */
QVQ_API qvq_status qvq_host_kmpp_trials(uint32_t K, uint32_t trials, uint32_t *L);
/* qvq_kmeans_par's sampling test on the host (quant_amd/csrc/kmeans_par_rule.hpp, the text the kernels
 * run): *joins = mulhi64(mix(mix(seed + r) + row), phi) < ell * m.  r in 1 .. 16, ell <= 2^17, m < 2^22
 * (QVQ_EINVAL otherwise). */
QVQ_API qvq_status qvq_host_kmeans_par_join(uint64_t seed, uint32_t r, uint64_t row, uint64_t phi, uint32_t ell, uint32_t m,
                                            int *joins);
/* qvq_kmeans_par's options with the defaults filled in and its launch shape over n rows of dim
 * components (quant_amd/csrc/kmeans_par_plan.hpp, the functions the entry point calls; QVQ_EINVAL
 * where qvq_kmeans_par gives it).  The row passes take qvq_kmeanspp's segments (block, segments,
 * seg_rows, segments_cap as in qvq_kmeanspp_plan); the update holds `chunk` new candidates in LDS per
 * trip; max_candidates = 1 + rounds * round_cap is the length of cand_rows and cand_weights.  The
 * reduction is one block of reduce_block lanes with lds_bytes of dynamic LDS: gw_lds: g and wt per
 * candidate sit there (global memory otherwise), codes_lds: so do the candidates' code words.  Both
 * follow from max_candidates and the padded width, not from the M a call reaches. */
typedef struct {
    uint32_t rounds, ell, round_cap;
    uint32_t block, segments, seg_rows, segments_cap;
    uint32_t chunk, max_candidates;
    uint32_t reduce_block, gw_lds, codes_lds, lds_bytes;
} qvq_kmeans_par_plan;
QVQ_API qvq_status qvq_host_kmeans_par_plan(uint64_t n, uint32_t dim, uint32_t K, const qvq_kmeans_par_opts *opts,
                                            qvq_kmeans_par_plan *out);
/* The launch shape of the K = 1 sums (the mean every qvq_lbg starts from) over n rows of dim
 * components (quant_amd/csrc/mean_plan.hpp, the function the launcher calls): `blocks` summing blocks
 * of `block` lanes.  A lane adds its rows' exact terms in 16-bit fields, 257 adds of 255 at the most,
 * and the kernel does not count them: `blocks` is what keeps every lane within that.  The rows go in
 * groups of group_rows consecutive rows.  chunk_loop (dim <= 16): chunks of chunk_groups groups, chunk
 * c to wave c mod (blocks * block / 64), chunks_in_flight of them per trip, a group of the chunk per
 * lane.  Then the groups left (all of them without the chunk loop), the g-th of them to lane g mod
 * (blocks * block), groups_in_flight per trip; then the last n mod group_rows rows, one each to the first lanes
 * of block 0.  n: 1 .. 2^32 - 1.  For tests (tests/helpers/sums_capacity_ref.py). */
typedef struct {
    uint32_t blocks, block, group_rows, chunk_groups, chunks_in_flight, groups_in_flight, chunk_loop;
} qvq_mean_grid;
QVQ_API qvq_status qvq_host_mean_grid(uint64_t n, uint32_t dim, qvq_mean_grid *out);
/* The Kahan centroids' sort by cell over K >= 1 keys: window_keys keys per launch
 * window (one u32 LDS counter each, within the 160 KB of a workgroup), windows = ceil(K /
 * window_keys) windows, lds_bytes of dynamic LDS per workgroup. */
typedef struct { uint32_t window_keys, windows, lds_bytes; } qvq_kahan_sort_plan;
QVQ_API qvq_status qvq_host_kahan_sort_plan(uint32_t K, qvq_kahan_sort_plan *out);
/* The engine's bounded-wait policy (quant_amd/csrc/wait.hpp) driven by scripted probes, for
 * tests: scenario 0 the work publishes after ~5 ms; 1 it never does, no communicator; 2 it
 * never does, a healthy communicator; 3 the communicator reports an error after ~5 ms; 4 the
 * stream fails; 5 the stream drains without publishing.  Returns the wait's status and its
 * duration in *elapsed_s. */
QVQ_API qvq_status qvq_host_wait_probe(int scenario, double timeout_s, double *elapsed_s);
/* The certificate's helper-thread pool (engine.cpp pool_run) over `rounds` jobs of 1..maxn (<= 64)
 * threads, the count changing from job to job: *errors = job slots that ran other than exactly
 * once.  Host only, for tests. */
QVQ_API qvq_status qvq_host_pool_stress(uint32_t rounds, uint32_t maxn, uint64_t *errors);

#ifdef __cplusplus
}
#endif
#endif /* QVQ_H */
