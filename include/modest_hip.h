/*
 * modest_hip.h — C ABI of libmodest_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the seed-label hot path of YurongYou/MODEST
 * (pre_compute_pp_score -> generate_mask -> gen_label_files).  Every entry
 * point names the reference interface it replaces (paths relative to the
 * reference checkout).  Conventions, all entry points:
 *
 *   - plain pointers and sizes; no torch / numpy types cross this boundary;
 *   - pointers marked [dev] are device (HBM) pointers, [host] are host
 *     pointers; the caller owns every buffer (reference convention:
 *     generate_cluster_mask/utils/iou3d_nms/iou3d_nms_utils.py:47,103);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     work is enqueued on it, the call does not synchronise unless the
 *     description says "blocking";
 *   - return value: 0 = ok, <0 = error (never exit(); the reference's
 *     CHECK_INPUT exits the process, src/iou3d_nms.cpp:14-26);
 *     modest_last_error() returns a thread-local message;
 *   - per-stream scratch lives in a modest_ctx (one per process x GPU).
 */
#ifndef MODEST_HIP_H
#define MODEST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MODEST_OK 0
#define MODEST_ERR_ARG (-1)
#define MODEST_ERR_HIP (-2)
#define MODEST_ERR_CAPACITY (-3)
#define MODEST_ERR_NODEVICE (-4)

typedef struct modest_ctx modest_ctx;

/* ---- library / context ------------------------------------------------ */
int modest_version(void);
const char *modest_last_error(void);
/* Number of visible HIP devices (0 when no GPU; never fails). */
int modest_device_count(void);
int modest_ctx_create(int device, modest_ctx **out);
int modest_ctx_destroy(modest_ctx *ctx);
/* Measurement hook (no reference counterpart): while enabled, the dominant
 * operation of the path -- the neighbour-count stage of modest_pp_count /
 * modest_pp_score / modest_pp_score_frames (every kernel of ONE scan between the
 * live index build and the last join) -- is bracketed by a HIP event pair on the launch stream; collect
 * returns the elapsed milliseconds of up to `cap` calls since begin and
 * disables the hook.                                                          */
/* The context's scratch arena grows on demand (a grow = device synchronise + free + allocate: tens of milliseconds when several
 * processes share the GPU).  A caller that knows what is coming -- the CLI before its first batch, which is shorter than the
 * later ones -- takes the arena in ONE driver call up front.  No reference counterpart (the reference allocates per call).  */
int modest_ctx_reserve_arena(modest_ctx *ctx, uint64_t bytes);
/* Loads the library's device code now (the HIP runtime loads a translation unit's code object at the first launch of one of its
 * kernels: ~0.1 s spread over the first scan of a process otherwise).  The CLIs call it before their loop clocks start.        */
int modest_warmup(modest_ctx *ctx);
int modest_ctx_profile_begin(modest_ctx *ctx, int capacity);
int modest_ctx_profile_collect(modest_ctx *ctx, float *ms_out_host, int cap,
                               int *n_out_host);

/* Calibration.project_velo_to_rect (utils/kitti_util.py:327-329) of the scan rows, float64:
 * out[i] = R0 @ (V2C @ [x y z 1]) with the rounding of numpy's two dgemm calls (one fma chain per
 * output element).  The rect-frame copy of the scan that get_obj's lowest-point search reads
 * (pointcloud_utils.py:278-290) is produced where it is consumed instead of being uploaded.
 * pts [dev] (n,stride) f32; V2C12 / R09 [host] row-major 3x4 / 3x3 f64; out [dev] (n,3) f64. */
int modest_project_velo_to_rect(modest_ctx *ctx, const float *pts_dev, int n, int stride,
                                const double *V2C12, const double *R09, double *out_dev,
                                void *stream);

/* ---- a4  transform_points  (utils/pointcloud_utils.py:11-19) ----------
 * out[i] = (x*T[r][0] (+fma) y*T[r][1] (+fma) z*T[r][2]) + T[r][3], float32,
 * i.e. [p,1] @ T^T, rows 0..2.  `in_stride` is 3 or 4 floats per point
 * (velodyne .bin frames are (n,4): load_velo_scan, pointcloud_utils.py:22-25).
 * T16 is a host pointer to a row-major 4x4 float32 matrix.
 * If remove_center != 0 (nuScenes, pre_compute_pp_score.py:48-52,141-142)
 * points with x in [-1.15,1.75) and y in [-0.65,0.65) of the UNtransformed
 * frame are dropped and the output is compacted in input order;
 * *n_out_dev [dev] receives the number written (may be NULL when
 * remove_center == 0).                                                     */
int modest_transform_points(modest_ctx *ctx, const float *in_dev, int64_t n,
                            int in_stride, const float *T16_host,
                            int remove_center, float *out_xyz_dev,
                            int64_t *n_out_dev, void *stream);

/* ---- a6+a7  cKDTree build + count_neighbors ---------------------------
 * (pre_compute_pp_score.py:54-60,188-193).  For every live point i and
 * traversal t: counts[i*T+t] = #{ h in hist[t] : |p_i-h|^2 <= radius^2 },
 * inclusive, predicate evaluated in float64 on the float32 coordinates
 * exactly as scipy's cKDTree.query_ball_point does.
 *   live_xyz [dev]  (n_live,3) f32, already in the common frame
 *   hist_xyz [dev]  (M,3) f32 stacked traversals, already transformed
 *   trav_offsets [host] (T+1) int64 prefix offsets into hist (points)
 *   counts [dev] (n_live,T) int32 (the reference returns int64; values
 *   are < 2^31 because M < 2^31 is required).                              */
int modest_pp_count(modest_ctx *ctx, const float *live_xyz_dev, int n_live,
                    const float *hist_xyz_dev, const int64_t *trav_offsets_host,
                    int n_trav, double radius, int32_t *counts_dev,
                    void *stream);

/* ---- a8  compute_ephe_score (pre_compute_pp_score.py:68-75) ------------
 * P = c/(sum_t c + 1e-8); H = sum_t -P ln(P+1e-8) / ln T, float64, stored
 * as float32 (np.save(...astype(float32)), :195-196).                      */
int modest_pp_entropy(modest_ctx *ctx, const int32_t *counts_dev, int n_live,
                      int n_trav, float *H_dev, void *stream);

/* a7+a8 fused: counts_dev may be NULL (scratch is used).                  */
int modest_pp_score(modest_ctx *ctx, const float *live_xyz_dev, int n_live,
                    const float *hist_xyz_dev, const int64_t *trav_offsets_host,
                    int n_trav, double radius, int32_t *counts_dev,
                    float *H_dev, void *stream);

/* ---- a1+a3+a4+a5+a6+a7 over a FRAME STORE (history assembly on the device) ------
 * The reference re-reads, transforms and stacks every history frame for every scan
 * (pre_compute_pp_score.py:132-150: load_velo_scan + remove_center + transform_points +
 * np.concatenate) and builds one cKDTree per traversal (:188-190).  Here a raw frame enters the
 * frame store ONCE: modest_frame_sort orders its points by the 8x8-cell tile of a world lattice
 * (cell edge c = r*(1+2^-10), the lattice is shared by all frames of a data set) and writes the
 * prefix table tile -> first point.  A scan then names its frames by descriptor
 * (modest_pp_frame: store buffers + traversal id + the float32 relative pose of
 * get_relative_pose, :27-28) and modest_pp_score_frames streams the frames through that table,
 * applies the pose on the fly (transform_points' float32 rounding) and counts neighbours: no
 * stacked, transformed copy of the history exists.
 *
 * W [host] 2x4 float64, rows x and y of (1/c) * (raw frame -> world lattice metres).
 * TX0, TY0: global tile coordinates of the table's first tile; the table covers
 * MODEST_FRAME_NTF x MODEST_FRAME_NTF tiles (callers centre it on the sensor origin).
 * Outputs [dev]: xyz (n,3) f32 tile-sorted raw points, perm (n) u32 sorted -> original index,
 * tab (NTF*NTF+1) u32 prefix offsets (row-major tiles); tab[NTF*NTF] = points inside the table,
 * the rest of xyz are outliers.  n_inside_host[k] receives that count (a scan whose frames have
 * outliers must use the stacked path, modest_pp_score).  Blocking.                             */
#define MODEST_FRAME_NTF 128
typedef struct {
    const float *raw_dev;   /* (n, stride) f32, stride 3 or 4 (velodyne .bin: load_velo_scan) */
    int32_t n, stride;
    int32_t TX0, TY0;
    double W[8];
    float *xyz_dev;
    uint32_t *perm_dev;
    uint32_t *tab_dev;
} modest_frame_sort_job;
int modest_frame_table_tiles(void);   /* MODEST_FRAME_NTF of the built library */
int modest_frame_sort(modest_ctx *ctx, const modest_frame_sort_job *jobs_host, int n_jobs,
                      int32_t *n_inside_host, void *stream);
/* The same sort, NOT blocking (an ingest thread keeps several batches in flight behind the compute stream's
 * kernels).  jobs_scratch_dev [dev]: n_jobs * MODEST_FRAME_SORT_JOB_BYTES, caller-owned, alive until the
 * launch has run; n_inside_pinned [PINNED host] (n_jobs) int32: written by the kernel itself, readable once
 * `stream` has passed the launch.  The grid sort of small batches also keeps per-point rank / bin words and its chunk
 * table in the CONTEXT's scratch arena, in stream order (and grows the arena on first use: a device synchronise): `ctx`
 * must not be shared with calls that run on another stream at the same time -- an ingest thread owns a context of its own
 * (pre_compute_pp_score.py: FrameLoader).                                                                           */
#define MODEST_FRAME_SORT_JOB_BYTES 128
int modest_frame_sort_async(modest_ctx *ctx, const modest_frame_sort_job *jobs_host, int n_jobs,
                            void *jobs_scratch_dev, int32_t *n_inside_pinned_host, void *stream);

#define MODEST_FRAME_REMOVE_CENTER 1   /* remove_center, pre_compute_pp_score.py:48-52 */
typedef struct {
    const float *xyz_dev;      /* store buffers of the frame */
    const uint32_t *tab_dev;
    int32_t n, TX0, TY0;
    int32_t trav;              /* traversal index in [0, n_trav) (ignored for the live scan) */
    int32_t flags;             /* MODEST_FRAME_REMOVE_CENTER */
    float rel[12];             /* rows 0..2 of get_relative_pose(...).astype(float32) */
} modest_pp_frame;
/* counts[i*T+t] / H[i] are indexed by the ORIGINAL point order of the live frame (perm).
 * A [host] 2x4 float64: rows x, y of (1/c) * (common frame -> world lattice metres); it must agree
 * with W * rel^-1 of every frame to better than r/1024 (callers check 1e-4 m).
 * counts_dev may be NULL (scratch) when only H is wanted; H_dev may be NULL.  n_trav <= 64.
 * Not blocking.                                                                              */
int modest_pp_score_frames(modest_ctx *ctx, const modest_pp_frame *live_host,
                           const uint32_t *live_perm_dev, const modest_pp_frame *frames_host,
                           int n_frames, int n_trav, const double *A8_host, double radius,
                           int32_t *counts_dev, float *H_dev, void *stream);

/* The same operation for SEVERAL scans in one chain of launches (the reference's scan loop,
 * pre_compute_pp_score.py:122-196, has no dependency between iterations): every kernel of the chain takes the
 * scan as a second grid dimension, so the nine sub-10 us launches are paid once per batch and the persistent
 * join workgroups take slices of any scan of the batch.  Results are those of n_scans separate calls, bit for
 * bit.  Arrays of n_scans entries [host]; counts_dev / H_dev (arrays or entries) may be NULL as above; scans the
 * batched kernels do not cover (no live points, no history) make the call fall back to separate calls.
 * Scratch: ~0.26 GB per Lyft-shape scan of the batch.  Not blocking.                                      */
int modest_pp_score_frames_batch(modest_ctx *ctx, int n_scans, const modest_pp_frame *const *live_host,
                                 const uint32_t *const *live_perm_dev, const modest_pp_frame *const *frames_host,
                                 const int32_t *n_frames, int n_trav, double radius,
                                 int32_t *const *counts_dev, float *const *H_dev, void *stream);

/* ---- the same operation for a BLOCK of scans that share history frames -------------------------
 * Consecutive scans of a shard share 35 of their 36 frames per traversal
 * (data_preprocessing/lyft/split_traintest.py:64,97): the reference re-stacks and re-indexes them scan
 * after scan (pre_compute_pp_score.py:132-150,188-190).  modest_pp_score_block takes the UNION of the
 * block's frames once -- every point is copied, raw, into the list of its world-lattice tile (list sizes
 * follow from the frames' prefix tables: no count pass) and every list is ordered by lattice cell -- and
 * then joins every scan against that store: records are read straight into registers, the scan's own
 * float32 relative pose (get_relative_pose, :27-28; transform_points' rounding) is applied per record,
 * neighbours are counted with scipy's float64 predicate (:54-60).  Results are those of
 * modest_pp_score_frames, bit for bit.
 *
 * frames_host [host] (n_frames): the union, one entry per (frame, occurrence): a frame that a scan's index list names
 *   k times (split_traintest.py:86-101; the reference stacks it k times, pre_compute_pp_score.py:132-150) is k entries
 *   with the same buffers, and that scan's member list names each of them once -- a member list that names one entry
 *   twice is refused (MODEST_ERR_ARG).  lat = the 2x4 float64 map the frame was
 *   sorted with (modest_frame_sort_job::W); flags: MODEST_FRAME_REMOVE_CENTER (all or none).  The ORDER of the table is
 *   the caller's: a scan reads, cell by cell, the records of the table range [its first frame, its last frame] (and masks
 *   the frames in between that are not its own), so an order in which every scan's frames are contiguous -- for the
 *   sliding windows of a shard: by (first scan, last scan) that uses the frame -- saves the other scans' records.
 * scans_host [host] (n_scans): the live frame of the store (xyz / perm / tab, lat as above, rel = its float32
 *   relative pose), the scan's history frames as (member_slot = index into frames_host, member_trav,
 *   member_rel = rows 0..2 of the frame's float32 relative pose IN THIS SCAN), outputs as above.
 * Requirements (the caller checks them; modest_pp_score_frames_batch has none of them): no frame has
 *   points outside its table; every pose agrees with the lattice to 1e-4 m (lat == (1/cell) * W and
 *   W ~ A * rel); cell >= radius * (1 + 2^-9); the live frames' tables lie within
 *   modest_pp_block_limits() tiles of each other.  n_trav <= 64.  Not blocking.                      */
typedef struct {
    const float *xyz_dev;
    const uint32_t *tab_dev;
    int32_t n, TX0, TY0, flags;
    double lat[8];
} modest_pp_block_frame;
typedef struct {
    const float *xyz_dev;
    const uint32_t *perm_dev;
    const uint32_t *tab_dev;
    int32_t n, TX0, TY0, n_members;
    double lat[8];
    float rel[12];
    const int32_t *member_slot;   /* [host] */
    const int32_t *member_trav;   /* [host] */
    const float *member_rel;      /* [host] (n_members, 12) */
    int32_t *counts_dev;          /* [dev] (n, n_trav) or NULL */
    float *H_dev;                 /* [dev] (n) or NULL */
} modest_pp_block_scan;
int modest_pp_block_limits(int32_t *max_window_tiles, int32_t *max_scans, int32_t *max_frames);
int modest_pp_score_block(modest_ctx *ctx, const modest_pp_block_frame *frames_host, int n_frames,
                          const modest_pp_block_scan *scans_host, int n_scans, int n_trav, double radius,
                          double cell, void *stream);
/* The same for scans with DIFFERENT numbers of traversals in one block: n_trav_scan [host] (n_scans), 1..64 each.
 * The reference accepts a traversal per scan (closest pose within 3 m, data_preprocessing/lyft/split_traintest.py:17,79)
 * and asks for at least two (:111; pre_compute_pp_score.py:125-126), so T changes along a sequence
 * (pre_compute_pp_score.py:132-150,181-194 run per scan with that scan's own list).  counts_dev of scan s is
 * (n, n_trav_scan[s]); member_trav of scan s < n_trav_scan[s]; H of scan s is normalised by ln n_trav_scan[s] (:72).       */
int modest_pp_score_block_mixed(modest_ctx *ctx, const modest_pp_block_frame *frames_host, int n_frames,
                                const modest_pp_block_scan *scans_host, int n_scans, const int32_t *n_trav_scan,
                                double radius, double cell, void *stream);

/* ---- the tables of a block call from a frame store's slot tables (host only) -------------------------------------------
 * What a caller of modest_pp_score_block[_mixed] has to build from the scans' index lists (valid_idx_info.pkl,
 * data_preprocessing/lyft/split_traintest.py:79-101; the reference stacks every scan's list anew, pre_compute_pp_score.py:132-150):
 * the union of the lists as (frame, occurrence) entries ordered by the middle of the interval of scans that use an entry, every scan's
 * members as indices into it, and the checks listed under modest_pp_score_block (no frame with points outside its table, every pose
 * within 1e-4 m of the lattice, the live tables within the block window, one remove_center flag).  store: slot -> modest_pp_frame record
 * (buffers and table origin), W (n_slots,4,4) float64 raw frame -> world, lat (n_slots,8) = modest_frame_sort_job::W, perm_dev
 * (n_slots) the frames' perm buffers as integers, clean (n_slots) bytes: 1 = no point outside the table.
 * Per scan s: live_host[s] = the live frame's record with rel = its float32 relative pose; members_host[s] = n_members[s] records
 * (trav, flags, rel = the frame's float32 relative pose in this scan); slots_host[s] = n_members[s] + 1 store slots: the members',
 * then the live frame's.  apply_rule != 0: the measured rule between block and chain (>= 4 scans, >= 12 entries per traversal and
 * scan, union <= 4 x a scan's entries and <= 2048).  Outputs [host]: frames_out (capacity frames_cap entries; *n_frames_out used),
 * scans_out (n_scans; counts_dev / H_dev left NULL for the caller), member_slot_out / member_trav_out (sum of n_members) and
 * member_rel_out (12 floats per member), which scans_out points into.
 * Returns MODEST_BLOCK_TABLES_BLOCK (tables built), _CHAIN (the block path does not apply: use modest_pp_score_frames_batch),
 * _SPLIT (worth the block path in two halves), -1 = bad arguments.                                                                 */
#define MODEST_BLOCK_TABLES_BLOCK 0
#define MODEST_BLOCK_TABLES_CHAIN 1
#define MODEST_BLOCK_TABLES_SPLIT 2
typedef struct {
    const modest_pp_frame *records;
    const double *W;
    const double *lat;
    const uint64_t *perm_dev;
    const uint8_t *clean;
    int64_t n_slots;
    double radius, cell;
    int32_t window_span;   /* tiles the live tables' origins may differ by (window of modest_pp_block_limits - table - 2) */
} modest_pp_store_view;
int modest_pp_block_tables(const modest_pp_store_view *store, int n_scans, const modest_pp_frame *const *live_host,
                           const modest_pp_frame *const *members_host, const int64_t *const *slots_host,
                           const int32_t *n_members, const int32_t *n_trav_scan, int apply_rule,
                           modest_pp_block_frame *frames_out, int32_t frames_cap, int32_t *n_frames_out,
                           modest_pp_block_scan *scans_out, int32_t *member_slot_out, int32_t *member_trav_out,
                           float *member_rel_out);

/* ---- a9  estimate_plane / RANSACRegressor inner loops -----------------
 * (utils/pointcloud_utils.py:44-65; sklearn RANSACRegressor defaults).
 * Candidate selection: z<max_hs, xlo<x<xhi, ylo<y<yhi (strict), compacted in
 * input order into cand_xyz [dev] (capacity n), *n_cand_dev [dev].
 * n_cand_dev may be any device-accessible word: device memory, or pinned host
 * memory (hipHostMalloc) -- then the count is on the host after a stream
 * synchronise, without a copy.  Same for n_kept_dev below.                   */
int modest_plane_candidates(modest_ctx *ctx, const float *pts_dev, int n,
                            int stride, float max_hs, float xlo, float xhi,
                            float ylo, float yhi, float *cand_xyz_dev,
                            int32_t *cand_idx_dev, int32_t *n_cand_dev,
                            void *stream);
/* MAD threshold: median(|z - median(z)|) over the candidates, float32
 * arithmetic, numpy.median semantics (mean of the two middle values when n
 * is even).  Blocking; result written to *mad_host.                         */
int modest_mad_threshold(modest_ctx *ctx, const float *cand_xyz_dev,
                         int n_cand, float *mad_host, void *stream);
/* The same for `count` candidate sets, one workgroup each, up to 16 sets per launch: a scan's two plane fits
 * (generate_mask.py:55-56 and clustering_utils.py:126) take their thresholds from one call.
 * cand_xyz_dev / n_cand: host arrays of `count` device pointers / sizes (each >= 1); mad_host[count].
 * Blocking.                                                                 */
int modest_mad_threshold_batch(modest_ctx *ctx, const float *const *cand_xyz_dev,
                               const int32_t *n_cand, int count, float *mad_host,
                               void *stream);
/* sklearn.linear_model.RANSACRegressor().fit as estimate_plane calls it (pointcloud_utils.py:52-53:
 * LinearRegression, min_samples 3, residual threshold = MAD(z) passed in as `thr`, max_trials 100,
 * stop_probability 0.99) behind one call: triplets drawn from numpy's legacy MT19937 stream exactly
 * as sklearn's sample_without_replacement consumes it (key624 / pos = RandomState.get_state()[1:3],
 * advanced in place by the EXECUTED trials), batches of `batch` <= 64 trials scored per device round
 * trip, the sequential accept rule with the dynamic trial bound, the final least-squares refit.
 * n_cand must exceed 300 (below that sklearn samples with another method: host path).
 * model64_out[3] = (c0, c1, b) of the refit; best_model_out[3] the winning trial's float32 plane;
 * triplets_out (max_trials,3) optional.  status_out: 0 ok, 1 no consensus set (sklearn raises
 * ValueError), 2 degenerate consensus set (refit on the host from best_model_out).            */
int modest_ransac_plane(modest_ctx *ctx, const float *cand_xyz_dev, int n_cand, float thr,
                        uint32_t *mt_key624, int32_t *mt_pos, int max_trials,
                        double stop_probability, int batch, double *model64_out,
                        float *best_model_out, int32_t *triplets_out, int32_t *n_trials_out,
                        int32_t *n_inliers_out, int32_t *status_out, void *stream);
/* The generator half alone (host only, no device work): n_trials triplets of
 * sample_without_replacement(n_population > 300, 3) from the same stream.                    */
int modest_mt19937_triplets(uint32_t *mt_key624, int32_t *mt_pos, uint32_t n_population,
                            int n_trials, int32_t *triplets_out);

/* The RNG-independent part of the two ground fits of a scan (generate_mask.py:55-56 and
 * clustering_utils.py:126) in one call: both candidate selections from one pass over the rows
 * (modest_plane_candidates semantics, compacted in row order) and both MAD thresholds, two
 * launches and one stream sync.  specs10 [host] = {max_hs, xlo, xhi, ylo, yhi} x 2;
 * candA / candB [dev] (n,3) f32 outputs; n_cand2_host[2]; mad2_host[2] (NaN for an empty set). */
int modest_plane_prepare(modest_ctx *ctx, const float *pts_dev, int n, int stride,
                         const float *specs10, float *candA_dev, float *candB_dev,
                         int32_t *n_cand2_host, float *mad2_host, void *stream);
/* Score K trial models z = c0*x + c1*y + b (float32, pred = fma chain
 * fmaf(y,c1,x*c0)+b) against all candidates in ONE launch:
 *   n_inliers[k] = #{ |z - pred| <= thr },  sse[k], sy[k], syy[k] over the
 *   inliers in float64 (for the R^2 tie-break).  models [host] (K,3) f32.
 *   outputs [host], blocking.                                               */
int modest_ransac_score_trials(modest_ctx *ctx, const float *cand_xyz_dev,
                               int n_cand, const float *models_host, int K,
                               float thr, int32_t *n_inliers_host,
                               double *sse_host, double *sy_host,
                               double *syy_host, void *stream);
/* One round trip for a batch of RANSAC trials: (optional) MAD threshold, the
 * exact-fit plane through the three candidates `triplets[k]` of every trial
 * (float64 -> float32; NaN for a degenerate triplet) and the scoring of all K
 * planes.  *thr_inout [host]: < 0 on entry = compute the MAD threshold on the
 * device (returned on exit), otherwise the threshold to use.  triplets [host]
 * (K,3) int32 indices into the candidates; models_out [host] (K,3) float32.
 * Blocking.                                                                   */
int modest_ransac_trials(modest_ctx *ctx, const float *cand_xyz_dev, int n_cand,
                         const int32_t *triplets_host, int K, float *thr_inout_host,
                         float *models_out_host, int32_t *n_inliers_host,
                         double *sse_host, double *sy_host, double *syy_host,
                         void *stream);
/* Least-squares refit of z ~ x,y over the inliers of `model` (float64
 * normal equations, centred); out_model [host] (3) float64. Blocking.       */
int modest_ransac_refit(modest_ctx *ctx, const float *cand_xyz_dev, int n_cand,
                        const float *model_host, float thr,
                        double *out_model_host, int32_t *n_inliers_host,
                        void *stream);

/* ---- a10+a11 above_plane & range mask (pointcloud_utils.py:68-81,
 * generate_mask.py:57-65).  keep[i] = !(dist<offset && in only_range) &&
 * (lx0 < x <= lx1) && (ly0 < y <= ly1); dist = (p . n + d)/|n| in float64.
 * Compacts kept points (input order) to kept_xyz/kept_idx; mask is uint8.   */
int modest_plane_range_mask(modest_ctx *ctx, const float *pts_dev, int n,
                            int stride, const double *plane4_host,
                            double offset, const double *only_range4_host,
                            const double *limit_range4_host,
                            uint8_t *mask_dev, float *kept_xyz_dev,
                            int32_t *kept_idx_dev, int32_t *n_kept_dev,
                            void *stream);

/* ---- a12+a13 precompute_affinity_matrix('radius_mutual_knn','l1') +
 * DBSCAN(metric='precomputed') (utils/clustering_utils.py:7-60,
 * generate_mask.py:75-81), evaluated on the implicit graph:
 *   edge(i,j) <=> d2(i,j) <= min(r2_k(i), r2_k(j), radius^2)   (float64 d2)
 *                 and (double)(float)|pp_i - pp_j| <= eps
 *   core(i)   <=> deg(i) + 1 >= min_samples
 *   label     =  rank of the component's smallest core index; border point
 *                -> smallest label among adjacent cores; noise -> -1.
 * xyz [dev] (n,3) f32, pp [dev] (n) f32, labels [dev] (n) int32.
 * kth_d2 [dev] (n) float64 optional output (squared distance to the k-th
 * neighbour, +inf when fewer than k neighbours lie within radius).          */
int modest_cluster_dbscan(modest_ctx *ctx, const float *xyz_dev,
                          const float *pp_dev, int n, int k_neighbors,
                          double radius, double eps, int min_samples,
                          int32_t *labels_dev, double *kth_d2_dev,
                          int32_t *n_clusters_host, void *stream);

/* Non-default graph / weight branches of precompute_affinity_matrix (SURVEY §8f-3;
 * utils/clustering_utils.py:16-56), same DBSCAN semantics as above:
 *   neighbor_type  RADIUS_MUTUAL_KNN (configs default) | RADIUS (edge <=> d2 <= radius^2)
 *   affinity_type  L1 |pp_i - pp_j| (default) | EXP exp((pp_i - pp_j)^2) | L2_4D the reference's
 *                  '3d_l2_distance': float32 norm of the difference of the (n,4) scan rows,
 *                  i.e. xyz AND intensity (intensity_dev (n) float32 required)
 *   KNN (directed: the rows of kneighbors_graph), SYM_KNN (graph + graph.T), MUTUAL_KNN
 *   (graph .* graph.T): exact k-th neighbour distances without a radius bound (the grid search
 *   grows until the k-th distance is certified); `radius` only sizes the grid cells there.
 *   For KNN sklearn's sequential DBSCAN on the directed graph is reproduced exactly:
 *   label(v) = rank of the smallest-index core point that reaches v through core points.     */
#define MODEST_GRAPH_RADIUS_MUTUAL_KNN 0
#define MODEST_GRAPH_RADIUS 1
#define MODEST_GRAPH_KNN 2
#define MODEST_GRAPH_SYM_KNN 3
#define MODEST_GRAPH_MUTUAL_KNN 4
#define MODEST_AFFINITY_L1 0
#define MODEST_AFFINITY_EXP 1
#define MODEST_AFFINITY_L2_4D 2
int modest_cluster_dbscan_ex(modest_ctx *ctx, const float *xyz_dev, const float *pp_dev,
                             const float *intensity_dev, int n, int neighbor_type,
                             int affinity_type, int k_neighbors, double radius, double eps,
                             int min_samples, int32_t *labels_dev, double *kth_d2_dev,
                             int32_t *n_clusters_host, void *stream);

/* The per-scan body of generate_mask.py:57-88 as ONE call: above_plane + limit_range mask of the
 * scan rows (modest_plane_range_mask), the affinity graph and DBSCAN of the kept rows
 * (modest_cluster_dbscan_ex) and `labels[ptc_mask] = cluster labels` on an array preset to -1.
 * The first kernel masks, compacts, presets the labels and counts the kept rows per cell of a grid
 * fixed around limit_range (no bounding-box pass, no separate gathers of pp / intensity, no label
 * scatter launch); one stream sync inside (the kept count sizes the launches that follow).
 * pts [dev] (n,stride) f32 scan rows, pp [dev] (n) f32, labels [dev] (n) int32: -1 = masked out or
 * noise, else the DBSCAN label.  n_kept_host / n_clusters_host: host words.  When the graph needs
 * k neighbours and only n_kept <= k rows are kept the call fails with MODEST_ERR_ARG and the
 * message sklearn's kneighbors raises (n_kept_host is valid).                                 */
int modest_mask_cluster(modest_ctx *ctx, const float *pts_dev, int n, int stride, const float *pp_dev,
                        const double *plane4, double offset, const double *only_range4,
                        const double *limit_range4, int neighbor_type, int affinity_type,
                        int k_neighbors, double radius, double eps, int min_samples,
                        int32_t *labels_dev, int32_t *n_kept_host, int32_t *n_clusters_host,
                        void *stream);

/* ---- the mask stage of one scan behind one call ------------------------------------------
 * generate_mask.py:52-88 + clustering_utils.py:119-135: estimate_plane (RANSAC) for the mask and for
 * filter_labels, above_plane + limit_range mask, affinity graph + DBSCAN, labels[ptc_mask] = ...,
 * is_valid_cluster on every cluster, relabelling to 0 = background / 1..C -- i.e. everything of
 * generate_mask_scan up to `labels_filtered`, with no interpreter between the device round trips.
 * The pieces are the entry points above (modest_plane_prepare, modest_ransac_plane x 2,
 * modest_mask_cluster, modest_cluster_stats); the scalar glue (plane_from_linear_model, the four
 * comparisons per cluster incl. numpy's float32 percentile interpolation, the relabel table) is
 * restated in the library with numpy's rounding.
 * mt_key624 / mt_pos: numpy RandomState (MT19937) words, advanced by the executed trials of both fits
 * (pass copies and commit them when info_out[3] == 0).  labels_out [host] (n) int64 = the
 * `labels_filtered` array; plane1_out / plane2_out [host] (4) f64.
 * info_out[8]: {kept rows, DBSCAN clusters, largest final label, status, candidates of fit 1, of fit 2,
 * trials of fit 1, of fit 2}.  status != 0: nothing was committed, take the host path --
 * SMALL_SET (a candidate set of <= 300 points: sklearn samples those with another method),
 * NO_CONSENSUS, DEGENERATE (consensus set without a unique plane), TOO_FEW_KEPT (sklearn's
 * kneighbors raises).                                                                          */
typedef struct modest_mask_params {
    float max_hs1, range1[4];        /* plane_estimate.max_hs, .range {xlo, xhi, ylo, yhi}           */
    float max_hs2, range2[4];        /* filter_labels' hard-coded second fit (clustering_utils.py:126) */
    double offset;                   /* plane_estimate.offset                                        */
    int32_t use_only_range;
    double only_range[4];            /* above_plane only_range                                       */
    double limit_range[4];
    int32_t neighbor_type, affinity_type, k_neighbors, min_samples;
    double radius, eps;
    int32_t min_points;              /* filtering.*                                                  */
    double max_min_height, min_max_height;
    double quantile;                 /* np.true_divide(percentile, np.float32(100)) as a double      */
    float min_percentile_pp_score;
    int32_t max_trials, batch;       /* RANSACRegressor defaults: 100; trials per device round trip  */
    double stop_probability;
} modest_mask_params;
#define MODEST_STAGE_SMALL_SET 1
#define MODEST_STAGE_NO_CONSENSUS 2
#define MODEST_STAGE_DEGENERATE 3
#define MODEST_STAGE_TOO_FEW_KEPT 4
#define MODEST_STAGE_HOST_RULE 5   /* a RANSAC trial bound on a rounding boundary: the host loop (host libm) decides */
int modest_mask_stage(modest_ctx *ctx, const float *pts_dev, int n, int stride, const float *pp_dev,
                      const modest_mask_params *params, uint32_t *mt_key624, int32_t *mt_pos,
                      double *plane1_out, double *plane2_out, int64_t *labels_out, int32_t *info_out,
                      void *stream);

/* The same stage for a CHAIN of scans (the reference's scan loop, generate_mask.py:52, has no dependency between
 * iterations): the ground fits stay per scan, from the mask kernel on the scans advance together -- one launch per
 * kernel of the mask / graph / DBSCAN block and of the cluster statistics for the whole chain (the scan is a second
 * grid dimension), three round trips per chain instead of three per scan.  Every scan works in its OWN context
 * (scratch, pinned words, persistent counters); arguments per scan as in modest_mask_stage.  Results are those of
 * separate calls, bit for bit; configurations the chain does not cover (k-NN graphs without a radius,
 * 3d_l2_distance) and chains of one scan take the separate calls.  Blocking.
 * The trial loops of the two fits run ON THE DEVICE for max_trials <= 128 (csrc/plane.hip: rsd_*; numpy's MT19937 as
 * sklearn's sample_without_replacement consumes it, the sequential accept rule, _dynamic_max_trials, refit and plane,
 * the generator advanced by the executed trials): one synchronise for both fits + the mask kernel.  A scan whose trial
 * bound sits on a rounding boundary of log / pow comes back with info_out[3] = MODEST_STAGE_HOST_RULE and an untouched
 * generator, like the other hand-back statuses.  MODEST_RANSAC_HOST=1 in the environment keeps the loops on the host
 * (batches of params->batch trials per round trip).                                                                */
typedef struct modest_mask_stage_scan {
    modest_ctx *ctx;
    const float *pts_dev;
    int32_t n, stride;
    const float *pp_dev;
    uint32_t *mt_key624;
    int32_t *mt_pos;
    double *plane1_out, *plane2_out;
    int64_t *labels_out;
    int32_t *info_out;
    /* optional (NULL: not wanted): the indices, ascending, of the points whose labels_out is > 0 (capacity n) and their number --
     * what the box tail (modest_boxes_scan::members) walks instead of all n points                                            */
    int32_t *members_out;
    int32_t *n_members_out;
} modest_mask_stage_scan;
int modest_mask_stage_batch(const modest_mask_stage_scan *scans, int n_scans, const modest_mask_params *params,
                            void *stream);

/* ---- a14 filter_labels / is_valid_cluster statistics ------------------
 * (utils/clustering_utils.py:94-135).  For each label c in [0, n_clusters):
 * out[c*6 + {0: member count, 1: min, 2: max signed distance to `plane`
 * ((p . n + d)/|n|, float64), 3: a, 4: b, 5: gamma}] where a, b are the two
 * order statistics of the members' PP scores that numpy.percentile(pp,
 * 100*quantile) interpolates between (method 'linear': virtual index
 * (n-1)*quantile = floor + gamma).  labels [dev] int32, -1 = noise.
 * out [host] (n_clusters,6) float64.  Blocking.                              */
int modest_cluster_stats(modest_ctx *ctx, const float *pts_dev, int n, int stride,
                         const float *pp_dev, const int32_t *labels_dev,
                         int n_clusters, const double *plane4_host,
                         double quantile, double *out_host, void *stream);

/* ---- a15-a19, a21 the second half of a scan behind three calls (generate_mask.py:88-103,
 * gen_label_files.py:44-52) ------------------------------------------------------------------------
 * modest_scan_boxes: labels_inout [host] (n) int64 holds `labels_filtered` (0 = background, 1..n_lab, every
 * label with members) and receives the final labels (generate_mask.py:100-103).  For every cluster: its
 * rect-frame points (Calibration.project_velo_to_rect, kitti_util.py:327-329), the closeness fit
 * (pointcloud_utils.py:167-216; 901 headings on the device, rectangle_at_angle's tail on the host),
 * get_obj (:292-317) with the lowest point from the device, the volume gate (generate_mask.py:91-98).
 * pts_dev / pts_host: the same (n,stride) float32 scan in both memories.  angles / cossin / cossin90 [host]:
 * the caller's numpy tables (heading, (cos, sin) of it, (cos, sin) of heading + pi/2): the library takes
 * no cosine of its own, so the host's numpy defines them as in the reference.
 * objs_out [host] (n_lab,8) float64 rows {t0, t1, t2, l, w, h, ry, volume} of ALL clusters in label order,
 * keep_out [host] (n_lab) int32 = passed the volume gate.  info_out[2]: {boxes kept, status}; status != 0:
 * nothing was written, take the host statement (1: a cluster too large for the extents kernel, 2: a box
 * footprint without any scan point -- numpy raises there).  Blocking (two round trips).               */
typedef struct modest_boxes_params {
    double V2C[12], R0[9];          /* Calibration, row major 3x4 / 3x3                                  */
    const double *angles;           /* (n_angles) headings of closeness_rectangle (:170-175)             */
    const double *cossin;           /* (n_angles,2)                                                      */
    const double *cossin90;         /* (n_angles,2) of heading + pi/2                                    */
    int32_t n_angles;
    double d0;                      /* closeness criterion floor (1e-2)                                  */
    double min_volume, max_volume;  /* filtering.min_volume / max_volume                                 */
} modest_boxes_params;
int modest_scan_boxes(modest_ctx *ctx, const float *pts_dev, const float *pts_host, int n, int stride,
                      int64_t *labels_inout_host, int n_lab, const modest_boxes_params *params,
                      double *objs_out_host, int32_t *keep_out_host, int32_t *info_out_host, void *stream);
/* The same for a CHAIN of scans: the host phases per scan, ONE closeness launch over all clusters of the chain and ONE
 * lowest-point launch over all boxes (two round trips per chain instead of two per scan).  Every scan in its own
 * context; arguments per scan as above.  info_out[1] == 1 on every scan when some cluster of the chain is too large
 * for the extents kernel (go scan by scan then).  Results are those of separate calls.  Blocking.               */
typedef struct modest_boxes_scan {
    modest_ctx *ctx;
    const float *pts_dev, *pts_host;
    int32_t n, stride;
    int64_t *labels_inout;
    int32_t n_lab;
    double *objs_out;
    int32_t *keep_out, *info_out;
    /* optional (NULL: every point is looked at): the indices, ascending, of the points with labels_inout > 0, as the mask stage
     * reports them (modest_mask_stage_scan::members_out); the host passes then touch the members only                    */
    const int32_t *members;
    int32_t n_members;
} modest_boxes_scan;
int modest_scan_boxes_batch(const modest_boxes_scan *scans, int n_scans, const modest_boxes_params *params, void *stream);
/* objs_nms' boxes [t0, t2, 0, l, w, h, -ry] as float32 (pointcloud_utils.py:322-324) and their BEV IoU
 * matrix (iou3d_nms_utils.boxes_iou_bev) -> iou_out [host] (k,k) float32.  Blocking.                  */
int modest_objs_iou(modest_ctx *ctx, const double *objs8_host, int k, float *iou_out_host, void *stream);
/* ... of the box sets of a chain of scans: one launch and one round trip for all (k[s] boxes, (k[s],k[s]) out each). */
int modest_objs_iou_batch(modest_ctx *ctx, const double *const *objs8_host, const int32_t *k, int n_sets,
                          float *const *iou_out_host, void *stream);
/* ---- stages 2 + 3 of a CHAIN of scans behind one call (generate_mask.py:52-103 + the IoU matrix of gen_label_files.py:44-45,
 * pointcloud_utils.py:320-327): modest_mask_stage_batch, modest_scan_boxes_batch and modest_objs_iou_batch in sequence, results
 * leaving the library once.  Per scan (own context, as in those calls): labels_out [host] (n) int64 = the FINAL labels
 * (generate_mask.py:100-103); objs_out [host] (max_boxes,8): the first info_out[9] rows = the boxes that passed the volume gate,
 * in label order; iou_out [host]: their (k,k) float32 BEV IoU, row major, packed (NULL when nms_enable == 0);
 * members_scratch [host] (n) int32.  info_out[12]: [0..7] as modest_mask_stage; [8] clusters before the volume gate; [9] k;
 * [10] 0 = done, 1 = the mask stage handed the scan back (generator untouched, nothing written), 2 = the box tail handed it
 * back, 3 = more than max_boxes clusters -- for 2 and 3 labels_out holds `labels_filtered` and the generator is advanced: the
 * caller runs modest_scan_boxes / its host statement on them.  np.diag(iou).argsort() and the label text stay with the caller
 * (modest_label_lines).  Blocking.                                                                                          */
typedef struct modest_seed_scan {
    modest_ctx *ctx;
    const float *pts_dev, *pts_host;
    int32_t n, stride;
    const float *pp_dev;
    uint32_t *mt_key624;
    int32_t *mt_pos;
    double *plane1_out, *plane2_out;
    int64_t *labels_out;
    int32_t *members_scratch;
    double *objs_out;
    float *iou_out;
    int32_t *info_out;
} modest_seed_scan;
int modest_seed_chain(const modest_seed_scan *scans, int n_scans, const modest_mask_params *mask_params,
                      const modest_boxes_params *boxes_params, int max_boxes, int nms_enable, void *stream);
/* objs_nms' greedy walk (pointcloud_utils.py:329-343) in the caller's `order` -- the reference's
 * np.diag(iou).argsort()[::-1], a numpy call whose tie order is numpy's own --, is_within_fov (:373-379),
 * objs2label (:347-370).  cossin_ry [host] (k,2) = numpy's (cos, sin) of every obj.ry (roty, kitti_util.py:
 * 383-389).  kept_out [host] (k) int32: indices of the boxes written, text_out: the label file's text
 * (lines joined by '\n', no trailing newline, fields %.4f).  Pure host code, no context.               */
typedef struct modest_labels_params {
    double P[12];                   /* Calibration.P (P2), row major 3x4                                 */
    int32_t nms_enable;
    float nms_threshold;
    int32_t fov_only;
    double image_h, image_w;        /* image_shape = [h, w]                                              */
} modest_labels_params;
int modest_label_lines(const double *objs8_host, const double *cossin_ry_host, int k, const int64_t *order_host,
                       const float *iou_host, const modest_labels_params *params, int32_t *kept_out_host,
                       int32_t *n_kept_out_host, char *text_out_host, int32_t text_cap, int32_t *text_len_out_host);

/* ---- host-side ingest: the `.bin` files of a group of scans, back to back into one (pinned) staging buffer -------------
 * Replaces the per-frame np.fromfile of load_velo_scan (utils/pointcloud_utils.py:22-25; one call per history frame from
 * pre_compute_pp_score.py:137-146).  paths[k]: NUL-terminated; dst [host] capacity_bytes; sizes_out [host] (n_files) = every
 * file's size in bytes (file k lands at the sum of the sizes before it); n_threads host threads share the files.
 * Returns 0 = read; a positive number = the bytes the files need when that exceeds capacity_bytes (or dst is NULL): nothing was
 * read, sizes_out is filled, call again with a larger buffer; -(k + 2) = file k could not be opened or read (errno holds the
 * cause); -1 = bad arguments.  Pure host code: no context, no stream, no device.                                              */
int64_t modest_host_read_files(const char *const *paths, int n_files, void *dst, uint64_t capacity_bytes, uint64_t *sizes_out,
                               int n_threads);

/* ---- §8f-2 combine_labels.py: filter_by_ppscore (combine_labels.py:41-60) -------
 * For each detector box the reference masks the scan's rect-frame points (offsets from the box
 * centre rotated into the box frame by `ptc_xz @ rot.T`, strict half-extent tests in x and z,
 * y in (t_y - h, t_y]) and takes numpy.percentile of the masked PP scores.
 * rect_xyz [dev] (n,3) float64 (calib.project_velo_to_rect output), pp [dev] (n,) float32.
 * boxes12 [host] (n_boxes,12) float64, the scalars numpy compares against, evaluated by the
 * caller in the box fields' own dtypes: cx, cz, rot00, rot01, rot10, rot11, -l/2, l/2, -w/2,
 * w/2, t_y - h, t_y.
 * out [host] (n_boxes,4) float64: {0: points inside, 1: a, 2: b, 3: gamma} with a, b the two
 * order statistics numpy.percentile(pp[mask], 100*quantile) interpolates between ('linear' on
 * float32 data: virtual index (n-1)*quantile = floor + gamma, all in float32).  Blocking.   */
int modest_boxes_pp_stats(modest_ctx *ctx, const double *rect_xyz_dev, int n,
                          const float *pp_dev, const double *boxes12_host, int n_boxes,
                          double quantile, double *out_host, void *stream);

/* ---- a16 closeness_rectangle angle search (pointcloud_utils.py:167-187)
 * For each cluster c (points pts_xz[offsets[c]..offsets[c+1]) , float64 (x,z)
 * pairs) and each of n_angles (cos,sin) table entries: beta = sum over points
 * of 1/max(min(Dx,Dy),d0) accumulated in numpy's pairwise order; returns the
 * index of the first strict maximum per cluster and the betas.               */
int modest_fit_boxes_closeness(modest_ctx *ctx, const double *pts_xz_dev,
                               const int32_t *offsets_host, int n_clusters,
                               const double *cossin_host, int n_angles,
                               double d0, int32_t *best_angle_host,
                               double *beta_host /* optional (C,n_angles) */,
                               void *stream);

/* The same call for cluster points in HOST memory (get_obj's callers hold them there): the points
 * travel with the offset / angle / summation-order tables in one staged copy.
 * extents_host (optional, (C,8) f64) with cossin90_host = (cos, sin) of angle + pi/2 per table
 * entry: the first half of rectangle_at_angle (pointcloud_utils.py:188-216) -- min_x, max_x,
 * min_y, max_y of pts @ [[c, s], [-s, c]]^T at the chosen heading, then the same four at
 * heading + pi/2 -- computed by the block that picked the heading (dgemm rounding: one fma per
 * element); an error is returned when a cluster is too large for that kernel (> ~90 k points). */
int modest_fit_boxes_closeness_host(modest_ctx *ctx, const double *pts_xz_host,
                                    const int32_t *offsets_host, int n_clusters,
                                    const double *cossin_host, int n_angles, double d0,
                                    int32_t *best_angle_host, const double *cossin90_host,
                                    double *extents_host, void *stream);

/* fit_method = 'variance_to_edge' (utils/pointcloud_utils.py:218-275): the same
 * angle table, criterion -var(Dx[Dx<Dy]) - var(Dy[Dy<Dx]) with numpy's var (pairwise sums of the
 * subsets in index order); returns the first strict maximum per cluster and the criteria.   */
int modest_fit_boxes_variance(modest_ctx *ctx, const double *pts_xz_dev,
                              const int32_t *offsets_host, int n_clusters,
                              const double *cossin_host, int n_angles,
                              int32_t *best_angle_host, double *crit_host, void *stream);

/* fit_method = 'PCA' (utils/pointcloud_utils.py:189-206): per cluster the two principal axes of
 * the centred (x,z) points with sklearn's sign convention (svd_flip, u_based_decision=False) and
 * the extent of the points along them.  out8 [host] (n_clusters,8) float64:
 * components row-major (4), min0, max0, min1, max1.  Agrees with sklearn to ~1e-13 relative
 * (LAPACK's SVD and the closed form differ in the last bits).                                */
int modest_fit_boxes_pca(modest_ctx *ctx, const double *pts_xz_dev, const int32_t *offsets_host,
                         int n_clusters, double *out8_host, void *stream);

/* ---- a17 get_lowest_point_rect (pointcloud_utils.py:278-290) ----------
 * For each box b = (cx, cz, l, w, cos(ry), sin(ry)) float64 [host] the max
 * rect-y over all scan points strictly inside the rotated footprint
 * ([dx dz] @ [[c,-s],[s,c]]^T as an FMA chain); -inf when no point is
 * inside (numpy raises there).  cos/sin come from the host so that the
 * host's libm, not the device's, defines them.  Blocking.                   */
int modest_lowest_point(modest_ctx *ctx, const double *pts_rect_dev, int n,
                        const double *boxes6_host, int n_boxes,
                        double *bottom_host, void *stream);

/* ---- a20 iou3d_nms_cuda (utils/iou3d_nms/src/iou3d_nms.h:9-12,
 * iou3d_cpu.h:9, bound at src/iou3d_nms_api.cpp:11-17) -------------------
 * boxes: (n,7) f32 [x,y,z,dx,dy,dz,heading], out: (n_a,n_b) f32 row-major. */
int modest_boxes_overlap_bev(const float *boxes_a_dev, int n_a,
                             const float *boxes_b_dev, int n_b,
                             float *out_dev, void *stream);
int modest_boxes_iou_bev(const float *boxes_a_dev, int n_a,
                         const float *boxes_b_dev, int n_b, float *out_dev,
                         void *stream);
/* nms_gpu / nms_normal_gpu: boxes sorted by score [dev]; keep [host] int64
 * (n); returns the number kept in *num_keep_host.  Blocking (the reference
 * also blocks on a cudaMemcpy, src/iou3d_nms.cpp:111-112).                  */
int modest_nms_bev(modest_ctx *ctx, const float *boxes_dev, int n,
                   float thresh, int64_t *keep_host, int *num_keep_host,
                   void *stream);
int modest_nms_normal(modest_ctx *ctx, const float *boxes_dev, int n,
                      float thresh, int64_t *keep_host, int *num_keep_host,
                      void *stream);
/* boxes_iou_bev_cpu (src/iou3d_cpu.cpp:232-252): host pointers in and out.
 * Runs the same kernel on the boxes staged in the context's pinned block (the
 * kernel reads them and writes the matrix there directly; there is no CPU
 * arithmetic path in this library).  Blocking.                              */
int modest_boxes_iou_bev_host(modest_ctx *ctx, const float *boxes_a_host,
                              int n_a, const float *boxes_b_host, int n_b,
                              float *out_host, void *stream);

/* ---- ground planes for detector training (data_preprocessing/RANSAC.py:9-68) -------------
 * For every frame of a batch: rect = project_velo_to_rect(rows[:, :3]) in float64 (the fma chain
 * of modest_project_velo_to_rect, bit for bit), the candidates min_h < y < max_h, -10 < z < 70,
 * -20 < x < 20 in row order (:32-38), and for n_cand >= 5 sklearn's RANSACRegressor() fitted to
 * X = rect[:, [0, 2]], y = rect[:, 1] (:44) in float64: threshold median(|y - median(y)|) (numpy
 * medians, exact), MT19937 triplets by tracking selection as sklearn consumes the generator,
 * inliers |y - pred| <= thr, the sequential accept rule with _dynamic_max_trials, the refit of the
 * consensus set (centred normal equations), and the plane (:45-52): w = (c0, -1, c1) / |.|,
 * h = b / |.|.  Fewer than 5 candidates: w = (0, -1, 0), h = 1.65 (:40-43).
 * rows_dev [dev] packed (R,4) float32 rows of all frames (16-byte aligned).
 * frames_host [host, in/out] n_frames descriptors.  key/pos are numpy's RandomState state; on
 * return they hold the generator advanced by the executed trials (untouched for a frame that is
 * not fitted here).  chain = 1 (--global_seed: one RandomState consumed in frame order by the
 * frames with >= 5 candidates): only frames_host[0].key/pos is read; frame k returns the state
 * after it; the first frame with status MODEST_GP_HOST returns the state BEFORE it, and every
 * later frame is MODEST_GP_HOST as well (the caller fits that frame and calls again on the rest).
 * Status MODEST_GP_HOST (generator untouched): 5 <= n_cand <= 300 (sklearn samples by permutation
 * below 301, utils/random.py), a degenerate triplet or consensus set, or a trial bound within 1e-7
 * of an integer (host and device libm could round it to different sides).
 * triplets_host [host, optional] (n_frames, max_trials, 3) int32: the drawn triplets.
 * gpu_ms_host [host, optional]: HIP event time of the batch's kernels.
 * Fixed launches per batch (selection + MAD, trials), one synchronise.  Blocking.               */
#define MODEST_GP_FITTED 0
#define MODEST_GP_DEFAULT 1        /* fewer than 5 candidates: the default plane */
#define MODEST_GP_HOST 2           /* handed back to the host mirror (modest_amd/utils/ransac.py) */
#define MODEST_GP_NO_CONSENSUS 3   /* sklearn raises ValueError */
typedef struct modest_gp_frame {
    int64_t row_offset;   /* first row of the frame in rows_dev */
    int32_t n;            /* rows */
    int32_t pos;          /* [in/out] RandomState.get_state()[2] */
    double v2c[12];       /* Tr_velo_to_cam, row major 3x4 */
    double r0[9];         /* R0_rect, row major 3x3 */
    uint32_t key[624];    /* [in/out] RandomState.get_state()[1] */
} modest_gp_frame;
typedef struct modest_gp_params {
    double min_h, max_h;       /* strict window on rect y */
    double stop_probability;   /* 0.99 */
    int32_t max_trials;        /* 100 (at most 4096) */
    int32_t chain;             /* 0: every frame its own generator; 1: one generator across the frames */
} modest_gp_params;
typedef struct modest_gp_result {
    double plane[4];           /* w0, w1, w2, h */
    double median, mad;        /* median(y), residual threshold (n_cand > 300) */
    int32_t n_cand, n_trials, n_inliers, status;
} modest_gp_result;
int modest_ground_planes(modest_ctx *ctx, const float *rows_dev, modest_gp_frame *frames_host, int n_frames,
                         const modest_gp_params *params_host, modest_gp_result *results_host,
                         int32_t *triplets_host, float *gpu_ms_host, void *stream);

/* ---- KITTI-style AP evaluation (kitti_object_eval_python/eval.py; csrc/kitti_eval.hip) ----
 * A set of frames, each with nd detections and ng ground-truth boxes.  Boxes are float64 camera boxes
 * (x, y, z, l, h, w, ry) in rows of 7, image boxes rows of 4; frame f's dt x gt block of overlaps is stored dt-major
 * at pair_off (overlaps[j, i] of eval.py). */
typedef struct {
    int64_t dt_off, gt_off, pair_off;   /* first detection / gt box / pair of the frame in the set */
    int32_t nd, ng;
} modest_eval_frame;

/* One configuration: a row of the ignore-flag tables (class x difficulty or range bucket) and a min overlap. */
typedef struct {
    int32_t flagset, pad;
    double min_overlap;
    int64_t num_valid_gt;               /* gt boxes with ignored_gt == 0 in this row (get_thresholds' num_gt) */
} modest_eval_config;

/* Device pointers of one statistics run (one metric, n_cfg configurations). */
typedef struct {
    const modest_eval_frame *frames;    /* [n_frames] */
    const modest_eval_config *cfg;      /* [n_cfg] */
    const double *dt_score;             /* [n_dt] */
    const double *dt_bbox, *gt_bbox;    /* [n][4] image boxes: metric 0 (DontCare pass) */
    const int8_t *gt_ign, *dt_ign;      /* [flagsets][n_gt] ignored_gt, [flagsets][n_dt] ignored_det (-1 / 0 / 1) */
    const uint8_t *gt_dc;               /* [flagsets][n_gt] DontCare boxes of the row, or NULL */
    const double *pair_sim;             /* (1 + cos(gt alpha - dt alpha)) / 2 per pair (aos, metric 0), or NULL */
    double *tp_scores;                  /* [n_cfg][n_gt] pass A: score of the detection matched to each tp gt
                                           (other slots keep the caller's fill value) */
    int32_t *tp_count;                  /* [n_cfg] pass A: tp count (zeroed by the caller) */
    double *thresholds;                 /* [n_cfg][64] */
    int32_t *n_thresh;                  /* [n_cfg]: threshold count, negative when more than 64 */
    int32_t *partial;                   /* [n_cfg][64][n_frames][4] pass B: tp, fp, fn per frame */
    double *sim_partial;                /* [n_cfg][64][n_frames] pass B similarity per frame (NaN: none), or NULL */
    int64_t n_gt, n_dt;
    int32_t n_frames, n_cfg, metric, max_nd;   /* max_nd: the largest nd (sizes the LDS bitmaps) */
} modest_eval_stats_args;

/* limits: thresholds per configuration, detections per frame */
int modest_eval_limits(int32_t *max_thresholds, int32_t *max_dt_per_frame);

/* Overlaps of pairs [pair_base, pair_base + n_pairs) of the set (outputs indexed from 0).  bev_out: devRotateIoUEval
 * (query = gt, box = dt) under crit_bev (-1 IoU, 0 / 1 over the gt / dt area, 2 area); d3_out: d3_box_overlap_kernel
 * under crit_3d; img_out: image_box_overlap under crit_img.  Any output may be NULL.  Enqueue only. */
int modest_eval_overlaps(const modest_eval_frame *frames_dev, int n_frames, int64_t pair_base, int64_t n_pairs,
                         const double *dt_boxes, const double *gt_boxes, const double *dt_bbox, const double *gt_bbox,
                         int crit_bev, int crit_3d, int crit_img, float *bev_out, float *d3_out, double *img_out,
                         void *stream);

/* compute_statistics_jit / get_thresholds / fused_compute_statistics, enqueue only.  stage 0: pass A over frames
 * [frame_begin, frame_end) whose overlaps (float32, or float64 if overlaps_f64) start at pair pair_base; stage 1:
 * thresholds from `sorted` (each row of tp_scores in descending order); stage 2: pass B over a frame range;
 * stage 3: pr_out[n_cfg][64][4] = tp, fp, fn, similarity summed over all frames. */
int modest_eval_statistics(int stage, const modest_eval_stats_args *args, int frame_begin, int frame_end,
                           const void *overlaps, int overlaps_f64, int64_t pair_base, const double *sorted,
                           double *pr_out, void *stream);

/* ---- dataset infos + ground-truth database (OpenPCDet create_kitti_infos) ----------------
 * csrc/kitti_infos.hip.  A batch of frames lies back to back in rows_dev as raw (n,4) float32 rows.
 * Per box the calls return
 *   hull_count   the rows inside the camera's field of view (all rows when fov_only = 0) that the float64
 *                box test decides inside: num_points_in_gt of kitti_dataset.py:239-251 up to the undecided
 *                rows (|margin| < tau), whose frame-local row numbers come back in und_idx (und_cap per box;
 *                und_n counts all of them, und_n > und_cap means the list overflowed) for the host's Delaunay;
 *   db_count     the members under check_pt_in_box3d_cpu (roiaware_pool3d.cpp:128-143, bit for bit) and, from
 *                modest_infos_gather, those rows in file order with the float64 centre subtracted and rounded
 *                once (kitti_dataset.py:290-292), box after box at box_base[box].
 * The FOV flag is kitti_dataset.py:158-173 + calibration_kitti.py:64-84 in float32 (see the .hip header).
 * Both calls only enqueue on `stream`; every buffer is the caller's.  frames / boxes are host tables (copied
 * into tables_dev, modest_infos_table_bytes, 256-byte aligned); wcount_dev holds the per-chunk counts between
 * the two calls (sum over frames of ceil(n / modest_infos_chunk_rows()) * box_count words).  A frame's boxes
 * are processed in passes of pass_boxes <= MODEST_INFOS_MAX_PASS that share LDS.                      */
#define MODEST_INFOS_MAX_PASS 256
typedef struct modest_infos_frame {
    int64_t row_offset;   /* first row of the frame in rows_dev */
    int64_t cnt_offset;   /* first word of the frame in wcount_dev: running sum of chunks * box_count */
    int32_t n;            /* rows */
    int32_t box_begin;    /* first box of the frame in the box table (frames in order, no gaps) */
    int32_t box_count;
    int32_t height, width;   /* image_shape */
    int32_t fov_only;     /* FOV_POINTS_ONLY: hull_count over the rows with the FOV flag only */
    int32_t pad[2];
    float m1[12];         /* V2C.T @ R0.T (float32 product of numpy), row major 4x3 */
    float p2t[12];        /* P2.T, row major 4x3 */
} modest_infos_frame;
typedef struct modest_infos_box {
    double b[7];          /* gt_boxes_lidar: x y z dx dy dz heading (float64) */
    double cs[2];         /* cos(heading), sin(heading) in float64 */
    double tau;           /* half width of the undecided band of the hull test, metres */
    float bf[7];          /* the same seven rounded to float32 (what points_in_boxes_cpu receives) */
    float cosa, sina;     /* the HOST libm's cosf(-bf[6]) / sinf(-bf[6]), the symbols the reference's host code binds to */
    float reject;         /* max(|x-cx|, |y-cy|) above this: neither a member nor undecided */
    float pad[2];
} modest_infos_box;
int modest_infos_chunk_rows(void);
int64_t modest_infos_table_bytes(int n_frames, int n_boxes);
/* fov_dev (optional): one byte per row of rows_dev, the FOV flag.  dense_dev (optional, zeroed by the caller):
 * (n_boxes, dense_stride) int32, 1 where the database predicate holds (points_in_boxes_cpu's dense mask). */
int modest_infos_count(const float *rows_dev, int64_t n_rows, const modest_infos_frame *frames_host, int n_frames,
                       const modest_infos_box *boxes_host, int n_boxes, int pass_boxes, int und_cap,
                       void *tables_dev, int64_t tables_bytes, int32_t *wcount_dev, int64_t wcount_words,
                       int32_t *hull_count_dev, int32_t *und_n_dev, int32_t *und_idx_dev, int32_t *db_count_dev,
                       uint8_t *fov_dev, int32_t *dense_dev, int64_t dense_stride, void *stream);
/* after modest_infos_count on the same tables_dev / wcount_dev and a read-back of db_count: box_base is the exclusive
 * sum of db_count over the batch's boxes (host copy for the bounds check, device copy for the kernel). */
int modest_infos_gather(const float *rows_dev, int64_t n_rows, const modest_infos_frame *frames_host, int n_frames,
                        int n_boxes, int pass_boxes, const void *tables_dev, const int32_t *wcount_dev,
                        int64_t wcount_words, const int64_t *box_base_dev, const int32_t *db_count_host,
                        const int64_t *box_base_host, float *out_rows_dev, int64_t out_rows, void *stream);

/* ---- a22 pointnet2_batch_cuda (pcdet/ops/pointnet2/pointnet2_batch/src/, bound at pointnet2_api.cpp:10-24) --------
 * The nine launchers of the PointNet++ set-abstraction ops.  Every buffer [dev], float32 / int32, contiguous; enqueue
 * only, no context.  Element offsets are 64-bit (the reference's int products overflow past 2^31 elements).  The
 * arithmetic, the order of hits and the tie rules are the contract of DESIGN.md section 7d.  An index outside its row
 * reads as 0 (forward) or is skipped (gradients); the reference reads or writes out of bounds.
 *
 * sampling_gpu.cu:100-216 furthest_point_sampling_kernel_launcher.  xyz (b,n,3), temp (b,n) (the caller fills it,
 * 1e10 in the reference; values >= 0), idx (b,m).  idx[0] = 0; ties at the maximum of temp go to the point the
 * reference's reduction tree picks (bs = min(1024, 2^floor(log2 n)): smallest bitreverse(k mod bs), then smallest k).
 * On return temp holds the running minimum distances after m - 1 rounds; m = 1 writes idx[0] only.  n >= 1.        */
int modest_pn2_furthest_point_sample(int b, int n, int m, const float *xyz_dev, float *temp_dev, int32_t *idx_dev,
                                     void *stream);
/* sampling_gpu.cu:15-31 gather_points_kernel_launcher_fast: points (b,c,n), idx (b,m) -> out (b,c,m).              */
int modest_pn2_gather(int b, int c, int n, int m, const float *points_dev, const int32_t *idx_dev, float *out_dev,
                      void *stream);
/* sampling_gpu.cu:53-70 gather_points_grad_kernel_launcher_fast: grad_out (b,c,m), idx (b,m); ADDS into
 * grad_points (b,c,n) (the caller zero-fills, as the reference's Python side does).                                */
int modest_pn2_gather_grad(int b, int c, int n, int m, const float *grad_out_dev, const int32_t *idx_dev,
                           float *grad_points_dev, void *stream);
/* ball_query_gpu.cu:15-51 ball_query_kernel_launcher_fast: new_xyz (b,m,3), xyz (b,n,3) -> idx (b,m,nsample): the
 * first nsample points with d2 < radius*radius (float32 product) in index order, short rows padded with the first
 * hit, rows without a hit untouched (the caller zero-fills).                                                       */
int modest_pn2_ball_query(int b, int n, int m, float radius, int nsample, const float *new_xyz_dev,
                          const float *xyz_dev, int32_t *idx_dev, void *stream);
/* group_points_gpu.cu:53-72 group_points_kernel_launcher_fast: points (b,c,n), idx (b,npoints,nsample) ->
 * out (b,c,npoints,nsample).                                                                                       */
int modest_pn2_group(int b, int c, int n, int npoints, int nsample, const float *points_dev, const int32_t *idx_dev,
                     float *out_dev, void *stream);
/* group_points_gpu.cu:14-31 group_points_grad_kernel_launcher_fast: grad_out (b,c,npoints,nsample); ADDS into
 * grad_points (b,c,n).                                                                                             */
int modest_pn2_group_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out_dev,
                          const int32_t *idx_dev, float *grad_points_dev, void *stream);
/* interpolate_gpu.cu:16-59 three_nn_kernel_launcher_fast: unknown (b,n,3), known (b,m,3) -> dist2 (b,n,3) SQUARED
 * distances ascending, idx (b,n,3); equal distances keep the lower index first; with m < 3 the unused slots hold
 * inf / 0.                                                                                                         */
int modest_pn2_three_nn(int b, int n, int m, const float *unknown_dev, const float *known_dev, float *dist2_dev,
                        int32_t *idx_dev, void *stream);
/* interpolate_gpu.cu:84-104 three_interpolate_kernel_launcher_fast: points (b,c,m), idx / weight (b,n,3) ->
 * out (b,c,n) = (w0*p0 + w1*p1) + w2*p2.                                                                           */
int modest_pn2_three_interpolate(int b, int c, int m, int n, const float *points_dev, const int32_t *idx_dev,
                                 const float *weight_dev, float *out_dev, void *stream);
/* interpolate_gpu.cu:127-149 three_interpolate_grad_kernel_launcher_fast: grad_out (b,c,n), idx / weight (b,n,3);
 * ADDS grad_out * weight into grad_points (b,c,m).                                                                 */
int modest_pn2_three_interpolate_grad(int b, int c, int n, int m, const float *grad_out_dev, const int32_t *idx_dev,
                                      const float *weight_dev, float *grad_points_dev, void *stream);

/* ---- a23 roipoint_pool3d_cuda.forward and roiaware_pool3d_cuda.points_in_boxes_gpu -------------------------------
 * The two box-membership ops of PointRCNN.  Every buffer [dev], float32 / int32, contiguous; enqueue only, no context,
 * no device allocation, no synchronise.  Element offsets are 64-bit.  Both use one predicate (check_pt_in_box3d,
 * roipoint_pool3d_kernel.cu:22-35 = roiaware_pool3d_kernel.cu:23-36); its arithmetic is the contract of DESIGN.md
 * section 7e: float32 differences, products and sums without contraction, cos / sin of -rz as the rounded double
 * functions, the three comparisons decided exactly as the reference's double expressions.
 *
 * roipoint_pool3d_kernel.cu:38-165 roipool3dLauncher.  xyz (b,n,3), boxes (b,m,7) [cx,cy,cz,dx,dy,dz,rz],
 * feat (b,n,c), pooled (b,m,s,3+c), empty_flag (b,m).  Per box the first s inside points in index order; with
 * 0 < cnt < s slot k >= cnt repeats slot k % cnt; a row is xyz[idx] followed by feat[idx], bit for bit.  cnt == 0 sets
 * the box's flag to 1 and leaves its rows as given; a box with an inside point keeps its flag, and its rows are written
 * only if that flag is 0 (the caller zero-fills both, as the reference's Python side does).  No (n, m) intermediate.
 * c == 0 is legal; b == 0 or m == 0 writes nothing; n == 0 or s == 0 sets every flag to 1.  s <= 15360.            */
int modest_roipoint_pool3d(int b, int n, int m, int c, int s, const float *xyz_dev, const float *boxes_dev,
                           const float *feat_dev, float *pooled_dev, int32_t *empty_flag_dev, void *stream);
/* roiaware_pool3d_kernel.cu:313-355 points_in_boxes_launcher.  boxes (b,m,7), pts (b,n,3) -> box_idx (b,n): the lowest
 * index of a box that contains the point; a point in no box is left as given (the caller fills -1).  An all-zero
 * (padding) box contains a point with z == 0 within 1e-5 of the origin in x and y.  Any size 0 writes nothing.      */
int modest_points_in_boxes(int b, int m, int n, const float *boxes_dev, const float *pts_dev, int32_t *box_idx_dev,
                           void *stream);

/* ---- a24 point-to-voxel grouping for PointPillars (spconv.utils.VoxelGenerator) ---------------
 * spconv 1.2's hard voxelisation, first come first served.  lo3 / vs3: the lower corner of the point cloud range and the
 * voxel size as float32, grid3 = [nx, ny, nz] (round((hi - lo) / vs) in float32, the caller's), at most 2^31 - 1 cells.
 * Point i lies in cell c_j = floorf((p_j - lo_j) / vs_j) (float32, a correctly rounded division) and is dropped unless
 * 0 <= c_j < (float)grid_j on all three axes (tested on the float: NaN and +-inf are dropped, -0.0 is cell 0).  Points
 * are walked in order; a cell that no earlier point opened becomes the next voxel unless max_voxels are open (the point
 * is dropped, the walk goes on); a point takes its voxel's next slot unless max_num_points are taken.
 *
 * Host path, one cloud: points [host] (n, c) float32, c >= 3, xyz first.  table [host] (cells) int32, all -1 on entry
 * and again on return (the caller allocates it once per generator).  Outputs [host], capacity max_voxels rows, may be
 * uninitialised: voxels (V, P, c) rows as raw words and +0.0 in unused slots, coords (V, 3) [z, y, x], num_points (V),
 * point_mask (V, P) the index of the point in each slot or -1.  Returns V, or a negative error.  No HIP call.         */
int64_t modest_voxelize_host(const float *points_host, int64_t n, int c, const float *lo3, const float *vs3,
                             const int32_t *grid3, int max_num_points, int max_voxels, int32_t *table_host,
                             float *voxels_host, int32_t *coords_host, int32_t *num_points_host, int32_t *point_mask_host);
/* Device path, a collated batch: points [dev] (n_rows, 1 + c) float32 with the batch index in column 0, integers in
 * [0, batch_cap) in non-decreasing order (anything else is found on the device and fails the plan call); max_voxels
 * applies per cloud.  Scratch is the caller's: workspace [dev], 256-byte aligned, modest_voxelize_workspace_bytes bytes
 * -- a function of n_rows and batch_cap only (grid3 is checked, a grid of more than 2^31 - 1 cells returns -1).  No
 * device allocation, no context; nothing depends on the order in which atomics land.
 * plan: enqueues everything up to the voxel counts and synchronises the stream ONCE.  counts [PINNED host]
 * (4 + batch_cap) int32, written by the last kernel itself: [0] error bits, [1] clouds seen (last batch index + 1),
 * [2] cells opened in the batch, [3] sum of V_b, [4 + b] V_b = min(cells of cloud b, max_voxels).
 * fill: enqueue only, on the same stream and workspace, same arguments, cells_opened = counts[2] and total_voxels =
 * counts[3].  Writes EVERY element of voxels (total, P, c), coords (total, 4) [b, z, y, x], num_points (total) and
 * point_mask (total, P) (row indices into points); clouds in batch order, voxels in the order they were opened.     */
int64_t modest_voxelize_workspace_bytes(int64_t n_rows, int batch_cap, const int32_t *grid3_host);
int modest_voxelize_plan(const float *points_dev, int64_t n_rows, int c, int batch_cap, const float *lo3_host,
                         const float *vs3_host, const int32_t *grid3_host, int max_num_points, int max_voxels,
                         void *workspace_dev, int64_t workspace_bytes, int32_t *counts_pinned_host, void *stream);
int modest_voxelize_fill(const float *points_dev, int64_t n_rows, int c, int batch_cap, const int32_t *grid3_host,
                         int max_num_points, int max_voxels, const void *workspace_dev, int64_t workspace_bytes,
                         int32_t cells_opened, int64_t total_voxels, float *voxels_dev, int32_t *coords_dev,
                         int32_t *num_points_dev, int32_t *point_mask_dev, void *stream);

/* ---- a25 sparse 3-D convolutions for SECOND (spconv 1.2's SubMConv3d / SparseConv3d) -----------
 * indices [dev] (n_in, 4) int32 [b, z, y, x], unique rows inside batch_size x shape3 = [D, H, W]; kernel3 / stride3 / pad3
 * in the same axis order, kernel sizes 1 .. 7.  subm != 0: odd kernels, stride and padding ignored, the output sites are
 * the input sites in input order.  Otherwise out_j = (in_j + 2 p_j - k_j) / s_j + 1 and output site o exists iff some
 * input i and offset k satisfy i = o * s - p + k; output rows ascend in (b, z, y, x).  Offset k = (kz * ky + ky_i) * kx + kx_i.
 * Sites are 64-bit keys: batch_size * D * H * W may exceed 2^32 (at most 2^56), no table over the grid is allocated.
 * Scratch is the caller's: workspace [dev], 256-byte aligned, modest_spconv_rulebook_workspace_bytes(n_in, kernel volume,
 * subm) bytes.  No device allocation, no context, nothing depends on the order in which atomics land.
 * plan: enqueues the sorts and synchronises the stream ONCE.  counts [PINNED host] 2 int32, written by the last kernel:
 * [0] error bits, [1] N_out.  A row outside the shape or a duplicate row fails the call (-1) and nothing is produced.
 * fill: enqueue only, same stream, workspace and arguments, n_out = counts[1].  Writes every element of out_indices
 * (n_out, 4) (not touched when subm), nbr (kvol, n_out): the input row of output o at offset k or -1, and nbr_t
 * (kvol, n_in): the output row that reads input i at offset k or -1.                                                   */
int64_t modest_spconv_rulebook_workspace_bytes(int64_t n_in, int kvol, int subm);
int modest_spconv_rulebook_plan(const int32_t *indices_dev, int64_t n_in, int batch_size, const int32_t *shape3_host,
                                const int32_t *kernel3_host, const int32_t *stride3_host, const int32_t *pad3_host, int subm,
                                void *workspace_dev, int64_t workspace_bytes, int32_t *counts_pinned_host, void *stream);
int modest_spconv_rulebook_fill(const int32_t *indices_dev, int64_t n_in, int batch_size, const int32_t *shape3_host,
                                const int32_t *kernel3_host, const int32_t *stride3_host, const int32_t *pad3_host, int subm,
                                const void *workspace_dev, int64_t workspace_bytes, int64_t n_out, int32_t *out_indices_dev,
                                int32_t *nbr_dev, int32_t *nbr_t_dev, void *stream);
/* out[r][n] = (((+0 + in[map[0][r]][0] * W_0[0][n]) + in[map[0][r]][1] * W_0[1][n]) + ...) over k ascending (rows with
 * map[k][r] < 0 skipped), m ascending; product and sum rounded separately in float32, no fused multiply-add; then
 * + bias[n] when bias is not NULL.  weight [dev] (kvol, w_cin, w_cout).  transposed == 0 (forward): in (n_in, w_cin),
 * map = nbr, W_k[m][n] = weight[k][m][n], out (n_out, w_cout).  transposed != 0 (feature gradient): in = dy (n_in, w_cout),
 * map = nbr_t, W_k[m][n] = weight[k][n][m], out (n_out, w_cin).  Channels 1 .. 128.  Writes every element of out; enqueue only. */
int modest_spconv_gather_gemm(const float *in_dev, int64_t n_in, int in_channels, const float *weight_dev, int kvol, int w_cin,
                              int w_cout, int transposed, const float *bias_dev, const int32_t *map_dev, int64_t n_out,
                              float *out_dev, void *stream);
/* dweight[k][ci][co] = sum over output rows o of x[nbr[k][o]][ci] * dy[o][co], dbias[co] = sum of dy[o][co] (dbias may be
 * NULL).  The rows are cut into min(32, ceil(n_out / 1024)) segments, summed in ascending row order inside a segment and
 * in ascending segment order after: the same bits on every run, no float atomics.  workspace [dev] 256-byte aligned,
 * modest_spconv_wgrad_workspace_bytes bytes.  Enqueue only.                                                            */
int64_t modest_spconv_wgrad_workspace_bytes(int64_t n_out, int kvol, int c_in, int c_out);
int modest_spconv_wgrad(const float *x_dev, int64_t n_in, int c_in, const float *dy_dev, int64_t n_out, int c_out,
                        const int32_t *nbr_dev, int kvol, void *workspace_dev, int64_t workspace_bytes, float *dweight_dev,
                        float *dbias_dev, void *stream);

/* ---- a26 pointnet2_stack_cuda (pcdet/ops/pointnet2/pointnet2_stack/src/, bound at pointnet2_api.cpp) ----
 * The stacked-batch PointNet++ ops of PV-RCNN and Voxel R-CNN.  All scans of a batch are rows of one (N1 + N2 + ..., C)
 * tensor; a *_batch_cnt buffer is [dev] int32 (b,), read on the device only: no call copies a count to the host or
 * synchronises.  Row p belongs to the first scan s with p < cnt[0] + ... + cnt[s], rows past the total to scan b - 1,
 * negative counts count as 0; the other tensor's rows of that scan are [start_s, start_s + cnt_s), clipped to its real
 * row count, which every entry point receives.  Every buffer [dev], float32 / int32, contiguous; enqueue only, no context,
 * 64-bit element offsets.  Furthest point sampling is modest_pn2_furthest_point_sample (the same kernel text).
 *
 * ball_query_gpu.cu ball_query_kernel_stack: new_xyz (m,3), xyz (n,3) -> idx (m,nsample): the first nsample rows of the
 * centre's scan with ((cx-x)^2 + (cy-y)^2) + (cz-z)^2 < radius*radius (float32 product, strict) in index order as
 * scan-local indices, short rows padded with the first hit; a row without a hit gets idx[0] = -1 and is otherwise left
 * as given.                                                                                                          */
int modest_pn2s_ball_query(int b, int m, float radius, int nsample, const float *new_xyz_dev,
                           const int32_t *new_xyz_batch_cnt_dev, const float *xyz_dev, const int32_t *xyz_batch_cnt_dev,
                           int n, int32_t *idx_dev, void *stream);
/* voxel_query_gpu.cu voxel_query_kernel_stack: new_xyz (m,3), xyz (n,3), new_coords (m,4) [batch, z, y, x],
 * point_indices (b,r1,r2,r3): the row of xyz held by a cell or a negative value.  Cells are visited in dz, dy, dx order
 * over [-range, +range] per axis; coordinates outside the grid, negative entries, entries >= n and a batch index outside
 * [0, b) are skipped; a cell is rejected only if d2 > radius*radius.  idx (m,nsample): the first nsample accepted rows of
 * xyz (global), padded with the first; an empty row gets idx[0] = -1.  At most 2^31 - 1 cells per query inside the grid. */
int modest_pn2s_voxel_query(int b, int m, int r1, int r2, int r3, int nsample, float radius, int z_range, int y_range,
                            int x_range, const float *new_xyz_dev, const float *xyz_dev, int n,
                            const int32_t *new_coords_dev, const int32_t *point_indices_dev, int32_t *idx_dev,
                            void *stream);
/* interpolate_gpu.cu three_nn_kernel_stack: unknown (n,3), known (m,3) -> dist2 (n,3) SQUARED distances ascending,
 * idx (n,3) GLOBAL rows of known (start_s + k); the three smallest (distance, index) pairs within the row's scan; unused
 * slots hold inf / start_s.                                                                                          */
int modest_pn2s_three_nn(int b, int n, int m, const float *unknown_dev, const int32_t *unknown_batch_cnt_dev,
                         const float *known_dev, const int32_t *known_batch_cnt_dev, float *dist2_dev, int32_t *idx_dev,
                         void *stream);
/* group_points_gpu.cu group_points_kernel_stack: features (n,c), idx (m,nsample) scan-local -> out (m,c,nsample);
 * an index outside [0, cnt_s) of the row's scan reads as 0.                                                           */
int modest_pn2s_group(int b, int m, int c, int nsample, int n, const float *features_dev,
                      const int32_t *features_batch_cnt_dev, const int32_t *idx_dev, const int32_t *idx_batch_cnt_dev,
                      float *out_dev, void *stream);
/* group_points_gpu.cu group_points_grad_kernel_stack: grad_out (m,c,nsample); ADDS into grad_features (n,c) (float
 * atomics, any order); an index outside its range is skipped, an element no term reaches is not written.             */
int modest_pn2s_group_grad(int b, int m, int c, int n, int nsample, const float *grad_out_dev, const int32_t *idx_dev,
                           const int32_t *idx_batch_cnt_dev, const int32_t *features_batch_cnt_dev,
                           float *grad_features_dev, void *stream);
/* interpolate_gpu.cu three_interpolate_kernel_stack: features (m,c), idx / weight (n,3) global rows ->
 * out (n,c) = (w0*f0 + w1*f1) + w2*f2; an index outside [0, m) reads as 0.                                            */
int modest_pn2s_three_interpolate(int n, int c, int m, const float *features_dev, const int32_t *idx_dev,
                                  const float *weight_dev, float *out_dev, void *stream);
/* interpolate_gpu.cu three_interpolate_grad_kernel_stack: grad_out (n,c); ADDS grad_out * weight into
 * grad_features (m,c) (float atomics, any order); an index outside [0, m) is skipped.                                 */
int modest_pn2s_three_interpolate_grad(int n, int c, int m, const float *grad_out_dev, const int32_t *idx_dev,
                                       const float *weight_dev, float *grad_features_dev, void *stream);

/* ---- a27 anchor target assignment (AxisAlignedTargetAssigner.assign_targets of OpenPCDet's anchor heads) ----
 * POS_FRACTION < 0, MATCH_HEIGHT and NORM_BY_NUM_EXAMPLES off.  A whole batch, all anchor classes, in one call: enqueue
 * only, no context, no device allocation, no synchronise, nothing read back; the (anchors, gts) IoU matrix is never stored.
 * Every buffer [dev].
 *   gt       (b, m, gt_cols) float32 with the three strides given in elements: 7 + Cg box values and the class id;
 *   anchors  (sum of rows, a_cols = 7 + Ca) float32, contiguous, the classes' blocks one after the other;
 *   cls      (n_cls, 5) int64: first row, rows, k, stride, offset -- row i of the class goes to output row
 *            (i / k) * stride + offset + i % k of its sample (k >= 1; the map over all classes is one to one onto [0, n_out));
 *   thr      (n_cls, 2) float32 matched, unmatched;
 *   match    (n_cls, n_names) uint8: 1 where class_names[n] is the anchor class's name.  Class id c names entry c - 1,
 *            id <= 0 wraps once as Python does; an id outside belongs to no class;
 *   max_cls_rows  the largest number of rows of a class (sizes the grid).
 * Outputs, every element written: labels int32 (b, n_out), targets float32 (b, n_out, 7 + sincos + min(Ca, Cg)),
 * weights float32 (b, n_out).  workspace 4-byte aligned, modest_anchor_targets_workspace_bytes(b, n_cls, m) bytes, need
 * not be initialised.  The column maxima are merged with integer atomicMax on float bits: no result depends on order. */
int64_t modest_anchor_targets_workspace_bytes(int b, int n_cls, int m);
int modest_anchor_targets(int b, int m, int gt_cols, const float *gt_dev, int64_t gt_stride_b, int64_t gt_stride_m,
                          int64_t gt_stride_c, const float *anchors_dev, int a_cols, int n_cls, const int64_t *cls_dev,
                          const float *thr_dev, const uint8_t *match_dev, int n_names, int64_t max_cls_rows, int sincos,
                          int64_t n_out, int32_t *labels_dev, float *targets_dev, float *weights_dev, void *workspace_dev,
                          int64_t workspace_bytes, void *stream);

/* ---- a28 roiaware_pool3d_cuda.forward / backward: the RoI-aware voxel pooling of PartA2 ---------
 * Every buffer [dev], float32 / int32, contiguous; enqueue only, no context, no device allocation, no synchronise.
 * Element offsets are 64-bit.  rois (boxes_num,7) [cx,cy,cz,dx,dy,dz,rz], pts (pts_num,3), pts_feature (pts_num,channels),
 * argmax and pooled_features (boxes_num,out_x,out_y,out_z,channels), pts_idx_of_voxels (boxes_num,out_x,out_y,out_z,
 * max_pts_each_voxel).  pool_method 0 = max, 1 = avg, anything else is an error.  out_x, out_y, out_z in 1..256 (the
 * reference packs each index into 8 bits) and out_x * out_y * out_z <= 13824 in the forward (one LDS counter per voxel):
 * a larger grid fails the call and launches nothing.  max_pts_each_voxel >= 1 (1: every list stays empty).
 *
 * roiaware_pool3d_kernel.cu:39-233 roiaware_pool3d_launcher.  A point inside a box by the predicate of a23 falls into the
 * voxel index = min(max((unsigned)(int)q, 0), out - 1), q = (l + d / 2.0f) / (d / (float)out) in float32 with correctly
 * rounded divisions, per axis (lx, ly of the predicate, lz = z - cz): NaN -> 0, q <= -1 -> out - 1, q >= out -> out - 1,
 * otherwise truncation toward zero.  Word 0 of a voxel's list is its count, capped at max_pts_each_voxel - 1, and is
 * WRITTEN whatever it held (the reference increments the given word: its caller zero-fills); words 1..count are the
 * voxel's points in ascending index, later ones are dropped; words beyond count are left as given.  No (boxes, points)
 * intermediate.  max: the list is walked in slot order, a value wins if it is > the best so far, from -inf (first of
 * equal maxima; -inf and NaN never win); argmax is written for every element (-1 for none), pooled_features only where
 * argmax != -1.  avg: the float32 sum in slot order from +0 divided by (float)count, written only where count > 0; argmax
 * is not touched.  channels == 0, boxes_num == 0 and pts_num == 0 are legal (no points: every count is written as 0).
 *
 * roiaware_pool3d_kernel.cu:236-310 roiaware_pool3d_backward_launcher.  ADDS into grad_in (pts_num,channels) (the caller
 * zero-fills, as the reference's Python side does): avg grad_out[b][v][c] * (1.0f / fmaxf((float)count, 1.0f)) to every
 * point of the voxel's list, max grad_out[b][v][c] to point argmax[b][v][c].  The sum for one (point, channel) runs over
 * the boxes in ascending index without float atomics, so its bits do not change from run to run (the reference's
 * atomicAdd order does).  pts_idx_of_voxels and argmax must come from one forward call; an argmax entry that names a
 * point outside that voxel's list contributes nothing, list entries outside [0, pts_num) are ignored.  workspace:
 * modest_roiaware_pool3d_backward_workspace_bytes(boxes_num, pts_num) bytes (a (pts_num, boxes_num) int32 table), 4-byte
 * aligned, need not be initialised.  Any size 0 writes nothing.                                                       */
int modest_roiaware_pool3d_forward(int boxes_num, int pts_num, int channels, int max_pts_each_voxel, int out_x, int out_y,
                                   int out_z, const float *rois_dev, const float *pts_dev, const float *pts_feature_dev,
                                   int32_t *argmax_dev, int32_t *pts_idx_of_voxels_dev, float *pooled_features_dev,
                                   int pool_method, void *stream);
int64_t modest_roiaware_pool3d_backward_workspace_bytes(int boxes_num, int pts_num);
int modest_roiaware_pool3d_backward(int boxes_num, int pts_num, int out_x, int out_y, int out_z, int channels,
                                    int max_pts_each_voxel, const int32_t *pts_idx_of_voxels_dev, const int32_t *argmax_dev,
                                    const float *grad_out_dev, float *grad_in_dev, int pool_method, void *workspace_dev,
                                    int64_t workspace_bytes, void *stream);

/* ---- a29 inverse sparse 3-D convolution (spconv 1.2's SparseInverseConv3d) ----------------------
 * An inverse convolution runs a strided convolution's rulebook backwards: its output rows are that convolution's input
 * sites, out[i] = sum over k ascending with nbr_t[k][i] >= 0, ci ascending, of x[nbr_t[k][i]][ci] * weight[k][ci][co].
 * That is modest_spconv_gather_gemm on nbr_t; the two entry points below do the same sum on tiles of one class.
 * The class of row i = [b, z, y, x] is ((z + p_z) % s_z * s_y + (y + p_y) % s_y) * s_x + (x + p_x) % s_x, one of
 * s_z s_y s_x classes (strides 1 .. 64): the row can only be read at offsets with k_j == residue_j (mod s_j).
 * class_order: perm [dev] (n_rows,) int32 = the rows stably ordered by class (numpy's argsort(class, kind="stable")),
 * class_start [dev] (classes + 1,) int32 = the exclusive counts, class_start[classes] = n_rows.  workspace [dev],
 * 256-byte aligned, modest_spconv_class_order_workspace_bytes bytes, a function of n_rows alone.  Enqueue only: no
 * synchronise, no count travels to the host, nothing depends on the order in which atomics land.                        */
int64_t modest_spconv_class_order_workspace_bytes(int64_t n_rows, int n_classes);
int modest_spconv_class_order(const int32_t *indices_dev, int64_t n_rows, const int32_t *stride3_host,
                              const int32_t *pad3_host, void *workspace_dev, int64_t workspace_bytes, int32_t *perm_dev,
                              int32_t *class_start_dev, void *stream);
/* in (n_in, in_channels), weight (kernel volume, in_channels, w_cout), map = nbr_t (kernel volume, n_out), perm and
 * class_start as class_order wrote them for the same rows and strides, at most 64 classes -> out (n_out, w_cout), every
 * element written exactly once (a row that nothing reads gets +0.0, or the bias).  A workgroup owns 64 consecutive
 * entries of perm inside one class and visits only that class's offsets, ascending; the grid is n_out / 64 + classes,
 * the surplus workgroups exit at once.  Bit for bit what modest_spconv_gather_gemm(transposed = 0) writes for the same
 * map.  Channels 1 .. 128, kernel sizes 1 .. 7.  Enqueue only.                                                          */
int modest_spconv_gather_gemm_classes(const float *in_dev, int64_t n_in, int in_channels, const float *weight_dev,
                                      const int32_t *kernel3_host, const int32_t *stride3_host, int w_cout,
                                      const float *bias_dev, const int32_t *map_dev, int64_t n_out, const int32_t *perm_dev,
                                      const int32_t *class_start_dev, float *out_dev, void *stream);

/* ---- a30 point-head target assignment (PointHeadTemplate.assign_stack_targets of OpenPCDet's point heads) ----
 * set_ignore_flag=True, use_ball_constraint=False.  A whole stacked batch in one call: enqueue only, no context, no
 * device allocation, no workspace, no atomics, no synchronise, nothing read back.  Every buffer [dev].
 *   points     (n, 4) float32 [bs_idx, x, y, z], points_stride elements from row to row (>= 4); a point belongs to sample
 *              k iff its first column equals (float)k for a k in [0, b), else to none (label 0, targets 0).  Points need
 *              not be grouped by sample;
 *   gt, ext    (b, m, 8) float32 [cx, cy, cz, dx, dy, dz, rz, class], each with its three strides in elements; all m rows
 *              take part, zero rows included;
 *   mean_size  (n_mean, 3) float32 contiguous, or NULL with n_mean = 0 for use_mean_size=False.  Class c names row c - 1,
 *              c <= 0 wraps once as Python does; a class beyond the table reads nothing (its six size-dependent labels
 *              are NaN; the reference asserts).
 * idx = the lowest box of the point's sample that holds it by the predicate of a23, fg = there is one, ext = some enlarged
 * box of the sample holds it.  Outputs, every element written:
 *   cls_labels   (n) int64: 0; -1 where fg != ext; where fg, 1 if num_class == 1 else the class column truncated;
 *   box_labels   (n, 8) float32 or NULL: 0 unless fg, else PointResidualCoder.encode_torch of box idx;
 *   part_labels  (n, 3) float32 or NULL: 0 unless fg, else the point in the box's frame / (dx, dy, dz) + 0.5; the sizes
 *                are clamped to 1e-5f iff box_labels is given (the reference's coder clamps them in place).
 * n == 0 launches nothing; m == 0 or b == 0 writes the background values.                                               */
int modest_point_targets(int64_t n, const float *points_dev, int64_t points_stride, int b, int m, const float *gt_dev,
                         int64_t gt_stride_b, int64_t gt_stride_m, int64_t gt_stride_c, const float *ext_dev,
                         int64_t ext_stride_b, int64_t ext_stride_m, int64_t ext_stride_c, const float *mean_size_dev,
                         int n_mean, int num_class, int64_t *cls_labels_dev, float *box_labels_dev,
                         float *part_labels_dev, void *stream);

/* ---- a31 RoI proposal layer (RoIHeadTemplate.proposal_layer of OpenPCDet's two-stage detectors) ----------
 * MULTI_CLASSES_NMS off.  The proposals of a whole batch in one call: enqueue only, no context, no device allocation, no
 * synchronise, nothing read back, no (n, n / 64) suppression mask.  Every buffer [dev], contiguous.
 *   box        (n_rows, box_cols = 7 + C) float32 [cx, cy, cz, dx, dy, dz, rz, ...]; NMS reads the first 7 columns;
 *   cls        (n_rows, cls_cols = K >= 1) float32;
 *   batch_index  NULL with kind 0 for the dense form, where row i belongs to sample i / rows_per_sample and
 *              n_rows = batch_size * rows_per_sample; else (n_rows) of kind 1 float32, 2 int64 or 3 int32 (rows_per_sample
 *              is not read): a row belongs to sample k iff its value equals k for a k in [0, batch_size), else to none.
 *              A sample's rows need not be contiguous.
 * Per sample: score = max over the class columns, label = its column (the LOWEST column among equal maxima; a NaN ranks
 * above every number).  The min(pre_maxsize, rows of the sample) highest scores -- NaN first, equal scores in ascending
 * row order, -0 == +0 -- are walked in that order by greedy NMS: a candidate is dropped iff its IoU with an earlier
 * survivor, iou(survivor, candidate) of nms_bev (rotated != 0) or nms_normal (rotated == 0), is > thresh.  The first
 * post_maxsize survivors go to rows 0.. of the outputs, every element of which is written:
 *   rois        (batch_size, post_maxsize, box_cols) float32, the survivors' rows of box, then zeros;
 *   roi_scores  (batch_size, post_maxsize) float32, then zeros;
 *   roi_labels  (batch_size, post_maxsize) int64, label + 1, then ones.
 * Limits (the call fails and launches nothing): post_maxsize <= 1024 (the kept list is held in LDS), batch_size <= 65535
 * (16 sample bits of the sort key), n_rows <= 2^31 - 1, box_cols and cls_cols <= 4096.
 * workspace 8-byte aligned, modest_proposals_workspace_bytes(n_rows) bytes, need not be initialised.                    */
int64_t modest_proposals_workspace_bytes(int64_t n_rows);
int modest_proposals(int64_t n_rows, int batch_size, int64_t rows_per_sample, const float *box_dev, int box_cols,
                     const float *cls_dev, int cls_cols, const void *batch_index_dev, int batch_index_kind,
                     int pre_maxsize, int post_maxsize, float thresh, int rotated, float *rois_dev,
                     float *roi_scores_dev, int64_t *roi_labels_dev, void *workspace_dev, int64_t workspace_bytes,
                     void *stream);

/* ---- a32 RoI target assignment (RoIHeadTemplate.assign_targets over ProposalTargetLayer.forward) ---------
 * Two calls, because the reference draws its samples from the host's generators with the list lengths as arguments.  No
 * context, no device allocation.  Every buffer [dev] and contiguous unless said otherwise.
 *   rois        (batch_size, n_rois, roi_cols = 7 + C) float32;   roi_scores (batch_size, n_rois) float32;
 *   roi_labels  (batch_size, n_rois) int64;
 *   gt          (batch_size, n_gt, roi_cols + 1) float32 by three strides counted in elements; the last column is the class.
 *
 * modest_roi_targets_match: BLOCKING -- one launch, one stream synchronise.  Per sample:
 *   trim      the valid gts are rows 0 .. k, k the last row whose float32 sum over all columns, added in column order, is
 *             not == 0 (a NaN sum is not), k = 0 if there is none; with n_gt = 0 the sample has one box of zeros;
 *   match     per roi the 3-D IoU with every valid gt: overlap_bev (as modest_boxes_overlap_bev) times
 *             clamp(min(tops) - max(bottoms), min = 0), over max(va + vb - overlap, 1e-6), volumes (dx * dy) * dz, all in
 *             float32; the maximum and its gt row -- the LOWEST row among equal maxima, a NaN above every number, the
 *             first NaN.  With by_class != 0 only gts whose (int64) class equals the roi's label compete; a roi without a
 *             competitor has maximum 0 and row 0;
 *   lists     in ascending roi order, list 0 fg: iou >= fg_thresh; list 1 hard: iou < reg_fg_thresh and
 *             iou >= bg_thresh_lo; list 2 easy: iou < bg_thresh_lo.  A NaN is in none; a roi may be in fg and hard.
 * The maxima, rows and lists stay in the workspace; the (batch_size, 3) int32 list lengths are written by the kernel into
 * counts_pinned_host (pinned host memory the device can address) and are valid when the call returns.
 *
 * modest_roi_targets_sample: enqueue only, nothing read back.  picks (batch_size, roi_per_image, 2) int32 in pinned host
 * or device memory: list (0 fg, 1 hard, 2 easy) and position in that list, of the workspace the match call with the same
 * batch_size and n_rois filled.  Slot (b, m) resolves its pick to roi row r and gt row g and writes, of every output every
 * element:
 *   out_rois (B, M, roi_cols) = rois[b, r];  out_roi_scores, out_roi_labels (int64), out_gt_iou (B, M);
 *   out_gt_of_rois_src (B, M, roi_cols + 1) = gt[b, g];  out_reg_valid (B, M) int64 = iou > reg_fg_thresh;
 *   out_cls_labels (B, M): score_type 0 (cls) int64 -- 1 if iou > cls_fg, -1 if cls_bg < iou < cls_fg, else 0 (a NaN: 0);
 *             score_type 1 (roi_iou) float32 -- 1 if iou > cls_fg, 0 if iou < cls_bg, else (iou - cls_bg) / fg_minus_bg,
 *             one division by the caller's float32 of the double difference (a NaN stays);
 *   out_gt_of_rois (B, M, roi_cols + 1), the canonical form: ry = remainder(roi[6], 2 pi); centre and ry subtracted;
 *             (x, y, z) times [[c, s, 0], [-s, c, 0], [0, 0, 1]] with c, s = cos, sin of -ry in double rounded once, every
 *             product rounded before the sums; the heading folded into [-pi / 2, pi / 2]; other columns as in gt.
 * A pick that names no list, or a position outside its list, writes a slot of zeros; nothing is read out of bounds.
 * Limits (the call fails and launches nothing): roi_cols in [7, 4096], batch_size <= 65535, roi_per_image >= 1, at most
 * 2^31 - 1 roi rows, gt rows and output rows in a call.
 * workspace 8-byte aligned, modest_roi_targets_workspace_bytes(batch_size, n_rois) bytes (20 bytes a roi and 12 a sample,
 * each of the six arrays rounded up to 256), need not be initialised.
 * Lifetime of picks: the sample call returns before its kernel has read them.  A pinned host table is read where it lies,
 * so the caller keeps it mapped and unwritten until the stream has passed the call.  A later match call on the SAME stream
 * synchronises it, after which the table may be written again; work on another stream needs a table of its own.  An
 * allocator that caches pinned blocks and knows nothing of this kernel (PyTorch's) must not get the block back earlier.
 * modest_roi_targets_gt_tile: the gts a match workgroup stages in LDS at a time (a test builds its shapes around it).
 * modest_roi_targets_workspace_offsets: the byte offsets in the workspace of the six arrays a match call leaves, into
 * offsets_host[6]: counts (batch_size, 3) int32; maxima (batch_size, n_rois) float32; gt rows (batch_size, n_rois) int32;
 * the fg, hard and easy lists, each (batch_size, n_rois) int32 of which a sample's first count entries are valid.  For
 * tests and tools that read the lists back; needs no device.                                                              */
int modest_roi_targets_gt_tile(void);
int64_t modest_roi_targets_workspace_bytes(int batch_size, int n_rois);
int modest_roi_targets_workspace_offsets(int batch_size, int n_rois, int64_t *offsets_host);
int modest_roi_targets_match(int batch_size, int n_rois, int n_gt, const float *rois_dev, int roi_cols,
                             const int64_t *roi_labels_dev, const float *gt_dev, int64_t gt_stride_b, int64_t gt_stride_n,
                             int64_t gt_stride_c, float fg_thresh, float bg_thresh_lo, float reg_fg_thresh, int by_class,
                             void *workspace_dev, int64_t workspace_bytes, int32_t *counts_pinned_host, void *stream);
int modest_roi_targets_sample(int batch_size, int n_rois, int n_gt, int roi_per_image, const int32_t *picks,
                              const float *rois_dev, int roi_cols, const float *roi_scores_dev,
                              const int64_t *roi_labels_dev, const float *gt_dev, int64_t gt_stride_b, int64_t gt_stride_n,
                              int64_t gt_stride_c, float reg_fg_thresh, float cls_fg_thresh, float cls_bg_thresh,
                              float fg_minus_bg, int score_type, const void *workspace_dev, int64_t workspace_bytes,
                              float *out_rois_dev, float *out_gt_of_rois_dev, float *out_gt_iou_dev,
                              float *out_roi_scores_dev, int64_t *out_roi_labels_dev, int64_t *out_reg_valid_dev,
                              void *out_cls_labels_dev, float *out_gt_of_rois_src_dev, void *stream);

/* ---- a33 post-processing (Detector3DTemplate.post_processing over class_agnostic_nms and generate_recall_record;
 * DESIGN.md 7o) ------------------------------------------------------------------------------------------------------
 * MULTI_CLASSES_NMS off.  The final boxes of a whole batch and its recall counters in one call: BLOCKING -- one stream
 * synchronise at the end, no context, no device allocation; nothing is read back but the caller's pinned table, which the
 * kernels write.  box, cls, batch_index, rows_per_sample and the two forms are those of modest_proposals.
 *   score     the maximum over the class columns (the LOWEST column among equal maxima, a NaN above every number); with
 *             normalized == 0 its sigmoid, (float)(1 / (1 + exp(-(double)x))), the double function rounded once;
 *   threshold with has_score_thresh != 0 a row is a candidate iff score >= score_thresh (a NaN is none); with 0 every row
 *             is, NaN scores first;
 *   walk      the sample's min(pre_maxsize, candidates) highest scores -- equal scores (equal AFTER the sigmoid) in
 *             ascending row order, -0 == +0 -- by the greedy NMS of modest_proposals, up to the post_maxsize-th survivor;
 *   outputs   the n_b survivors of sample b in keep order at the front of row b of
 *               pred_boxes (batch_size, post_maxsize, box_cols) float32, the rows of box bit for bit;
 *               pred_scores (batch_size, post_maxsize) float32, the score, or with output_raw_score != 0 the maximum itself;
 *               pred_labels (batch_size, post_maxsize) int64: column + 1, or labels_dev[row] where labels_dev
 *                 (batch_size, rows_per_sample) int64 is given (dense form only);
 *             rows n_b.. of the outputs are NOT written.
 *   recall    with with_gt != 0.  gt (batch_size, n_gt, box_cols + 1) float32 by three strides counted in elements, trimmed
 *             as modest_roi_targets_match trims (through the last row whose float32 sum in column order is not == 0, row 0
 *             at the least; n_gt = 0: none).  Per valid gt the maximum over a list of boxes of the 3-D IoU iou(box, gt) of
 *             modest_roi_targets_match, a NaN staying the maximum; the gt counts for threshold t iff maximum > t (a NaN
 *             never, an empty list never).  The "rcnn" list: without rois (n_rois = -1) the sample's n_b final boxes; with
 *             rois (batch_size, n_rois >= 0, roi_cols) float32 (dense form only) ALL rows of the sample, and a second
 *             "roi" list, the sample's rois.
 *   table     table_pinned_host (batch_size, 2 + 2 * n_thresh) int32 in pinned host memory the device can address, valid
 *             when the call returns: n_b, valid gts, rcnn counts per threshold, roi counts per threshold (without gts the
 *             words behind n_b are not written; without rois the roi counts are 0).  Per sample, no atomics on memory: the
 *             caller adds the samples up.
 * recall_thresh_host: n_thresh float32 in host memory, read before the call returns.
 * Limits (the call fails and launches nothing): post_maxsize <= 1024, batch_size <= 65535, n_rows <= 2^31 - 1, box_cols,
 * cls_cols and roi_cols <= 4096, n_thresh <= 16 (modest_post_process_max_thresholds), at most 2^31 - 1 gt and roi rows.
 * n_gt, n_rois and the length of a list have no limit: a lane per gt, the list staged in LDS modest_post_process_tile()
 * boxes at a time (a test builds its shapes around it).
 * workspace 8-byte aligned, modest_post_process_workspace_bytes(n_rows, batch_size) bytes, need not be initialised.       */
int modest_post_process_tile(void);
int modest_post_process_max_thresholds(void);
int64_t modest_post_process_workspace_bytes(int64_t n_rows, int batch_size);
int modest_post_process(int64_t n_rows, int batch_size, int64_t rows_per_sample, const float *box_dev, int box_cols,
                        const float *cls_dev, int cls_cols, const void *batch_index_dev, int batch_index_kind,
                        int normalized, int has_score_thresh, float score_thresh, int output_raw_score,
                        const int64_t *labels_dev, int pre_maxsize, int post_maxsize, float nms_thresh, int rotated,
                        int with_gt, int n_gt, const float *gt_dev, int64_t gt_stride_b, int64_t gt_stride_n,
                        int64_t gt_stride_c, int n_rois, const float *rois_dev, int roi_cols, int n_thresh,
                        const float *recall_thresh_host, float *pred_boxes_dev, float *pred_scores_dev,
                        int64_t *pred_labels_dev, int32_t *table_pinned_host, void *workspace_dev,
                        int64_t workspace_bytes, void *stream);

/* ---- a34 anchor-head loss with its gradients (AnchorHeadTemplate.get_loss over SigmoidFocalClassificationLoss,
 * WeightedSmoothL1Loss / WeightedL1Loss and WeightedCrossEntropyLoss) ----------------------------------------
 * The three losses of a whole batch and, where wanted, their gradients in one call: enqueue only -- no synchronise, no
 * context, no device allocation, nothing read back.  All buffers are contiguous device memory, float32 unless said:
 *   cls_preds (B, N, num_class), box_preds (B, N, code), dir_preds (B, N, bins) or NULL (no direction head),
 *   labels (B, N) int32, or int64 with labels_int64 != 0: < 0 ignored, 0 background, c + 1 class c (with num_class == 1
 *   every label > 0 is the one class; a label above num_class matches no class and is a positive of the box terms),
 *   reg_targets (B, N, code), anchors (N, anchor_cols >= 7) NOT repeated over the batch, code_weights (code).
 * Per sample cnt = the number of labels > 0 and w = 1.0f / max(cnt, 1); per anchor the classification weight is w where
 * label >= 0 and the box / direction weight w where label > 0, else 0.
 *   classification  t = 1 for the anchor's class column, s = sigmoid(x), aw = t alpha + (1 - t)(1 - alpha),
 *                   pt = t (1 - s) + (1 - t) s, bce = max(x, 0) - x t + log1p(exp(-|x|)), value ((aw pt pt) bce) w;
 *   box             positives only; column 6 is sin(p) cos(t) against cos(p) sin(t); a target that is NaN after that is
 *                   replaced by the input; d = (in - tg) code_weight, n = |d|, value (n < beta ? 0.5 n n / beta :
 *                   n - 0.5 beta) w, plain n w with beta < 1e-5;
 *   direction       positives only; rot = tg[6] + anchor[6], v = rot - dir_offset, v - floor(v / 2pi) 2pi, the bin
 *                   floor(. / (2pi / bins)) clamped to [0, bins - 1] (a NaN: bin 0); value -log_softmax(logits)[bin] w.
 * float32 in this order, one rounding per operation, Python's scalars (beta, dir_offset, the weights, 2pi, 2pi / bins,
 * 0.5 beta) rounded to float32 first; exp, log, log1p, sin, cos and the sigmoid are the double function rounded once.
 * losses (4): cls = (sum / B) cls_weight, loc, dir likewise (0 without a direction head), rpn = cls + (loc + dir).  The
 * sums run over a fixed tree: no float atomics, the same bits at every run.
 * grad_cls / grad_box / grad_dir: all NULL (no gradients), or buffers of the predictions' shapes (grad_dir NULL without a
 * direction head) that receive d rpn / d prediction -- the loss weights and 1 / B inside -- as autograd's chain through the
 * expressions above gives it (at a logit of +-0 the bce derivative is 1 - t); EVERY element is written, the rows of anchors
 * that are not positive with zeros.
 * Limits (the call fails and launches nothing): 1 <= batch_size <= 65535, num_class <= 32, 7 <= code <= 16, bins <= 8,
 * gamma == 2, n_anchors < 2^39.  workspace 4-byte aligned, modest_anchor_loss_workspace_bytes(batch_size, n_anchors) bytes,
 * need not be initialised.
 * modest_anchor_loss_backward multiplies the three gradient buffers (n_cls, n_box, n_dir elements; n_dir = 0 without a
 * direction head) in place by the float32 upstream gradient at upstream_dev, one rounding per element: enqueue only.          */
int64_t modest_anchor_loss_workspace_bytes(int batch_size, int64_t n_anchors);
int modest_anchor_loss(int batch_size, int64_t n_anchors, int num_class, int code, int bins, const float *cls_preds_dev,
                       const float *box_preds_dev, const float *dir_preds_dev, const void *labels_dev, int labels_int64,
                       const float *reg_targets_dev, const float *anchors_dev, int anchor_cols,
                       const float *code_weights_dev, float beta, float dir_offset, float cls_weight, float loc_weight,
                       float dir_weight, float alpha, float gamma, float *losses_dev, float *grad_cls_dev,
                       float *grad_box_dev, float *grad_dir_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int modest_anchor_loss_backward(int64_t n_cls, int64_t n_box, int64_t n_dir, float *grad_cls_dev, float *grad_box_dev,
                                float *grad_dir_dev, const float *upstream_dev, void *stream);

/* ---- a35 RoI-head loss with its gradients (RoIHeadTemplate.get_loss over BinaryCrossEntropy, ResidualCoder,
 * WeightedSmoothL1Loss and get_corner_loss_lidar) ------------------------------------------------------------
 * The losses of all R = B x ROI_PER_IMAGE rows and, where wanted, their gradients in one call: enqueue only -- no
 * synchronise, no context, no device allocation, nothing read back.  Device memory, float32 and contiguous unless said:
 *   rcnn_cls (R) logits, rcnn_reg (R, code),
 *   cls_labels (R) int32 (label_kind 0), int64 (1) or float32 (2): a row counts iff label >= 0, t = float(label),
 *   reg_valid_mask (R) int32, or int64 with mask_int64 != 0: a row is foreground iff mask > 0,
 *   gt_of_rois (R, >= code) in the roi's canonical frame and gt_of_rois_src (R, >= code) in the scene's, each read through
 *   its row stride (in elements); rois (R, code); code_weights (code).
 * With fg = the foreground rows and valid = the counted rows:
 *   classification  s = sigmoid(x), (t - 1) max(log1p(-s), -100) - t max(log(s), -100) over the counted rows,
 *                   rcnn_loss_cls = (sum / max(valid, 1)) cls_weight;
 *   regression      foreground rows; the target is ResidualCoder.encode_torch of gt_of_rois against the roi with centre and
 *                   heading zeroed, both sets of sizes clamped at 1e-5; a NaN target is replaced by the input;
 *                   d = (in - tg) code_weight, n = |d|, value n < beta ? 0.5 n n / beta : n - 0.5 beta (plain n with
 *                   beta < 1e-5), summed over the columns in order; rcnn_loss_reg = (sum / max(fg, 1)) reg_weight;
 *   corner          with corner != 0 and fg > 0, foreground rows: rcnn_reg decoded against the roi with zero centre (sizes
 *                   NOT clamped), its centre rotated by the roi's heading and moved to the roi's centre; the 8 corners of
 *                   that box, of gt_of_rois_src[0:7] and of that gt with heading + float32(pi); per corner the smaller of
 *                   the two distances sqrt((dx dx + dy dy) + dz dz) through smooth L1 with beta 1; the mean of the 8, the
 *                   mean over fg, times corner_weight;
 *   rcnn_loss       cls + (reg + corner), or cls + reg without the corner term.
 * float32 in the order DESIGN.md 7q writes down, one rounding per operation, Python's scalars rounded to float32 first; exp,
 * log, log1p, sin, cos and the sigmoid are the double function rounded once; sqrt and / are correctly rounded.  The sums run
 * over the fixed tree of 7p: no float atomics, the same bits at every run.  A row that is not counted / not foreground is
 * not read for that term (a non-finite value there poisons the reference's sum; it does not reach ours).
 * table (6): rcnn_loss_cls, rcnn_loss_reg (the smooth-L1 part alone), rcnn_loss_corner (0 without), rcnn_loss, fg, valid.
 * grad_cls (R) / grad_reg (R, code): both NULL (no gradients), or buffers that receive d rcnn_loss / d prediction as
 * autograd's chain through the expressions above gives it (min of two equal distances hands half to each side, the norm
 * of a zero vector hands on 0, columns >= 7 get nothing from the corner term); EVERY element is written.
 * Limits (the call fails and launches nothing): n_rows <= modest_roi_loss_max_rows() = 2^20, 7 <= code <= 16, the row
 * strides >= code.  workspace 4-byte aligned, modest_roi_loss_workspace_bytes(n_rows) bytes, need not be initialised.
 * modest_roi_loss_backward multiplies the two gradient buffers (n_cls, n_reg elements) in place by the float32 upstream
 * gradient at upstream_dev, one rounding per element: enqueue only.                                                          */
int64_t modest_roi_loss_max_rows(void);
int64_t modest_roi_loss_workspace_bytes(int64_t n_rows);
int modest_roi_loss(int64_t n_rows, int code, const float *rcnn_cls_dev, const float *rcnn_reg_dev,
                    const void *cls_labels_dev, int label_kind, const void *reg_valid_mask_dev, int mask_int64,
                    const float *gt_of_rois_dev, int64_t gt_row_stride, const float *gt_of_rois_src_dev,
                    int64_t src_row_stride, const float *rois_dev, const float *code_weights_dev, float beta,
                    float cls_weight, float reg_weight, float corner_weight, int corner, float *table_dev,
                    float *grad_cls_dev, float *grad_reg_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int modest_roi_loss_backward(int64_t n_cls, int64_t n_reg, float *grad_cls_dev, float *grad_reg_dev,
                             const float *upstream_dev, void *stream);

/* ---- a36 point-head loss with its gradients (PointHeadBox / PointIntraPartOffsetHead / PointHeadSimple .get_loss over
 * get_cls_layer_loss, get_part_layer_loss and get_box_layer_loss of PointHeadTemplate) ------------------------
 * The losses of all N points of a stacked batch and, where wanted, their gradients in one call: enqueue only -- no
 * synchronise, no context, no device allocation, nothing read back.  Contiguous device memory, float32 unless said:
 *   cls_preds (N, num_class) logits,
 *   labels (N) int32, or int64 with labels_int64 != 0: < 0 ignored, 0 background, c + 1 class c (strictly: no override for
 *   num_class == 1; a label above num_class matches no class and counts as a positive),
 *   part_preds (N, 3) logits and part_labels (N, 3), both or both NULL (no part term),
 *   box_preds (N, code), box_labels (N, code) and code_weights (code), all three or all NULL (no box term).
 * P = the number of labels > 0 over ALL N points (not per sample; nothing is divided by a batch size), w = 1.0f / max(P, 1):
 *   classification  weight w where label >= 0, else 0; t = 1 iff label == c + 1, s = sigmoid(x), aw = 0.25 t + 0.75 (1 - t),
 *                   pt = t (1 - s) + (1 - t) s, bce = max(x, 0) - x t + log1p(exp(-|x|)), value ((aw pt pt) bce) w, a point's
 *                   columns added in class order; point_loss_cls = sum cls_weight;
 *   part            positive rows only; per column s = sigmoid(x), (t - 1) max(log1p(-s), -100) - t max(log(s), -100), the
 *                   three columns added in order; point_loss_part = (sum / float(3 max(P, 1))) part_weight;
 *   box             positive rows only; a NaN target is replaced by the input; d = (in - tg) code_weight, n = |d|, value
 *                   (n < beta ? 0.5 n n / beta : n - 0.5 beta) w, plain n w with beta < 1e-5, the columns added in order;
 *                   point_loss_box = sum box_weight;
 *   point_loss      cls, (cls + part), (cls + box) or ((cls + part) + box): absent terms are skipped.
 * float32 in this order, one rounding per operation, Python's scalars rounded to float32 first; exp, log, log1p and the
 * sigmoid are the double function rounded once; / is correctly rounded.  The sums run over the fixed tree of 7p: no float
 * atomics, the same bits at every run.  A row that is not positive is not read for the part and box terms.
 * table (5): point_loss_cls, point_loss_part, point_loss_box (0 for an absent term), point_loss, point_pos_num = P.
 * grad_cls / grad_part / grad_box: grad_cls NULL (no gradients, the others NULL too), or one buffer of the prediction's shape
 * per term present (NULL for an absent term) that receives d point_loss / d prediction as autograd's chain through the
 * expressions above gives it (at a logit of +-0 the bce derivative is 1 - t; the part gradient is (g (s - t)) / max((1 - s) s,
 * 1e-12) through the sigmoid with g = part_weight / float(3 max(P, 1))); EVERY element is written, the part and box rows of
 * points that are not positive with zeros.
 * Limits (the call fails and launches nothing): n_rows <= modest_point_loss_max_rows() = 2^24 (P stays exact in float32),
 * 1 <= num_class <= 32, 1 <= code <= 16.  workspace 4-byte aligned, modest_point_loss_workspace_bytes(n_rows) bytes, need
 * not be initialised.
 * modest_point_loss_backward multiplies the three gradient buffers (n_cls, n_part, n_box elements; 0 for an absent term) in
 * place by the float32 upstream gradient at upstream_dev, one rounding per element: enqueue only.                             */
int64_t modest_point_loss_max_rows(void);
int64_t modest_point_loss_workspace_bytes(int64_t n_rows);
int modest_point_loss(int64_t n_rows, int num_class, int code, const float *cls_preds_dev, const void *labels_dev,
                      int labels_int64, const float *part_preds_dev, const float *part_labels_dev,
                      const float *box_preds_dev, const float *box_labels_dev, const float *code_weights_dev, float beta,
                      float cls_weight, float part_weight, float box_weight, float *grad_cls_dev, float *grad_part_dev,
                      float *grad_box_dev, float *table_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int modest_point_loss_backward(int64_t n_cls, int64_t n_part, int64_t n_box, float *grad_cls_dev, float *grad_part_dev,
                               float *grad_box_dev, const float *upstream_dev, void *stream);

/* ---- a37: box decoding of the three kinds of head (csrc/box_decode.hip) -------------------------------
 * generate_predicted_boxes of AnchorHeadTemplate, PointHeadTemplate and RoIHeadTemplate over ResidualCoder /
 * PointResidualCoder .decode_torch.  Each call only enqueues on `stream`: no allocation, no wait on the host, nothing read
 * back; EVERY output element is written, so the output need not be initialised.  All tensors float32, contiguous but `points`.
 * Arithmetic: float32, one rounding per operation in the order written here, sqrt and / correctly rounded, exp / sin / cos /
 * atan2 the double function rounded once, x ** 2 as x * x; the scalars arrive as float32 (Python floats rounded first).
 * ARGMAX (direction bins and classes): torch's max(dim=-1) on the CPU -- the first index of the maximum, a NaN counts as the
 * maximum and the first NaN wins.
 * With an anchor row (xa ya za dxa dya dza ra extras..) and an encoding (xt yt zt dxt dyt dzt rt.. extras..):
 *   diag = sqrt(dxa dxa + dya dya); xg = xt diag + xa; yg = yt diag + ya; zg = zt dza + za; dxg = exp(dxt) dxa (dy, dz alike);
 *   an extra column is t + a.
 * modest_anchor_decode: box_preds (batch, n_anchors, code_in), anchors (n_anchors, cols) read once per row for every sample,
 *   cols = code_in, or code_in - 1 with sincos; dir_cls_preds (batch, n_anchors, bins) or NULL; boxes (batch, n_anchors, cols).
 *   rg = rt + ra, or with sincos (encoding columns 6, 7 = cost, sint) atan2(sint + sin ra, cost + cos ra).  With dir_cls_preds:
 *   label = ARGMAX of the bins, period = float32(2 pi / bins), v = rg - dir_offset,
 *   rot = v - floor(v / period + dir_limit_offset) period, rg = (rot + dir_offset) + period float(label).
 * modest_point_decode: box_preds (n_rows, code_in) with columns 6, 7 = cost, sint; points: row i at points + i point_stride,
 *   three floats (the caller's view point_coords[:, 1:4]); cls_preds (n_rows, num_class); mean_size (num_class, 3) or NULL;
 *   boxes (n_rows, code_in - 1).  c = ARGMAX of the classes; (dxa dya dza) = mean_size[c] and the expressions above with
 *   (xa ya za) = the point; without mean_size xg = xt + xa (y, z alike) and dxg = exp(dxt); rg = atan2(sint, cost); an extra
 *   column is copied.
 * modest_roi_decode: rois and box_preds (n_rows, code) -> boxes (n_rows, code).  The expressions above against the roi with
 *   (xa ya za) = 0 (xg = xt diag + 0), rg = rt + ra; then with c = cos ra, s = sin ra:
 *   x = ((xg c + yg (-s)) + zg 0) + roi x;  y = ((xg s + yg c) + zg 0) + roi y;  z = (((xg 0) + (yg 0)) + zg 1) + roi z
 *   (the zero terms make an infinite coordinate a NaN in the others, as a matrix product does).
 * Limits (the call fails and launches nothing): rows (batch n_anchors, n_rows) <= modest_box_decode_max_rows() = 2^31 - 1 (a
 * row index is an int, element offsets are int64), code <= 16 and >= 7 (8 where the encoding carries cost and sint),
 * 1 <= bins <= 8, 1 <= num_class <= 32, point_stride >= 3, buffers 4-byte aligned.                                          */
int64_t modest_box_decode_max_rows(void);
int modest_anchor_decode(int batch, int64_t n_anchors, int code_in, int sincos, const float *box_preds_dev,
                         const float *anchors_dev, const float *dir_cls_preds_dev, int bins, float dir_offset,
                         float dir_limit_offset, float *boxes_dev, void *stream);
int modest_point_decode(int64_t n_rows, int code_in, int num_class, const float *box_preds_dev, const float *points_dev,
                        int64_t point_stride, const float *cls_preds_dev, const float *mean_size_dev, float *boxes_dev,
                        void *stream);
int modest_roi_decode(int64_t n_rows, int code, const float *rois_dev, const float *box_preds_dev, float *boxes_dev,
                      void *stream);

/* ---- a38: PointPillars' PillarVFE and BEV scatter with fused backward (csrc/pillar_vfe.hip) -----------
 * PillarVFE.forward with one PFN layer (features, Linear without bias, BatchNorm1d, ReLU, max over the slots) and
 * PointPillarScatter.forward, each with its backward.  Every call only enqueues on `stream`: no allocation, no wait on the host,
 * nothing read back; every output element is written (the canvas: zero-filled, then the rows in range).
 * voxels (n_pillars, slots, point_features) float32; num_points (n_pillars) and coords (n_pillars, 4) = [b, z, y, x] of the
 * dtype their code names: 0 float32, 1 int32, 2 int64.  geometry_host: six floats on the HOST, voxel x y z and the offsets
 * float32(voxel / 2 + range) x y z.  parts: a mask of 1 (the points' own xyz; without it columns 3.. only), 2 (cluster offset),
 * 4 (centre offset), 8 (distance); the features of a slot, K of them, stand in that order.
 * Arithmetic: float32, one rounding per operation in the order written, / and sqrt correctly rounded.
 *   sum_j = v[0][j] + v[1][j] + .. over ALL slots, mean_j = sum_j / float32(num); cluster: v_j - mean_j;
 *   centre: v_0 - (float32(coord x) vx + xoff) (y with coords[2], z with coords[1]); distance: sqrt((x x + y y) + z z);
 *   every feature times float32(int(num) > slot): a MULTIPLICATION (num = 0 gives NaN features in every slot);
 *   x = f_0 W[c][0], then + f_k W[c][k] for k = 1 .. K - 1;  xhat = (x - mean32) invstd32;  t = xhat gamma + beta;
 *   y = t where t > 0 or t is a NaN, else +0;  out[p][c] = the maximum of y over ALL slots, winner[p][c] its FIRST slot; a NaN
 *   counts as the maximum and the first NaN wins.
 * training != 0: mean32 / invstd32 = float32 of mean = sum x / N and 1 / sqrt(var + eps), var = max(sum x x / N - mean mean, 0)
 *   (a NaN kept), N = n_pillars slots (padded rows count), all float64.  The float64 sums -- sum x, sum x x, sum x f_k per
 *   channel and sum f_k, kept in sums as [C] [C] [K][C] [K] -- are added over a tree that depends on n_pillars and slots only:
 *   a wavefront adds modest_pillar_vfe_run() consecutive pillars in pillar then slot order, modest_pillar_vfe_group() such
 *   partials are added in ascending order, then the groups in ascending order, each from +0.0; x x and x f_k are exact products.
 *   stat = mean32 [C], invstd32 [C].  The running buffers (NULL: none) are updated in place, in float64 rounded to float32:
 *   r = (1 - m) r + m new with the unbiased var N / (N - 1) for running_var; m = momentum, or 1 / (tracked + 1) where
 *   momentum < 0; num_batches_tracked (NULL: none) += 1.  N < 2 is refused, as the reference refuses it.
 * training == 0: mean32 = running_mean, invstd32 = float32(1 / sqrt(float64(running_var) + eps)); winner may be NULL, sums, stat
 *   and the workspace are not used and no buffer changes.
 * modest_pillar_vfe_backward: dy = grad_out where out > 0, else 0, at the winner's slot; over the same tree in float64
 *   dbeta = sum dy, dgamma = sum dy xhat, A[c][k] = sum dy f_k (exact products), xhat recomputed as in the forward; then with
 *   g = gamma, mean = float64(mean32), invstd = float64(invstd32):
 *   dW[c][k] = invstd (((g A) - ((g dbeta) / N) sum f_k) - (((g dgamma) / N) invstd) (sum x f_k - mean sum f_k)), rounded to
 *   float32 as dgamma and dbeta are.  The voxels get no gradient.
 * modest_pillar_scatter: canvas (batch, channels, ny, nx) := 0, then canvas[b][c][y][x] = features[p][c] (cell z + y nx + x,
 *   nz = 1).  A row whose b, z, y or x is out of range (z: other than 0) is skipped.  Two rows of one cell are a precondition
 *   not to occur.  modest_pillar_scatter_backward: grad_features[p][c] = grad_canvas[b][c][y][x], zeros for a row out of range.
 * Limits (the call fails and launches nothing): 1 <= out_channels <= 64, 1 <= K <= 16, point_features >= 3, 1 <= slots <= 255,
 * n_pillars slots <= 2^31 - 1, batch <= 65535, float buffers 4-byte and int64 / float64 buffers 8-byte aligned, a workspace
 * of modest_pillar_vfe_workspace_bytes(n_pillars, out_channels, K) bytes (negative: a refusal).                              */
int modest_pillar_vfe_run(void);
int modest_pillar_vfe_group(void);
int64_t modest_pillar_vfe_workspace_bytes(int64_t n_pillars, int out_channels, int features);
int modest_pillar_vfe(int64_t n_pillars, int slots, int point_features, int out_channels, int parts,
                      const float *voxels_dev, const void *num_points_dev, int num_code, const void *coords_dev,
                      int coord_code, const float *geometry_host, const float *weight_dev, const float *gamma_dev,
                      const float *beta_dev, float *running_mean_dev, float *running_var_dev,
                      int64_t *num_batches_tracked_dev, double eps, double momentum, int training, float *out_dev,
                      uint8_t *winner_dev, double *sums_dev, float *stat_dev, void *workspace_dev,
                      int64_t workspace_bytes, void *stream);
int modest_pillar_vfe_backward(int64_t n_pillars, int slots, int point_features, int out_channels, int parts,
                               const float *voxels_dev, const void *num_points_dev, int num_code,
                               const void *coords_dev, int coord_code, const float *geometry_host,
                               const float *weight_dev, const float *gamma_dev, const float *out_dev,
                               const uint8_t *winner_dev, const float *grad_out_dev, const double *sums_dev,
                               const float *stat_dev, float *grad_weight_dev, float *grad_gamma_dev,
                               float *grad_beta_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int modest_pillar_scatter(int64_t n_pillars, int channels, int batch, int ny, int nx, const float *features_dev,
                          const void *coords_dev, int coord_code, float *canvas_dev, void *stream);
int modest_pillar_scatter_backward(int64_t n_pillars, int channels, int batch, int ny, int nx,
                                   const float *grad_canvas_dev, const void *coords_dev, int coord_code,
                                   float *grad_features_dev, void *stream);

/* ---- a39: training-batch preparation (csrc/batch_prep.hip) ---------------------------------------------
 * gt sampling (DataBaseSampler), random_world_flip / _rotation / _scaling, mask_points_and_boxes_outside_range and the near /
 * far lists of sample_points for a whole batch; the arithmetic is stated at the top of csrc/batch_prep.hip.
 * modest_batch_prep_stage1 BLOCKS: it ends with the call's one stream synchronise, after which table_pinned_host holds, per
 * sample, modest_batch_prep_table_words() = 6 int32: points kept, far points, boxes kept, candidates kept, candidates dropped, 0.
 * Tables (host copies are checked against every bound before anything is launched; the device copies must equal them):
 *   samp (batch, 10) int64: first row of the sample in the virtual concatenation, object rows, first scene row, scene rows,
 *     first box, gts, candidates, first candidate, first tile, 0 -- each "first" the running sum over the samples before;
 *     a sample's tiles: ceil((object rows + scene rows) / modest_batch_prep_tile())
 *   boxes (n_boxes, 12) float32: per sample its gts, then its candidates: x y z dx dy dz heading, cosf(h) sinf(h) cosf(-h)
 *     sinf(-h) of the HOST's libm, the class index (0: a name outside class_names)
 *   cand (n_cand, 3) int64: first row and rows in the database points, first object row within the sample;
 *   cand_f64 (n_cand, 2): mv_height, the lowered box z (read with road_plane);  cand_group (n_cand) int32: equal numbers in a
 *     run form a class group;  xf (batch, 8) float32: flip x, flip y (non-zero: drawn), cos, sin, float(angle), float(scale), 0, 0
 *   ops_host: the augmentor steps in order, 1 flip x, 2 flip y, 3 rotation, 4 scaling;  range_host: x0 y0 z0 x1 y1 z1;
 *   extra_width_host: REMOVE_EXTRA_WIDTH.
 * Outputs: valid (n_cand) int32; points (n_rows, 1 + features), of which the first sum(points kept) rows are written: the
 *   survivors of sample 0 in the concatenation's order, then sample 1's ..., column 0 the sample; lists (n_rows) int32: with
 *   want_near, at the sample's first output row its near survivors' places among its survivors, in order, then its far ones';
 *   gt_boxes (batch, gt_capacity, 8): the kept boxes with the class index, zeros behind them.
 * modest_batch_prep_order only enqueues: out row i = the row that picks[i] = (4 sample + list, place) names -- list 0: the
 *   sample's survivor `place`, 1 / 2: the survivor that entry `place` of its near / far list names -- read from the points, lists
 *   and workspace a stage-1 call of the same n_rows and batch_size left.  perm (n_rows) int32 or NULL: shuffle_points ahead of
 *   sample_points -- at the sample's first output row the order of its survivors (place i holds survivor perm[i]); places and
 *   the near / far lists (rebuilt in lists2 (n_rows) int32 by one more launch) are then those of that order.
 * Limits (the call fails and launches nothing): gts + candidates of a sample <= modest_batch_prep_max_boxes() = 512, 4 <= features
 * <= 8, batch <= 65535, rows <= 2^31 - 1, a workspace of modest_batch_prep_workspace_bytes(n_rows, batch) (negative: a refusal).  */
int modest_batch_prep_max_boxes(void);
int modest_batch_prep_tile(void);
int modest_batch_prep_table_words(void);
int64_t modest_batch_prep_workspace_bytes(int64_t n_rows, int batch_size);
int modest_batch_prep_stage1(int batch_size, int features, int64_t n_scene_rows, const float *scene_dev,
                             int64_t n_db_rows, const float *db_dev, const int64_t *samp_host, const int64_t *samp_dev,
                             int64_t n_boxes, const float *boxes_dev, int64_t n_cand, const int64_t *cand_host,
                             const int64_t *cand_dev, const double *cand_f64_dev, const int32_t *cand_group_dev,
                             const float *xf_dev, int n_ops, const int32_t *ops_host, const float *range_host,
                             const float *extra_width_host, int road_plane, int want_near, int remove_outside_boxes,
                             int min_num_corners, int64_t n_rows, int32_t *valid_dev, float *points_dev,
                             int32_t *lists_dev, float *gt_boxes_dev, int gt_capacity, int32_t *table_pinned_host,
                             void *workspace_dev, int64_t workspace_bytes, void *stream);
int modest_batch_prep_order(int batch_size, int features, int64_t n_rows, const float *points_dev,
                            const int32_t *lists_dev, const void *workspace_dev, int64_t workspace_bytes,
                            int64_t n_out, const int32_t *picks_dev, const int32_t *perm_dev, int32_t *lists2_dev,
                            float *out_dev, void *stream);

/* ---- a40: the optimiser step (csrc/optim_step.hip) -------------------------------------------------------
 * clip_grad_norm_ and OptimWrapper.step (decoupled weight decay + torch.optim.Adam.step) over one table of the whole parameter
 * set; the arithmetic and the summation order are stated at the top of csrc/optim_step.hip.  Every call only enqueues on
 * `stream`; it waits for the device only where the host has run a whole ring of the context's pinned staging slots ahead.
 * Tables (host copies; every bound is checked on them before anything is launched), one record per tensor, none without elements:
 *   static (n_tensors, 40 bytes): uint64 p, m, v (device addresses, 4-byte aligned; m and v may be 0 on a tensor without a
 *     gradient, all three where the call reads no state), int64 n, int32 first chunk (the running sum of ceil(n /
 *     modest_optim_chunk())), int32 0.  Copied to the workspace only with upload_static: pass 0 while the workspace holds a copy
 *     of the same table.
 *   step (n_tensors, 48 bytes): uint64 g (0: no gradient this step), float32 dec, w, omw = 1 - w, b2, omb2, bc2s, eps, nss,
 *     uint32 flags (1: w >= 0.5, the other branch of lerp), int32 norm_first (the running sum of the chunks of the tensors with
 *     a gradient; -1 without one).
 * modest_optim_grad_norm: *norm_out_dev = (float) sqrt(sum g^2).  modest_optim_clip: that, then g *= coef in place.
 * modest_optim_step: the step with the gradients as they are.  modest_optim_norm_step: the norm, then the step on fl(g * coef);
 * the gradients are not written.  n_chunks: the sum of the tensors' chunks.  finish_launch 0: every workgroup of the consumer
 * sums the chunk partials itself (two launches); non-zero: a one-workgroup launch between the two sums them once and the
 * consumer reads the coefficient it left (three launches) -- the same bits either way.
 * Limits (the call fails and launches nothing): 1 <= n_tensors <= 2^20, n_chunks <= 2^31 - 1, a 256-byte aligned workspace of
 * modest_optim_workspace_bytes(n_tensors, n_chunks) bytes (negative: a refusal).                                                 */
int modest_optim_chunk(void);
int64_t modest_optim_workspace_bytes(int64_t n_tensors, int64_t n_chunks);
int modest_optim_grad_norm(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host,
                           const void *step_host, int upload_static, float *norm_out_dev, void *workspace_dev,
                           int64_t workspace_bytes, void *stream);
int modest_optim_clip(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host,
                      const void *step_host, int upload_static, float max_norm, int finish_launch,
                      float *norm_out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);
int modest_optim_step(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host,
                      const void *step_host, int upload_static, void *workspace_dev, int64_t workspace_bytes,
                      void *stream);
int modest_optim_norm_step(modest_ctx *ctx, int64_t n_tensors, int64_t n_chunks, const void *static_host,
                           const void *step_host, int upload_static, float max_norm, int finish_launch,
                           float *norm_out_dev, void *workspace_dev, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MODEST_HIP_H */
