/* viso_amd — MI355X-native (gfx950) visual-odometry hot path, C ABI.
 *
 * This is the drop-in boundary for the reference's per-frame path
 * (Seasandwpy/viso).  Each entry point names the reference interface it
 * replaces (file:line under the reference tree).  Conventions:
 *   - every function returns int: VISO_OK (0) or a negative VISO_ERR_*;
 *     nothing throws across this boundary;
 *   - the caller owns host buffers; inputs are consumed (uploaded) before a
 *     call returns unless the name says "_device" (then the pointers are HIP
 *     device pointers that must stay valid until viso_synchronize());
 *   - a viso_ctx is bound to one HIP device and one HIP stream; it is not
 *     thread-safe; distinct contexts may run concurrently;
 *   - no C++ or torch types cross this boundary.
 */
#ifndef VISO_C_H
#define VISO_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VISO_OK 0
#define VISO_ERR_ARG (-1)
#define VISO_ERR_HIP (-2)
#define VISO_ERR_CAPACITY (-3)
#define VISO_ERR_STATE (-4)
#define VISO_ERR_NODEVICE (-5)

/* include/viso.h:13-17 */
#define VISO_STATE_INITIALIZATION 0
#define VISO_STATE_RUNNING 1
#define VISO_STATE_FINISHED 2

/* Constructor arguments Viso(fx, fy, cx, cy) (include/viso.h:47) plus the
 * reference's hard-coded constants (include/viso.h:20-26) and the switches
 * the reference does not have. */
typedef struct viso_params {
    double fx, fy, cx, cy;            /* include/viso.h:47-50 */
    int32_t width, height;            /* level-0 frame size (continuous rows) */
    int32_t reinitialize_after;       /* 10     include/viso.h:20 */
    int32_t fast_thresh;              /* 50     include/viso.h:21 */
    double projection_error_thresh;   /* 0.3    include/viso.h:22 */
    double parallax_thresh;           /* 1 deg  include/viso.h:23 */
    double disparity_squared_thresh;  /* 225    include/viso.h:24 */
    double photometric_error_thresh;  /* 14400  include/viso.h:26 */
    int32_t enable_tracking;          /* 0: as shipped (kFinished after init,
                                         src/viso.cpp:97); 1: kRunning */
    int32_t ransac_e_iters;           /* 1000 (OpenCV findEssentialMat default) */
    int32_t ransac_h_iters;           /* 2000 (src/viso.cpp:240) */
    double ransac_confidence;         /* 0.99 (src/viso.cpp:222,240) */
    uint64_t ransac_seed;             /* counter-RNG seed of the samplers */
    int32_t max_features;             /* capacity of FAST / KLT arrays (1..65536) */
    int32_t max_poses;                /* capacity of the pose log */
    int32_t batch_frames;             /* frames per viso_process_frames_device
                                         chunk (frame-slot pool size) */
    int32_t precision;                /* VISO_PRECISION_FAITHFUL (default) or
                                         VISO_PRECISION_FAST (tracking stages) */
    int32_t reserved[6];
} viso_params;

/* viso_params.precision.
 * FAITHFUL: fp64 wherever the reference is fp64, results bit-identical to
 *   the oracle (canonical tree sums, Eigen PartialPivLU inverse).
 * FAST: tolerance mode for the tracking stages (direct pose, LK alignment):
 *   fp32 per-pixel sampling / Jacobians / products with fp64 per-point and
 *   per-map sums, an LDL^T solve of the 6x6 normal equations; validated
 *   against the oracle at the north star's 1e-4 rel-Frobenius pose bar
 *   (tests/test_fast_mode.py).  Initialisation stages are always faithful. */
#define VISO_PRECISION_FAITHFUL 0
#define VISO_PRECISION_FAST 1

typedef struct viso_ctx viso_ctx;

/* Defaults = the reference's constants (include/viso.h:20-26). */
int viso_default_params(viso_params* p, double fx, double fy, double cx, double cy,
                        int32_t width, int32_t height);

/* Viso::Viso(fx,fy,cx,cy) (include/viso.h:47-52) on HIP device `device`. */
int viso_create(const viso_params* p, int device, viso_ctx** out);
int viso_destroy(viso_ctx* ctx);

/* FrameSequence::FrameHandler::OnNewFrame(Keyframe::Ptr)
 * (include/frame_sequence.h:13-16, implemented by Viso::OnNewFrame,
 * src/viso.cpp:7-145).  `grey`: width x height u8 rows, `stride` bytes apart
 * (copied before the call returns).  Builds the 4-level pyramid (Keyframe
 * ctor, include/keyframe.h:28-46).  Asynchronous: while tracking, the
 * frame's last pose step and its LK alignment may still be queued when the
 * call returns; every other call on the context (getters,
 * viso_synchronize, setters, stage calls, device ingest) launches them
 * first, so results read through the API are always complete.  An error of
 * that deferred work (frame k's final solve or LK batch) is returned by the
 * call that launches it — the next call on the context — not by frame k's. */
int viso_process_frame(viso_ctx* ctx, const uint8_t* grey, int32_t width, int32_t height,
                       int32_t stride);

/* North-star facade VisualOdometryStereo::process(left, right, dims):
 * dims = {width, height, stride}.  The left image drives the reference path;
 * the right image (level 0 only, no pyramid) feeds the stereo initialisation
 * and stereo keyframe insertion (viso_set_stereo).  (No reference
 * counterpart: the reference is monocular) */
int viso_process_stereo(viso_ctx* ctx, const uint8_t* left, const uint8_t* right,
                        const int32_t dims[3]);

/* Batched ingest of n consecutive frames already resident in HBM (device
 * pointers, frame f at d_left + f * frame_stride, rows continuous).  Builds
 * all left pyramids of the chunk in one batched launch, then runs OnNewFrame
 * per frame in order.  d_right may be NULL (mono).
 * Buffer contract: the frames are read in place, asynchronously, on the
 * context stream.  Their producer must have completed before the call (the
 * caller synchronises its own stream), and the buffers must stay valid and
 * unmodified until viso_synchronize(ctx) returns.  Frames the context retains
 * (reference / last / keyframes) are copied into its own pool before that. */
int viso_process_frames_device(viso_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right,
                               int32_t n, size_t frame_stride);

/* Wait for all queued work of the context. */
int viso_synchronize(viso_ctx* ctx);

/* State (include/viso.h:44) */
int viso_get_state(viso_ctx* ctx, int32_t* state);
/* Viso::poses (include/viso.h:54): Tcw per tracked frame, 12 doubles each
 * (R row-major, t); the first min(cap, count, max_poses) are copied (one
 * device round trip).  *n receives the total count, which is host state: with
 * Tcw12 NULL or cap 0 the call does not touch the device. */
int viso_get_poses(viso_ctx* ctx, double* Tcw12, size_t cap, size_t* n);
/* Viso::GetPoints() (include/viso.h:60-67): map points, 3 doubles each. */
int viso_get_points(viso_ctx* ctx, double* xyz, size_t cap, size_t* n);
/* Initialisation tracks: init_.kp1 / init_.kp2 (float x,y) and
 * init_.success (include/viso.h:33-41). */
int viso_get_init_tracks(viso_ctx* ctx, float* kp1, float* kp2, uint8_t* success, size_t cap,
                         size_t* n);
/* Last LKAlignment outputs (src/viso.cpp:768-843), dense over map points:
 * pair_kf (-1 = no pair), success, uv_before, uv_after (2 doubles each). */
int viso_get_alignment(viso_ctx* ctx, int32_t* pair_kf, uint8_t* success, double* uv_before,
                       double* uv_after, size_t cap, size_t* n);
/* Per-frame statistics of the last processed frame (16 doubles):
 * [0] state, [1] tracked points, [2] nr_inliers, [3] best motion,
 * [4] candidates, [5] init frame_cnt, [6] alignment pairs,
 * [7] alignment successes, [8] disparity_squared, [9] direct-pose nGood
 * (level 0), [10] direct-pose cost (level 0), [11] frames processed,
 * [12] init succeeded on this frame, [13..15] reserved. */
int viso_get_frame_stats(viso_ctx* ctx, double stats[16]);
/* Per-frame log (structured per-frame statistics, every tracking frame
 * rather than the last one; no reference counterpart — the reference prints
 * nGood / cost per level, src/viso.cpp:755-757).  enable != 0 allocates
 * max_poses rows of 4 doubles on the device: for the tracking frame with
 * pose index k (the k-th entry of viso_get_poses), row k = {level-0 nGood,
 * level-0 cost (as viso_get_frame_stats [9], [10]), LK alignment pairs,
 * LK alignment successes (as [6], [7])}, written by the kernels themselves
 * (the direct pose's logging thread; one counting launch per LK batch);
 * rows of frames processed while it was off read NaN.  enable = 0 frees it. */
int viso_set_frame_log(viso_ctx* ctx, int32_t enable);
/* The context's execution resources (no reference counterpart), 8 ints:
 * [0] LK alignment of device-ingest chunks in the background of the direct
 *     chain (1) or batched after it (0: VISO_LK_BG=0, serialised kernels, or
 *     no side queue of its own could be made),
 * [1] the LK side stream has a hardware queue of its own (CU-masked stream),
 * [2] the host-upload stream likewise (-1: not created yet, it is made by the
 *     first host frame),
 * [3] frame slots in the pool, [4] per-frame log on, [5] batch_frames,
 * [6] level-0 bytes the last ingest's pyramid tail launch copied into the
 *     pool beside levels 2-3 (its last frame, kept as last_frame: 0 or
 *     width x height), [7] background-LK words (int32) it cleared.
 * See INTEGRATION.md §4 for the queue budget. */
int viso_get_config(viso_ctx* ctx, int32_t info[8]);
/* The first min(cap, poses) rows (4 doubles each) of the per-frame log; *n =
 * the pose count.  VISO_ERR_STATE when the log is off. */
int viso_get_frame_log(viso_ctx* ctx, double* rows, size_t cap, size_t* n);

/* Kernel timing (HIP events on the context stream) for roofline accounting.
 * kernel ids: see VISO_KERNEL_*.  When enabled, every launch of the kernel
 * is bracketed by events; viso_timing_get returns the launch count and the
 * summed milliseconds. */
#define VISO_KERNEL_PYRAMID 0
#define VISO_KERNEL_FAST 1
#define VISO_KERNEL_KLT 2
#define VISO_KERNEL_RANSAC 3
#define VISO_KERNEL_SELECT 4
#define VISO_KERNEL_DIRECT 5
#define VISO_KERNEL_LKALIGN 6
#define VISO_KERNEL_STEREO 7
#define VISO_KERNEL_UPLOAD 8 /* host -> device copy of a frame (viso_process_frame / _stereo) */
#define VISO_KERNEL_MAPWIN 9 /* one retirement of the sliding-window map (viso_set_map_window) */
#define VISO_KERNEL_REFINE 10 /* one frame's pose refinement (viso_set_pose_refine) */
#define VISO_KERNEL_CULL 11 /* the record update and cull launches (viso_set_point_cull) */
#define VISO_KERNEL_POINTS 12 /* the record and refine launches (viso_set_point_refine) */
#define VISO_KERNEL_LKWARP 13 /* a batched launch of the warped LK alignment (viso_set_lk_warp) */
#define VISO_KERNEL_SEEDS 14 /* the depth seeds' creation, update and promotion launches (viso_depth_seeds_*) */
#define VISO_KERNEL_RELOC 15 /* one relocalisation attempt: the candidates and the choice (viso_set_relocalise) */
#define VISO_KERNEL_RECTIFY 16 /* a batched rectification launch ahead of the pyramid (viso_set_rectify) */
#define VISO_KERNEL_PYRAMID_L1 17 /* viso_pyramid's level-1 launch alone (the stage entry only; the yardstick of
                                    tools/bench_rectify.py) */
#define VISO_KERNEL_RELOC_SEED 18 /* one relocalisation seed stage behind its FAST launches (viso_set_reloc_seed) */
#define VISO_KERNEL_BRIGHT 19 /* one frame's brightness-compensated chain (viso_set_brightness, viso_track_affine) */
#define VISO_KERNEL_COUNT 20
/* (timing_get first launches what host-frame calls left pending, as the
 * getters do; an error of a frame's deferred work — its final solve or LK
 * batch — is returned by the next call on the context that launches it) */
int viso_timing_enable(viso_ctx* ctx, int32_t enable);
/* Restrict timing to the kernels whose bit (1 << VISO_KERNEL_*) is set
 * (default: all).  Each timed region records two events on its stream. */
int viso_timing_select(viso_ctx* ctx, uint32_t kernel_mask);
int viso_timing_get(viso_ctx* ctx, int32_t kernel, int64_t* launches, double* total_ms);

/* ------------------------------------------------------------------------
 * Stage-level entry points (host buffers in/out; synchronous).  Used by the
 * parity tests; each runs the same device kernels as the frame path.
 * ---------------------------------------------------------------------- */

/* Sizes of the 4 pyramid levels: dims[2l] = w_l, dims[2l+1] = h_l;
 * w_l = (int)(w_{l-1} * 0.5) (include/keyframe.h:42-43). */
int viso_pyramid_dims(int32_t width, int32_t height, int32_t dims[8], size_t* total_bytes);

/* Keyframe::Keyframe pyramid (include/keyframe.h:28-46) for n images at once:
 * in: n * w * h bytes; out: n * total_bytes (levels concatenated). */
int viso_pyramid(viso_ctx* ctx, const uint8_t* images, int32_t n, int32_t width, int32_t height,
                 uint8_t* out);

/* cv::FAST(img, kps, thresh) with NMS (src/viso.cpp:104): row-major
 * keypoints; *n = total count (only cap written). */
int viso_fast(viso_ctx* ctx, const uint8_t* image, int32_t width, int32_t height, int32_t thresh,
              int32_t* xs, int32_t* ys, int32_t* scores, size_t cap, size_t* n);

/* OpticalFlowMultiLevel(ref, cur, kp1, kp2, success, inverse=true)
 * (src/viso.cpp:353-391): pyramids as produced by viso_pyramid. */
int viso_klt(viso_ctx* ctx, const uint8_t* ref_pyr, const uint8_t* cur_pyr, int32_t width,
             int32_t height, const float* kp1, float* kp2, uint8_t* success, int32_t n);

/* DirectPoseEstimationMultiLayer (src/viso.cpp:760-766, one GN step per
 * level as shipped).  poses: 12 doubles (R row-major, t). */
int viso_direct_pose(viso_ctx* ctx, const uint8_t* last_pyr, const uint8_t* cur_pyr,
                     int32_t width, int32_t height, const double* points, int32_t n_points,
                     const double pose_last[12], double pose_io[12]);

/* The serial Gauss-Newton step of one direct-pose level
 * (DirectPoseEstimationSingleLayer, src/viso.cpp:731-753, first iteration) on
 * given sums, by the faithful solve of the level kernels: sums[28] = the 21
 * upper-triangle entries of H (row-major), b (6), the cost sum; n_good;
 * state[7] = T21 as quaternion (x, y, z, w) and translation.  stats[50] =
 * {nGood, cost / nGood, H (36), b (6), update (6)}; state_out[7] = the new
 * T21 (the given one when the update is NaN). */
int viso_direct_solve(viso_ctx* ctx, const double sums[28], int32_t n_good, const double state[7],
                      double stats[50], double state_out[7]);

/* LKAlignment (src/viso.cpp:768-843) against n_kf keyframes. */
int viso_lk_align(viso_ctx* ctx, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf,
                  const uint8_t* cur_pyr, const double cur_pose[12], int32_t width,
                  int32_t height, const double* points, int32_t n_points, int32_t* pair_kf,
                  uint8_t* success, double* uv_before, double* uv_after);

/* Viso::PoseEstimation2d2d (src/viso.cpp:178-256) followed by SelectMotion
 * (src/viso.cpp:520-638) on normalised coordinates p1, p2 (n x 3 doubles,
 * z = 1).  Outputs: R, T (T normalised by mean depth), inliers (n),
 * points3d (n x 3; rows of outliers are zero), candidates (<= 5 x 12),
 * stats = {nr_inliers, best_motion, n_candidates, disparity_sq,
 *          e_inliers, h_inliers, e_iters, h_iters}. */
int viso_pose_2d2d(viso_ctx* ctx, const double* p1, const double* p2, int32_t n, double R[9],
                   double T[3], uint8_t* inliers, double* points3d, double* candidates,
                   double stats[8]);

/* North-star stereo stage: for each left keypoint (x, y integer pixels) find
 * the right-image column by 8x8 SAD along the same row, disparities
 * 0..max_disp (winner = smallest SAD, ties -> smallest disparity).  Outputs
 * disparity (-1 = invalid) and best SAD.  No reference counterpart. */
int viso_stereo_match(viso_ctx* ctx, const uint8_t* left, const uint8_t* right, int32_t width,
                      int32_t height, const int32_t* xs, const int32_t* ys, int32_t n,
                      int32_t max_disp, int32_t* disparity, int32_t* sad);

/* Stereo initialisation (north star: metric depth from the right image
 * replacing the 2D-2D init of Viso::PoseEstimation2d2d, src/viso.cpp:178-256
 * and the map creation of src/viso.cpp:79-96; the repo's own spec, restated in
 * oracle/oracle_stereo.cpp).  baseline > 0 enables it (metres; 0 disables):
 * while initialising, a frame given with its right image (viso_process_stereo
 * or viso_process_frames_device with d_right) runs FAST on the left image,
 * the SAD disparity of every corner (as viso_stereo_match, d in
 * 0..min(max_disp, x - 4)), keeps corners with min_disp <= d < that upper end,
 * refines d by the parabola through SAD(d-1), SAD(d), SAD(d+1) and
 * back-projects Z = fx * baseline / d.  More than 50 such points create the
 * map at once (the frame is the only keyframe, at R = I, T = 0; points in its
 * camera frame; metric scale; stats[3] = -2); otherwise the frame goes
 * through the monocular initialisation.  VISO_ERR_ARG unless
 * 1 <= min_disp < max_disp when enabled. */
int viso_set_stereo(viso_ctx* ctx, double baseline, int32_t max_disp, int32_t min_disp);

/* Stereo keyframe insertion (map maintenance the
 * reference lacks: its map is frozen after src/viso.cpp:79-96; the repo's own
 * spec, restated in oracle/oracle_viso.cpp).  With stereo enabled and
 * interval > 0: after every interval-th tracking frame whose level-0 direct-
 * pose nGood is below ngood_permille / 1000 of the map size, the frame's
 * stereo points (as viso_set_stereo, in world coordinates R^T (Pc - T) with
 * its pose) are appended to the map, the frame becomes a keyframe (LK
 * alignment may pair points with it) and stats[14] = points added;
 * stats[15] = keyframes.  At most 8 keyframes and 16384 map points.  Each
 * check is one host synchronisation.  interval 0 (default) = off, the
 * reference's frozen map. */
int viso_set_keyframes(viso_ctx* ctx, int32_t interval, int32_t ngood_permille);

/* Monocular keyframe insertion (the repo's own spec, restated in
 * tests/mono_kf_ref.py; DESIGN.md §Monocular keyframe insertion): the map of
 * src/viso.cpp:79-96 grows without a right image, by the two-view
 * triangulation the reference sketches in Viso::Reconstruct
 * (src/viso.cpp:434-501) and never calls.  The schedule and the gate are
 * those of viso_set_keyframes: after every interval-th tracking frame c whose
 * level-0 nGood is below ngood_permille / 1000 of the map size, with fewer
 * than 8 keyframes, against the latest keyframe k:
 *  - the map points that project into c mark their cell of a grid of
 *    cell x cell pixels; every unmarked cell keeps its FAST corner
 *    (src/viso.cpp:104, fast_thresh) with the highest score;
 *  - the winners are tracked into k by OpticalFlowMultiLevel
 *    (src/viso.cpp:353-391, inverse), seeded by the rotation-only warp
 *    K R_kc K^-1, R_kc = R_k R_c^T;
 *  - each track is triangulated (Viso::Triangulate, src/viso.cpp:393-431)
 *    for the known motion [R_kc | t_k - R_kc t_c] and kept when both depths
 *    are positive, both reprojection errors (src/viso.cpp:476-497) are within
 *    projection_error_thresh and the parallax angle at the point is at least
 *    min_parallax_deg (the reference's disabled block, src/viso.cpp:458-474,
 *    rejects such points instead).
 * The kept points are appended in world coordinates (up to 16384 map points),
 * c becomes a keyframe, viso_set_bundle_adjust's BA runs if it is on, and
 * stats[14] = points added, stats[15] = keyframes; when no point is kept no
 * keyframe is made.  Each check is one host synchronisation, an insertion one
 * more (the count of kept points).  interval 0 (default) = off.
 * VISO_ERR_ARG unless 8 <= cell <= 64 and 0 <= min_parallax_deg < 90;
 * VISO_ERR_STATE while viso_set_keyframes is on (and viso_set_keyframes with
 * interval > 0 returns VISO_ERR_STATE while this is on). */
int viso_set_mono_keyframes(viso_ctx* ctx, int32_t interval, int32_t ngood_permille, int32_t cell,
                            double min_parallax_deg);
/* Stage entry (parity tests): the new points of one such insertion on host
 * data, by the launches of the frame path.  cur_pyr, kf_pyr: the pyramids of
 * c and k (as viso_klt takes them); pose_c, pose_k: their Tcw poses; points:
 * n_points x 3 world (the map; 0..16384).  Outputs: new_points (world; *n =
 * the number kept, only the first cap written, as viso_fast), winners_xy
 * (x, y per cell winner in corner order) and accept (1 = kept) for
 * ceil(width / cell) * ceil(height / cell) entries at most (either may be
 * NULL), counts = {corners, winners, KLT successes, kept}. */
int viso_mono_points(viso_ctx* ctx, const uint8_t* cur_pyr, const uint8_t* kf_pyr, int32_t width,
                     int32_t height, const double pose_c[12], const double pose_k[12],
                     const double* points, int32_t n_points, int32_t cell, double min_parallax_deg,
                     double* new_points, int32_t* winners_xy, uint8_t* accept, size_t cap, size_t* n,
                     int32_t counts[4]);

/* Sliding-window map (the repo's own spec, restated in
 * tests/map_window_ref.py; DESIGN.md §Sliding-window map): the map follows the
 * camera instead of filling up.  With window > 0, an insertion check (stereo
 * or monocular, their schedule and gate) is made while the map holds at most
 * `window` keyframes; one that passes its gate with exactly `window` of them
 * first retires the oldest keyframe (index 0), with c the check frame:
 *  - a pose "sees" a point P when Pc = R P + t has Pc.z > 0 and its
 *    projection (u, v) lies in [0, width) x [0, height); P's cell in c is
 *    (int(u / cell), int(v / cell));
 *  - points hosted by another keyframe stay (host - 1) and, where c sees
 *    them, mark their cell;
 *  - a point hosted by the retired keyframe is a candidate when c sees it in
 *    an unmarked cell and at least one remaining keyframe sees it; of a
 *    cell's candidates the one with the highest index survives, hosted by the
 *    newest remaining keyframe that sees it; every other such point is culled;
 *  - kept points keep their order, the keyframe poses move down one index.
 * If nothing would be kept the retirement is abandoned and that check inserts
 * nothing.  Otherwise the check's insertion follows against the culled map.
 * A retirement is one more host synchronisation.  window 0 (default) = off:
 * at most 8 keyframes, nothing leaves the map.  VISO_ERR_ARG unless
 * window == 0, or 2 <= window <= 8 and 8 <= cell <= 64; VISO_ERR_STATE when
 * the map already holds more than `window` keyframes. */
int viso_set_map_window(viso_ctx* ctx, int32_t window, int32_t cell);
/* info = {window, cell, keyframes retired, points culled, and of the last
 * retirement: the number of frames processed before its check frame (-1: no
 * retirement yet), the points its keyframe hosted, the survivors among them,
 * the map size after it}. */
int viso_get_map_window(viso_ctx* ctx, int64_t info[8]);
/* Every map point's host keyframe (an index into viso_get_keyframe_poses; the
 * array the BA is given): the first min(cap, points) are written; *n = the
 * point count. */
int viso_get_point_hosts(viso_ctx* ctx, int32_t* host, size_t cap, size_t* n);
/* Stage entry (parity tests): one retirement on host data, by the launches of
 * the frame path.  pose_c: the check frame's Tcw; kf_poses: n_kf x 12
 * (1..8), keyframe 0 the one retired; points: n x 3 world (0..16384); host: n
 * indices in [0, n_kf).  Outputs: keep (n flags), out_points / out_host (the
 * kept points in order with their new hosts; room for n), *n_out = the number
 * kept, counts = {hosted by keyframe 0, of those seen by c, candidates,
 * survivors}.  VISO_ERR_ARG on any out-of-range argument. */
int viso_map_retire(viso_ctx* ctx, int32_t width, int32_t height, const double pose_c[12],
                    const double* kf_poses, int32_t n_kf, const double* points, const int32_t* host,
                    int32_t n, int32_t cell, double* out_points, int32_t* out_host, uint8_t* keep,
                    size_t* n_out, int32_t counts[4]);

/* Pose refinement (the repo's own spec, restated in tests/pose_refine_ref.py;
 * DESIGN.md §Pose refinement): the third step of a semi-direct VO.  The
 * reference computes, for every map point, the position at which its keyframe
 * patch is found in the current image (LKAlignment, src/viso.cpp:121) and only
 * draws it (src/viso.cpp:123-135).  With iterations > 0 every tracking frame's
 * direct pose X is refined on those positions before anything reads it:
 *  - point i is an observation when pair_kf[i] >= 0, success[i] != 0 and
 *    |uv_after_i - uv_before_i|^2 <= max_shift_px^2 (the frame's LK row, as
 *    viso_get_alignment gives it; computed at X);
 *  - pass k = 0..iterations at T_k (T_0 = X): for every observation with
 *    Pc.z > 0 the residual r = uv_after - projection, e = |r|, the 2x6 Jacobian
 *    of dPixeldXi (src/viso.cpp:640-658), the Huber weight w = 1 (e <= huber_px)
 *    or huber_px / e, rho = e^2 / 2 or huber_px (e - huber_px / 2); n_k the
 *    observations used, cost_k = sum rho, H = sum w J^T J, b = sum w J^T r;
 *  - in this order: n_0 < 6 -> X, status 1; for k >= 1, cost_k >= cost_{k-1}
 *    -> T_{k-1}, status 3; k == iterations -> T_k, status 0; xi = H^-1 b not
 *    finite -> T_k, status 2; else T_{k+1} = exp(xi) T_k.
 * The refined pose replaces X in viso_get_poses, seeds the next frame's direct
 * pose and is what a keyframe insertion, the BA and a retirement see;
 * viso_get_alignment still reports the alignment computed at X.  One more
 * launch per tracking frame; the frame's LK alignment runs at once on the
 * context stream (no background or batched alignment while it is on).  fp64 in
 * both precision modes.  iterations 0 (default) = off.  VISO_ERR_ARG unless
 * iterations == 0, or 1 <= iterations <= 20, huber_px > 0 and
 * max_shift_px > 0.  May be set while tracking: the next frame sees it. */
int viso_set_pose_refine(viso_ctx* ctx, int32_t iterations, double huber_px, double max_shift_px);
/* The last refined frame's report = {observations, steps applied, cost_0,
 * cost at the result, inliers (e <= huber_px) at the result, status, rms of e
 * at T_0, rms at the result}; all NaN before the first refinement. */
int viso_get_pose_refine(viso_ctx* ctx, double report[8]);
/* Stage entry (parity tests): one refinement on host data, by the launch of
 * the frame path, with the context's intrinsics.  points: n x 3 world
 * (0..16384); pair_kf, success, uv_before, uv_after: the LK row (n; uv n x 2).
 * VISO_ERR_ARG on any out-of-range or NULL argument. */
int viso_refine_pose(viso_ctx* ctx, const double* points, const int32_t* pair_kf, const uint8_t* success,
                     const double* uv_before, const double* uv_after, int32_t n, const double pose_in[12],
                     int32_t iterations, double huber_px, double max_shift_px, double pose_out[12],
                     double report[8]);

/* Map point culling (the repo's own spec, restated in
 * tests/point_cull_ref.py; DESIGN.md §Map point culling): a point whose
 * keyframe patch keeps not being found leaves the map.  The reference computes
 * the alignment of every map point in every tracking frame (LKAlignment,
 * src/viso.cpp:768-843) and only draws it.  With interval > 0 every map point
 * has a track record of four int32 {age, seen, found, fail_run}, zero when the
 * point enters the map (initialisation, an insertion) and when the mode is
 * switched on.
 *  - Update, once per tracking frame, behind the frame's LK alignment (and its
 *    refinement, viso_set_pose_refine), ahead of the insertion check, with the
 *    frame's final pose T (as viso_get_poses) and its LK row (as
 *    viso_get_alignment): age + 1; with pair_kf < 0 nothing else; otherwise
 *    seen + 1 and the observation is good when success != 0, Pc = R P + t has
 *    Pc.z > 0 and |uv_after - projection of Pc|^2 <= reproj_px^2; good:
 *    found + 1, fail_run = 0; else fail_run + 1.
 *  - Cull, on every interval-th tracking frame right behind its update: the
 *    points with fail_run >= max_fail_run are candidates.  With none nothing
 *    happens; when fewer than min_points would survive the cull is abandoned
 *    (map and records unchanged); otherwise the survivors keep their order,
 *    coordinates, hosts and records, the keyframes stay (also one that hosts
 *    no point) and the LK templates are rebuilt.  The same frame's insertion
 *    check sees the culled map.
 * A retirement (viso_set_map_window) carries the kept points' records; the BA
 * moves coordinates only.  One more launch per tracking frame, the frame's LK
 * alignment at once on the context stream (no background or batched alignment
 * while it is on); a cull frame is one more host synchronisation.  interval 0
 * (default) = off.  VISO_ERR_ARG unless interval == 0, or interval >= 1,
 * 1 <= max_fail_run <= 1000, reproj_px > 0 and 1 <= min_points <= 16384.  May
 * be set while tracking: the next frame sees it. */
int viso_set_point_cull(viso_ctx* ctx, int32_t interval, int32_t max_fail_run, double reproj_px,
                        int32_t min_points);
/* info = {interval, max_fail_run, culls applied, points culled in all, culls
 * abandoned, and of the last applied cull: the number of frames processed
 * before its frame (-1: none yet), the points it removed, the map size after
 * it}. */
int viso_get_point_cull(viso_ctx* ctx, int64_t info[8]);
/* Every map point's track record (4 int32 each): the first min(cap, points)
 * rows are written; *n = the point count.  VISO_ERR_STATE when the mode is
 * off. */
int viso_get_point_tracks(viso_ctx* ctx, int32_t* tracks4, size_t cap, size_t* n);
/* Stage entry (parity tests): one update on host data, by the launch of the
 * frame path, with the context's intrinsics.  points: n x 3 world (0..16384);
 * pair_kf, success, uv_after: the LK row (n; uv n x 2); tracks4: n x 4, in and
 * out; counts = {paired, good, failed, the longest fail_run after the update}.
 * VISO_ERR_ARG on any out-of-range or NULL argument. */
int viso_point_tracks_update(viso_ctx* ctx, const double* points, const int32_t* pair_kf, const uint8_t* success,
                             const double* uv_after, int32_t n, const double pose[12], double reproj_px,
                             int32_t* tracks4, int32_t counts[4]);
/* Stage entry (parity tests): one cull on host data, by the launch of the
 * frame path.  points: n x 3 (0..16384); host: n; tracks4: n x 4;
 * 1 <= max_fail_run <= 1000, 0 <= min_points <= 16384.  Outputs: keep (n
 * flags), out_points / out_host / out_tracks4 (the kept rows in order; room
 * for n), *n_out = the number kept, counts = {candidates, survivors = n -
 * candidates, n_out, abandoned}.  On abandonment *n_out = n, the outputs equal
 * the inputs and every keep is 1.  VISO_ERR_ARG on any out-of-range or NULL
 * argument. */
int viso_points_cull(viso_ctx* ctx, const double* points, const int32_t* host, const int32_t* tracks4, int32_t n,
                     int32_t max_fail_run, int32_t min_points, double* out_points, int32_t* out_host,
                     int32_t* out_tracks4, uint8_t* keep, size_t* n_out, int32_t counts[4]);

/* Point refinement (the repo's own spec, restated in
 * tests/point_refine_ref.py; DESIGN.md §Point refinement): the structure half
 * of the "pose and structure refinement" on the LK-aligned positions, which
 * the reference only draws.  A point's LK template is its anchor keyframe's
 * patch at the point's projection there, so the aligned positions measure the
 * depth along the ray from the anchor's centre C through the point: the
 * refinement moves P along that ray and nothing else (its projection in the
 * anchor, the templates and its identity stay).
 *  - Record, once per tracking frame, behind the frame's LK alignment, its pose
 *    refinement and its track update, with the frame's final pose (as
 *    viso_get_poses) and its LK row (as viso_get_alignment), into slot
 *    count % window of an observation ring, count + 1: point i is flagged when
 *    pair_kf >= 0, success != 0 and |uv_after - uv_before|^2 <= max_shift_px^2;
 *    the stored uv is uv_after.  count = 0 whenever the LK templates are
 *    rebuilt (map creation, an insertion, a retirement, an applied cull) and
 *    when the mode is switched on (or its window changed); the live slots are
 *    the first min(count, window).
 *  - Refinement, on every interval-th tracking frame right behind its record,
 *    ahead of the cull and the insertion check, per point: a = the template's
 *    keyframe; a < 0 -> status 5.  Fewer than min_obs flagged live slots ->
 *    status 1.  Pass k = 0..iterations at P_k (P_0 = P), D = P_k - C: per
 *    flagged live slot with Pc = R_s P_k + t_s, Pc.z > 0: r = uv - projection,
 *    e = |r|, the Huber weight and rho of viso_set_pose_refine, g = the
 *    projection's derivative along -D; H = sum w g.g, b = sum w g.r, cost =
 *    sum rho, each the pairwise tree over slots 0..7.  In this order: k = 0 and
 *    fewer than min_obs slots used -> status 1; k = 0 and H max_rel_sigma^2 < 1
 *    (a 1 px error moves the depth by more than max_rel_sigma, relative) ->
 *    status 4; k >= 1 and cost_k >= cost_{k-1} -> P_{k-1}, status 3;
 *    k = iterations -> P_k, status 0; delta = b / H not finite or 1 + delta
 *    outside (0.5, 2) -> P_k, status 2; else P_{k+1} = C + D / (1 + delta).
 * The cull, the insertion check, the BA and the next frame see the refined
 * points; no template rebuild follows.  Two more launches on a refinement
 * frame, one on the others, no host synchronisation; the frame's LK alignment
 * runs at once on the context stream (no background or batched alignment while
 * it is on).  fp64 in both precision modes.  interval 0 (default) = off.
 * VISO_ERR_ARG unless interval == 0, or interval >= 1, 2 <= window <= 8,
 * 1 <= iterations <= 10, huber_px > 0, max_shift_px > 0, 1 <= min_obs <=
 * window, 0 < max_rel_sigma <= 1, all finite.  May be set while tracking: the
 * next frame sees it. */
int viso_set_point_refine(viso_ctx* ctx, int32_t interval, int32_t window, int32_t iterations, double huber_px,
                          double max_shift_px, int32_t min_obs, double max_rel_sigma);
/* info = {interval, window, refinements run, points moved in all, and of the
 * last refinement: the number of frames processed before its frame (-1: none
 * yet), its eligible points (an anchor and min_obs flagged slots), the points
 * it moved (steps >= 1), its status-4 points}. */
int viso_get_point_refine(viso_ctx* ctx, int64_t info[8]);
/* The last refinement's status and kept steps per point (of the map it ran
 * on): the first min(cap, points) are written; *n = that map's point count (0:
 * no refinement yet).  VISO_ERR_STATE when the mode is off. */
int viso_get_point_refine_status(viso_ctx* ctx, uint8_t* status, uint8_t* steps, size_t cap, size_t* n);
/* Stage entry (parity tests): one frame's record on host data, by the launch
 * of the frame path.  The LK row (n, 0..16384; uv n x 2); valid_out: n flags;
 * uv_out: n x 2.  VISO_ERR_ARG on any out-of-range or NULL argument. */
int viso_point_obs_record(viso_ctx* ctx, const int32_t* pair_kf, const uint8_t* success, const double* uv_before,
                          const double* uv_after, int32_t n, double max_shift_px, uint8_t* valid_out,
                          double* uv_out);
/* Stage entry (parity tests): one refinement on host data, by the launch of
 * the frame path, with the context's intrinsics.  points: n x 3 world
 * (0..16384); anchor_kf: n keyframe indices (< n_kf; < 0: none); kf_poses:
 * n_kf x 12 (1..8); frame_poses: m x 12, the live slots (1..8); obs_valid:
 * m x n; obs_uv: m x n x 2; 1 <= iterations <= 10, huber_px > 0,
 * 1 <= min_obs <= 8, 0 < max_rel_sigma <= 1.  Outputs: out_points (n x 3),
 * status, steps (n each), costs (n x 2: cost_0 and the cost at the result; 0
 * where no pass ran), counts = {eligible, moved, status 4, status 2}.
 * VISO_ERR_ARG on any out-of-range or NULL argument. */
int viso_points_refine(viso_ctx* ctx, const double* points, const int32_t* anchor_kf, int32_t n,
                       const double* kf_poses, int32_t n_kf, const double* frame_poses, int32_t m,
                       const uint8_t* obs_valid, const double* obs_uv, int32_t iterations, double huber_px,
                       int32_t min_obs, double max_rel_sigma, double* out_points, uint8_t* status, uint8_t* steps,
                       double* costs, int32_t counts[4]);

/* Warped LK alignment (the repo's own spec; no reference
 * counterpart).  LKAlignment's template is the unwarped 8x8 patch of the
 * point's anchor keyframe at the current image's pyramid level, which stops
 * being found as the patch's scale or orientation changes.  With mode 1 every
 * tracking frame's alignment first forms, per map point, the affine map A
 * (anchor level 0 -> current level 0) that the point's depth in the anchor
 * and the two poses imply (finite differences of 4 px on the plane z = depth
 * of the anchor camera), takes the template of every level through A^-1 from
 * the pyramid level r = l + shift of the anchor that matches its scale
 * (|det A| > 3: one level coarser per factor 4; < 1/3: finer), and then runs
 * LKAlignmentSingle's iterations unchanged, the bounds test on the current
 * coordinates.  A warp whose area ratio |det A| is outside
 * [1 / max_area_ratio, max_area_ratio], that is not finite, or whose plane
 * points are not in front of both cameras is rejected: the point counts as
 * paired and not aligned, uv_after = uv_before.  A level whose template taps
 * leave the reference level is skipped.  fp64 in both precision modes.
 * mode 0 = off (default): nothing changes.  mode: 0 or 1; max_area_ratio in
 * [4, 64] (64 suggested); anything else VISO_ERR_ARG.  May be called while
 * tracking (pending work is settled first).  While on, LK alignment runs as
 * batched launches of the warped kernel (VISO_KERNEL_LKWARP) instead of the
 * chunk-resident grid. */
int viso_set_lk_warp(viso_ctx* ctx, int32_t mode, double max_area_ratio);
/* info = {mode, frames aligned with the mode on, then of the last frame's row:
 * points paired, aligned (success), rejected warps (status 2), points with
 * shift < 0, with shift > 0, skipped levels summed over the points}. */
int viso_get_lk_warp(viso_ctx* ctx, int64_t info[8]);
/* The last frame's warp rows, as viso_get_alignment returns its LK row: A4
 * (n x 4: A00, A01, A10, A11), shift (n), status (n): 0 aligned through the
 * warp, 1 not paired (out of view or no keyframe), 2 warp rejected; bits 4-6
 * the number of skipped levels.  The first min(cap, n) are written; *n = the
 * row's points.  VISO_ERR_STATE while the mode is off. */
int viso_get_lk_warp_rows(viso_ctx* ctx, double* A4, int8_t* shift, uint8_t* status, size_t cap, size_t* n);
/* Stage entry (parity tests): viso_lk_align's arguments and outputs by the
 * warped kernel, plus max_area_ratio and the three warp outputs. */
int viso_lk_align_warped(viso_ctx* ctx, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf,
                         const uint8_t* cur_pyr, const double cur_pose[12], int32_t width, int32_t height,
                         const double* points, int32_t n_points, double max_area_ratio, int32_t* pair_kf,
                         uint8_t* success, double* uv_before, double* uv_after, double* A4, int8_t* shift,
                         uint8_t* status);

/* Illumination-invariant LK alignment (the repo's own spec; no
 * reference counterpart): a form of the warped alignment that removes a
 * per-patch affine brightness change (gain, offset) between the keyframe
 * patch and the current image, by the project-out form of the inverse-
 * compositional iterations: per level the Jacobian is projected off
 * span{1, T}, H stays constant, and the cost is the energy of the residual
 * with its mean and its component along the centred template removed.  A
 * level whose template is flat (sum of squared deviations < 64) is skipped as
 * a level whose taps leave the reference level.  After level 0 an aligned
 * point's gain has to lie in [1 / max_gain, max_gain]; one outside gets
 * success 0 and status 3 (uv_after stays where the iterations ended).  fp64 in
 * both precision modes.  It runs while viso_set_lk_warp is on; with the warp
 * off the mode is kept, inert (nothing is launched or allocated for it).
 * mode 0 = off (default): nothing changes.  mode: 0 or 1; max_gain finite, in
 * [1.5, 16] (4 suggested); anything else VISO_ERR_ARG.  May be called while
 * tracking (pending work is settled first).  Frames are timed under
 * VISO_KERNEL_LKWARP. */
int viso_set_lk_illum(viso_ctx* ctx, int32_t mode, double max_gain);
/* info = {mode, frames aligned with the mode on, then of the last frame's row:
 * points paired, aligned (success), points whose gain was out of bounds
 * (status 3), 0, 0, 0}.  All 0 while the mode or the warp is off. */
int viso_get_lk_illum(viso_ctx* ctx, int64_t info[8]);
/* The last frame's gain/offset rows (n x 2 doubles): the last accepted
 * level-0 iteration's (gain, offset), current = gain * keyframe + offset; NaN
 * where there was none.  The first min(cap, n) are written; *n = the row's
 * points.  VISO_ERR_STATE while the mode is off or the warp is off. */
int viso_get_lk_illum_rows(viso_ctx* ctx, double* gain_offset2, size_t cap, size_t* n);
/* Stage entry (parity tests): viso_lk_align_warped's arguments and outputs by
 * the illumination-invariant form, plus max_gain and gain_offset (n x 2).  A4,
 * shift, status and gain_offset may each be NULL. */
int viso_lk_align_illum(viso_ctx* ctx, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf,
                        const uint8_t* cur_pyr, const double cur_pose[12], int32_t width, int32_t height,
                        const double* points, int32_t n_points, double max_area_ratio, double max_gain,
                        int32_t* pair_kf, uint8_t* success, double* uv_before, double* uv_after, double* A4,
                        int8_t* shift, uint8_t* status, double* gain_offset);

/* Depth seeds (the repo's own spec; no reference counterpart):
 * the map grows by an epipolar search over the frames after a keyframe.  A
 * seed is a corner (u, v) of keyframe h (level 0) with an inverse depth mu of
 * z in h's camera and its variance s2, the counters good, bad and lost and the
 * status of its last update.  With rho_min = 1 / depth_max and rho_max =
 * 1 / depth_min a new seed has mu = (rho_min + rho_max) / 2, s2 =
 * ((rho_max - rho_min) / 4)^2 and counters 0.  The three stages below run on
 * host data through the launches a frame path uses (VISO_KERNEL_SEEDS); a seed
 * row travels as h (int32), uv (2 doubles), mu, s2 and counters (4 int32:
 * good, bad, lost, status).  At most 8192 seeds.  fp64 in both precision
 * modes.  Every out-of-range or NULL argument returns VISO_ERR_ARG.
 *
 * viso_set_depth_seeds switches the mode on in the frame path (interval >= 1;
 * 0 = off, the default: nothing changes, and the other arguments are not
 * read).  A seed set is created (see Creation below, with `cell`) whenever a
 * keyframe is created: at map creation (of the latest keyframe), at a stereo
 * and at a monocular insertion, behind that step's own points.  Every tracking
 * frame updates every seed at the frame's final pose (after the pose
 * refinement, where that is on).  Every interval-th tracking frame, behind
 * that frame's update and ahead of the cull and the insertion check, the
 * converged seeds are appended to the map (host = h, a zero track record; the
 * LK templates are rebuilt when any was appended) and the failed ones are
 * dropped (see Promotion below).  A retirement (viso_set_map_window) drops the
 * retired keyframe's seeds and renumbers the others' h.  While on, frames are
 * finished one by one, as with keyframe insertion.  8 <= cell <= 64, 8 <=
 * max_steps <= 64, 0 < depth_min < depth_max, max_score > 0, uniqueness >= 1,
 * 1 <= min_good <= 1000, 0 < conv_rel <= 1, 1 <= max_bad, max_lost <= 1000,
 * every value finite.  May be called while tracking (pending work is settled
 * first); switching off frees the seeds. */
int viso_set_depth_seeds(viso_ctx* ctx, int32_t interval, int32_t cell, int32_t max_steps, double depth_min,
                         double depth_max, double max_score, double uniqueness, int32_t min_good, double conv_rel,
                         int32_t max_bad, int32_t max_lost);
/* info = {interval, live seeds, seeds created in all, promoted in all, dropped
 * in all (failed or retired with their keyframe), then of the live seeds by
 * the status of their last update: status 0, status 7-9, status 1-6 (a seed no
 * update has seen yet is not counted)}.  All 0 while the mode is off. */
int viso_get_depth_seeds(viso_ctx* ctx, int64_t info[8]);
/* The live seeds' rows: the first min(cap, n) are written (any output may be
 * NULL); *n = the live seeds.  VISO_ERR_STATE while the mode is off. */
int viso_get_depth_seed_rows(viso_ctx* ctx, int32_t* h, double* uv, double* mu, double* s2, int32_t* counters,
                             size_t cap, size_t* n);
/*
 * Creation: the seeds a new keyframe adds.  The map (points, n_points, world)
 * projected by pose marks the occupancy grid of `cell` (8..64) pixels as a
 * monocular insertion does; the cell winners of the level-0 image's FAST
 * corners (the context's fast_thresh and max_features) in the unmarked cells
 * become seeds of keyframe `host` in corner order, as many as 8192 - n_live.
 * The first min(cap, appended) rows are written; *n = the seeds appended,
 * counts = {cell winners, seeds appended}. */
int viso_depth_seeds_create(viso_ctx* ctx, const uint8_t* image, int32_t width, int32_t height, const double pose[12],
                            const double* points, int32_t n_points, int32_t cell, int32_t host, double depth_min,
                            double depth_max, int32_t n_live, int32_t* h, double* uv, double* mu, double* s2,
                            int32_t* counters, size_t cap, size_t* n, int32_t counts[2]);
/* Update: one frame (cur_pyr, cur_pose) against n seeds hosted on the n_kf
 * keyframes (kf_pyrs, kf_poses; every h in [0, n_kf)).  Per seed the segment
 * mu +- 2 sigma of its epipolar line, clipped to [rho_min, rho_max], is
 * searched at the finest pyramid level that holds it in max_steps (8..64)
 * one-pixel steps, for the host patch warped by the affine map of DESIGN.md
 * §17 (zero-mean sum of squared differences over the 8x8 patch); the best
 * step, refined by a parabola, gives an inverse depth that is fused into (mu,
 * s2).  status: 0 fused (good += 1); 1 behind the camera or out of view, 2
 * warp rejected, 5 template outside the host level, 6 fewer than 3 steps
 * inside the image (lost += 1 each); 3 segment longer than max_steps at level
 * 3, 4 shorter than one pixel (nothing changes); 7 best score above max_score,
 * 8 best score x uniqueness above the best score two or more steps away, 9
 * depth out of range (bad += 1 each); 0 and 7..9 set lost = 0.  mu, s2 and
 * counters are updated in place; level_step (may be NULL) receives per seed
 * the search level and the best step (-1 where not reached).  0 < depth_min <
 * depth_max, max_score > 0, uniqueness >= 1, all finite. */
int viso_depth_seeds_update(viso_ctx* ctx, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf,
                            const uint8_t* cur_pyr, const double cur_pose[12], int32_t width, int32_t height,
                            int32_t n, int32_t max_steps, double depth_min, double depth_max, double max_score,
                            double uniqueness, const int32_t* h, const double* uv, double* mu, double* s2,
                            int32_t* counters, int32_t* level_step);
/* Promotion.  In seed order: a seed with good >= min_good and s2 <=
 * (conv_rel mu)^2 has converged; otherwise one with bad >= max_bad or lost >=
 * max_lost is dropped.  The first `room` converged seeds become the world
 * points R_h^T (f / mu - t_h) (points, hosts: min(room, n) rows of space);
 * every seed neither promoted nor dropped survives, and the survivors' rows
 * are written back compacted in order.  counts = {converged, promoted,
 * dropped, survivors}.  1 <= min_good, max_bad, max_lost <= 1000, 0 <
 * conv_rel <= 1, 0 <= room <= 16384. */
int viso_depth_seeds_promote(viso_ctx* ctx, const double* kf_poses, int32_t n_kf, int32_t n, int32_t min_good,
                             double conv_rel, int32_t max_bad, int32_t max_lost, int32_t room, int32_t* h, double* uv,
                             double* mu, double* s2, int32_t* counters, double* points, int32_t* hosts,
                             int32_t counts[4]);

/* Relocalisation (the repo's own spec; no reference
 * counterpart): a lost pose is recovered by direct alignment to the keyframes.
 *
 * viso_kf_align is one attempt on host data, through the launches of the frame
 * path (VISO_KERNEL_RELOC).  kf_pyrs: n_kf (1..8) pyramids, kf_poses: n_kf x
 * 12 (Tcw); cur_pyr: the current frame's pyramid; points: n_points x 3 world,
 * 0 <= n_points <= 16384; the context's intrinsics.  Candidate c =
 * (1 + n_extra) k + s (at most 16) aligns keyframe k to the current frame from
 * k's own pose (s = 0) or from extra_seed12 (s = 1; n_extra in {0, 1},
 * extra_seed12 NULL when 0), over the first max_points (64..1024) map points
 * keyframe k sees (depth > 0, level-0 projection inside the image), in map
 * order (m of them; m < 6: status 1, the pose out is the seed).  Levels 3..0,
 * each from the result of the level above; pass j = 0..iterations (1..20) at
 * T_j sums the direct pose's 28 terms of every good point (both 8x8 patches
 * inside the level, depth > 0 in both cameras; n_j of them), cost_j = the
 * squared-error sum / n_j, and then, in this order: n_j < 6 or cost_j not
 * finite keeps T_j (exit 4, j = 0: no cost) or T_{j-1} (exit 5); cost_j >=
 * cost_{j-1} keeps T_{j-1} (exit 1); 1 - cost_j / cost_{j-1} < 0.005 keeps T_j
 * (exit 2); j = iterations keeps T_j (exit 0); a non-finite step H^-1 b keeps
 * T_j (exit 3); otherwise T_{j+1} = exp(step) T_j.  Status, from level 0's
 * result (n points, cost): 2 level 0 ended with exit 4; 3 n * 1000 <
 * min_good_permille (1..1000) * m; 4 not (cost <= max_cost) (max_cost > 0);
 * 0 accepted.  poses_out: n_cand x 12; report: n_cand x 20 = {status, m, n,
 * cost, then for levels 3, 2, 1, 0: exit (-1: not run), steps applied, n,
 * cost}, the cost NaN where there is none; *winner = the accepted candidate of
 * the least cost (ties: the lowest index), -1 when none.  fp64 in both
 * precision modes.  Every out-of-range or NULL argument returns VISO_ERR_ARG. */
int viso_kf_align(viso_ctx* ctx, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf, const uint8_t* cur_pyr,
                  int32_t width, int32_t height, const double* points, int32_t n_points, const double* extra_seed12,
                  int32_t n_extra, int32_t iterations, int32_t max_points, double max_cost, int32_t min_good_permille,
                  double* poses_out, double* report, int32_t* winner);
/* The mode in the frame path.  lost_after = 0 (default): off, nothing changes
 * and the other arguments are not read.  On (lost_after 1..1000, lk_permille
 * 0..1000, the rest as viso_kf_align's) frames are finished one by one, as with
 * keyframe insertion, and every tracking frame is judged right behind its
 * final solve and LK row (one host sync): it is bad when not (level-0 cost <=
 * max_cost), when level-0 nGood * 1000 < min_good_permille * map points, or
 * when lk_permille > 0 and LK successes * 1000 < lk_permille * LK pairs.  A
 * good frame's pose becomes the last good pose.  lost_after consecutive bad
 * frames lose the context, from the last of them on.  Every lost frame runs no
 * direct pose and no LK alignment of its own but one attempt: all keyframes,
 * extra seed = the last good pose.  No winner: the frame is logged with the
 * last good pose (status 2, a NaN frame-log row).  A winner: the frame takes
 * its pose (status 3), its LK alignment runs at that pose, the pose becomes the
 * last good pose and tracking goes on from it.  Lost and recovered frames skip
 * everything a tracking frame does behind its LK alignment (pose refinement,
 * track records, observation ring, seeds, cull, insertion check) and do not
 * count as tracking frames there.  The state stays VISO_STATE_RUNNING.  May be
 * called while tracking (pending work is settled first). */
int viso_set_relocalise(viso_ctx* ctx, int32_t lost_after, double max_cost, int32_t min_good_permille,
                        int32_t lk_permille, int32_t iterations, int32_t max_points);
/* info = {lost_after, lost now (0/1), losses in all, attempts in all,
 * recoveries in all, then of the last attempt: frames processed before its
 * frame (-1: none), its winner (-1: none), its candidates}. */
int viso_get_relocalise(viso_ctx* ctx, int64_t info[8]);
/* The last attempt's candidate rows, as viso_kf_align returns them: the first
 * min(cap, n) are written (either output may be NULL); *n = its candidates (0
 * before the first attempt).  VISO_ERR_STATE while the mode is off. */
int viso_get_relocalise_report(viso_ctx* ctx, double* poses, double* report, size_t cap, size_t* n);
/* One byte per pose index, as viso_get_poses counts them: 0 tracked, 1 tracked
 * with a bad verdict, 2 lost (the pose is the held one), 3 recovered.  All 0
 * with the mode off.  The first min(cap, n) are written; *n = the poses. */
int viso_get_frame_status(viso_ctx* ctx, uint8_t* status, size_t cap, size_t* n);

/* The keyframe alignment with an affine brightness map per candidate (the
 * repo's own spec, restated in tests/kf_align_illum_ref.py):
 * viso_kf_align, with every candidate's state (T, g, o) in place of T — (seed,
 * 1, 0) on level 3, each lower level from the state the level above kept.
 * Points, good points, levels, passes, the order of the sums across points
 * (list position p into accumulator p mod 16, the 16 added neighbours first)
 * and the report are viso_kf_align's.  Per good point: R = the keyframe's
 * sample, C = the current frame's, e = (g_j R + o_j) - C, and the 44 terms of
 * viso_track_affine (below) with keyframe k's level as "last" and keyframe k's
 * pose as L; d11 = 64 n_j.  The step is viso_track_affine's: (g, o) eliminated
 * by the explicit 2x2 inverse, viso_kf_align's 6x6 solve on A' and b', then dg
 * and do.  The decisions are viso_kf_align's with (T, g, o) for T: exits 1 and
 * 5 restore pass j - 1's g and o too, and exit 3 is also taken when dg or do is
 * not finite (a constant keyframe patch set: det = 0).  Status, from level 0's
 * result, in this order: 2; 3; 5 not (1 / max_gain <= g <= max_gain) (max_gain
 * finite, > 1: a foreign frame is otherwise explained by g -> 0); 4; 0.  The
 * cost is the compensated residual at the current frame's scale, so it scales
 * with g^2; max_cost keeps its meaning.  gain_offset: n_cand x 2, the kept g
 * and o ((1, 0) when m < 6).  fp64 in both precision modes.  Every out-of-range
 * or NULL argument returns VISO_ERR_ARG. */
int viso_kf_align_illum(viso_ctx* ctx, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf,
                        const uint8_t* cur_pyr, int32_t width, int32_t height, const double* points, int32_t n_points,
                        const double* extra_seed12, int32_t n_extra, int32_t iterations, int32_t max_points,
                        double max_cost, int32_t min_good_permille, double max_gain, double* poses_out, double* report,
                        double* gain_offset, int32_t* winner);
/* The form in the frame path.  mode 0 (default): off, max_gain is not read,
 * nothing is launched or allocated.  mode 1: while viso_set_relocalise is on,
 * every attempt of a lost frame (the first one and the one behind
 * viso_set_reloc_seed's stage) runs as viso_kf_align_illum with this max_gain;
 * the verdict, the bad run, the held pose, the pose-log and frame-log rows and
 * viso_get_relocalise_report are unchanged.  With the relocalisation off the
 * mode is kept, inert.  May be called while tracking (pending work is settled
 * first). */
int viso_set_reloc_illum(viso_ctx* ctx, int32_t mode, double max_gain);
/* info = {mode, attempts run in this form, recoveries through it, the last
 * such attempt's winner (-1: none), 0, 0, 0, 0}. */
int viso_get_reloc_illum(viso_ctx* ctx, int64_t info[8]);
/* The (g, o) rows of the last attempt run in this form, candidate by
 * candidate: the first min(cap, n) are written (gain_offset2 may be NULL);
 * *n = its candidates (0 before the first).  VISO_ERR_STATE while the mode is
 * off. */
int viso_get_reloc_illum_rows(viso_ctx* ctx, double* gain_offset2, size_t cap, size_t* n);

/* Relocalisation seed (the repo's own spec, restated in
 * tests/reloc_seed_ref.py): a pose seed for viso_kf_align from
 * descriptor matches, independent of where tracking stopped.
 *
 * viso_reloc_seed is one stage on host data, through the launches of the frame
 * path (VISO_KERNEL_RELOC_SEED behind VISO_KERNEL_FAST).  kf_pyrs, kf_poses,
 * cur_pyr, width, height, points, n_points: as viso_kf_align's; hosts: every
 * point's host keyframe (0 <= hosts[i] < n_kf); start12: the start pose S.
 *  1. Descriptor: 256 bits on pyramid level 1 at (x1, y1) = (x >> 1, y >> 1) of
 *     a level-0 integer pixel; bit b = I1(x1 + ax, y1 + ay) < I1(x1 + bx, y1 +
 *     by), its four offsets mix64(4 b + c) % 13 - 6 for c = 0..3 (mix64: z +=
 *     0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >>
 *     27) * 0x94D049BB133111EB; z ^ z >> 31); valid when 6 <= x1 < w1 - 6 and
 *     6 <= y1 < h1 - 6; eight little-endian 32-bit words, bit b in word b / 32.
 *  2. Point i is described in its host keyframe (that keyframe's pose and level
 *     1) at x = (int)(u + 0.5), y = (int)(v + 0.5) of its divide-first
 *     projection when its depth is > 0, (u, v) is inside the image and the
 *     descriptor is valid.
 *  3. The first max_features FAST corners of cur_pyr's level 0 (the context's
 *     fast_thresh, the detector's order) are described on cur_pyr's level 1;
 *     those without a valid descriptor are dropped, the order kept.
 *  4. Every described point's best and second-best Hamming distance over the
 *     kept corners (ties: the lowest corner index; fewer than two corners:
 *     second = 257).  Accepted: best <= max_hamming (1..256), best * 1000 <
 *     ratio_permille (1..1000) * second, and the corner's own best described
 *     point is this one (ties: the lowest point index).  The match list: the
 *     accepted points in ascending point index, M of them.
 *  5. M < 3: status 1.  Hypothesis h (hypotheses: 1..4096) draws three distinct
 *     list positions from r_k = mix64(seed + 4 h + k): i0 = r0 % M; i1 = r1 %
 *     (M - 1), + 1 if >= i0; i2 = r2 % (M - 2), stepped past the smaller and
 *     then the larger of i0, i1; ten unweighted Gauss-Newton passes from S on
 *     their reprojection residuals (viso_refine_pose's residual and Jacobian,
 *     sums ((m0 + m1) + m2), its solve and update); unsolved when a depth is
 *     <= 0 or a step is not finite in any pass.  Score = the matches with depth
 *     > 0 and squared reprojection error <= inlier_px^2 (inlier_px > 0).  Best:
 *     the highest score, ties to the lowest h.  None solved, or the best score
 *     < min_inliers (>= 6): status 2.
 *  6. viso_refine_pose's rule (10 iterations, huber_px = inlier_px) from the
 *     best hypothesis's pose on its inliers (uv_before = uv_after = the corner
 *     pixel): the seed pose is its result when its status is 0 or 3, else the
 *     hypothesis's pose; k* = the keyframe hosting the most inliers (ties: the
 *     lowest index).  Status 0.
 * report = {status, described points, kept corners, M, solved hypotheses, best
 * h (-1: none), best score, the refinement's status (-1: not run), its cost at
 * the result (NaN), its inliers at the result, k* (-1), 0}; pose: the seed pose
 * (S unless the status is 0).  matches (cap x 3: point, kept corner, distance)
 * and inliers (cap: the best hypothesis's flags) receive the first min(cap, M)
 * rows, *n_matches = M.  Every out-of-range or NULL argument returns
 * VISO_ERR_ARG (matches and inliers may be NULL when cap is 0). */
int viso_reloc_seed(viso_ctx* ctx, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf, const uint8_t* cur_pyr,
                    int32_t width, int32_t height, const double* points, const int32_t* hosts, int32_t n_points,
                    const double start12[12], int32_t hypotheses, int32_t max_hamming, int32_t ratio_permille,
                    double inlier_px, int32_t min_inliers, uint64_t seed, double report[12], double pose[12],
                    int32_t* matches, uint8_t* inliers, size_t cap, size_t* n_matches);
/* The mode in the frame path.  hypotheses = 0 (default): off, nothing changes,
 * nothing is launched and the other arguments are not read.  On, it takes
 * effect only while viso_set_relocalise is on: a lost frame whose attempt has
 * no winner runs the stage with S = the last good pose, and on status 0 a
 * second attempt with keyframe k* alone and the seed pose as its extra seed
 * (two candidates); its winner is handled as the first attempt's.  The second
 * attempt counts as an attempt, and viso_get_relocalise_report returns the
 * rows of the last attempt that ran. */
int viso_set_reloc_seed(viso_ctx* ctx, int32_t hypotheses, int32_t max_hamming, int32_t ratio_permille,
                        double inlier_px, int32_t min_inliers, uint64_t seed);
/* info = {on (0/1), seed stages run, stages with status 0, recoveries through a
 * seed, then of the last stage: M, its best score, its k*, its status (-1:
 * none)}. */
int viso_get_reloc_seed(viso_ctx* ctx, int64_t info[8]);
/* The last stage's report and seed pose (NaN before the first).
 * VISO_ERR_STATE while the mode is off. */
int viso_get_reloc_seed_report(viso_ctx* ctx, double report[12], double pose[12]);

/* Brightness-compensated tracking (the repo's own spec, restated in
 * tests/bright_ref.py; no reference counterpart): the frame's
 * pose estimated together with an affine brightness map (g, o) from the last
 * frame to the current one, for cameras whose exposure changes.
 *
 * viso_track_affine is the stage on host data, through the launches of the
 * frame path (VISO_KERNEL_BRIGHT).  last_pyr, cur_pyr: the two pyramids;
 * points: n_points x 3 world, 0 <= n_points <= 16384; pose_last12: the last
 * frame's pose L (Tcw); seed12: the seed pose; the context's intrinsics.  All
 * arithmetic is fp64, uncontracted, in both precision modes.  The state is (T,
 * g, o), (seed, 1, 0) on level 3; each lower level starts from the result of
 * the level above.  Pass j = 0..iterations (1..20) on a level at (T_j, g_j,
 * o_j): a point is good as in viso_kf_align (both 8x8 patches inside the level,
 * depth > 0 under L and under T_j; n_j of them).  Per patch pixel (x outer, y
 * inner, -4..3): R = the last level's sample at the point's pixel under L, C
 * and (g0, g1) = the current level's sample and gradient at its pixel under
 * T_j, e = (g_j R + o_j) - C.  A point's 14 pixel sums, each by the descending
 * 64-leaf tree: g0 g0, g0 g1, g1 g1, e g0, e g1, e e, g0 R, g1 R, g0, g1, R R,
 * R, e R, e.  With J0, J1 the rows of dPixeldXi at the level's scale, its 44
 * terms: 0..27 viso_kf_align's 28 (A's upper triangle row-major, A_ab = (G0
 * (J0a J0b) + G1 (J0a J1b + J1a J0b)) + G2 (J1a J1b); b_a = G3 J0a + G4 J1a; the
 * cost G5), computed with this e; B_a0 = -((sum g0 R) J0a + (sum g1 R) J1a) and
 * B_a1 = -((sum g0) J0a + (sum g1) J1a) for a = 0..5; d00 = sum R R; d01 = sum
 * R; c0 = -(sum e R); c1 = -(sum e); d11 = 64 n_j.  Across points every term is
 * summed by the direct pose's canonical map tree (tiles of min(64, ceil(n /
 * 256)) consecutive points, a pairwise tree per tile and one over the tiles,
 * +0.0 for a point that is not good); cost_j = S[27] / n_j.  The step, (g, o)
 * eliminated: det = d00 d11 - d01 d01; q0 = (d11 c0 - d01 c1) / det; q1 = (d00
 * c1 - d01 c0) / det; Y0[a] = (d11 B_a0 - d01 B_a1) / det; Y1[a] = (d00 B_a1 -
 * d01 B_a0) / det; A'_ab = A_ab - (B_a0 Y0[b] + B_a1 Y1[b]) for a <= b,
 * mirrored; b'_a = b_a - (B_a0 q0 + B_a1 q1); xi = inverse6(A') b' (viso_kf_align's
 * solve); dg = q0 - sum_a Y0[a] xi_a, do = q1 - sum_a Y1[a] xi_a, both ascending
 * from a = 0.  The decisions are viso_kf_align's, in its order and with its
 * exits 0..5 and its 0.005, on (T, g, o) in place of T: exit 1 and 5 restore
 * (T, g, o) of pass j - 1, and exit 3 is taken when any of xi, dg, do is not
 * finite; otherwise T_{j+1} = exp(xi) T_j, g_{j+1} = g_j + dg, o_{j+1} = o_j +
 * do.  There are no candidates, no max_points and no max_cost: pose_out12 is
 * always the state behind level 0.  report24 = {status (0, or 2: level 0 ended
 * with exit 4), n_points, level-0 n, level-0 cost, then for levels 3, 2, 1, 0:
 * exit, steps applied, n, cost (NaN where there is none), then g, o, the steps
 * applied over all levels, 0}.  Every out-of-range or NULL argument returns
 * VISO_ERR_ARG (points may be NULL when n_points is 0). */
int viso_track_affine(viso_ctx* ctx, const uint8_t* last_pyr, const uint8_t* cur_pyr, int32_t width, int32_t height,
                      const double* points, int32_t n_points, const double* pose_last12, const double* seed12,
                      int32_t iterations, double* pose_out12, double* report24);
/* The mode in the frame path.  iterations = 0 (default): off, nothing changes,
 * nothing is launched and nothing is allocated.  On (1..20; anything else
 * returns VISO_ERR_ARG) every tracking frame runs this chain, seeded by the
 * last frame's pose, instead of the direct pose, and frames are finished one by
 * one, as with keyframe insertion.  The chain writes the frame's pose, its
 * pose-log and frame-log rows and the level-0 n and cost (viso_get_frame_stats
 * [9], [10]: the compensated cost) where the direct pose writes them, so
 * everything behind the pose runs unchanged on it: LK alignment, the
 * relocalisation verdict, refinement, records, seeds, cull, insertion.  Lost
 * frames (viso_set_relocalise) are unchanged: viso_kf_align keeps its own
 * arithmetic.  (g, o) is estimated afresh for every frame pair.  May be called
 * while tracking (pending work is settled first). */
int viso_set_brightness(viso_ctx* ctx, int32_t iterations);
/* info = {iterations, frames tracked with the mode on, passes applied in all,
 * frames whose level 0 ended with exit 4, then of the last such frame: its
 * level-0 exit, its steps over all levels, its level-0 n, 0}. */
int viso_get_brightness(viso_ctx* ctx, int64_t info[8]);
/* One row of 4 doubles per pose index, as viso_get_poses counts them: {g, o,
 * level-0 exit, steps over all levels}; NaN for frames tracked with the mode
 * off and for lost frames.  The first min(cap, n) rows are written; *n = the
 * poses.  VISO_ERR_STATE while the mode is off. */
int viso_get_brightness_log(viso_ctx* ctx, double* rows, size_t cap, size_t* n);
/* The last frame's report, as viso_track_affine returns it (zeros before the
 * first).  VISO_ERR_STATE while the mode is off. */
int viso_get_brightness_report(viso_ctx* ctx, double report[24]);

/* Robust tracking (the repo's own spec, restated in tests/robust_ref.py;
 * DESIGN.md §23; no reference counterpart): viso_track_affine's chain with a
 * Huber weight per patch pixel, so that an occluder, a specular patch or a map
 * point of wrong depth no longer votes at full weight.  huber_k is in grey
 * levels of the current image; no scale is estimated from the residuals.
 *
 * viso_track_robust is the stage on host data, through the launches of the
 * frame path (VISO_KERNEL_BRIGHT).  It is viso_track_affine's rule with these
 * changes and no others; all arithmetic is fp64 and uncontracted.  Per patch
 * pixel, with e = (g_j R + o_j) - C: r = |e|; out = r > k (strict); w = out ? k
 * / r : 1.0.  Each of the 14 pixel sums has the leaf w * x, x being
 * viso_track_affine's leaf computed as there (w * (g0 * g0), w * (e * R), ...);
 * the exception is sum 5, the cost, whose leaf is out ? k * (2.0 * r - k) : e *
 * e (twice the Huber function).  A fifteenth sum, sum w, by the same descending
 * 64-leaf tree, and the point's count of `out` pixels (an exact integer in a
 * double).  A point's 46 terms: 0..43 as in viso_track_affine from the weighted
 * sums, 44 = sum w, 45 = the count; all 46 go through the canonical map tree,
 * +0.0 for a point that is not good.  The step takes d11 = S[44] in place of 64
 * n_j and is otherwise unchanged; cost_j = S[27] / n_j is the Huber cost.  The
 * decisions, the exits 0..5, the restore on exits 1 and 5, exit 3 on a
 * non-finite value and the level hand-down are unchanged.  With a k that no
 * residual exceeds every w is 1.0, S[44] is 64 n_j exactly and the result is
 * viso_track_affine's bit for bit.
 * report28 = {columns 0..22 as viso_track_affine's, k, then S[44] and S[45] of
 * the last pass evaluated on level 0, 0, 0}.  weights (n_points doubles, or
 * NULL): that pass's sum w per point, 0 where the point is not good.  "The last
 * pass evaluated" is the last pass whose sums were formed: after exit 1 or 5
 * that is the rejected pass, not the one whose state was kept.
 * Arguments as viso_track_affine's; huber_k must be finite with 0 < k <= 1e300
 * (anything else, NaN included, returns VISO_ERR_ARG). */
int viso_track_robust(viso_ctx* ctx, const uint8_t* last_pyr, const uint8_t* cur_pyr, int32_t width, int32_t height,
                      const double* points, int32_t n_points, const double* pose_last12, const double* seed12,
                      int32_t iterations, double huber_k, double* pose_out12, double* report28, double* weights);
/* The mode in the frame path.  huber_k = 0 (default): off.  While on (finite, 0
 * < k <= 1e300; anything else returns VISO_ERR_ARG), every frame that the
 * brightness chain tracks (viso_set_brightness) runs the robust form with this
 * k; the value is kept across viso_set_brightness off and on.  With the
 * brightness mode off it changes nothing, launches nothing and allocates
 * nothing until that mode is on.  Everything behind the pose runs unchanged and
 * reads the Huber level-0 cost from viso_get_frame_stats [10]; the
 * relocalisation verdict (viso_set_relocalise's max_cost) therefore judges the
 * Huber cost, which is at most the plain one.  The brightness log, report and
 * counters are kept as with the mode off.  May be called while tracking
 * (pending work is settled first). */
int viso_set_robust(viso_ctx* ctx, double huber_k);
/* info = {on (0/1), frames tracked robustly, then of the last such frame: its
 * down-weighted pixels (report column 25) and its level-0 n, 0, 0, 0, 0}. */
int viso_get_robust(viso_ctx* ctx, int64_t info[8]);
/* The last robust frame's report, as viso_track_robust returns it (zeros before
 * the first).  This and the two getters below return VISO_ERR_STATE until the
 * mode and the brightness mode have been on together for the first time. */
int viso_get_robust_report(viso_ctx* ctx, double report[28]);
/* The last robust frame's weight mass per map point (the stage's weights): the
 * first min(cap, n) values are written; *n = the map points that frame tracked.
 * The order is the map's when that frame was tracked (viso_get_points then).
 * Insertion behind the frame appends points, which have no value here; culling
 * or a retired keyframe compacts the map, after which index i here is no longer
 * point i of viso_get_points: read the weights before the next call that may
 * change the map, or keep the points read at the same time. */
int viso_get_robust_weights(viso_ctx* ctx, double* w, size_t cap, size_t* n);
/* One row of 2 doubles per pose index, as viso_get_poses counts them: {report
 * column 24 / (64 x level-0 n): the mean weight, report column 25}; NaN for
 * frames not tracked robustly and for lost frames. */
int viso_get_robust_log(viso_ctx* ctx, double* rows, size_t cap, size_t* n);

/* Photometric bundle adjustment (the repo's own spec of the BA that
 * include/bundle_adjuster.h:22-106 sketches with g2o, SURVEY.md §8(f) row 4;
 * oracle/oracle_ba.cpp): after every stereo keyframe insertion, `iterations`
 * Levenberg-Marquardt steps refine every keyframe pose but the first and
 * every map point over 16-residual 4x4 patch edges (each point against every
 * keyframe but its host), points marginalised (Schur complement).
 * 0 = off (default). */
int viso_set_bundle_adjust(viso_ctx* ctx, int32_t iterations);
/* The map's keyframe poses (Map::keyframes_, include/map.h; Tcw, 12 doubles
 * each, in insertion order, as the BA last left them): the first
 * min(cap, keyframes) are written; *n = the keyframe count. */
int viso_get_keyframe_poses(viso_ctx* ctx, double* Tcw12, size_t cap, size_t* n);
/* Stage entry (parity tests): the same BA on host data.  kf_images: n_kf
 * (2..8) level-0 images of the context's size; kf_poses: n_kf x 12 (in/out;
 * keyframe 0 fixed); points: n x 3 world (in/out), 1 <= n <= 16384; host: n
 * keyframe indices (an edge's host pose stays at its value from the start of
 * the call); report (may be NULL): iterations x 4 (cost, candidate cost,
 * damping, accepted).  src: bundle_adjuster.h:58-100 (EdgeDirectProjection).
 * VISO_ERR_ARG on any out-of-range argument. */
int viso_photometric_ba(viso_ctx* ctx, const uint8_t* const* kf_images, int32_t n_kf, double* kf_poses,
                        double* points, const int32_t* host, int32_t n, int32_t iterations, double* report);

/* Rectification (the repo's own spec, restated in tests/rectify_ref.py;
 * DESIGN.md §20; no reference counterpart: src/main.cpp:14-17 hard-codes the
 * intrinsics of an ideal pinhole camera).  A per-camera lens model and
 * rectifying rotation, applied on the device to every incoming frame ahead of
 * the pyramid, one batched launch per ingest chunk (VISO_KERNEL_RECTIFY).
 *
 * The output image is width x height with the intrinsics K = (fx, fy, cx, cy)
 * of the context (viso_params); the raw image is raw_width x raw_height with
 * the intrinsics of this struct.  All in fp64, uncontracted, in this order,
 * for output pixel (x, y), model VISO_RECTIFY_RADTAN:
 *   a = (x - K.cx) / K.fx, b = (y - K.cy) / K.fy,
 *   X = (R0 a + R1 b) + R2, Y = (R3 a + R4 b) + R5, Z = (R6 a + R7 b) + R8;
 *   not (Z > 0): the pixel is outside;
 *   xn = X / Z, yn = Y / Z, r2 = xn xn + yn yn, xy = xn yn,
 *   rad = 1 + r2 (k1 + r2 (k2 + r2 k3)),
 *   xd = xn rad + ((2 p1) xy + p2 (r2 + 2 (xn xn))),
 *   yd = yn rad + (p1 (r2 + 2 (yn yn)) + (2 p2) xy),
 *   u = fx xd + cx, v = fy yd + cy.
 * R (row-major) takes rays of the rectified camera into the raw camera: it is
 * the transpose of the R1 / R2 that OpenCV's stereoRectify returns (identity
 * for a single camera).  It is not checked for orthonormality.
 * Model VISO_RECTIFY_TABLE: (u, v) = the two floats of map[y][x], widened to
 * fp64 (any lens; viso_amd.rectify has numpy helpers that make such maps).
 * Sampling, both models: the pixel is outside unless u > -1, u < raw_width,
 * v > -1 and v < raw_height (a NaN is outside), and then out = fill.  Else
 *   qu = floor(32 u + 0.5), x0 = qu >> 5, ax = qu & 31 (v likewise: y0, ay),
 *   T.. = the raw byte at the tap, or fill where the tap is outside the raw image,
 *   out = (T00 (32-ax)(32-ay) + T01 ax (32-ay) + T10 (32-ax) ay + T11 ax ay + 512) >> 10.
 * Two counts per camera, made on the device when the mode is set: outside =
 * the outside pixels; clipped = those plus the pixels with a tap of non-zero
 * weight outside the raw image (the black border the chosen K leaves). */
#define VISO_RECTIFY_OFF 0
#define VISO_RECTIFY_RADTAN 1
#define VISO_RECTIFY_TABLE 2
typedef struct viso_rectify_params {
    int32_t model;                 /* VISO_RECTIFY_* */
    int32_t raw_width, raw_height; /* same limits as viso_params width / height */
    int32_t fill;                  /* 0..255 */
    double fx, fy, cx, cy;         /* raw intrinsics (RADTAN) */
    double k1, k2, p1, p2, k3;     /* radial-tangential coefficients, OpenCV's order */
    double R[9];
    const float* map;              /* TABLE: [height][width][2] (u, v), copied */
    int32_t reserved[4];
} viso_rectify_params;
/* Switches camera `cam` (0: the left or only camera, 1: the right one) on, or
 * off (p NULL or model 0; the default: nothing changes, no launch, buffer or
 * wait is added).  With camera 0 on viso_process_frame and viso_process_stereo
 * expect frames of the raw size and viso_process_frames_device a frame_stride
 * of at least raw_width x raw_height; the rectified image is level 0 of the
 * frame's own pyramid slot.  A right image is rectified by camera 1's
 * parameters; with camera 1 off it passes through.  viso_process_stereo has
 * one dims for both images, so there the left and right inputs must have one
 * size: two cameras that are both on need the same raw size, and with camera 0
 * on and camera 1 off the raw size must equal the output size (otherwise the
 * call returns VISO_ERR_ARG; rectify such a right image to the output size
 * with camera 1 on, or use viso_rectify).  viso_process_frames_device likewise
 * has one frame_stride, at least the larger of the two inputs.  VISO_ERR_ARG on a bad cam,
 * model, size or fill, on a non-finite number, on fx or fy <= 0 (RADTAN) and
 * on a NULL map (TABLE); VISO_ERR_STATE once the context has taken a frame. */
int viso_set_rectify(viso_ctx* ctx, int32_t cam, const viso_rectify_params* p);
/* info = {model, raw width, raw height, fill, outside, clipped, rectify
 * launches that held an image of this camera, images rectified}. */
int viso_get_rectify(viso_ctx* ctx, int32_t cam, int64_t info[8]);
/* Stage entry (parity tests; the rig and SVO contexts' way in): n raw images
 * (host, raw_width x raw_height each, packed) -> n rectified width x height
 * images (host) with the output intrinsics K = {fx, fy, cx, cy}, by the launch
 * of the frame path; counts (may be NULL) = {outside, clipped} of one image.
 * 1 <= sizes <= 4096, n >= 1; otherwise viso_set_rectify's argument rules. */
int viso_rectify(viso_ctx* ctx, const viso_rectify_params* p, const double K[4], int32_t width, int32_t height,
                 const uint8_t* raw, int32_t n, uint8_t* out, int64_t counts[2]);

/* Library build/version string, "viso_amd 0.1 gfx950 (HIP) src:<hash>": the
 * hash of the sources and flags it was built from (viso_amd/build.py
 * source_hash), so a stale prebuilt library can be detected. */
const char* viso_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VISO_C_H */
