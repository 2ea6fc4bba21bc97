// viso_amd — host-side launcher declarations (one translation unit per stage).
#pragma once

#include "../../include/viso/viso_c.h"
#include "common.hpp"

namespace viso {

// ---------------------------------------------------------------- image pass
// Builds levels 1..3 of n_images pyramids; image i's level-0 bytes live at
// base + i*img_stride (levels follow, PyrGeom offsets).
void launch_pyramid(const PyrGeom& g, uint8_t* base, int n_images, size_t img_stride,
                    hipStream_t stream, hipEvent_t l1_done = nullptr);
// Batched pyramid over frames whose level 0 is at l0[i] and whose levels
// 1..3 go to slot[i] + g.off[l] (n <= kPyrBatch per launch; more are split).
constexpr int kPyrBatch = 128;
// Two launches: level 1 (streaming bands), levels 2-3 (pyr_tail_kernel).
// own (optional): for frame img, its level 0 copied from l0[img] into
// slot[img] (when they differ and the batch is small enough: copied says
// whether it was) and, when ident_pose is set, the identity pose written
// there — done by the tail launch (a frame-by-frame caller's copy and pose
// launches folded into it).
// zero (optional): n_zero ints cleared by the same launch (the chunk's
// background-LK words, bg_begin).
// FAST device scratch (image.hip): per (row, tile) keypoint counts and
// slots, per-tile totals; carved from fast_scratch_bytes(w, h) bytes.
struct FastScratch {
    int* cnt = nullptr;  // [h][tiles across]
    int* tot = nullptr;  // [bands][tiles across]
    int* lst = nullptr;  // [h][tiles across][64]
};

// A one-image ingest whose frame starts with FAST (the initialisation's
// detection frame): the FAST tiles of `img` (the frame's level 0) run as
// extra workgroups of the level-1 launch (pyr1_fast_kernel) instead of a
// launch of their own behind the pyramid; done = they were launched, so the
// frame's launch_fast only orders them (tiles_done).
struct FastPre {
    const uint8_t* img = nullptr;
    int w = 0, h = 0, thresh = 0;
    FastScratch s;
    bool done = false;
};

struct PyrOwn {
    int img;
    double* ident_pose;
    bool copied;
    int* zero = nullptr;
    int n_zero = 0;
    FastPre* fast = nullptr;
    hipEvent_t l1_done = nullptr;  // recorded behind the level-1 launch, ahead of the tail (timing)
};
void launch_pyramid_frames(const PyrGeom& g, const uint8_t* const* l0, uint8_t* const* slot,
                           int n, hipStream_t stream, PyrOwn* own = nullptr);
size_t fast_scratch_bytes(int w, int h);
FastScratch fast_scratch_at(void* base, int w, int h);
// FAST + NMS on a level-0 image; writes up to cap keypoints (float2 and/or
// raw int4 {x, y, score, 0}) and the total count to *n_out (device).
// det (a re-detection frame, src/viso.cpp:100-108): the count is stored
// capped at cap, the keypoints also go to kp_copy (kp2 = kp1) and the capped
// count also to host_n (pinned host memory, device-mapped; may be null).
struct FastDetect {
    float2* kp_copy;
    int* host_n;
};
void launch_fast(const uint8_t* img, int w, int h, int thresh, FastScratch& s, float2* kp_out,
                 int4* raw_out, int cap, int* n_out, hipStream_t stream, const FastDetect* det = nullptr,
                 bool tiles_done = false);

// ---------------------------------------------------------------- tracking
// OpticalFlowMultiLevel(inverse=true): kp2 in/out, success out (level 0).
void launch_klt(const FrameDev& ref, const FrameDev& cur, const PyrGeom& g, const float2* kp1,
                float2* kp2, uint8_t* success, int n, double thresh, hipStream_t stream);
// the same with the track count in device memory (*n_dev, capped at cap)
void launch_klt_dev(const FrameDev& ref, const FrameDev& cur, const PyrGeom& g, const float2* kp1,
                    float2* kp2, uint8_t* success, const int* n_dev, int cap, double thresh, hipStream_t stream);

constexpr int kMaxKeyframes = 8;
// One frame of a batched LKAlignment launch: its pyramid and pose (device).
struct LkFrame {
    FrameDev cur;
    const double* pose;  // 12 doubles
};
constexpr int kLkBatch = 64;  // frames per launch (kernel arguments stay < 4 KB)
struct LkAlignArgs {
    FrameDev kf[kMaxKeyframes];
    const double* kf_poses;  // n_kf x 12 (device)
    int n_kf;
    int n_frames;            // <= kLkBatch
    LkFrame frames[kLkBatch];
    const double* points;    // n x 3
    int n;
    double K[4];
    double thresh;
    struct {
        int w[4], h[4];
        unsigned long long off[4];
    } g;
    // outputs of frame f at f * out_stride (elements)
    size_t out_stride;
    int32_t* pair_kf;
    uint8_t* success;
    double* uv_before;  // 2 per point
    double* uv_after;
    // per-map templates (lk_template_kernel); tmpl == nullptr: computed inline
    double* tmpl = nullptr;    // [n][4 levels][3][64]
    double* tmpl_h = nullptr;  // [n][4][4]
    int32_t* tmpl_kf = nullptr;
    double* tmpl_uv = nullptr;  // [n][2]
    // tolerance mode (VISO_PRECISION_FAST): tmpl / tmpl_h hold floats, same
    // layout; the iterations run in fp32 (lk_align_kernel<true>)
    int fast = 0;
    // background mode (launch_lk_bg): items = frames x n, taken from eight
    // heads bg_next[32 x] (one per XCD, each a segment of every frame's points,
    // frames in order); frame f's pose is valid once bg_ready[f] != 0
    int* bg_ready = nullptr;
    int* bg_next = nullptr;
    int* bg_err = nullptr;
    // the error word's pinned host copy (device address): set with bg_err[0]
    // by the (rare) failing wave, so the end of a chunk copies nothing back
    int* bg_err_host = nullptr;
    int bg_inject_fail = 0;  // tests (VISO_LK_BG_INJECT_FAIL): the drain reports a failed wait
    int bg_items = 0;
    // leftovers: [0] drain cursor, [1] count, [32 ..] items (head * per_head + k)
    int* bg_left = nullptr;
    int bg_drain = 0;  // this launch is the end-of-chunk drain
    // a resident wave's longest wait for its item's frame before handing the
    // item to the drain (s_memrealtime ticks, 100 MHz)
    unsigned int bg_idle = 30000;
    // warped alignment (launch_lk_warp; viso_set_lk_warp): the largest area
    // ratio |det A| (and its inverse) a warp may have, and the per-point warp
    // rows, laid out as the outputs above (frame f at f * out_stride): A
    // (4 doubles: A00, A01, A10, A11), the level shift and the status byte
    double warp_ratio = 0.0;
    double* warp_A = nullptr;
    int8_t* warp_shift = nullptr;
    uint8_t* warp_status = nullptr;
    // illumination-invariant form of the warped alignment (viso_set_lk_illum;
    // DESIGN.md §24): lk_warp_kernel<true>.  illum_max_gain bounds the level-0
    // gain to [1 / max_gain, max_gain]; illum_go (optional): per point the
    // last accepted level-0 iteration's (gain, offset), NaN where none, laid
    // out as the outputs above
    int illum = 0;
    double illum_max_gain = 0.0;
    double* illum_go = nullptr;
};
void launch_lk_align(const LkAlignArgs& a, hipStream_t stream);
// LK alignment with every keyframe patch warped into the current view by the
// affine map its point's depth and the two poses imply, and taken from the
// pyramid level that matches its scale (track.hip lk_warp_kernel; DESIGN.md
// §17).  The geometry of launch_lk_align; fp64 in both precision modes.
void launch_lk_warp(const LkAlignArgs& a, hipStream_t stream);
// LK alignment of an ingest chunk's frames beside its direct-pose chain: grid
// workgroups (one per CU) resident for the chunk (track.hip lk_item_kernel)
void launch_lk_bg(const LkAlignArgs& a, int grid, hipStream_t stream);
// the items of a background launch it has not taken yet, at full occupancy
// (after the chunk's last pose): grid workgroups pull from the same counter
void launch_lk_drain(const LkAlignArgs& a, int grid, hipStream_t stream);
// the background kernel's attribute and first launches (context init)
void warm_lk_bg(hipStream_t stream);
// Keyframe choice + per-level templates of every map point (once per map).
void launch_lk_template(const LkAlignArgs& a, hipStream_t stream);
// The per-frame log's LK columns (viso_set_frame_log): for batch row f with
// log index idx[f] >= 0, flog[4 idx + 2] = points paired with a keyframe
// (pair_kf >= 0), flog[4 idx + 3] = successes, over the row's n points.
struct LkCountArgs {
    int idx[kLkBatch];
};
void launch_lk_count(const int32_t* pair_kf, const uint8_t* success, size_t stride, int n, int n_rows,
                     const LkCountArgs& rows, double* flog, hipStream_t stream);

// ---------------------------------------------------------------- stereo (north star)
// stereo initialisation (stereo.hip): per keypoint flag / camera point, then
// the kept points compacted in keypoint order into out (<= cap), *count kept
struct StereoCam {
    double fx, fy, cx, cy, base;
};
void launch_stereo_points(const uint8_t* left, const uint8_t* right, int w, int h, const float2* kp,
                          int n, int max_disp, int min_disp, const StereoCam& cam, int* flag,
                          double* pts, double* out, int cap, int* count, hipStream_t stream);
// pts (n x 3, device) <- R^T (pts - T) with the Tcw pose (12 doubles, device)
void launch_points_to_world(double* pts, int n, const double* pose12, hipStream_t stream);
void launch_stereo_sad(const uint8_t* left, const uint8_t* right, int w, int h, const int* xs,
                       const int* ys, int n, int max_disp, int* disp, int* sad,
                       hipStream_t stream);

// ---------------------------------------------------------------- monocular keyframe insertion
// One insertion of viso_set_mono_keyframes (monokf.hip): the current frame c
// against the latest keyframe k.  Poses and points in device memory; the
// scratch members are carved from mono_kf_scratch_bytes() bytes by
// mono_kf_scratch_at (cap_win = the grid's cells: a cell has one winner).
struct MonoKfArgs {
    int w, h, cell, ncx, ncy;
    double K[4];  // fx, fy, cx, cy
    double Kinv[9];
    double proj_thresh;     // pixels
    double cos_thresh;      // cos(min_parallax_deg)
    const double* pose_c;   // 12, Tcw
    const double* pose_k;
    const double* map_pts;  // n_map x 3 (world)
    int n_map;
    const int4* corners;    // FAST's {x, y, score, 0}, row-major
    const int* n_corners;   // FAST's count (uncapped)
    int cap_corners;
    unsigned long long* cell_key;  // [ncy][ncx]: marked, or the best (score, first index)
    float2* kp1;                   // winners (c), KLT seed / result (k)
    float2* kp2;
    int2* win_xy;
    uint8_t* success;  // KLT's
    uint8_t* accept;
    int* wave_cnt;     // accepted per wave of the triangulation grid
    double* cand_pts;  // cap_win x 3 (c's camera frame)
    int cap_win;
    int* counts;  // {corners, winners, KLT successes, accepted}
    double* out;  // accepted points in candidate order (c's camera frame)
    int out_cap;
};
int mono_kf_cells(int w, int h, int cell);
size_t mono_kf_scratch_bytes(int w, int h, int cell, int cap_corners);
size_t mono_kf_scratch_at(MonoKfArgs& a, void* base, int w, int h, int cell, int cap_corners);
// the map's occupancy of c, the cell winners of a.corners compacted in
// corner order into kp1 / win_xy with the KLT seed in kp2; counts[0..1]
void launch_mono_candidates(const MonoKfArgs& a, hipStream_t stream);
// behind the KLT (kp2, success): triangulation, filter, ordered compaction
// of the accepted points into out; counts[2..3]
void launch_mono_triangulate(const MonoKfArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- depth seeds
// viso_set_depth_seeds (depthseed.hip): everything in device
// memory.  A seed row: host keyframe h, corner uv (host level 0), inverse
// depth mu and its variance s2, cnt = {good, bad, lost, last status}.
constexpr int kMaxSeeds = 8192;
constexpr double kSeedAreaRatio = 64.0;  // a seed's warp is rejected outside 1/64 <= |det A| <= 64
struct SeedRows {
    int32_t* h;
    double* uv;  // 2 per seed
    double* mu;
    double* s2;
    int4* cnt;
};
// rows of n seeds carved from seed_rows_bytes(n) bytes
size_t seed_rows_bytes(int n);
size_t seed_rows_at(SeedRows& r, void* base, int n);
struct SeedUpdateArgs {
    FrameDev kf[kMaxKeyframes];
    const double* kf_poses;  // n_kf x 12 (device)
    int n_kf;
    FrameDev cur;
    const double* cur_pose;  // 12
    struct {
        int w[4], h[4];
    } g;
    double K[4];
    struct {
        int max_steps;
        double rho_min, rho_max, max_score, uniqueness;
    } p;
    SeedRows rows;  // updated in place
    int n;
    int2* diag;  // per seed {search level, best step} (-1: not reached), or null
};
// one frame's update: one wave per seed
void launch_seed_update(const SeedUpdateArgs& a, hipStream_t stream);
struct SeedPromoteArgs {
    SeedRows rows;  // survivors compacted in place, in order
    int n;
    const double* kf_poses;
    double K[4];
    int min_good, max_bad, max_lost;
    double conv_rel;
    int room;          // points that fit
    double* out_pts;   // room x 3 (world), in seed order
    int32_t* out_host;
    int* counts;       // {converged, promoted, dropped, survivors}
};
void launch_seed_promote(const SeedPromoteArgs& a, hipStream_t stream);
// keyframe 0 retired: its seeds leave, the others' h moves down; counts[0] = survivors
void launch_seed_retire(const SeedRows& rows, int n, int* counts, hipStream_t stream);
bool seed_params_ok(int max_steps, double depth_min, double depth_max, double max_score, double uniqueness);
bool seed_promote_params_ok(int min_good, double conv_rel, int max_bad, int max_lost);
// behind launch_mono_candidates: the winners (m.win_xy, m.counts[1]) become
// fresh rows from row dst on, at most kMaxSeeds - n_live of them; counts =
// {winners, seeds appended} (device)
void launch_seed_rows(const SeedRows& rows, const MonoKfArgs& m, int n_live, int dst, int host, double depth_min,
                      double depth_max, int* counts, hipStream_t stream);

// ---------------------------------------------------------------- sliding-window map
// One retirement of viso_set_map_window (mapwin.hip): keyframe 0 leaves, the
// check frame is c.  Poses, points and hosts in device memory; the scratch
// members are carved from map_window_scratch_bytes() bytes by
// map_window_scratch_at (cap_points: the most points a launch is given).
struct MapWinArgs {
    int w, h, cell, ncx, ncy;
    double K[4];            // fx, fy, cx, cy
    const double* pose_c;   // 12, Tcw
    double* kf_poses;       // n_kf x 12; row k + 1 -> row k when shift_poses and a point is kept
    int n_kf;
    int shift_poses;
    const double* pts;      // n x 3 (world)
    const int* host;        // n host keyframe indices
    int n;
    int* counts;            // {retired-host, of those seen by c, candidates, survivors, kept}
    int* cell_mark;         // [ncy][ncx]: 1 = a live point projects into it
    size_t zero_bytes;      // counts and cell_mark, cleared together
    int* cell_win;          // [ncy][ncx]: the highest candidate index (-1: none)
    int* pt_cell;           // n: the point's cell in c (-1: c does not see it)
    int* new_host;          // n: host - 1, a candidate's newest seeing keyframe - 1, or -1
    uint8_t* keep;          // n
    int* out_host;          // kept points' hosts and coordinates, in index order
    double* out_pts;
    // the points' track records (viso_set_point_cull), or null: a kept
    // point's row moves with it into out_rec
    const int4* rec;
    int4* out_rec;
};
size_t map_window_scratch_bytes(int w, int h, int cell, int cap_points);
size_t map_window_scratch_at(MapWinArgs& a, void* base, int w, int h, int cell, int cap_points);
// marks, claims, keep flags, the stable compaction and the counts
void launch_map_retire(const MapWinArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- pose refinement
// One frame's refinement on its LK row (viso_set_pose_refine, refine.hip):
// everything in device memory, one launch of one workgroup.
struct RefineArgs {
    double K[4];               // fx, fy, cx, cy
    const double* pts;         // n x 3 (world)
    const int32_t* pair_kf;    // the LK row: n each (uv: n x 2)
    const uint8_t* success;
    const double* uv_before;
    const double* uv_after;
    int n;
    int iterations;
    double huber, max_shift;
    const double* pose_in;     // 12, Tcw (may be pose_out)
    double* pose_out;          // 12
    double* log;               // the pose log (null: not logged), row log_index
    double* log_host;          // its pinned host copy (device address) or null
    int log_index;
    double* report;            // 8
};
void launch_refine_pose(const RefineArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- map point culling
// One frame's track-record update and one cull of viso_set_point_cull
// (pointcull.hip): everything in device memory.  A record is {age, seen,
// found, fail_run}.
struct PointCullArgs {
    double K[4];              // fx, fy, cx, cy
    const double* pts;        // n x 3 (world)
    int n;
    // the update: the frame's LK row, its final pose, the bound
    const int32_t* pair_kf;
    const uint8_t* success;
    const double* uv_after;   // n x 2
    const double* pose;       // 12, Tcw
    double reproj;            // pixels
    int4* tracks;             // n records, in place (the cull only reads them)
    int* fcounts;             // {paired, good, failed, longest fail_run}; zero before the launch
    // the cull
    const int* host;          // n host keyframe indices
    int max_fail_run, min_points;
    uint8_t* keep;            // n
    double* out_pts;          // the kept points, hosts and records in index order
    int* out_host;
    int4* out_tracks;
    int* ccounts;             // {candidates, survivors, kept, abandoned}
};
// scratch of one cull (keep flags and the compacted map) for n points
size_t point_cull_scratch_bytes(int n);
size_t point_cull_scratch_at(PointCullArgs& a, void* base, int n);
void launch_point_tracks(const PointCullArgs& a, hipStream_t stream);
void launch_point_cull(const PointCullArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- point refinement
// The observation ring's record and one refinement of viso_set_point_refine
// (pointrefine.hip): everything in device memory.  Slot s of the ring holds a
// frame's pose at poses + 12 s and, for point i, a flag at valid[s stride + i]
// and uv at uv[2 (s stride + i)].
constexpr int kMaxObsSlots = 8;
struct PointObsArgs {
    int n;
    const int32_t* pair_kf;   // the frame's LK row: n each (uv: n x 2)
    const uint8_t* success;
    const double* uv_before;
    const double* uv_after;
    double max_shift;         // pixels
    const double* pose;       // 12, Tcw (null: no pose is stored)
    uint8_t* valid_out;       // the slot's n flags and n x 2 uv
    double* uv_out;
    double* pose_out;         // the slot's 12 doubles
};
struct PointRefineArgs {
    double K[4];              // fx, fy, cx, cy
    double* pts;              // n x 3 (world), refined in place
    int n;
    const int32_t* anchor_kf; // n: the LK template's keyframe (< 0: none)
    const double* kf_poses;   // n_kf x 12
    int n_kf;
    const double* poses;      // m x 12: the live slots' poses
    const uint8_t* valid;     // m x stride
    const double* uv;         // m x stride x 2
    size_t stride;
    int m;                    // live slots, 1..kMaxObsSlots
    int iterations, min_obs;
    double huber, max_rel_sigma;
    uint8_t* status;          // n each
    uint8_t* steps;
    double* costs;            // n x 2: cost_0, the cost at the result (0: no pass ran)
    int* counts;              // {eligible, moved, status 4, status 2}; zero before the launch
    unsigned long long* moved_total;  // += moved (null: not kept)
};
void launch_point_obs(const PointObsArgs& a, hipStream_t stream);
void launch_point_refine(const PointRefineArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- relocalisation
// One attempt of the keyframe alignment (reloc.hip):
// everything in device memory.  Candidate c = (1 + n_extra) k + s aligns
// keyframe k to `cur` from k's own pose (s = 0) or from extra_seed (s = 1).
constexpr int kMaxAlignCands = 16;
constexpr int kAlignReport = 20;  // doubles per candidate
struct KfAlignArgs {
    double K[4];               // fx, fy, cx, cy
    FrameDev kf[kMaxKeyframes];
    const double* kf_poses;    // n_kf x 12
    int n_kf;
    FrameDev cur;
    int w[4], h[4];            // the pyramid's level sizes
    const double* points;      // n x 3 (world)
    int n;
    const double* extra_seed;  // 12 (n_extra = 1)
    int n_extra, iterations, max_points, min_good_permille;
    double max_cost;
    double* poses_out;         // n_cand x 12
    double* report;            // n_cand x kAlignReport
    int* winner;               // 1
    // the frame path: the winner's pose (the held pose when none wins) goes to
    // pose_dst and, with log_index >= 0, to the pose log and its pinned mirror;
    // a winner's pose to good_dst (the last good pose) too; the frame-log row
    // becomes {the winner's n, its cost, NaN, NaN} (all NaN when none wins).
    // All may be null.
    const double* hold_pose;
    double* pose_dst;
    double* good_dst;
    double* log;
    double* log_host;
    double* flog;
    int log_index;
    // the illumination form: gain_offset non-null selects it;
    // the kept (g, o) of every candidate, n_cand x 2
    double max_gain;
    double* gain_offset;
};
// two launches: the candidates (one workgroup each; kf_align_kernel<true> when
// a.gain_offset is set), then the choice
void launch_kf_align(const KfAlignArgs& a, hipStream_t stream);

// ---------------------------------------------------------------- relocalisation seed
// One seed stage (relocseed.hip): everything in device memory.
// The map's points are described in their host keyframes, the FAST corners of
// `cur` in cur (256-bit BRIEF on level 1), matched both ways, and the pose is
// solved from `start` by three-point hypotheses and §14's refinement.  The
// scratch members are carved from reloc_seed_scratch_bytes() bytes by
// reloc_seed_scratch_at.
constexpr int kSeedReport = 12;   // doubles
constexpr int kSeedMaxHyp = 4096;
struct RelocSeedArgs {
    double K[4];               // fx, fy, cx, cy
    FrameDev kf[kMaxKeyframes];
    const double* kf_poses;    // n_kf x 12
    int n_kf;
    FrameDev cur;
    int w[4], h[4];            // the pyramid's level sizes
    const double* points;      // n x 3 (world)
    const int* host;           // n host keyframe indices
    int n;
    const double* start;       // 12: S
    const int4* corners;       // FAST's {x, y, score, 0}, in the detector's order
    const int* n_corners;      // FAST's count (uncapped)
    int cap_corners;
    int hypotheses, max_hamming, ratio_permille, min_inliers;
    double inlier_px;
    unsigned long long seed;
    // scratch
    int* counts;               // {described, kept corners, M, 0}; zero before the launches
    int2* kept_xy;             // the kept corners' pixels, in order
    uint32_t* pdesc;           // n x 8
    uint8_t* pvalid;           // n
    uint32_t* cdesc;           // cap_corners x 8
    int4* pbest;               // n: {best, second, corner, 0}
    int2* cbest;               // cap_corners: {best, point}
    int4* matches;             // n: {point, corner, distance, inlier of the best hypothesis}
    double* hyp_pose;          // hypotheses x 12
    int* hyp_score;            // hypotheses: -1 unsolved (set before the launches)
    int32_t* pair_kf;          // the inliers as an LK row over the map: n each (uv: n x 2)
    uint8_t* success;
    double* uv;
    double* hyp_best;          // 12: the best hypothesis's pose (S when the status is not 0)
    double* refine_pose;       // 12
    double* refine_rep;        // 8
    // results
    double* report;            // kSeedReport
    double* pose_out;          // 12
};
size_t reloc_seed_scratch_bytes(int n, int cap_corners, int hypotheses);
size_t reloc_seed_scratch_at(RelocSeedArgs& a, void* base, int n, int cap_corners, int hypotheses);
// behind FAST (a.corners, a.n_corners): ten launches and the refinement's
void launch_reloc_seed(const RelocSeedArgs& a, hipStream_t stream);
bool reloc_seed_params_ok(int hypotheses, int max_hamming, int ratio_permille, double inlier_px, int min_inliers);

// ---------------------------------------------------------------- brightness-compensated tracking
// One frame's chain (bright.hip): everything in device memory.
// part / good / state are carved from bright_scratch_bytes() bytes by
// bright_scratch_at; tile and n_tiles are set by launch_bright.
constexpr int kBrightReport = 24;  // doubles
constexpr int kBrightTerms = 44;   // the sums of a pass
constexpr int kBrightState = 64;   // doubles of a state block
struct BrightArgs {
    double K[4];               // fx, fy, cx, cy
    FrameDev last, cur;
    int w[4], h[4];            // the pyramid's level sizes
    const double* points;      // n x 3 (world)
    int n;
    const double* pose_last;   // 12: the last frame's pose L
    const double* seed;        // 12
    int iterations;
    int tile, n_tiles;         // the canonical map tree's tiles
    // scratch
    double* part;              // 2 x 256 tiles x kBrightTerms
    int* good;                 // 2 x 256
    double* state;             // 2 x kBrightState
    // results (the chain's last launch)
    double* pose_out;          // 12
    double* report;            // kBrightReport
    double* stats;             // the direct pose's level-0 stats row ([0] n, [1] cost), or null
    double* log;               // the pose log, its pinned host copy, the per-frame
    double* log_host;          // log and the brightness log: row log_index of each
    double* flog;              // (null: not written)
    double* blog;
    int log_index;
    long long* info;           // viso_get_brightness's counters, or null
};
size_t bright_scratch_bytes();
void bright_scratch_at(BrightArgs& a, void* base);
int bright_launches(int iterations);  // 4 (iterations + 1) + 1
void launch_bright(BrightArgs a, hipStream_t stream);

// The robust form of the chain (viso_track_robust, viso_set_robust; DESIGN.md
// §23): a Huber weight per patch pixel, 46 sums per pass.  b is the plain
// form's arguments with part sized for kRobustTerms (robust_scratch_at) and
// report (the plain 24 columns) null where nobody reads them.
constexpr int kRobustReport = 28;  // doubles
constexpr int kRobustTerms = 46;   // + sum w, the count of pixels with |e| > k
struct RobustArgs {
    BrightArgs b;
    double huber_k;
    double* weights;           // n: every pass writes its points' sum w (0: not good)
    double* report;            // kRobustReport
    double* rlog;              // the robust log (2 doubles per pose index): row b.log_index, or null
    long long* info;           // viso_get_robust's counters, or null
};
size_t robust_scratch_bytes();
void robust_scratch_at(RobustArgs& a, void* base);
void launch_robust(RobustArgs a, hipStream_t stream);

// ---------------------------------------------------------------- direct pose
constexpr int kMaxMapPoints = 16384;
// Device scratch of the direct pose (carved from one buffer of
// direct_scratch_bytes() by direct_scratch_at).
struct DirectScratch {
    double* part = nullptr;       // [kLevels][4][16][56][2] tile partial sums (direct.hip partial_index)
    int* good = nullptr;          // [kLevels][256]
    double* state = nullptr;      // [kLevels + 1][8] T21 per level (+ result)
    double* cont_part = nullptr;  // [256 workgroups][256][28] continuation scratch
    int* cont_good = nullptr;     // [256 workgroups][256]
};
size_t direct_scratch_bytes();
DirectScratch direct_scratch_at(void* base);
// DirectPoseEstimationMultiLayer (src/viso.cpp:760-766): levels 3..0, each a
// faithful DirectPoseEstimationSingleLayer (:661-758), starting from
// T21 = SE3(R, t) of pose_seed12 (src/viso.cpp:114); the patch reference is
// `last` at pose_last12.  Five launches: the tiles of level l run in a launch
// whose prologue solves level l+1 from its tile partials; a final one-
// workgroup launch solves level 0.
// stats (device, may be null): per level [nGood, cost, H(36), b(6), update(6)].
// pose_out (device, may be null) receives R, t of the result, also stored at
// log[12*log_index] when log is non-null.
void launch_direct_pose(const FrameDev& last, const FrameDev& cur, const PyrGeom& g,
                        const double K[4], const double* points, int n,
                        const double* pose_last12, const double* pose_seed12,
                        const DirectScratch& s, double* stats, double* pose_out, double* log,
                        int log_index, hipStream_t stream, int precision = VISO_PRECISION_FAITHFUL,
                        bool scalar_pass = true);
// One faithful Gauss-Newton solve of a level (iteration 0) on one wave, as the
// level kernels' solver runs it: sums28 = the 21 upper-triangle sums of H,
// b (6), the cost sum; state7 = T21 (quaternion xyzw, t).  Device pointers.
// stats50 = [nGood, cost, H(36), b(6), update(6)]; state_out7 = the new T21.
void launch_direct_solve(const double* sums28, int ngood, const double* state7, double* stats50,
                         double* state_out7, hipStream_t stream);
// The same call split for the frame pipeline: L(3..0) of this frame, then F
// later.  With `merge`, L(3) also runs the previous frame's pending F (its
// level-0 solve; the solved pose is this frame's `last` pose and seed, so
// pose_last12 / pose_seed12 are read only by L(2..0), after L(3) wrote them
// to merge->pose_out).
// scalar_pass: faithful tiles of 9 or 10 points take their per-point scalars
// from the workgroup's two idle waves (direct.hip scalar_pass; same bits).
struct DirectPrev {
    FrameDev last, cur;         // the previous frame's pair (rare continuation)
    const double* pose_last12;  // its `last` pose
    double* pose_out;           // its pose (= this frame's pose_last12)
    double* log;
    int log_index;
    int* ready = nullptr;  // background LK alignment's flag for that pose (or null)
    double* log_host = nullptr;  // the log's pinned host copy (device address), same index
    double* flog = nullptr;      // the per-frame log (viso_set_frame_log), same index, or null
};
// true when a direct-pose workgroup leaves its CU room for the background LK
// alignment's (12 waves of 128 VGPRs + <= 76 KB LDS beside 4 waves + 84 KB)
bool direct_fits_background();
void launch_direct_levels(const FrameDev& last, const FrameDev& cur, const PyrGeom& g,
                          const double K[4], const double* points, int n,
                          const double* pose_last12, const double* pose_seed12,
                          const DirectScratch& s, double* stats, const DirectPrev* merge,
                          hipStream_t stream, int precision = VISO_PRECISION_FAITHFUL, bool bg = false,
                          bool scalar_pass = true);
void launch_direct_final(const FrameDev& last, const FrameDev& cur, const PyrGeom& g,
                         const double K[4], const double* points, int n,
                         const double* pose_last12, const DirectScratch& s, double* stats,
                         double* pose_out, double* log, int log_index, hipStream_t stream,
                         int precision = VISO_PRECISION_FAITHFUL, int* ready = nullptr,
                         double* log_host = nullptr, double* flog = nullptr);
// ---------------------------------------------------------------- rig direct pose
// Multi-camera photometric rig (the repo's own spec;
// oracle/oracle_rig.cpp): levels 3..0 of one rig Gauss-Newton step each over
// every camera's map points, camera c at E_c T, per-camera 28 sums combined
// through Ad(E_c); then F writes the rig pose (+ log) and each camera's next
// `last` pose E_c T.  5 launches.
constexpr int kMaxRigCams = 4;
struct RigCamDev {
    FrameDev last, cur;          // the camera's pyramids
    const double* points;        // its map points (world), n x 3
    int n;
    const double* pose_last12;   // its `last` pose (device, E_c T_last)
    double E[12];                // rig -> camera
    const double* Ad;            // device, 36
    void* scratch;               // rig_scratch_bytes()
};
size_t rig_scratch_bytes();
// state: [kLevels + 1][8] device; seed12: last rig pose (device); stats:
// [kLevels][50] or null; cam_last: n_cams x 12 device.  Returns -1 on a bad
// camera count.
// One rig timestep's direct pose: levels (L(3..0), when `levels`) and the
// final level-0 solve F (when `final_solve`); merge_prev: L(3) first solves
// the previous timestep's level 0 (its F, deferred) and logs it at
// prev_log_index.  An F alone (levels = 0, final_solve = 1) flushes a
// deferred one.
int launch_rig_direct(const RigCamDev* cams, int n_cams, const PyrGeom& g, const double K[4], double* state,
                      const double* seed12, double* stats, double* pose_out, double* log, int log_index,
                      double* cam_last, hipStream_t stream, int precision, int merge_prev = 0,
                      int prev_log_index = -1, int levels = 1, int final_solve = 1);
// ---------------------------------------------------------------- photometric BA
// The BA include/bundle_adjuster.h:22-106 sketches (SURVEY.md §8(f) row 4;
// spec oracle/oracle_ba.cpp): keyframe poses (n_kf x 12 device, keyframe 0
// fixed) and map points (n x 3 device) refined in place by `iterations`
// Levenberg-Marquardt steps over 16-residual 4x4 patch edges point -> every
// non-host keyframe (host: n device ints).  kf_l0: the keyframes' level-0
// images (device).  report (device, may be null): [iterations][4] cost,
// candidate cost, mu, accepted.  scratch: ba_scratch_bytes(n).  Returns -1
// on bad sizes.
size_t ba_scratch_bytes(int n);
int launch_photometric_ba(const uint8_t* const* kf_l0, int n_kf, int w, int h, const double K[4], double* poses,
                          double* pts, const int* host, int n, int iterations, void* scratch, double* report,
                          hipStream_t stream);
// dst (12 doubles, device) <- src (host values, passed by value)
void launch_set_pose(double* dst, const double src[12], hipStream_t stream);
// map creation: cur_pose <- pose, pts_dst <- pts_src (n_pts x 3), kf_poses[0]
// <- *ref_pose, kf_poses[1] <- pose (one launch)
void launch_map_create(double* cur_pose, const double pose[12], const double* pts_src, double* pts_dst, int n_pts,
                       const double* ref_pose, double* kf_poses, hipStream_t stream);

// ---------------------------------------------------------------- rectification
// viso_set_rectify (rectify.hip; the rule: viso_c.h).  One
// camera: the lens model, the raw image's size and intrinsics, the rotation.
struct RectCam {
    int model = 0;  // VISO_RECTIFY_*
    int rw = 0, rh = 0, fill = 0;
    double Kr[4] = {};  // fx, fy, cx, cy of the raw image
    double k[5] = {};   // k1, k2, p1, p2, k3
    double R[9] = {};
    const float* map = nullptr;  // TABLE: [h][w][2] (device)
};
constexpr int kRectBatch = 128;  // images per launch (kernel arguments stay < 4 KB)
// n images of one launch: raw src[i] (cams[cam[i]]'s raw size) -> dst[i]
// (w x h, output intrinsics K).
struct RectifyArgs {
    const uint8_t* src[kRectBatch];
    uint8_t* dst[kRectBatch];
    uint8_t cam[kRectBatch];
    RectCam cams[2];
    double K[4];
    int w, h;
};
// src / dst / cam: n entries (more than kRectBatch are split; cameras of
// different models go in a launch each).  Every camera named is on.
void launch_rectify(const RectCam cams[2], const double K[4], int w, int h, const uint8_t* const* src,
                    uint8_t* const* dst, const uint8_t* cam, int n, hipStream_t stream);
// counts[0] += the outside pixels of one w x h image of `cam`, counts[1] +=
// its clipped pixels (device ints, cleared by the caller).
void launch_rectify_count(const RectCam& cam, const double K[4], int w, int h, int* counts, hipStream_t stream);

}  // namespace viso
