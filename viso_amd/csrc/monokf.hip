// viso_amd — monocular keyframe insertion: the map grows by two-view
// triangulation between the current tracking frame c and the latest keyframe
// k (viso_set_mono_keyframes, include/viso/viso_c.h; DESIGN.md §Monocular
// keyframe insertion).  The repo's own spec, restated in tests/mono_kf_ref.py:
// the reference sketches the triangulation and its reprojection filter in
// Viso::Reconstruct (src/viso.cpp:434-501) and never calls it, so its
// monocular map stays the one of src/viso.cpp:79-96.
//
// One insertion: (1) the map's points mark the cells of frame c they project
// into, (2) FAST corners of c: every unmarked cell keeps its best corner,
// winners compacted in corner order with their rotation-only warp into k as
// the KLT seed, (3) the pyramidal KLT c -> k (track.hip), (4) Triangulate
// ([I|0], [R_kc|T_kc]) per candidate, filtered by depth sign, reprojection
// error and parallax, accepted points compacted in candidate order.
//
// Mapping: one lane per map point / corner / candidate.  Every count stays on
// the device (the launches cover the capacities and lanes past the count
// idle), so the host reads back one count per insertion.  Orders are fixed:
// cell winners by a 64-bit integer maximum of (score, first index), both
// compactions by ballot / popcount prefixes in index order; no float atomics.
// fp64 in the operand order of tests/mono_kf_ref.py, -ffp-contract=off.
#include <algorithm>
#include <cmath>

#include "block_rank.hpp"
#include "context.hpp"
#include "device_math.hpp"
#include "linalg.hpp"

namespace viso {

namespace {

constexpr unsigned long long kCellMarked = ~0ULL;

// K^-1 [x, y, 1] from the float keypoint (src/viso.cpp:46-47)
__device__ inline void normalise_px(const double* Ki, float2 kp, double* x) {
    const double u0 = (double)kp.x, u1 = (double)kp.y;
#pragma unroll
    for (int r = 0; r < 3; ++r) x[r] = Ki[3 * r] * u0 + Ki[3 * r + 1] * u1 + Ki[3 * r + 2] * 1.0;
}

// (1) occupancy: a map point in front of c that projects inside the image
// marks its cell (every marking lane stores the same value)
__global__ __launch_bounds__(256) void mono_occupancy_kernel(MonoKfArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_map) return;
    const int cell = seen_cell(a, a.pose_c, a.map_pts + 3 * (size_t)i);
    if (cell >= 0) a.cell_key[cell] = kCellMarked;
}

__device__ inline int corner_cell(const MonoKfArgs& a, const int4& c) {
    const int cx = c.x / a.cell, cy = c.y / a.cell;
    return (c.x < 0 || c.y < 0 || cx >= a.ncx || cy >= a.ncy) ? -1 : cy * a.ncx + cx;
}

__device__ inline unsigned long long corner_key(const int4& c, int i) {
    return ((unsigned long long)(unsigned int)c.z << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)i);
}

// (2a) every unmarked cell keeps the largest (score, first index) key
__global__ __launch_bounds__(256) void mono_cell_winner_kernel(MonoKfArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = min(*a.n_corners, a.cap_corners);
    if (i >= n) return;
    const int4 c = a.corners[i];
    const int cell = corner_cell(a, c);
    if (cell < 0) return;
    if (a.cell_key[cell] == kCellMarked) return;
    atomicMax(a.cell_key + cell, corner_key(c, i));
}

// (2b) winners compacted in corner order (one workgroup, block_rank.hpp),
// with the KLT seed: the rotation-only warp of the corner into k (R_kc = R_k
// R_c^T, T_kc = t_k - R_kc t_c)
__global__ __launch_bounds__(1024) void mono_compact_kernel(MonoKfArgs a) {
    __shared__ int s_w[16];
    const int tid = threadIdx.x;
    const int n = min(*a.n_corners, a.cap_corners);
    double R[9], T[3];
    relative_motion(a.pose_c, a.pose_k, R, T);
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        int4 c = make_int4(0, 0, 0, 0);
        bool f = false;
        if (i < n) {
            c = a.corners[i];
            const int cell = corner_cell(a, c);
            f = cell >= 0 && a.cell_key[cell] == corner_key(c, i);
        }
        const BlockRank r = block_rank<16>(f, s_w);
        const int j = base + r.rank;
        if (f && j < a.cap_win) {
            const float2 k1 = make_float2((float)c.x, (float)c.y);
            double x1[3], q[3];
            normalise_px(a.Kinv, k1, x1);
            mat3_vec(R, x1, q);
            double u, v;
            pixel_mul_first(a.K, q[0], q[1], q[2], u, v);
            a.kp1[j] = k1;
            a.kp2[j] = make_float2((float)u, (float)v);
            a.win_xy[j] = make_int2(c.x, c.y);
        }
        base += r.total;
    }
    if (tid == 0) {
        a.counts[0] = n;
        a.counts[1] = min(base, a.cap_win);
        a.counts[2] = 0;
        a.counts[3] = 0;
    }
}

// (4a) one lane per candidate: Triangulate for the known motion, the filter
// of Viso::Reconstruct (src/viso.cpp:476-497) plus depth signs and parallax;
// accept flag, camera-frame point and the wave's accepted count
__global__ __launch_bounds__(256) void mono_triangulate_kernel(MonoKfArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int n = min(a.counts[1], a.cap_win);
    const bool tracked = i < n && a.success[i] != 0;
    bool ok = false;
    double P[3] = {0.0, 0.0, 0.0};
    if (tracked) {
        double R[9], T[3], x1[3], x2[3], X[4];
        relative_motion(a.pose_c, a.pose_k, R, T);
        normalise_px(a.Kinv, a.kp1[i], x1);
        normalise_px(a.Kinv, a.kp2[i], x2);
        triangulate_h(R, T, x1[0], x1[1], x2[0], x2[1], X);
        P[0] = X[0] / X[3];
        P[1] = X[1] / X[3];
        P[2] = X[2] / X[3];
        double P2[3];
        mat3_vec(R, P, P2);
        P2[0] = P2[0] + T[0];
        P2[1] = P2[1] + T[1];
        P2[2] = P2[2] + T[2];
        ok = __builtin_isfinite(P[0]) && __builtin_isfinite(P[1]) && __builtin_isfinite(P[2]) && P[2] > 0 &&
             P2[2] > 0;
        double dx = (P[0] / P[2] - x1[0]) * a.K[0];
        double dy = (P[1] / P[2] - x1[1]) * a.K[1];
        ok = ok && sqrt(dx * dx + dy * dy) <= a.proj_thresh;
        dx = (P2[0] / P2[2] - x2[0]) * a.K[0];
        dy = (P2[1] / P2[2] - x2[1]) * a.K[1];
        ok = ok && sqrt(dx * dx + dy * dy) <= a.proj_thresh;
        // O2 = -R_kc^T T_kc: k's centre in c's frame
        double n2[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            n2[r] = P[r] - (((-R[r]) * T[0] + (-R[3 + r]) * T[1]) + (-R[6 + r]) * T[2]);
        const double d1 = sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]);
        const double d2 = sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2]);
        const double cosang = ((P[0] * n2[0] + P[1] * n2[1]) + P[2] * n2[2]) / (d1 * d2);
        ok = ok && cosang <= a.cos_thresh;
    }
    const unsigned long long bt = __ballot(tracked), bo = __ballot(ok);
    if (lane == 0) {
        a.wave_cnt[i >> 6] = __popcll(bo);
        if (bt) atomicAdd(a.counts + 2, __popcll(bt));
    }
    if (i < a.cap_win) {
        a.accept[i] = ok ? 1 : 0;
        a.cand_pts[3 * (size_t)i] = P[0];
        a.cand_pts[3 * (size_t)i + 1] = P[1];
        a.cand_pts[3 * (size_t)i + 2] = P[2];
    }
}

// (4b) accepted points in candidate order: a wave's offset is the sum of the
// counts of the waves before it (integers: any order), a lane's its rank in
// the workgroup (block_rank.hpp); the last workgroup stores the total
__global__ __launch_bounds__(256) void mono_emit_kernel(MonoKfArgs a) {
    __shared__ int s_sum[4], s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * 256 + tid;
    const bool ok = i < a.cap_win && a.accept[i] != 0;
    int acc = 0;
    for (int k = tid; k < (int)blockIdx.x * 4; k += 256) acc += a.wave_cnt[k];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) s_sum[wave] = acc;
    const BlockRank r = block_rank<4>(ok, s_w);  // (its first barrier publishes s_sum too)
    const int before = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    const int j = before + r.rank;
    if (ok && j < a.out_cap) {
        a.out[3 * (size_t)j] = a.cand_pts[3 * (size_t)i];
        a.out[3 * (size_t)j + 1] = a.cand_pts[3 * (size_t)i + 1];
        a.out[3 * (size_t)j + 2] = a.cand_pts[3 * (size_t)i + 2];
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) a.counts[3] = before + r.total;
}

}  // namespace

int mono_kf_cells(int w, int h, int cell) { return ((w + cell - 1) / cell) * ((h + cell - 1) / cell); }

size_t mono_kf_scratch_bytes(int w, int h, int cell, int cap_corners) {
    MonoKfArgs a{};
    return mono_kf_scratch_at(a, nullptr, w, h, cell, cap_corners);
}

size_t mono_kf_scratch_at(MonoKfArgs& a, void* base, int w, int h, int cell, int cap_corners) {
    const size_t cells = (size_t)mono_kf_cells(w, h, cell);
    const size_t waves = 4 * ((cells + 255) / 256);  // the triangulation grid's waves
    Bump b;
    const size_t o_key = b.take(8 * cells), o_cnt = b.take(32), o_cor = b.take(16 * (size_t)cap_corners),
                 o_k1 = b.take(8 * cells), o_k2 = b.take(8 * cells), o_xy = b.take(8 * cells),
                 o_s = b.take(cells), o_acc = b.take(cells), o_wc = b.take(4 * waves), o_p = b.take(24 * cells);
    if (base) {
        char* p = (char*)base;
        a.w = w;
        a.h = h;
        a.cell = cell;
        a.ncx = (w + cell - 1) / cell;
        a.ncy = (h + cell - 1) / cell;
        a.cell_key = (unsigned long long*)(p + o_key);
        a.counts = (int*)(p + o_cnt);
        a.n_corners = a.counts + 4;  // FAST's own (uncapped) count
        a.corners = (int4*)(p + o_cor);
        a.cap_corners = cap_corners;
        a.kp1 = (float2*)(p + o_k1);
        a.kp2 = (float2*)(p + o_k2);
        a.win_xy = (int2*)(p + o_xy);
        a.success = (uint8_t*)(p + o_s);
        a.accept = (uint8_t*)(p + o_acc);
        a.wave_cnt = (int*)(p + o_wc);
        a.cand_pts = (double*)(p + o_p);
        a.cap_win = (int)cells;
    }
    return b.off;
}

void launch_mono_candidates(const MonoKfArgs& a, hipStream_t stream) {
    (void)hipMemsetAsync(a.cell_key, 0, 8 * (size_t)a.ncx * a.ncy, stream);
    if (a.n_map > 0) mono_occupancy_kernel<<<(a.n_map + 255) / 256, 256, 0, stream>>>(a);
    if (a.cap_corners > 0) mono_cell_winner_kernel<<<(a.cap_corners + 255) / 256, 256, 0, stream>>>(a);
    mono_compact_kernel<<<1, 1024, 0, stream>>>(a);
}

void launch_mono_triangulate(const MonoKfArgs& a, hipStream_t stream) {
    const int blocks = (a.cap_win + 255) / 256;
    mono_triangulate_kernel<<<blocks, 256, 0, stream>>>(a);
    mono_emit_kernel<<<blocks, 256, 0, stream>>>(a);
}

}  // namespace viso

using namespace viso;

// One insertion's launches on the context stream (scratch: mono_kf_scratch_at
// bytes): FAST on c, candidates, KLT c -> k, triangulation; the accepted
// points (c's camera frame) at out (<= out_cap), every count in a.counts.
int viso_ctx::mono_launch(MonoKfArgs& a, const FrameDev& fc, const FrameDev& fk, const PyrGeom& g, FastScratch& fs,
                          const double* pose_c, const double* pose_k, const double* points, int n_points, int cell,
                          double min_parallax_deg, double* out, int out_cap) {
    intrinsics(a.K);
    for (int k = 0; k < 9; ++k) a.Kinv[k] = Kinv[k];
    a.proj_thresh = p.projection_error_thresh;
    a.cos_thresh = std::cos(min_parallax_deg * 3.14159265358979323846 / 180.0);
    a.pose_c = pose_c;
    a.pose_k = pose_k;
    a.map_pts = points;
    a.n_map = n_points;
    a.out = out;
    a.out_cap = out_cap;
    {
        TimedRegion t(timing, VISO_KERNEL_FAST, stream);
        launch_fast(fc.l[0], g.w[0], g.h[0], p.fast_thresh, fs, nullptr, (int4*)a.corners, a.cap_corners,
                    (int*)a.n_corners, stream);
    }
    launch_mono_candidates(a, stream);
    {
        TimedRegion t(timing, VISO_KERNEL_KLT, stream);
        launch_klt_dev(fc, fk, g, a.kp1, a.kp2, a.success, a.counts + 1, a.cap_win, p.photometric_error_thresh,
                       stream);
    }
    launch_mono_triangulate(a, stream);
    VISO_HIP_CHECK(hipGetLastError());
    return VISO_OK;
}

// Monocular keyframe insertion (the kRunning case's insertion branch, as
// insert_keyframe): new points by triangulation against the latest keyframe,
// appended up to the map's free capacity; nothing accepted = no keyframe.
// One host sync: the accepted count (n_map is host state).
int viso_ctx::insert_mono_keyframe(int cur) {
    const PyrGeom& g = geom;
    const int cap = kMaxMapPoints - n_map;
    const int k = kf_slots.back();
    int rc = mono_buf.ensure(mono_kf_scratch_bytes(g.w[0], g.h[0], mkf_cell, p.max_features));
    if (rc) return rc;
    MonoKfArgs a{};
    mono_kf_scratch_at(a, mono_buf.ptr, g.w[0], g.h[0], mkf_cell, p.max_features);
    double* dst = (double*)map_pts.ptr + 3 * (size_t)n_map;
    rc = mono_launch(a, frame(cur), frame(k), g, fast, pose_of(cur),
                     (const double*)kf_poses.ptr + 12 * (kf_slots.size() - 1), (const double*)map_pts.ptr, n_map,
                     mkf_cell, mkf_parallax_deg, dst, cap);
    if (rc) return rc;
    VISO_HIP_CHECK(hipMemcpyAsync(h_int + 4, a.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    const int m = std::max(0, std::min(h_int[7], cap));
    if (m == 0) return VISO_OK;  // (stats[14] stays 0)
    return append_keyframe(cur, m);
}

extern "C" {

int viso_set_mono_keyframes(viso_ctx* c, int32_t interval, int32_t ngood_permille, int32_t cell,
                            double min_parallax_deg) {
    if (!c || interval < 0 || ngood_permille < 0 || ngood_permille > 1000 || cell < 8 || cell > 64 ||
        !(min_parallax_deg >= 0 && min_parallax_deg < 90))
        return VISO_ERR_ARG;
    if (interval > 0 && c->kf_interval > 0) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    c->mkf_interval = interval;
    c->mkf_permille = ngood_permille;
    c->mkf_cell = cell;
    c->mkf_parallax_deg = min_parallax_deg;
    return VISO_OK;
}

int viso_mono_points(viso_ctx* c, const uint8_t* cur_pyr, const uint8_t* kf_pyr, int32_t width, int32_t height,
                     const double pose_c[12], const double pose_k[12], const double* points, int32_t n_points,
                     int32_t cell, double min_parallax_deg, double* new_points, int32_t* winners_xy,
                     uint8_t* accept, size_t cap, size_t* n, int32_t counts[4]) {
    if (!c || !cur_pyr || !kf_pyr || !pose_c || !pose_k || width < 16 || height < 16 || width > kMaxWidth ||
        n_points < 0 || n_points > kMaxMapPoints || cell < 8 || cell > 64 ||
        !(min_parallax_deg >= 0 && min_parallax_deg < 90) || (n_points > 0 && !points) || (cap > 0 && !new_points))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const PyrGeom g = make_geom(width, height);
    const int cells = mono_kf_cells(width, height, cell);
    const int out_cap = (int)std::min<size_t>(cap, (size_t)cells);
    Bump b;
    const size_t o_c = b.take(g.bytes), o_k = b.take(g.bytes), o_pc = b.take(96), o_pk = b.take(96),
                 o_p = b.take(24 * (size_t)std::max(n_points, 1)), o_out = b.take(24 * (size_t)std::max(out_cap, 1));
    int rc = c->scratch_a.ensure(b.off);
    if (!rc) rc = c->scratch_b.ensure(fast_scratch_bytes(width, height));
    if (!rc) rc = c->scratch_c.ensure(mono_kf_scratch_bytes(width, height, cell, c->p.max_features));
    if (rc) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_c, cur_pyr, g.bytes, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_k, kf_pyr, g.bytes, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_pc, pose_c, 96, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_pk, pose_k, 96, hipMemcpyHostToDevice, c->stream));
    if (n_points > 0)
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n_points, hipMemcpyHostToDevice, c->stream));
    FastScratch fs = fast_scratch_at(c->scratch_b.ptr, width, height);
    MonoKfArgs a{};
    mono_kf_scratch_at(a, c->scratch_c.ptr, width, height, cell, c->p.max_features);
    rc = c->mono_launch(a, frame_from_base((const uint8_t*)(base + o_c), g),
                        frame_from_base((const uint8_t*)(base + o_k), g), g, fs, (const double*)(base + o_pc),
                        (const double*)(base + o_pk), (const double*)(base + o_p), n_points, cell, min_parallax_deg,
                        (double*)(base + o_out), out_cap);
    if (rc) return rc;
    int32_t cnt[4] = {0, 0, 0, 0};
    VISO_HIP_CHECK(hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int nw = std::max(0, std::min(cnt[1], cells));
    const int m = std::max(0, std::min(cnt[3], out_cap));
    launch_points_to_world((double*)(base + o_out), m, (const double*)(base + o_pc), c->stream);
    VISO_HIP_CHECK(hipGetLastError());
    if (m > 0)
        VISO_HIP_CHECK(hipMemcpyAsync(new_points, base + o_out, 24 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (nw > 0 && winners_xy)
        VISO_HIP_CHECK(hipMemcpyAsync(winners_xy, a.win_xy, 8 * (size_t)nw, hipMemcpyDeviceToHost, c->stream));
    if (nw > 0 && accept)
        VISO_HIP_CHECK(hipMemcpyAsync(accept, a.accept, (size_t)nw, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n) *n = (size_t)std::max(cnt[3], 0);
    if (counts)
        for (int k = 0; k < 4; ++k) counts[k] = cnt[k];
    return VISO_OK;
}

}  // extern "C"
