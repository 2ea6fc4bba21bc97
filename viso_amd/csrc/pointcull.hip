// viso_amd — map point culling (viso_set_point_cull, include/viso/viso_c.h;
// DESIGN.md §Map point culling).  The repo's own spec, restated in
// tests/point_cull_ref.py: the reference computes, for every map point,
// whether its keyframe patch is found in the current image (LKAlignment,
// src/viso.cpp:768-843) and only draws the result; its map (src/viso.cpp:79-96)
// never loses a point.
//
// Every map point carries a track record {age, seen, found, fail_run}.  The
// update, once per tracking frame behind the frame's LK row and final pose T:
// age + 1; a paired point is seen + 1 and either good (the alignment
// succeeded, Pc = R P + t is in front of the camera and uv_after lies within
// reproj pixels of its projection at T: found + 1, fail_run = 0) or failed
// (fail_run + 1).  The cull, on every interval-th tracking frame: the points
// with fail_run >= max_fail_run leave, unless fewer than min_points would
// stay; the survivors keep their order.
//
// Mapping: the update is one lane per point, the record one 16-byte load and
// one 16-byte store.  The cull is one workgroup walking the map 1024 points a
// round, twice: the candidates are counted (the abandonment is decided on the
// device), then keep flags and the stable compaction (block_rank.hpp).  The
// only atomics are integer (three sums and a
// maximum), so the result depends on nothing but the data.  fp64 in the
// operand order of tests/point_cull_ref.py, -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <vector>

#include "block_rank.hpp"
#include "context.hpp"
#include "device_math.hpp"
#include "linalg.hpp"

namespace viso {

namespace {

__global__ __launch_bounds__(256) void point_tracks_kernel(PointCullArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < a.n;
    bool paired = false, good = false;
    int run = 0;
    if (in) {
        int4 r = a.tracks[i];
        r.x += 1;
        paired = a.pair_kf[i] >= 0;
        if (paired) {
            r.y += 1;
            const double* P = a.pts + 3 * (size_t)i;
            double Pc[3];
            mat3_vec(a.pose, P, Pc);
            const double x = Pc[0] + a.pose[9], y = Pc[1] + a.pose[10], z = Pc[2] + a.pose[11];
            if (a.success[i] != 0 && z > 0) {
                double u, v;
                pixel_mul_first(a.K, x, y, z, u, v);
                const double r0 = a.uv_after[2 * (size_t)i] - u;
                const double r1 = a.uv_after[2 * (size_t)i + 1] - v;
                const double e2 = r0 * r0 + r1 * r1;
                good = e2 <= a.reproj * a.reproj;
            }
            if (good) {
                r.z += 1;
                r.w = 0;
            } else {
                r.w += 1;
            }
        }
        a.tracks[i] = r;
        run = r.w;
    }
    const unsigned long long bp = __ballot(paired), bg = __ballot(good);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) run = max(run, __shfl_xor(run, off, 64));
    if (lane == 0) {
        if (bp) {
            atomicAdd(a.fcounts + 0, __popcll(bp));
            if (bg) atomicAdd(a.fcounts + 1, __popcll(bg));
            if (bp & ~bg) atomicAdd(a.fcounts + 2, __popcll(bp & ~bg));
        }
        if (run > 0) atomicMax(a.fcounts + 3, run);
    }
}

__global__ __launch_bounds__(1024) void point_cull_kernel(PointCullArgs a) {
    __shared__ int s_w[16];
    const int tid = threadIdx.x;
    // the candidates
    int cand = 0;
    for (int i0 = 0; i0 < a.n; i0 += 1024) {
        const int i = i0 + tid;
        cand += block_rank<16>(i < a.n && a.tracks[i].w >= a.max_fail_run, s_w).total;
    }
    const int surv = a.n - cand;
    const bool abandoned = cand > 0 && surv < a.min_points;
    // keep flags and the stable compaction (an abandoned cull keeps all)
    int base = 0;
    for (int i0 = 0; i0 < a.n; i0 += 1024) {
        const int i = i0 + tid;
        bool f = false;
        int4 r = make_int4(0, 0, 0, 0);
        if (i < a.n) {
            r = a.tracks[i];
            f = abandoned || r.w < a.max_fail_run;
            a.keep[i] = f ? 1 : 0;
        }
        const BlockRank k = block_rank<16>(f, s_w);
        if (f) {
            const size_t j = (size_t)(base + k.rank);
            a.out_pts[3 * j] = a.pts[3 * (size_t)i];
            a.out_pts[3 * j + 1] = a.pts[3 * (size_t)i + 1];
            a.out_pts[3 * j + 2] = a.pts[3 * (size_t)i + 2];
            a.out_host[j] = a.host[i];
            a.out_tracks[j] = r;
        }
        base += k.total;
    }
    if (tid == 0) {
        a.ccounts[0] = cand;
        a.ccounts[1] = surv;
        a.ccounts[2] = base;
        a.ccounts[3] = abandoned ? 1 : 0;
    }
}

}  // namespace

size_t point_cull_scratch_bytes(int n) {
    PointCullArgs a{};
    return point_cull_scratch_at(a, nullptr, n);
}

size_t point_cull_scratch_at(PointCullArgs& a, void* base, int n_) {
    const size_t n = (size_t)std::max(n_, 1);
    Bump b;
    const size_t o_cnt = b.take(32), o_keep = b.take(n), o_oh = b.take(4 * n), o_ot = b.take(16 * n),
                 o_op = b.take(24 * n);
    if (base) {
        char* p = (char*)base;
        a.fcounts = (int*)(p + o_cnt);
        a.ccounts = a.fcounts + 4;
        a.keep = (uint8_t*)(p + o_keep);
        a.out_host = (int*)(p + o_oh);
        a.out_tracks = (int4*)(p + o_ot);
        a.out_pts = (double*)(p + o_op);
    }
    return b.off;
}

void launch_point_tracks(const PointCullArgs& a, hipStream_t stream) {
    (void)hipMemsetAsync(a.fcounts, 0, 4 * sizeof(int), stream);
    if (a.n > 0) point_tracks_kernel<<<(a.n + 255) / 256, 256, 0, stream>>>(a);
}

void launch_point_cull(const PointCullArgs& a, hipStream_t stream) {
    point_cull_kernel<<<1, 1024, 0, stream>>>(a);
}

}  // namespace viso

using namespace viso;

namespace {

bool cull_params_ok(int32_t interval, int32_t max_fail_run, double reproj_px, int32_t min_points) {
    return interval >= 1 && max_fail_run >= 1 && max_fail_run <= 1000 && reproj_px > 0 && std::isfinite(reproj_px) &&
           min_points >= 1 && min_points <= kMaxMapPoints;
}

}  // namespace

// New map points [first, first + count) start with a zero record (map
// creation, an insertion's appended points).
int viso_ctx::tracks_zero(int first, int count) {
    if (!cull_on() || count <= 0) return VISO_OK;
    VISO_HIP_CHECK(hipMemsetAsync((char*)pt_tracks.ptr + 16 * (size_t)first, 0, 16 * (size_t)count, stream));
    return VISO_OK;
}

// One tracking frame's record update in the frame path (on_new_frame, behind
// finish_call on the context stream — cur's final solve, its LK alignment as
// the last row of the LK buffers — and behind the refinement when that is
// on: cur's pose is final).  No host synchronisation.
int viso_ctx::update_tracks(int cur) {
    if (n_map <= 0 || lk_last_rows < 1 || lk_last_pts != n_map) return VISO_ERR_STATE;
    const size_t o = (size_t)(lk_last_rows - 1) * kMaxMapPoints;  // cur's row: the batch's last
    PointCullArgs a{};
    point_cull_scratch_at(a, cull_buf.ptr, kMaxMapPoints);
    intrinsics(a.K);
    a.pts = (const double*)map_pts.ptr;
    a.n = n_map;
    a.pair_kf = (const int32_t*)lk_pair.ptr + o;
    a.success = (const uint8_t*)lk_succ.ptr + o;
    a.uv_after = (const double*)lk_after.ptr + 2 * o;
    a.pose = pose_of(cur);
    a.reproj = cull_reproj;
    a.tracks = (int4*)pt_tracks.ptr;
    {
        TimedRegion t(timing, VISO_KERNEL_CULL, stream);
        launch_point_tracks(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    return VISO_OK;
}

// One cull in the frame path (on_new_frame, right behind the frame's update,
// ahead of its insertion check).  One host sync for the counts and the
// survivors' hosts (n_map and point_host are host state).  A cull that
// removed something rewrites map_pts and the records in place and rebuilds
// the LK templates: a map rewrite (begin_map_rewrite, mapwin.hip).
int viso_ctx::cull_points() {
    const int n = n_map;
    if (n <= 0) return VISO_OK;
    if ((int)point_host.size() != n) return VISO_ERR_STATE;
    if (int rc = point_host_dev.ensure(4 * (size_t)kMaxMapPoints)) return rc;
    if (int rc = begin_map_rewrite(true)) return rc;
    PointCullArgs a{};
    point_cull_scratch_at(a, cull_buf.ptr, kMaxMapPoints);
    a.pts = (const double*)map_pts.ptr;
    a.n = n;
    a.tracks = (int4*)pt_tracks.ptr;
    a.host = (const int*)point_host_dev.ptr;
    a.max_fail_run = cull_max_fail;
    a.min_points = cull_min_points;
    {
        TimedRegion t(timing, VISO_KERNEL_CULL, stream);
        launch_point_cull(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> hosts((size_t)n);
    VISO_HIP_CHECK(hipMemcpyAsync(h_int + 16, a.ccounts, 4 * sizeof(int), hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipMemcpyAsync(hosts.data(), a.out_host, 4 * (size_t)n, hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    const int cand = h_int[16], kept = std::max(0, std::min(h_int[18], n));
    if (h_int[19]) {
        cull_abandoned += 1;
        return VISO_OK;
    }
    if (cand <= 0 || kept == n) return VISO_OK;
    if (int rc = end_map_rewrite(a.out_pts, a.out_tracks, hosts, kept)) return rc;
    cull_applied += 1;
    cull_removed += n - kept;
    cull_last[0] = frames;
    cull_last[1] = n - kept;
    cull_last[2] = kept;
    return build_lk_templates();
}

extern "C" {

int viso_set_point_cull(viso_ctx* c, int32_t interval, int32_t max_fail_run, double reproj_px, int32_t min_points) {
    if (!c || !(interval == 0 || cull_params_ok(interval, max_fail_run, reproj_px, min_points))) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    if (interval > 0) {
        if (!c->cull_on()) {
            // existing points start fresh
            int rc = c->pt_tracks.ensure(16 * (size_t)kMaxMapPoints);
            if (!rc) rc = c->cull_buf.ensure(point_cull_scratch_bytes(kMaxMapPoints));
            if (!rc) rc = c->point_host_dev.ensure(4 * (size_t)kMaxMapPoints);
            if (rc) return rc;
            VISO_HIP_CHECK(hipMemsetAsync(c->pt_tracks.ptr, 0, 16 * (size_t)kMaxMapPoints, c->stream));
        }
        c->cull_max_fail = max_fail_run;
        c->cull_reproj = reproj_px;
        c->cull_min_points = min_points;
    } else if (c->cull_on()) {
        VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
        c->pt_tracks.release();
        c->cull_buf.release();
    }
    c->cull_interval = interval;
    return VISO_OK;
}

int viso_get_point_cull(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    info[0] = c->cull_interval;
    info[1] = c->cull_on() ? c->cull_max_fail : 0;
    info[2] = c->cull_applied;
    info[3] = c->cull_removed;
    info[4] = c->cull_abandoned;
    for (int k = 0; k < 3; ++k) info[5 + k] = c->cull_last[k];
    return VISO_OK;
}

int viso_get_point_tracks(viso_ctx* c, int32_t* tracks4, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (!c->cull_on()) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t m = std::min(cap, (size_t)c->n_map);
    if (m > 0 && tracks4)
        VISO_HIP_CHECK(hipMemcpyAsync(tracks4, c->pt_tracks.ptr, 16 * m, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n) *n = (size_t)c->n_map;
    return VISO_OK;
}

int viso_point_tracks_update(viso_ctx* c, const double* points, const int32_t* pair_kf, const uint8_t* success,
                             const double* uv_after, int32_t n, const double pose[12], double reproj_px,
                             int32_t* tracks4, int32_t counts[4]) {
    if (!c || n < 0 || n > kMaxMapPoints || !pose || !counts || !(reproj_px > 0) || !std::isfinite(reproj_px) ||
        (n > 0 && (!points || !pair_kf || !success || !uv_after || !tracks4)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t m = (size_t)std::max(n, 1);
    Bump b;
    const size_t o_pose = b.take(96), o_cnt = b.take(32), o_p = b.take(24 * m), o_pk = b.take(4 * m),
                 o_sc = b.take(m), o_ua = b.take(16 * m), o_t = b.take(16 * m);
    if (int rc = c->scratch_a.ensure(b.off)) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_pose, pose, 96, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_pk, pair_kf, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_sc, success, (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_ua, uv_after, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_t, tracks4, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    PointCullArgs a{};
    c->intrinsics(a.K);
    a.pts = (const double*)(base + o_p);
    a.n = n;
    a.pair_kf = (const int32_t*)(base + o_pk);
    a.success = (const uint8_t*)(base + o_sc);
    a.uv_after = (const double*)(base + o_ua);
    a.pose = (const double*)(base + o_pose);
    a.reproj = reproj_px;
    a.tracks = (int4*)(base + o_t);
    a.fcounts = (int*)(base + o_cnt);
    launch_point_tracks(a, c->stream);
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_int + 20, a.fcounts, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (n > 0) VISO_HIP_CHECK(hipMemcpyAsync(tracks4, a.tracks, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; ++k) counts[k] = c->h_int[20 + k];
    return VISO_OK;
}

int viso_points_cull(viso_ctx* c, const double* points, const int32_t* host, const int32_t* tracks4, int32_t n,
                     int32_t max_fail_run, int32_t min_points, double* out_points, int32_t* out_host,
                     int32_t* out_tracks4, uint8_t* keep, size_t* n_out, int32_t counts[4]) {
    if (!c || n < 0 || n > kMaxMapPoints || max_fail_run < 1 || max_fail_run > 1000 || min_points < 0 ||
        min_points > kMaxMapPoints || !n_out || !counts ||
        (n > 0 && (!points || !host || !tracks4 || !out_points || !out_host || !out_tracks4 || !keep)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t m = (size_t)std::max(n, 1);
    Bump b;
    const size_t o_p = b.take(24 * m), o_h = b.take(4 * m), o_t = b.take(16 * m);
    int rc = c->scratch_a.ensure(b.off);
    if (!rc) rc = c->scratch_c.ensure(point_cull_scratch_bytes(n));
    if (rc) return rc;
    char* base = (char*)c->scratch_a.ptr;
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_h, host, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_t, tracks4, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    PointCullArgs a{};
    point_cull_scratch_at(a, c->scratch_c.ptr, n);
    a.pts = (const double*)(base + o_p);
    a.n = n;
    a.tracks = (int4*)(base + o_t);
    a.host = (const int*)(base + o_h);
    a.max_fail_run = max_fail_run;
    a.min_points = min_points;
    launch_point_cull(a, c->stream);
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_int + 16, a.ccounts, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int kept = std::max(0, std::min(c->h_int[18], n));
    if (n > 0) VISO_HIP_CHECK(hipMemcpyAsync(keep, a.keep, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (kept > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(out_points, a.out_pts, 24 * (size_t)kept, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(out_host, a.out_host, 4 * (size_t)kept, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(out_tracks4, a.out_tracks, 16 * (size_t)kept, hipMemcpyDeviceToHost,
                                      c->stream));
    }
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    *n_out = (size_t)kept;
    counts[0] = c->h_int[16];
    counts[1] = c->h_int[17];
    counts[2] = kept;
    counts[3] = c->h_int[19];
    return VISO_OK;
}

}  // extern "C"
