// viso_amd — point refinement (viso_set_point_refine, include/viso/viso_c.h;
// DESIGN.md §Point refinement).  The repo's own spec, restated in
// tests/point_refine_ref.py: the structure half of the "pose and structure
// refinement" on the LK-aligned positions (LKAlignment, src/viso.cpp:768-843),
// which the reference only draws; its map points (src/viso.cpp:79-96) keep
// the coordinates of their creation.
//
// A point's LK template is its anchor keyframe's patch at the point's
// projection there, so the aligned positions measure the depth along the ray
// from the anchor's centre C through the point: P = C + D moves to
// C + D / (1 + delta), a Gauss-Newton step on the relative inverse depth over
// the observations of an observation ring (the last frames' poses and, per
// point, a flag and the aligned position).
//
// Mapping: the record is one lane per point.  The refinement gives a point
// eight lanes, one per ring slot, eight points a wave: the three sums of a
// pass (H, b, cost) are the pairwise tree over slots 0..7 by xor shuffles 1,
// 2, 4 — every lane of a point ends with the same bits, those of one lane
// adding in tree order — so a point's decisions are uniform over its lanes
// and a per-point done flag stands in for an early return.  The frame counts
// go through ballots and integer atomics.  fp64 in the operand order of
// tests/point_refine_ref.py, -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <vector>

#include "context.hpp"
#include "linalg.hpp"

namespace viso {

namespace {

constexpr int kPtsPerBlock = 256 / kMaxObsSlots;

__global__ __launch_bounds__(256) void point_obs_kernel(PointObsArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 12 && a.pose) a.pose_out[threadIdx.x] = a.pose[threadIdx.x];
    if (i >= a.n) return;
    const double u = a.uv_after[2 * (size_t)i], v = a.uv_after[2 * (size_t)i + 1];
    const double d0 = u - a.uv_before[2 * (size_t)i], d1 = v - a.uv_before[2 * (size_t)i + 1];
    const bool f = a.pair_kf[i] >= 0 && a.success[i] != 0 && d0 * d0 + d1 * d1 <= a.max_shift * a.max_shift;
    a.valid_out[i] = f ? 1 : 0;
    a.uv_out[2 * (size_t)i] = u;
    a.uv_out[2 * (size_t)i + 1] = v;
}

// ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) in every lane of a point
__device__ inline double tree8(double v) {
    v = v + __shfl_xor(v, 1, 64);
    v = v + __shfl_xor(v, 2, 64);
    v = v + __shfl_xor(v, 4, 64);
    return v;
}

__device__ inline int sum8(int v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

__global__ __launch_bounds__(256) void point_refine_kernel(PointRefineArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, s = tid & (kMaxObsSlots - 1);
    const int i = blockIdx.x * kPtsPerBlock + (tid >> 3);
    const bool in = i < a.n;
    // the slot's observation of the point and its pose
    bool has = false;
    double T[12], u = 0.0, v = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = 0.0;
    if (in && s < a.m) {
        const size_t o = (size_t)s * a.stride + (size_t)i;
        has = a.valid[o] != 0;
        if (has) {
            u = a.uv[2 * o];
            v = a.uv[2 * o + 1];
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = a.poses[12 * s + k];
        }
    }
    const int n_obs = sum8(has ? 1 : 0);
    // the point, its anchor's centre
    int anchor = -1;
    double P[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
    if (in) {
        anchor = a.anchor_kf[i];
        if (anchor >= a.n_kf) anchor = -1;
#pragma unroll
        for (int j = 0; j < 3; ++j) P[j] = a.pts[3 * (size_t)i + j];
        if (anchor >= 0) {
            const double* A = a.kf_poses + 12 * (size_t)anchor;
#pragma unroll
            for (int j = 0; j < 3; ++j) C[j] = -((A[j] * A[9] + A[3 + j] * A[10]) + A[6 + j] * A[11]);
        }
    }
    const bool eligible = in && anchor >= 0 && n_obs >= a.min_obs;
    int status = !in ? 0 : anchor < 0 ? 5 : 1;
    int steps = 0;
    bool done = !eligible;
    double Pp[3] = {P[0], P[1], P[2]};  // P_{k-1}
    double cost0 = 0.0, cost_res = 0.0, cost_prev = 0.0;
    const double sig2 = a.max_rel_sigma * a.max_rel_sigma;
    for (int k = 0; k <= a.iterations; ++k) {
        double hs = 0.0, bs = 0.0, cs = 0.0;
        int us = 0;
        const double D[3] = {P[0] - C[0], P[1] - C[1], P[2] - C[2]};
        if (has && !done) {
            double Pc[3], Dc[3];
            mat3_vec(T, P, Pc);
            const double x = Pc[0] + T[9], y = Pc[1] + T[10], z = Pc[2] + T[11];
            if (z > 0) {
                mat3_vec(T, D, Dc);
                const double r0 = u - (a.K[0] * x / z + a.K[2]);
                const double r1 = v - (a.K[1] * y / z + a.K[3]);
                const double e2 = r0 * r0 + r1 * r1;
                const double e = sqrt(e2);
                const bool inl = e <= a.huber;
                const double w = inl ? 1.0 : a.huber / e;
                const double rho = inl ? 0.5 * e2 : a.huber * (e - 0.5 * a.huber);
                const double g0 = a.K[0] * (x * Dc[2] / (z * z) - Dc[0] / z);
                const double g1 = a.K[1] * (y * Dc[2] / (z * z) - Dc[1] / z);
                hs = w * (g0 * g0 + g1 * g1);
                bs = w * (g0 * r0 + g1 * r1);
                cs = rho;
                us = 1;
            }
        }
        const double H = tree8(hs), b = tree8(bs), cost = tree8(cs);
        const int used = sum8(us);
        if (done) continue;  // (uniform over the point's lanes; the shuffles above are not skipped)
        if (k == 0) {
            cost0 = cost;
            cost_res = cost;
            if (used < a.min_obs) {
                status = 1;
                done = true;
                continue;
            }
            if (H * sig2 < 1.0) {
                status = 4;
                done = true;
                continue;
            }
        } else if (cost >= cost_prev) {
            P[0] = Pp[0];
            P[1] = Pp[1];
            P[2] = Pp[2];
            status = 3;
            steps = k - 1;
            cost_res = cost_prev;
            done = true;
            continue;
        }
        steps = k;
        cost_res = cost;
        if (k == a.iterations) {
            status = 0;
            done = true;
            continue;
        }
        const double delta = b / H, q = 1.0 + delta;
        if (!isfinite(delta) || !(0.5 < q && q < 2.0)) {
            status = 2;
            done = true;
            continue;
        }
        cost_prev = cost;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Pp[j] = P[j];
            P[j] = C[j] + D[j] / q;
        }
    }
    const bool lead = in && s == 0;
    if (lead) {
        if (steps >= 1) {
#pragma unroll
            for (int j = 0; j < 3; ++j) a.pts[3 * (size_t)i + j] = P[j];
        }
        a.status[i] = (uint8_t)status;
        a.steps[i] = (uint8_t)steps;
        a.costs[2 * (size_t)i] = cost0;
        a.costs[2 * (size_t)i + 1] = cost_res;
    }
    const unsigned long long be = __ballot(lead && eligible), bm = __ballot(lead && steps >= 1),
                             b4 = __ballot(lead && status == 4), b2 = __ballot(lead && status == 2);
    if (lane == 0) {
        if (be) atomicAdd(a.counts + 0, __popcll(be));
        if (bm) {
            atomicAdd(a.counts + 1, __popcll(bm));
            if (a.moved_total) atomicAdd(a.moved_total, (unsigned long long)__popcll(bm));
        }
        if (b4) atomicAdd(a.counts + 2, __popcll(b4));
        if (b2) atomicAdd(a.counts + 3, __popcll(b2));
    }
}

}  // namespace

void launch_point_obs(const PointObsArgs& a, hipStream_t stream) {
    point_obs_kernel<<<std::max(1, (a.n + 255) / 256), 256, 0, stream>>>(a);
}

void launch_point_refine(const PointRefineArgs& a, hipStream_t stream) {
    (void)hipMemsetAsync(a.counts, 0, 4 * sizeof(int), stream);
    if (a.n > 0) point_refine_kernel<<<(a.n + kPtsPerBlock - 1) / kPtsPerBlock, 256, 0, stream>>>(a);
}

}  // namespace viso

using namespace viso;

namespace {

bool prefine_params_ok(int32_t interval, int32_t window, int32_t iterations, double huber_px, double max_shift_px,
                       int32_t min_obs, double max_rel_sigma) {
    return interval >= 1 && window >= 2 && window <= kMaxObsSlots && iterations >= 1 && iterations <= 10 &&
           std::isfinite(huber_px) && huber_px > 0 && std::isfinite(max_shift_px) && max_shift_px > 0 &&
           min_obs >= 1 && min_obs <= window && std::isfinite(max_rel_sigma) && max_rel_sigma > 0 &&
           max_rel_sigma <= 1;
}

// the mode's device buffer: the counters, the ring, the last refinement's
// per-point results
struct PrefineBuf {
    int* counts;                  // 4: the last refinement's
    unsigned long long* moved;    // points moved in all
    double* poses;                // window x 12
    uint8_t* valid;               // window x kMaxMapPoints
    double* uv;                   // window x kMaxMapPoints x 2
    uint8_t *status, *steps;      // kMaxMapPoints each
    double* costs;                // kMaxMapPoints x 2
};

size_t prefine_buf_at(PrefineBuf& r, void* base, int window) {
    const size_t n = (size_t)kMaxMapPoints, w = (size_t)window;
    Bump b;
    const size_t o_cnt = b.take(32), o_pose = b.take(96 * w), o_valid = b.take(w * n), o_uv = b.take(16 * w * n),
                 o_st = b.take(n), o_sp = b.take(n), o_c = b.take(16 * n);
    if (base) {
        char* p = (char*)base;
        r.counts = (int*)(p + o_cnt);
        r.moved = (unsigned long long*)(p + o_cnt + 16);
        r.poses = (double*)(p + o_pose);
        r.valid = (uint8_t*)(p + o_valid);
        r.uv = (double*)(p + o_uv);
        r.status = (uint8_t*)(p + o_st);
        r.steps = (uint8_t*)(p + o_sp);
        r.costs = (double*)(p + o_c);
    }
    return b.off;
}

}  // namespace

// One tracking frame's record in the frame path (on_new_frame, behind
// finish_call on the context stream, the pose refinement and the track
// update: cur's pose is final, its LK alignment is the last row of the LK
// buffers).  No host synchronisation.
int viso_ctx::record_obs(int cur) {
    if (n_map <= 0 || lk_last_rows < 1 || lk_last_pts != n_map) return VISO_ERR_STATE;
    const size_t o = (size_t)(lk_last_rows - 1) * kMaxMapPoints;  // cur's row: the batch's last
    PrefineBuf r{};
    prefine_buf_at(r, prefine_buf.ptr, prefine_window);
    const size_t slot = (size_t)(prefine_count % prefine_window);
    PointObsArgs a{};
    a.n = n_map;
    a.pair_kf = (const int32_t*)lk_pair.ptr + o;
    a.success = (const uint8_t*)lk_succ.ptr + o;
    a.uv_before = (const double*)lk_before.ptr + 2 * o;
    a.uv_after = (const double*)lk_after.ptr + 2 * o;
    a.max_shift = prefine_max_shift;
    a.pose = pose_of(cur);
    a.valid_out = r.valid + slot * kMaxMapPoints;
    a.uv_out = r.uv + 2 * slot * kMaxMapPoints;
    a.pose_out = r.poses + 12 * slot;
    {
        TimedRegion t(timing, VISO_KERNEL_POINTS, stream);
        launch_point_obs(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    prefine_count += 1;
    return VISO_OK;
}

// One refinement in the frame path (on_new_frame, right behind the frame's
// record, ahead of its cull and its insertion check).  map_pts is rewritten
// in place, so the context stream is first ordered behind every reader on
// lk_stream, as a cull (pointcull.hip).  No host synchronisation: the getters
// read the counters.
int viso_ctx::refine_points() {
    const int n = n_map;
    if (n <= 0 || prefine_count <= 0 || !lk_tmpl_kf.ptr) return VISO_OK;
    if (int rc = order_after_lk(lk_seq - 1, stream)) return rc;
    if (bg_done) VISO_HIP_CHECK(hipStreamWaitEvent(stream, bg_done, 0));
    PrefineBuf r{};
    prefine_buf_at(r, prefine_buf.ptr, prefine_window);
    PointRefineArgs a{};
    intrinsics(a.K);
    a.pts = (double*)map_pts.ptr;
    a.n = n;
    a.anchor_kf = (const int32_t*)lk_tmpl_kf.ptr;
    a.kf_poses = (const double*)kf_poses.ptr;
    a.n_kf = (int)kf_slots.size();
    a.poses = r.poses;
    a.valid = r.valid;
    a.uv = r.uv;
    a.stride = kMaxMapPoints;
    a.m = (int)std::min<int64_t>(prefine_count, prefine_window);
    a.iterations = prefine_iterations;
    a.min_obs = prefine_min_obs;
    a.huber = prefine_huber;
    a.max_rel_sigma = prefine_sigma;
    a.status = r.status;
    a.steps = r.steps;
    a.costs = r.costs;
    a.counts = r.counts;
    a.moved_total = r.moved;
    {
        TimedRegion t(timing, VISO_KERNEL_POINTS, stream);
        launch_point_refine(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    prefine_runs += 1;
    prefine_last_frame = frames;
    prefine_last_n = n;
    return VISO_OK;
}

extern "C" {

int viso_set_point_refine(viso_ctx* c, int32_t interval, int32_t window, int32_t iterations, double huber_px,
                          double max_shift_px, int32_t min_obs, double max_rel_sigma) {
    if (!c || !(interval == 0 ||
                prefine_params_ok(interval, window, iterations, huber_px, max_shift_px, min_obs, max_rel_sigma)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    if (interval > 0) {
        PrefineBuf r{};
        const size_t bytes = prefine_buf_at(r, nullptr, window);
        if (!c->prefine_on() || window != c->prefine_window) {
            // the ring and the counters start empty (with another window
            // too: the buffer is laid out by it)
            VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
            if (int rc = c->prefine_buf.ensure(bytes)) return rc;
            prefine_buf_at(r, c->prefine_buf.ptr, window);
            VISO_HIP_CHECK(hipMemsetAsync(r.counts, 0, 32, c->stream));
            c->prefine_runs = 0;
            c->prefine_last_frame = -1;
            c->prefine_last_n = 0;
            c->prefine_count = 0;
        }
        c->prefine_window = window;
        c->prefine_iterations = iterations;
        c->prefine_huber = huber_px;
        c->prefine_max_shift = max_shift_px;
        c->prefine_min_obs = min_obs;
        c->prefine_sigma = max_rel_sigma;
    } else if (c->prefine_on()) {
        VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
        c->prefine_buf.release();
        c->prefine_window = 0;
        c->prefine_count = 0;
    }
    c->prefine_interval = interval;
    return VISO_OK;
}

int viso_get_point_refine(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[4] = -1;
    if (!c->prefine_on()) return VISO_OK;
    VISO_HIP_CHECK(hipSetDevice(c->device));
    PrefineBuf r{};
    prefine_buf_at(r, c->prefine_buf.ptr, c->prefine_window);
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_int + 24, r.counts, 32, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    unsigned long long moved = 0;
    std::memcpy(&moved, c->h_int + 28, sizeof(moved));
    info[0] = c->prefine_interval;
    info[1] = c->prefine_window;
    info[2] = c->prefine_runs;
    info[3] = (int64_t)moved;
    info[4] = c->prefine_last_frame;
    if (c->prefine_runs > 0) {
        info[5] = c->h_int[24];
        info[6] = c->h_int[25];
        info[7] = c->h_int[26];
    }
    return VISO_OK;
}

int viso_get_point_refine_status(viso_ctx* c, uint8_t* status, uint8_t* steps, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (!c->prefine_on()) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    PrefineBuf r{};
    prefine_buf_at(r, c->prefine_buf.ptr, c->prefine_window);
    const size_t m = std::min(cap, (size_t)c->prefine_last_n);
    if (m > 0 && status) VISO_HIP_CHECK(hipMemcpyAsync(status, r.status, m, hipMemcpyDeviceToHost, c->stream));
    if (m > 0 && steps) VISO_HIP_CHECK(hipMemcpyAsync(steps, r.steps, m, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n) *n = (size_t)c->prefine_last_n;
    return VISO_OK;
}

int viso_point_obs_record(viso_ctx* c, const int32_t* pair_kf, const uint8_t* success, const double* uv_before,
                          const double* uv_after, int32_t n, double max_shift_px, uint8_t* valid_out,
                          double* uv_out) {
    if (!c || n < 0 || n > kMaxMapPoints || !(max_shift_px > 0) || !std::isfinite(max_shift_px) ||
        (n > 0 && (!pair_kf || !success || !uv_before || !uv_after || !valid_out || !uv_out)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t m = (size_t)std::max(n, 1);
    Bump b;
    const size_t o_pk = b.take(4 * m), o_sc = b.take(m), o_ub = b.take(16 * m), o_ua = b.take(16 * m),
                 o_v = b.take(m), o_uv = b.take(16 * m);
    if (int rc = c->scratch_a.ensure(b.off)) return rc;
    char* base = (char*)c->scratch_a.ptr;
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_pk, pair_kf, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_sc, success, (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_ub, uv_before, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_ua, uv_after, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    PointObsArgs a{};
    a.n = n;
    a.pair_kf = (const int32_t*)(base + o_pk);
    a.success = (const uint8_t*)(base + o_sc);
    a.uv_before = (const double*)(base + o_ub);
    a.uv_after = (const double*)(base + o_ua);
    a.max_shift = max_shift_px;
    a.valid_out = (uint8_t*)(base + o_v);
    a.uv_out = (double*)(base + o_uv);
    launch_point_obs(a, c->stream);
    VISO_HIP_CHECK(hipGetLastError());
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(valid_out, a.valid_out, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(uv_out, a.uv_out, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

int viso_points_refine(viso_ctx* c, const double* points, const int32_t* anchor_kf, int32_t n, const double* kf_poses,
                       int32_t n_kf, const double* frame_poses, int32_t m, const uint8_t* obs_valid,
                       const double* obs_uv, int32_t iterations, double huber_px, int32_t min_obs,
                       double max_rel_sigma, double* out_points, uint8_t* status, uint8_t* steps, double* costs,
                       int32_t counts[4]) {
    if (!c || n < 0 || n > kMaxMapPoints || m < 1 || m > kMaxObsSlots || n_kf < 1 || n_kf > kMaxKeyframes ||
        !kf_poses || !frame_poses || !counts || iterations < 1 || iterations > 10 || !std::isfinite(huber_px) ||
        !(huber_px > 0) || min_obs < 1 || min_obs > kMaxObsSlots || !std::isfinite(max_rel_sigma) ||
        !(max_rel_sigma > 0) || max_rel_sigma > 1 ||
        (n > 0 && (!points || !anchor_kf || !obs_valid || !obs_uv || !out_points || !status || !steps || !costs)))
        return VISO_ERR_ARG;
    for (int32_t i = 0; i < n; ++i)
        if (anchor_kf[i] >= n_kf) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t q = (size_t)std::max(n, 1), w = (size_t)m;
    Bump b;
    const size_t o_cnt = b.take(32), o_kf = b.take(96 * (size_t)n_kf), o_fp = b.take(96 * w), o_p = b.take(24 * q),
                 o_a = b.take(4 * q), o_v = b.take(w * q), o_uv = b.take(16 * w * q), o_st = b.take(q),
                 o_sp = b.take(q), o_c = b.take(16 * q);
    if (int rc = c->scratch_a.ensure(b.off)) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_kf, kf_poses, 96 * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_fp, frame_poses, 96 * w, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_a, anchor_kf, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_v, obs_valid, w * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_uv, obs_uv, 16 * w * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    PointRefineArgs a{};
    c->intrinsics(a.K);
    a.pts = (double*)(base + o_p);
    a.n = n;
    a.anchor_kf = (const int32_t*)(base + o_a);
    a.kf_poses = (const double*)(base + o_kf);
    a.n_kf = n_kf;
    a.poses = (const double*)(base + o_fp);
    a.valid = (const uint8_t*)(base + o_v);
    a.uv = (const double*)(base + o_uv);
    a.stride = (size_t)n;
    a.m = m;
    a.iterations = iterations;
    a.min_obs = min_obs;
    a.huber = huber_px;
    a.max_rel_sigma = max_rel_sigma;
    a.status = (uint8_t*)(base + o_st);
    a.steps = (uint8_t*)(base + o_sp);
    a.costs = (double*)(base + o_c);
    a.counts = (int*)(base + o_cnt);
    a.moved_total = nullptr;
    launch_point_refine(a, c->stream);
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_int + 24, a.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(out_points, a.pts, 24 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(status, a.status, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(steps, a.steps, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(costs, a.costs, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; ++k) counts[k] = c->h_int[24 + k];
    return VISO_OK;
}

}  // extern "C"
