// viso_amd — sliding-window map: the oldest keyframe is retired and the points
// it hosts are culled (viso_set_map_window, include/viso/viso_c.h; DESIGN.md
// §Sliding-window map).  The repo's own spec, restated in
// tests/map_window_ref.py: the reference's map (src/viso.cpp:79-96) never
// loses a point.
//
// One retirement, keyframe 0 leaving, check frame c: (1) every point is
// projected into c (the arithmetic of the monocular occupancy, monokf.hip) and
// the live ones (host != 0) mark their cell, (2) a retired-host point that c
// sees in an unmarked cell and that a remaining keyframe sees claims its
// cell, the highest index winning, its new host the newest keyframe that sees
// it, (3) keep flags, a stable compaction of points and hosts into scratch,
// the keyframe poses shifted down one row.
//
// Mapping: one lane per point in (1) and (2); (3) is one workgroup walking
// the map 1024 points a round (block_rank.hpp).  Every count is formed on the
// device; the only atomics are integer (a maximum per cell, three sums), so
// the result depends on nothing but the data.  fp64 in the operand order of tests/map_window_ref.py,
// -ffp-contract=off.
#include <algorithm>
#include <vector>

#include "block_rank.hpp"
#include "context.hpp"
#include "device_math.hpp"
#include "linalg.hpp"

namespace viso {

namespace {

// (1) every point's cell in c; a live point marks it (every marking lane
// stores the same value)
__global__ __launch_bounds__(256) void mapwin_project_kernel(MapWinArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int cell = seen_cell(a, a.pose_c, a.pts + 3 * (size_t)i);
    a.pt_cell[i] = cell;
    if (cell >= 0 && a.host[i] != 0) a.cell_mark[cell] = 1;
}

// (2) retired-host points: a candidate (seen by c in an unmarked cell and by
// a remaining keyframe, scanned newest first for the new host) claims its
// cell with its index; every point's new host (-1: a retired-host point that
// is no candidate)
__global__ __launch_bounds__(256) void mapwin_claim_kernel(MapWinArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < a.n;
    const int h = in ? a.host[i] : 1;
    const bool retired = in && h == 0;
    const int cell = retired ? a.pt_cell[i] : -1;
    int nh = -1;
    if (cell >= 0 && a.cell_mark[cell] == 0) {
        const double* P = a.pts + 3 * (size_t)i;
        for (int k = a.n_kf - 1; k >= 1; --k) {
            if (seen_cell(a, a.kf_poses + 12 * k, P) >= 0) {
                nh = k - 1;
                break;
            }
        }
    }
    if (nh >= 0) atomicMax(a.cell_win + cell, i);
    if (in) a.new_host[i] = retired ? nh : h - 1;
    const unsigned long long br = __ballot(retired), bv = __ballot(cell >= 0), bc = __ballot(nh >= 0);
    if (lane == 0 && br) {
        atomicAdd(a.counts + 0, __popcll(br));
        if (bv) atomicAdd(a.counts + 1, __popcll(bv));
        if (bc) atomicAdd(a.counts + 2, __popcll(bc));
    }
}

// (3) keep flags and the stable compaction (one workgroup), then the pose
// rows: kept points and their new hosts in index order into out_pts /
// out_host (and, with track records, their rows into out_rec); counts[3] =
// survivors, counts[4] = kept; with something kept and shift_poses set,
// keyframe pose row k + 1 moves to row k
__global__ __launch_bounds__(1024) void mapwin_compact_kernel(MapWinArgs a) {
    __shared__ int s_w[2 * 16];
    const int tid = threadIdx.x;
    int base = 0, surv = 0;
    for (int i0 = 0; i0 < a.n; i0 += 1024) {
        const int i = i0 + tid;
        bool f = false, s = false;
        int nh = -1;
        if (i < a.n) {
            nh = a.new_host[i];
            if (a.host[i] != 0) {
                f = true;
            } else if (nh >= 0) {
                s = a.cell_win[a.pt_cell[i]] == i;
                f = s;
            }
            a.keep[i] = f ? 1 : 0;
        }
        const bool flags[2] = {f, s};
        BlockRank r[2];  // (of the survivors only the count)
        block_rank<16>(flags, s_w, r);
        if (f) {
            const size_t j = (size_t)(base + r[0].rank);
            a.out_pts[3 * j] = a.pts[3 * (size_t)i];
            a.out_pts[3 * j + 1] = a.pts[3 * (size_t)i + 1];
            a.out_pts[3 * j + 2] = a.pts[3 * (size_t)i + 2];
            a.out_host[j] = nh;
            if (a.rec) a.out_rec[j] = a.rec[i];
        }
        base += r[0].total;
        surv += r[1].total;
    }
    if (tid == 0) {
        a.counts[3] = surv;
        a.counts[4] = base;
    }
    // (the claim pass, the rows' last reader, ran in an earlier launch)
    if (a.shift_poses && base > 0) {
        const int m = 12 * (a.n_kf - 1);
        const double v = tid < m ? a.kf_poses[12 + tid] : 0.0;
        __syncthreads();
        if (tid < m) a.kf_poses[tid] = v;
    }
}

}  // namespace

size_t map_window_scratch_bytes(int w, int h, int cell, int cap_points) {
    MapWinArgs a{};
    return map_window_scratch_at(a, nullptr, w, h, cell, cap_points);
}

size_t map_window_scratch_at(MapWinArgs& a, void* base, int w, int h, int cell, int cap_points) {
    const size_t cells = (size_t)mono_kf_cells(w, h, cell), n = (size_t)std::max(cap_points, 1);
    Bump b;
    // (marks and counts share the zero fill)
    const size_t o_cnt = b.take(32), o_mark = b.take(4 * cells), o_zero_end = b.off, o_win = b.take(4 * cells),
                 o_pc = b.take(4 * n), o_nh = b.take(4 * n), o_keep = b.take(n), o_oh = b.take(4 * n),
                 o_op = b.take(24 * n), o_or = b.take(16 * n);
    if (base) {
        char* p = (char*)base;
        a.w = w;
        a.h = h;
        a.cell = cell;
        a.ncx = (w + cell - 1) / cell;
        a.ncy = (h + cell - 1) / cell;
        a.counts = (int*)(p + o_cnt);
        a.cell_mark = (int*)(p + o_mark);
        a.zero_bytes = o_zero_end - o_cnt;
        a.cell_win = (int*)(p + o_win);
        a.pt_cell = (int*)(p + o_pc);
        a.new_host = (int*)(p + o_nh);
        a.keep = (uint8_t*)(p + o_keep);
        a.out_host = (int*)(p + o_oh);
        a.out_pts = (double*)(p + o_op);
        a.out_rec = (int4*)(p + o_or);
    }
    return b.off;
}

void launch_map_retire(const MapWinArgs& a, hipStream_t stream) {
    (void)hipMemsetAsync(a.counts, 0, a.zero_bytes, stream);
    (void)hipMemsetAsync(a.cell_win, 0xFF, 4 * (size_t)a.ncx * a.ncy, stream);  // -1: no candidate
    if (a.n > 0) {
        const int blocks = (a.n + 255) / 256;
        mapwin_project_kernel<<<blocks, 256, 0, stream>>>(a);
        mapwin_claim_kernel<<<blocks, 256, 0, stream>>>(a);
    }
    mapwin_compact_kernel<<<1, 1024, 0, stream>>>(a);
}

}  // namespace viso

using namespace viso;

int viso_ctx::begin_map_rewrite(bool upload_hosts) {
    if (int rc = order_after_lk(lk_seq - 1, stream)) return rc;
    if (bg_done) VISO_HIP_CHECK(hipStreamWaitEvent(stream, bg_done, 0));
    if (upload_hosts && n_map > 0)
        VISO_HIP_CHECK(hipMemcpyAsync(point_host_dev.ptr, point_host.data(), 4 * (size_t)n_map,
                                      hipMemcpyHostToDevice, stream));
    return VISO_OK;
}

int viso_ctx::end_map_rewrite(const double* pts, const void* rec, const std::vector<int32_t>& hosts, int kept) {
    if (kept > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(map_pts.ptr, pts, 24 * (size_t)kept, hipMemcpyDeviceToDevice, stream));
        if (rec)
            VISO_HIP_CHECK(hipMemcpyAsync(pt_tracks.ptr, rec, 16 * (size_t)kept, hipMemcpyDeviceToDevice, stream));
    }
    point_host.assign(hosts.begin(), hosts.begin() + kept);
    n_map = kept;
    return VISO_OK;
}

// One retirement in the frame path (on_new_frame's insertion check, ahead of
// the check's insertion; cur's pose is final and every earlier LK batch has
// been launched: finish_call).  The cull rewrites map_pts and kf_poses in
// place and the LK templates are rebuilt behind it: a map rewrite
// (begin_map_rewrite).  Two read-backs in one host sync: the counts and the new
// hosts.  *retired = false: nothing would be kept, map and keyframes are
// unchanged.
int viso_ctx::retire_keyframe(int cur, bool* retired) {
    *retired = false;
    const PyrGeom& g = geom;
    const int n = n_map, nk = (int)kf_slots.size();
    if (nk < 1 || (int)point_host.size() != n) return VISO_ERR_STATE;
    int rc = mapwin_buf.ensure(map_window_scratch_bytes(g.w[0], g.h[0], win_cell, kMaxMapPoints));
    if (!rc) rc = point_host_dev.ensure(4 * (size_t)kMaxMapPoints);
    if (rc) return rc;
    if (int r2 = begin_map_rewrite(true)) return r2;
    MapWinArgs a{};
    map_window_scratch_at(a, mapwin_buf.ptr, g.w[0], g.h[0], win_cell, kMaxMapPoints);
    intrinsics(a.K);
    a.pose_c = pose_of(cur);
    a.kf_poses = (double*)kf_poses.ptr;
    a.n_kf = nk;
    a.shift_poses = 1;
    a.pts = (const double*)map_pts.ptr;
    a.host = (const int*)point_host_dev.ptr;
    a.n = n;
    a.rec = cull_on() ? (const int4*)pt_tracks.ptr : nullptr;  // (viso_set_point_cull: a kept point's record moves with it)
    {
        TimedRegion t(timing, VISO_KERNEL_MAPWIN, stream);
        launch_map_retire(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    std::vector<int32_t> hosts((size_t)std::max(n, 1));
    VISO_HIP_CHECK(hipMemcpyAsync(h_int + 8, a.counts, 5 * sizeof(int), hipMemcpyDeviceToHost, stream));
    if (n > 0)
        VISO_HIP_CHECK(hipMemcpyAsync(hosts.data(), a.out_host, 4 * (size_t)n, hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    const int kept = std::max(0, std::min(h_int[12], n));
    if (kept == 0) return VISO_OK;
    if (int r2 = end_map_rewrite(a.out_pts, a.rec ? a.out_rec : nullptr, hosts, kept)) return r2;
    // the slot's readers on lk_stream are its lk_use batch, those on the
    // context stream end with this call's epoch: acquire_slot / wait_freed
    // order its reuse behind both
    const int s = kf_slots.front();
    kf_slots.erase(kf_slots.begin());
    drop(s);
    win_retired += 1;
    win_culled += n - kept;
    win_last[0] = frames;
    win_last[1] = h_int[8];
    win_last[2] = h_int[11];
    win_last[3] = kept;
    *retired = true;
    return retire_seeds();  // (viso_set_depth_seeds: the retired keyframe's seeds go with it)
}

extern "C" {

int viso_set_map_window(viso_ctx* c, int32_t window, int32_t cell) {
    if (!c || !(window == 0 || (window >= 2 && window <= kMaxKeyframes && cell >= 8 && cell <= 64)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    if (window > 0 && (int)c->kf_slots.size() > window) return VISO_ERR_STATE;
    if (window > 0) {
        // the retirement's buffers now, not inside its first check frame
        VISO_HIP_CHECK(hipSetDevice(c->device));
        int rc = c->mapwin_buf.ensure(map_window_scratch_bytes(c->geom.w[0], c->geom.h[0], cell, kMaxMapPoints));
        if (!rc) rc = c->point_host_dev.ensure(4 * (size_t)kMaxMapPoints);
        if (rc) return rc;
        c->win_cell = cell;
    }
    c->win_size = window;
    return VISO_OK;
}

int viso_get_map_window(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    info[0] = c->win_size;
    info[1] = c->win_cell;
    info[2] = c->win_retired;
    info[3] = c->win_culled;
    for (int k = 0; k < 4; ++k) info[4 + k] = c->win_last[k];
    return VISO_OK;
}

int viso_get_point_hosts(viso_ctx* c, int32_t* host, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    const size_t m = std::min(cap, c->point_host.size());
    if (host)
        for (size_t i = 0; i < m; ++i) host[i] = c->point_host[i];
    if (n) *n = c->point_host.size();
    return VISO_OK;
}

int viso_map_retire(viso_ctx* c, int32_t width, int32_t height, const double pose_c[12], const double* kf_poses,
                    int32_t n_kf, const double* points, const int32_t* host, int32_t n, int32_t cell,
                    double* out_points, int32_t* out_host, uint8_t* keep, size_t* n_out, int32_t counts[4]) {
    if (!c || !pose_c || !kf_poses || width < 16 || height < 16 || width > kMaxWidth || n_kf < 1 ||
        n_kf > kMaxKeyframes || n < 0 || n > kMaxMapPoints || cell < 8 || cell > 64 ||
        (n > 0 && (!points || !host || !out_points || !out_host || !keep)))
        return VISO_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (host[i] < 0 || host[i] >= n_kf) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    Bump b;
    const size_t o_pc = b.take(96), o_pk = b.take(96 * (size_t)n_kf), o_p = b.take(24 * (size_t)std::max(n, 1)),
                 o_h = b.take(4 * (size_t)std::max(n, 1));
    int rc = c->scratch_a.ensure(b.off);
    if (!rc) rc = c->scratch_c.ensure(map_window_scratch_bytes(width, height, cell, n));
    if (rc) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_pc, pose_c, 96, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_pk, kf_poses, 96 * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_h, host, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    MapWinArgs a{};
    map_window_scratch_at(a, c->scratch_c.ptr, width, height, cell, n);
    c->intrinsics(a.K);
    a.pose_c = (const double*)(base + o_pc);
    a.kf_poses = (double*)(base + o_pk);
    a.n_kf = n_kf;
    a.shift_poses = 0;
    a.pts = (const double*)(base + o_p);
    a.host = (const int*)(base + o_h);
    a.n = n;
    launch_map_retire(a, c->stream);
    VISO_HIP_CHECK(hipGetLastError());
    int32_t cnt[5] = {0, 0, 0, 0, 0};
    VISO_HIP_CHECK(hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int m = std::max(0, std::min(cnt[4], n));
    if (n > 0) VISO_HIP_CHECK(hipMemcpyAsync(keep, a.keep, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (m > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(out_points, a.out_pts, 24 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(out_host, a.out_host, 4 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    }
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n_out) *n_out = (size_t)m;
    if (counts)
        for (int k = 0; k < 4; ++k) counts[k] = cnt[k];
    return VISO_OK;
}

}  // extern "C"
