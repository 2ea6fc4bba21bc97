// viso_amd — pose refinement on the LK-aligned features (viso_set_pose_refine,
// include/viso/viso_c.h; DESIGN.md §Pose refinement).  The repo's own spec,
// restated in tests/pose_refine_ref.py: the reference computes the aligned
// positions (LKAlignment, src/viso.cpp:121) and only draws them
// (src/viso.cpp:123-135).
//
// One frame: Gauss-Newton with Huber weights on the reprojection error of the
// frame's LK row (uv_after against the projection of the map points), from the
// direct pose X.  Pass k at T_k forms n_k, cost_k, H = sum w J^T J and
// b = sum w J^T r (J = dPixeldXi, src/viso.cpp:640-658, scale 1); the decisions
// (too few observations, a cost that did not fall, the last pass, a
// non-finite step) and the update T_{k+1} = exp(xi) T_k are made on the device.
//
// Mapping: one launch of one workgroup of 1,024 lanes.  Lane l takes the
// points l, l + 1024, ... in ascending order (at most 16: the map's capacity),
// every sum starting at +0.0; a wave adds its 64 lane values by xor shuffles
// (neighbours first: 1, 2, 4, ... 32), the 16 wave values are added
// neighbours first through LDS — one balanced binary tree over the 1,024
// lanes, the order tests/pose_refine_ref.py restates.  No float atomics, no
// inline assembly; wave 0 solves and decides, the pose goes round through
// LDS.  fp64 in both precision modes, -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <limits>

#include "context.hpp"
#include "device_math.hpp"

namespace viso {

namespace {

constexpr int kRefLanes = 1024;
constexpr int kRefWaves = kRefLanes / 64;
constexpr int kRefSums = 29;  // H upper triangle (21, row-major), b (6), cost, sum of e^2

struct RefineLds {
    double red[kRefWaves][kRefSums];
    int cnt[kRefWaves][3];
    double S[kRefSums];
    int N[3];  // used, inliers, observations
    double T[12];
    int done;
    // wave 0's: pass k - 1 (T_{k-1} and its sums) and pass 0
    double prevT[12], prev_cost, prev_rms, cost0, rms0;
    int prev_inl;
};

// balanced tree over the 16 wave values of one sum, neighbours first
__device__ inline double tree16(const double (*red)[kRefSums], int s) {
    double v[kRefWaves];
#pragma unroll
    for (int w = 0; w < kRefWaves; ++w) v[w] = red[w][s];
#pragma unroll
    for (int m = kRefWaves / 2; m >= 1; m >>= 1)
#pragma unroll
        for (int w = 0; w < m; ++w) v[w] = v[2 * w] + v[2 * w + 1];
    return v[0];
}

// The decisions of pass k and the step, on wave 0 behind the pass's sums in
// L.S / L.N: either the result (pose, log row, report; L.done) or T_{k+1} in
// L.T.  Every lane computes the same values (the LU of inverse6 replicated in
// registers, as the direct pose's solve_wave0_rep: the pivot row is
// wave-uniform, so nothing is indexed at run time); lane c < 6 solves column c
// of the inverse; lane 0 stores.
__device__ __attribute__((always_inline)) inline void refine_decide(const RefineArgs& a, RefineLds& L, int k,
                                                                    int lane) {
    const int n = L.N[0], inl = L.N[1];
    const double cost = L.S[27];
    const double rms = n > 0 ? sqrt(L.S[28] / (double)n) : 0.0;
    const double cost0 = k == 0 ? cost : L.cost0, rms0 = k == 0 ? rms : L.rms0;
    int status = -1, steps = k, r_inl = inl;
    double r_cost = cost, r_rms = rms;
    bool use_prev = false;
    if (k == 0 && n < 6) status = 1;
    if (status < 0 && k >= 1 && cost >= L.prev_cost) {
        status = 3;
        steps = k - 1;
        use_prev = true;
        r_cost = L.prev_cost;
        r_inl = L.prev_inl;
        r_rms = L.prev_rms;
    }
    if (status < 0 && k == a.iterations) status = 0;
    double T[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = L.T[q];
    double xi[6];
    if (status < 0) {
        // ---- inverse6 (Eigen PartialPivLU: first maximal |pivot| wins)
        double A[36];
        int tr[6];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const int r1 = r < c ? r : c, c1 = r < c ? c : r;
                A[6 * r + c] = L.S[r1 * 6 - (r1 * (r1 - 1)) / 2 + (c1 - r1)];
            }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            int p = j;
            double best = fabs(A[7 * j]);
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                const double v = fabs(A[6 * i + j]);
                if (v > best) {
                    best = v;
                    p = i;
                }
            }
            p = __builtin_amdgcn_readfirstlane(p);
            tr[j] = p;
            if (__builtin_amdgcn_readfirstlane(best != 0.0 ? 1 : 0)) {
#pragma unroll
                for (int i = j + 1; i < 6; ++i) {
                    if (p == i) {
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            const double tmp = A[6 * j + c];
                            A[6 * j + c] = A[6 * i + c];
                            A[6 * i + c] = tmp;
                        }
                    }
                }
                const double piv = A[7 * j];
#pragma unroll
                for (int i = j + 1; i < 6; ++i) A[6 * i + j] = A[6 * i + j] / piv;
            }
#pragma unroll
            for (int i = j + 1; i < 6; ++i)
#pragma unroll
                for (int c = j + 1; c < 6; ++c) A[6 * i + c] = A[6 * i + c] - A[6 * i + j] * A[6 * j + c];
        }
        // column c of X = P I by forward (unit L) and backward (U) substitution
        const int cc = lane < 6 ? lane : 0;
        int pos = cc;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (pos == j) pos = tr[j];
            else if (pos == tr[j]) pos = j;
        }
        double x[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) x[r] = (r == pos) ? 1.0 : 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int i = j + 1; i < 6; ++i) x[i] = x[i] - A[6 * i + j] * x[j];
#pragma unroll
        for (int j = 5; j >= 0; --j) {
            x[j] = x[j] / A[7 * j];
#pragma unroll
            for (int i = 0; i < j; ++i) x[i] = x[i] - A[6 * i + j] * x[j];
        }
        // xi = H^-1 b, row-wise in ascending columns (H^-1[r][c] is lane c's x[r])
        bool finite = true;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v = readlane_f64(x[r], 0) * L.S[21];
#pragma unroll
            for (int c = 1; c < 6; ++c) v = v + readlane_f64(x[r], c) * L.S[21 + c];
            xi[r] = v;
            finite = finite && isfinite(v);
        }
        if (!finite) status = 2;
    }
    if (status >= 0) {
        if (lane == 0) {
            double out[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) out[q] = use_prev ? L.prevT[q] : T[q];
#pragma unroll
            for (int q = 0; q < 12; ++q) a.pose_out[q] = out[q];
            if (a.log && a.log_index >= 0) {
#pragma unroll
                for (int q = 0; q < 12; ++q) a.log[12 * (size_t)a.log_index + q] = out[q];
                if (a.log_host)
#pragma unroll
                    for (int q = 0; q < 12; ++q)
                        __hip_atomic_store(a.log_host + 12 * (size_t)a.log_index + q, out[q], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
            }
            a.report[0] = (double)L.N[2];
            a.report[1] = (double)steps;
            a.report[2] = cost0;
            a.report[3] = r_cost;
            a.report[4] = (double)r_inl;
            a.report[5] = (double)status;
            a.report[6] = rms0;
            a.report[7] = r_rms;
            L.done = 1;
        }
    } else {
        // T_{k+1} = exp(xi) T_k (Sophus left-multiplication)
        SE3d t0;
        quat_from_matrix(T, t0.q);
        t0.t[0] = T[9];
        t0.t[1] = T[10];
        t0.t[2] = T[11];
        const SE3d t1 = se3_mul(se3_exp(xi), t0);
        double nT[12];
        se3_to_pose12(t1, nT);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                L.prevT[q] = T[q];
                L.T[q] = nT[q];
            }
            L.prev_cost = cost;
            L.prev_inl = inl;
            L.prev_rms = rms;
            L.cost0 = cost0;
            L.rms0 = rms0;
        }
    }
}

__global__ __launch_bounds__(kRefLanes) void refine_pose_kernel(RefineArgs a) {
    __shared__ RefineLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < 12) L.T[tid] = a.pose_in[tid];
    if (tid == 0) L.done = 0;
    // the lane's observations (bit j: point tid + 1024 j): they do not depend
    // on the pose
    unsigned mask = 0;
    {
        const double m2 = a.max_shift * a.max_shift;
        for (int j = 0, i = tid; i < a.n; ++j, i += kRefLanes) {
            bool ob = a.pair_kf[i] >= 0 && a.success[i] != 0;
            if (ob) {
                const double d0 = a.uv_after[2 * (size_t)i] - a.uv_before[2 * (size_t)i];
                const double d1 = a.uv_after[2 * (size_t)i + 1] - a.uv_before[2 * (size_t)i + 1];
                const double d2 = d0 * d0 + d1 * d1;
                ob = d2 <= m2;
            }
            if (ob) mask |= 1u << j;
        }
    }
    __syncthreads();
    const double fx = a.K[0], fy = a.K[1], cx = a.K[2], cy = a.K[3];
    const double huber = a.huber;
    for (int k = 0;; ++k) {
        double T[12];
#pragma unroll
        for (int q = 0; q < 12; ++q) T[q] = L.T[q];
        double acc[kRefSums];
#pragma unroll
        for (int s = 0; s < kRefSums; ++s) acc[s] = 0.0;
        int n_used = 0, n_inl = 0;
        for (int j = 0, i = tid; i < a.n; ++j, i += kRefLanes) {
            if (!((mask >> j) & 1u)) continue;
            const double* P = a.pts + 3 * (size_t)i;
            double Pc[3];
            mat3_vec(T, P, Pc);
            const double x = Pc[0] + T[9], y = Pc[1] + T[10], z = Pc[2] + T[11];
            if (!(z > 0)) continue;
            const double r0 = a.uv_after[2 * (size_t)i] - (fx * x / z + cx);
            const double r1 = a.uv_after[2 * (size_t)i + 1] - (fy * y / z + cy);
            const double e2 = r0 * r0 + r1 * r1;
            const double e = sqrt(e2);
            const double zz = z * z, xy = x * y;
            double J[12];
            J[0] = fx / z;
            J[1] = 0;
            J[2] = -fx * x / zz;
            J[3] = -fx * xy / zz;
            J[4] = fx + fx * x * x / zz;
            J[5] = -fx * y / z;
            J[6] = 0;
            J[7] = fy / z;
            J[8] = -fy * y / zz;
            J[9] = -fy - fy * y * y / zz;
            J[10] = fy * xy / zz;
            J[11] = fy * x / z;
            const bool inl = e <= huber;
            const double w = inl ? 1.0 : huber / e;
            const double rho = inl ? 0.5 * e2 : huber * (e - 0.5 * huber);
            int s = 0;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int q = p; q < 6; ++q, ++s) acc[s] = acc[s] + w * (J[p] * J[q] + J[6 + p] * J[6 + q]);
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[21 + p] = acc[21 + p] + w * (J[p] * r0 + J[6 + p] * r1);
            acc[27] = acc[27] + rho;
            acc[28] = acc[28] + e2;
            n_used += 1;
            n_inl += inl ? 1 : 0;
        }
        // the wave's 64 lane values, neighbours first
#pragma unroll
        for (int s = 0; s < kRefSums; ++s) {
            double v = acc[s];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
            if (lane == 0) L.red[wave][s] = v;
        }
        {
            int c0 = n_used, c1 = n_inl, c2 = __popc(mask);
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                c0 += __shfl_xor(c0, off, 64);
                c1 += __shfl_xor(c1, off, 64);
                c2 += __shfl_xor(c2, off, 64);
            }
            if (lane == 0) {
                L.cnt[wave][0] = c0;
                L.cnt[wave][1] = c1;
                L.cnt[wave][2] = c2;
            }
        }
        __syncthreads();
        if (tid < kRefSums) L.S[tid] = tree16(L.red, tid);
        if (tid >= 64 && tid < 67) {
            int c = 0;
            for (int w = 0; w < kRefWaves; ++w) c += L.cnt[w][tid - 64];
            L.N[tid - 64] = c;
        }
        __syncthreads();
        if (wave == 0) refine_decide(a, L, k, lane);
        __syncthreads();
        if (L.done) break;
    }
}

}  // namespace

void launch_refine_pose(const RefineArgs& a, hipStream_t stream) {
    refine_pose_kernel<<<1, kRefLanes, 0, stream>>>(a);
}

}  // namespace viso

using namespace viso;

namespace {

bool refine_params_ok(int32_t iterations, double huber_px, double max_shift_px) {
    return iterations >= 1 && iterations <= 20 && huber_px > 0 && max_shift_px > 0 && std::isfinite(huber_px) &&
           std::isfinite(max_shift_px);
}

}  // namespace

// One tracking frame's refinement in the frame path (on_new_frame, behind
// finish_call on the context stream: cur's final solve, then its LK alignment
// as a batch of one, row 0 of the LK buffers).  The launch rewrites cur's
// pose, its pose-log row and that row's pinned mirror.
int viso_ctx::refine_frame(int cur) {
    if (n_map <= 0 || lk_last_rows < 1 || lk_last_pts != n_map) return VISO_ERR_STATE;
    const size_t o = (size_t)(lk_last_rows - 1) * kMaxMapPoints;  // cur's row: the batch's last
    RefineArgs a{};
    intrinsics(a.K);
    a.pts = (const double*)map_pts.ptr;
    a.pair_kf = (const int32_t*)lk_pair.ptr + o;
    a.success = (const uint8_t*)lk_succ.ptr + o;
    a.uv_before = (const double*)lk_before.ptr + 2 * o;
    a.uv_after = (const double*)lk_after.ptr + 2 * o;
    a.n = n_map;
    a.iterations = refine_iterations;
    a.huber = refine_huber;
    a.max_shift = refine_max_shift;
    a.pose_in = pose_of(cur);
    a.pose_out = pose_of(cur);
    const int li = slots[(size_t)cur].log_index;
    a.log = li >= 0 ? (double*)pose_log.ptr : nullptr;
    a.log_host = log_host(li);
    a.log_index = li;
    a.report = (double*)refine_rep.ptr;
    {
        TimedRegion t(timing, VISO_KERNEL_REFINE, stream);
        launch_refine_pose(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    return VISO_OK;
}

extern "C" {

int viso_set_pose_refine(viso_ctx* c, int32_t iterations, double huber_px, double max_shift_px) {
    if (!c || !(iterations == 0 || refine_params_ok(iterations, huber_px, max_shift_px))) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    if (iterations > 0) {
        VISO_HIP_CHECK(hipSetDevice(c->device));
        if (!c->refine_rep.ptr) {
            if (int rc = c->refine_rep.ensure(8 * sizeof(double))) return rc;
            // NaN until the first refinement
            VISO_HIP_CHECK(hipMemsetAsync(c->refine_rep.ptr, 0xff, 8 * sizeof(double), c->stream));
        }
        c->refine_huber = huber_px;
        c->refine_max_shift = max_shift_px;
    }
    c->refine_iterations = iterations;
    return VISO_OK;
}

int viso_get_pose_refine(viso_ctx* c, double report[8]) {
    if (!c || !report) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    for (int k = 0; k < 8; ++k) report[k] = std::numeric_limits<double>::quiet_NaN();
    if (!c->refine_rep.ptr) return VISO_OK;
    VISO_HIP_CHECK(hipSetDevice(c->device));
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_dbl + 16, c->refine_rep.ptr, 8 * sizeof(double), hipMemcpyDeviceToHost,
                                  c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 8; ++k) report[k] = c->h_dbl[16 + k];
    return VISO_OK;
}

int viso_refine_pose(viso_ctx* c, const double* points, const int32_t* pair_kf, const uint8_t* success,
                     const double* uv_before, const double* uv_after, int32_t n, const double pose_in[12],
                     int32_t iterations, double huber_px, double max_shift_px, double pose_out[12],
                     double report[8]) {
    if (!c || n < 0 || n > kMaxMapPoints || !pose_in || !pose_out || !report ||
        !refine_params_ok(iterations, huber_px, max_shift_px) ||
        (n > 0 && (!points || !pair_kf || !success || !uv_before || !uv_after)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t m = (size_t)std::max(n, 1);
    Bump b;
    const size_t o_pose = b.take(96), o_out = b.take(96), o_rep = b.take(64), o_p = b.take(24 * m),
                 o_pk = b.take(4 * m), o_sc = b.take(m), o_ub = b.take(16 * m), o_ua = b.take(16 * m);
    if (int rc = c->scratch_a.ensure(b.off)) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_pose, pose_in, 96, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_pk, pair_kf, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_sc, success, (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_ub, uv_before, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_ua, uv_after, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    RefineArgs a{};
    c->intrinsics(a.K);
    a.pts = (const double*)(base + o_p);
    a.pair_kf = (const int32_t*)(base + o_pk);
    a.success = (const uint8_t*)(base + o_sc);
    a.uv_before = (const double*)(base + o_ub);
    a.uv_after = (const double*)(base + o_ua);
    a.n = n;
    a.iterations = iterations;
    a.huber = huber_px;
    a.max_shift = max_shift_px;
    a.pose_in = (const double*)(base + o_pose);
    a.pose_out = (double*)(base + o_out);
    a.log = nullptr;
    a.log_host = nullptr;
    a.log_index = -1;
    a.report = (double*)(base + o_rep);
    launch_refine_pose(a, c->stream);
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_dbl + 16, a.pose_out, 96, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_dbl + 32, a.report, 64, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 12; ++k) pose_out[k] = c->h_dbl[16 + k];
    for (int k = 0; k < 8; ++k) report[k] = c->h_dbl[32 + k];
    return VISO_OK;
}

}  // extern "C"
