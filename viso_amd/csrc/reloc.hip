// viso_amd — relocalisation: the keyframe alignment (viso_kf_align,
// viso_set_relocalise; include/viso/viso_c.h).  The repo's own
// spec, restated in tests/kf_align_ref.py; the per-point arithmetic is the
// direct pose's (oracle_track.cpp direct_point_partials, the factored form).
//
// One attempt: every candidate (keyframe k, seed s) runs an iterated
// photometric Gauss-Newton from keyframe k to the current frame over the first
// max_points map points k sees, levels 3..0, each level from the result of the
// one above.  Pass j at T_j forms n_j, cost_j = S[27] / n_j and the 28 sums;
// the decisions (too few points, a cost that did not fall or fell by less than
// delta_thresh, the last pass, a non-finite step) and the update T_{j+1} =
// exp(xi) T_j are made on the device.
//
// Mapping: one workgroup of 16 waves per candidate, all candidates in one
// launch.  The list of points is built by ordered compaction (block_rank) into
// LDS.  Wave a owns accumulator a: it walks the list positions p = a, a + 16,
// ... in ascending order, lane = patch pixel (x outer, y inner).  The template
// is resampled from the keyframe's level in every pass (1,024 points x 4
// levels x 64 taps do not fit LDS as doubles; the bytes stay in L2).  The six
// pixel sums are the descending wave tree (tree_sum_desc64); lane t < 28 then
// forms term t and adds it to its own running value.  The 16 accumulators are
// added neighbours first through LDS; wave 0 solves and decides (the LU of
// inverse6 replicated in registers, as refine_pose_kernel), the pose goes
// round through LDS.  A second launch of one wave picks the winner.  No
// atomics, no inline assembly; fp64 in both precision modes,
// -ffp-contract=off.
//
// The illumination form (viso_kf_align_illum, viso_set_reloc_illum; DESIGN.md
// §25, restated in tests/kf_align_illum_ref.py) is kf_align_kernel<true>: the
// state of a candidate is (T, g, o), the error (g R + o) - C, a point has the
// brightness chain's 44 terms (five wave trees, lane t < 44 forms term t), wave
// 0 eliminates (g, o) ahead of the same 6x6 solve, and a gain outside
// [1 / max_gain, max_gain] is status 5.
#include <algorithm>
#include <cmath>
#include <limits>

#include "block_rank.hpp"
#include "context.hpp"
#include "device_math.hpp"

namespace viso {

namespace {

constexpr int kAlWaves = 16;
constexpr int kAlLanes = 64 * kAlWaves;
constexpr int kAlTerms = 28;       // H upper triangle (21, row-major), b (6), cost
constexpr int kAlIllumTerms = 44;  // the illumination form (§25): then B (12), d00, d01, c0, c1
constexpr int kAlMaxPoints = 1024;
constexpr double kAlDeltaThresh = 0.005;  // the reference's delta_thresh

// kIllum (viso_kf_align_illum): 44 terms, and the state carries
// g and o behind the pose (T[12], T[13])
template <bool kIllum>
struct AlignLds {
    static constexpr int kTerms = kIllum ? kAlIllumTerms : kAlTerms;
    static constexpr int kState = kIllum ? 14 : 12;
    int table[kAlWaves];
    unsigned short idx[kAlMaxPoints];  // the map index of list position p
    double acc[kAlWaves][kTerms];
    int cnt[kAlWaves];
    double S[kTerms];
    int n;
    double T[kState];
    int done;
    // wave 0's: pass j - 1, and the level's result
    double prevT[kState], prev_cost;
    int prev_n;
    int res_exit, res_n;
    double res_cost;
};

// neighbours first over the 16 accumulators of one sum
template <int kTerms>
__device__ inline double tree16(const double (*acc)[kTerms], int s) {
    double v[kAlWaves];
#pragma unroll
    for (int w = 0; w < kAlWaves; ++w) v[w] = acc[w][s];
#pragma unroll
    for (int m = kAlWaves / 2; m >= 1; m >>= 1)
#pragma unroll
        for (int w = 0; w < m; ++w) v[w] = v[2 * w] + v[2 * w + 1];
    return v[0];
}

__device__ inline double pick6(const double* v, int i) {
    const double v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3], v4 = v[4], v5 = v[5];
    return i == 5 ? v5 : i == 4 ? v4 : i == 3 ? v3 : i == 2 ? v2 : i == 1 ? v1 : v0;
}

// Keyframe::Project at a level's scale, with the depth (project_px's order)
__device__ inline double project_level(const double* pose, const double* K, const double* P, double scale, double& u,
                                       double& v, double* Pc) {
    mat3_vec(pose, P, Pc);
    Pc[0] = Pc[0] + pose[9];
    Pc[1] = Pc[1] + pose[10];
    Pc[2] = Pc[2] + pose[11];
    const double z = Pc[2];
    const double x = Pc[0] / z, y = Pc[1] / z;
    u = scale * (x * K[0] + K[2]);
    v = scale * (y * K[1] + K[3]);
    return z;
}

// The decisions of pass j and the step, on wave 0 behind the pass's sums in
// L.S / L.n: either the level's result (L.T, the report's level row, L.done) or
// T_{j+1} in L.T.  Every lane computes the same values; lane c < 6 solves
// column c of the inverse; lane 0 stores.  kIllum: (g, o) are eliminated from
// the 44 sums first (bright_decide's Schur complement, d11 = 64 n), the 6x6
// solve runs on A' and b', and g, o and pass j - 1's copies move with the pose.
template <bool kIllum>
__device__ __attribute__((always_inline)) inline void align_decide(AlignLds<kIllum>& L, int j, int iterations,
                                                                   double* row, int lane) {
    const int n = L.n;
    const double cost = L.S[27] / (double)n;
    int ex = -1;
    bool use_prev = false;
    if (n < 6 || !finite_f64(cost)) {
        ex = j == 0 ? 4 : 5;
        use_prev = j > 0;
    } else if (j >= 1 && cost >= L.prev_cost) {
        ex = 1;
        use_prev = true;
    } else if (j >= 1 && (1 - cost / L.prev_cost) < kAlDeltaThresh) {
        ex = 2;
    } else if (j == iterations) {
        ex = 0;
    }
    double T[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = L.T[q];
    double xi[6];
    double dg = 0.0, dof = 0.0;
    if (ex < 0) {
        // ---- inverse6 (Eigen PartialPivLU: first maximal |pivot| wins)
        double A[36];
        int tr[6];
        double Y0[6], Y1[6], bp[6], q0 = 0.0, q1 = 0.0;
        if constexpr (kIllum) {
            // (g, o) eliminated: A' = A - B D^-1 B^T, b' = b - B D^-1 c
            const double* S = L.S;
            const double d00 = S[40], d01 = S[41], c0 = S[42], c1 = S[43];
            const double d11 = 64.0 * (double)n;
            const double det = d00 * d11 - d01 * d01;
            q0 = (d11 * c0 - d01 * c1) / det;
            q1 = (d00 * c1 - d01 * c0) / det;
#pragma unroll
            for (int e = 0; e < 6; ++e) {
                Y0[e] = (d11 * S[28 + e] - d01 * S[34 + e]) / det;
                Y1[e] = (d00 * S[34 + e] - d01 * S[28 + e]) / det;
            }
            int k = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c, ++k) {
                    const double v = S[k] - (S[28 + r] * Y0[c] + S[34 + r] * Y1[c]);
                    A[6 * r + c] = v;
                    A[6 * c + r] = v;
                }
#pragma unroll
            for (int e = 0; e < 6; ++e) bp[e] = S[21 + e] - (S[28 + e] * q0 + S[34 + e] * q1);
        } else {
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const int r1 = r < c ? r : c, c1 = r < c ? c : r;
                    A[6 * r + c] = L.S[r1 * 6 - (r1 * (r1 - 1)) / 2 + (c1 - r1)];
                }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            int p = k;
            double best = fabs(A[7 * k]);
#pragma unroll
            for (int i = k + 1; i < 6; ++i) {
                const double v = fabs(A[6 * i + k]);
                if (v > best) {
                    best = v;
                    p = i;
                }
            }
            p = __builtin_amdgcn_readfirstlane(p);
            tr[k] = p;
            if (__builtin_amdgcn_readfirstlane(best != 0.0 ? 1 : 0)) {
#pragma unroll
                for (int i = k + 1; i < 6; ++i) {
                    if (p == i) {
#pragma unroll
                        for (int c = 0; c < 6; ++c) {
                            const double tmp = A[6 * k + c];
                            A[6 * k + c] = A[6 * i + c];
                            A[6 * i + c] = tmp;
                        }
                    }
                }
                const double piv = A[7 * k];
#pragma unroll
                for (int i = k + 1; i < 6; ++i) A[6 * i + k] = A[6 * i + k] / piv;
            }
#pragma unroll
            for (int i = k + 1; i < 6; ++i)
#pragma unroll
                for (int c = k + 1; c < 6; ++c) A[6 * i + c] = A[6 * i + c] - A[6 * i + k] * A[6 * k + c];
        }
        // column c of X = P I by forward (unit L) and backward (U) substitution
        const int cc = lane < 6 ? lane : 0;
        int pos = cc;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if (pos == k) pos = tr[k];
            else if (pos == tr[k]) pos = k;
        }
        double x[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) x[r] = (r == pos) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int i = k + 1; i < 6; ++i) x[i] = x[i] - A[6 * i + k] * x[k];
#pragma unroll
        for (int k = 5; k >= 0; --k) {
            x[k] = x[k] / A[7 * k];
#pragma unroll
            for (int i = 0; i < k; ++i) x[i] = x[i] - A[6 * i + k] * x[k];
        }
        // xi = H^-1 b, row-wise in ascending columns (H^-1[r][c] is lane c's x[r])
        bool finite = true;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v;
            if constexpr (kIllum) {
                v = readlane_f64(x[r], 0) * bp[0];
#pragma unroll
                for (int c = 1; c < 6; ++c) v = v + readlane_f64(x[r], c) * bp[c];
            } else {
                v = readlane_f64(x[r], 0) * L.S[21];
#pragma unroll
                for (int c = 1; c < 6; ++c) v = v + readlane_f64(x[r], c) * L.S[21 + c];
            }
            xi[r] = v;
            finite = finite && finite_f64(v);
        }
        if constexpr (kIllum) {
            double s0 = Y0[0] * xi[0], s1 = Y1[0] * xi[0];
#pragma unroll
            for (int e = 1; e < 6; ++e) {
                s0 = s0 + Y0[e] * xi[e];
                s1 = s1 + Y1[e] * xi[e];
            }
            dg = q0 - s0;
            dof = q1 - s1;
            finite = finite && finite_f64(dg) && finite_f64(dof);
        }
        if (!finite) ex = 3;
    }
    if (ex >= 0) {
        if (lane == 0) {
            const int r_n = use_prev ? L.prev_n : n;
            const double r_cost = ex == 4 ? std::numeric_limits<double>::quiet_NaN() : use_prev ? L.prev_cost : cost;
            if (use_prev)
#pragma unroll
                for (int q = 0; q < AlignLds<kIllum>::kState; ++q) L.T[q] = L.prevT[q];
            row[0] = (double)ex;
            row[1] = (double)(use_prev ? j - 1 : ex == 4 ? 0 : j);
            row[2] = (double)r_n;
            row[3] = r_cost;
            L.res_exit = ex;
            L.res_n = r_n;
            L.res_cost = r_cost;
            L.done = L.done + 1;
        }
    } else {
        // T_{j+1} = exp(xi) T_j (Sophus left-multiplication)
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
            if constexpr (kIllum) {
                const double g = L.T[12], o = L.T[13];
                L.prevT[12] = g;
                L.prevT[13] = o;
                L.T[12] = g + dg;
                L.T[13] = o + dof;
            }
            L.prev_cost = cost;
            L.prev_n = n;
        }
    }
}

// kIllum: the candidate's state is (T, g, o), the error is
// (g R + o) - C, a point has bright_pass_kernel's 44 terms (five wave trees,
// lane t < 44 forms term t); status 5 and the gain_offset row at the end.
template <bool kIllum>
__global__ __launch_bounds__(kAlLanes) void kf_align_kernel(KfAlignArgs a) {
    constexpr int kTerms = AlignLds<kIllum>::kTerms;
    __shared__ AlignLds<kIllum> L;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int cand = blockIdx.x;
    const int per_kf = 1 + a.n_extra;
    const int k = cand / per_kf, s = cand - k * per_kf;
    double* rep = a.report + (size_t)kAlignReport * cand;
    double* pose_out = a.poses_out + 12 * (size_t)cand;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    double kfp[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) kfp[q] = a.kf_poses[12 * (size_t)k + q];
    const double* seed = s ? a.extra_seed : a.kf_poses + 12 * (size_t)k;
    if (tid < 12) L.T[tid] = seed[tid];
    if constexpr (kIllum)
        if (tid == 12 || tid == 13) L.T[tid] = tid == 12 ? 1.0 : 0.0;  // (g, o) = (1, 0)
    if (tid == 0) L.done = 0;  // the levels finished

    // ---- step 1: the first max_points map points keyframe k sees, in map order
    int base = 0;
    {
        const Intrinsics Kin{a.K[0], a.K[1], a.K[2], a.K[3]};
        for (int start = 0; start < a.n && base < a.max_points; start += kAlLanes) {
            const int i = start + tid;
            bool sees = false;
            if (i < a.n) {
                double u, v;
                const double z = project_px_depth(kfp, Kin, a.points + 3 * (size_t)i, u, v);
                sees = z > 0 && inside_px(u, v, a.w[0], a.h[0]);
            }
            const BlockRank r = block_rank<kAlWaves>(sees, L.table);
            const int pos = base + r.rank;
            if (sees && pos < a.max_points) L.idx[pos] = (unsigned short)i;
            base += r.total;
        }
    }
    const int m = base < a.max_points ? base : a.max_points;
    __syncthreads();
    if (m < 6) {
        if (tid == 0) {
            rep[0] = 1.0;
            rep[1] = (double)m;
            rep[2] = 0.0;
            rep[3] = qnan;
            for (int q = 0; q < 4; ++q) {
                rep[4 + 4 * q] = -1.0;
                rep[5 + 4 * q] = 0.0;
                rep[6 + 4 * q] = 0.0;
                rep[7 + 4 * q] = qnan;
            }
            if constexpr (kIllum) {
                a.gain_offset[2 * (size_t)cand] = 1.0;
                a.gain_offset[2 * (size_t)cand + 1] = 0.0;
            }
        }
        if (tid < 12) pose_out[tid] = seed[tid];
        return;
    }

    // the term lane t forms: H entry (ta, tb) for t < 21, b entry ta for t < 27,
    // the cost for t = 27
    int ta = 0, tb = 0;
    {
        int t = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int q = p; q < 6; ++q, ++t)
                if (t == lane) {
                    ta = p;
                    tb = q;
                }
        if (lane >= 21 && lane < 27) ta = lane - 21;
        if constexpr (kIllum) {  // entry ta of B's columns for 28 <= t < 40
            if (lane >= 28 && lane < 34) ta = lane - 28;
            if (lane >= 34 && lane < 40) ta = lane - 34;
        }
    }
    const double px = (double)((lane >> 3) - kHalfPatch), py = (double)((lane & 7) - kHalfPatch);
    const double hp = 4.0;

    for (int q = 0; q < kLevels; ++q) {
        const int level = kLevels - 1 - q;
        const double scale = kScale[level];
        const int w = a.w[level], h = a.h[level];
        const uint8_t* kimg = a.kf[k].l[level];
        const uint8_t* cimg = a.cur.l[level];
        const double fxs = a.K[0] * scale, fys = a.K[1] * scale;
        for (int j = 0;; ++j) {
            double T[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) T[e] = L.T[e];
            double gain = 1.0, offs = 0.0;
            if constexpr (kIllum) {
                gain = L.T[12];
                offs = L.T[13];
            }
            double acc = 0.0;
            int cnt = 0;
            for (int p = wave; p < m; p += kAlWaves) {
                const int i = __builtin_amdgcn_readfirstlane((int)L.idx[p]);
                const double* Pp = a.points + 3 * (size_t)i;
                const double P[3] = {Pp[0], Pp[1], Pp[2]};
                double ur, vr, uc, vc, Pr[3], Pc[3];
                const double zr = project_level(kfp, a.K, P, scale, ur, vr, Pr);
                const double zc = project_level(T, a.K, P, scale, uc, vc, Pc);
                const bool good = inside_px(ur - hp, vr - hp, w, h) && inside_px(ur + hp, vr + hp, w, h) &&
                                  inside_px(uc - hp, vc - hp, w, h) && inside_px(uc + hp, vc + hp, w, h) && zr > 0 &&
                                  zc > 0;
                if (!__builtin_amdgcn_readfirstlane(good ? 1 : 0)) continue;
                // dPixeldXi at the level scale
                const double x = Pc[0], y = Pc[1], z = Pc[2];
                const double zz = z * z, xy = x * y;
                double J0[6], J1[6];
                J0[0] = fxs / z;
                J0[1] = 0;
                J0[2] = -fxs * x / zz;
                J0[3] = -fxs * xy / zz;
                J0[4] = fxs + fxs * x * x / zz;
                J0[5] = -fxs * y / z;
                J1[0] = 0;
                J1[1] = fys / z;
                J1[2] = -fys * y / zz;
                J1[3] = -fys - fys * y * y / zz;
                J1[4] = fys * xy / zz;
                J1[5] = fys * x / z;
                // the lane's pixel
                const double xc = uc + px, yc = vc + py;
                const double R = sample_px(kimg, w, h, ur + px, vr + py);
                const double C = sample_px(cimg, w, h, xc, yc);
                double err = R - C;
                if constexpr (kIllum) err = (gain * R + offs) - C;
                double g0, g1;
                gradient_px(cimg, w, h, xc, yc, g0, g1);
                double G[6];
                wave_tree_sum3_desc(g0 * g0, g0 * g1, g1 * g1, G[0], G[1], G[2]);
                wave_tree_sum3_desc(err * g0, err * g1, err * err, G[3], G[4], G[5]);
                const double J0a = pick6(J0, ta), J0b = pick6(J0, tb), J1a = pick6(J1, ta), J1b = pick6(J1, tb);
                const double th = (G[0] * (J0a * J0b) + G[1] * (J0a * J1b + J1a * J0b)) + G[2] * (J1a * J1b);
                const double tbv = G[3] * J0a + G[4] * J1a;
                double term = lane < 21 ? th : lane < 27 ? tbv : G[5];
                if constexpr (kIllum) {
                    // the nine sums of B, D and c, as bright_pass_kernel forms them
                    double B[9];
                    wave_tree_sum3_desc(g0 * R, g1 * R, g0, B[0], B[1], B[2]);
                    wave_tree_sum3_desc(g1, R * R, R, B[3], B[4], B[5]);
                    wave_tree_sum3_desc(err * R, err, 0.0, B[6], B[7], B[8]);
                    const double tB0 = -(B[0] * J0a + B[1] * J1a);
                    const double tB1 = -(B[2] * J0a + B[3] * J1a);
                    term = lane < 28    ? term
                           : lane < 34  ? tB0
                           : lane < 40  ? tB1
                           : lane == 40 ? B[4]
                           : lane == 41 ? B[5]
                           : lane == 42 ? -B[6]
                                        : -B[7];
                }
                acc = acc + term;
                cnt += 1;
            }
            if (lane < kTerms) L.acc[wave][lane] = acc;
            if (lane == 0) L.cnt[wave] = cnt;
            __syncthreads();
            if (tid < kTerms) L.S[tid] = tree16(L.acc, tid);
            if (tid == 64) {
                int c = 0;
                for (int v = 0; v < kAlWaves; ++v) c += L.cnt[v];
                L.n = c;
            }
            __syncthreads();
            if (wave == 0) align_decide(L, j, a.iterations, rep + 4 + 4 * q, lane);
            __syncthreads();
            if (L.done > q) break;
        }
    }
    // ---- the status, from level 0's result
    if (tid == 0) {
        const int ex = L.res_exit, n = L.res_n;
        const double cost = L.res_cost;
        int status = 0;
        bool gain_ok = true;  // (the negated form rejects a NaN too)
        if constexpr (kIllum) {
            gain_ok = 1.0 / a.max_gain <= L.T[12] && L.T[12] <= a.max_gain;
            a.gain_offset[2 * (size_t)cand] = L.T[12];
            a.gain_offset[2 * (size_t)cand + 1] = L.T[13];
        }
        if (ex == 4) status = 2;
        else if (n * 1000 < a.min_good_permille * m) status = 3;
        else if (!gain_ok) status = 5;
        else if (!(cost <= a.max_cost)) status = 4;
        rep[0] = (double)status;
        rep[1] = (double)m;
        rep[2] = (double)n;
        rep[3] = cost;
    }
    if (tid < 12) pose_out[tid] = L.T[tid];
}

// The accepted candidate of least cost (ties: the lowest index), and the frame
// path's copies of the chosen pose.
__global__ __launch_bounds__(64) void kf_align_pick_kernel(KfAlignArgs a, int n_cand) {
    if (threadIdx.x != 0) return;
    int win = -1;
    double best = 0.0;
    for (int c = 0; c < n_cand; ++c) {
        const double st = a.report[(size_t)kAlignReport * c], cost = a.report[(size_t)kAlignReport * c + 3];
        if (st == 0.0 && (win < 0 || cost < best)) {
            win = c;
            best = cost;
        }
    }
    a.winner[0] = win;
    if (a.flog && a.log_index >= 0) {
        const double qnan = std::numeric_limits<double>::quiet_NaN();
        double* row = a.flog + 4 * (size_t)a.log_index;
        row[0] = win >= 0 ? a.report[(size_t)kAlignReport * win + 2] : qnan;
        row[1] = win >= 0 ? best : qnan;
        row[2] = qnan;
        row[3] = qnan;
    }
    const double* src = win >= 0 ? a.poses_out + 12 * (size_t)win : a.hold_pose;
    if (!src) return;
    double out[12];
    for (int q = 0; q < 12; ++q) out[q] = src[q];
    if (a.pose_dst)
        for (int q = 0; q < 12; ++q) a.pose_dst[q] = out[q];
    if (win >= 0 && a.good_dst)
        for (int q = 0; q < 12; ++q) a.good_dst[q] = out[q];
    if (a.log && a.log_index >= 0) {
        for (int q = 0; q < 12; ++q) a.log[12 * (size_t)a.log_index + q] = out[q];
        if (a.log_host)
            for (int q = 0; q < 12; ++q)
                __hip_atomic_store(a.log_host + 12 * (size_t)a.log_index + q, out[q], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

void launch_kf_align(const KfAlignArgs& a, hipStream_t stream) {
    const int n_cand = a.n_kf * (1 + a.n_extra);
    if (a.gain_offset) kf_align_kernel<true><<<n_cand, kAlLanes, 0, stream>>>(a);
    else kf_align_kernel<false><<<n_cand, kAlLanes, 0, stream>>>(a);
    kf_align_pick_kernel<<<1, 64, 0, stream>>>(a, n_cand);
}

}  // namespace viso

using namespace viso;

namespace {

bool align_params_ok(int32_t iterations, int32_t max_points, double max_cost, int32_t min_good_permille) {
    return iterations >= 1 && iterations <= 20 && max_points >= 64 && max_points <= kAlMaxPoints && max_cost > 0 &&
           std::isfinite(max_cost) && min_good_permille >= 1 && min_good_permille <= 1000;
}

}  // namespace

// The verdict of the tracking frame just finished in the frame path
// (on_new_frame, behind finish_call on the context stream: its final solve,
// then its LK alignment as the last row of the batch): one host sync for the
// level-0 nGood and cost and the row's LK pairs and successes.
int viso_ctx::reloc_verdict(bool* bad) {
    *bad = false;
    if (n_map <= 0 || lk_last_rows < 1 || lk_last_pts != n_map) return VISO_ERR_STATE;
    const size_t o = (size_t)(lk_last_rows - 1) * kMaxMapPoints;
    LkCountArgs rows{};
    rows.idx[0] = 0;
    launch_lk_count((const int32_t*)lk_pair.ptr + o, (const uint8_t*)lk_succ.ptr + o, kMaxMapPoints, n_map, 1, rows,
                    reloc_counts(), stream);
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(h_dbl + 64, direct_stats.ptr, 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipMemcpyAsync(h_dbl + 66, reloc_counts(), 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    const double n_good = h_dbl[64], cost = h_dbl[65], pairs = h_dbl[68], succ = h_dbl[69];
    *bad = !(cost <= reloc_max_cost) || n_good * 1000.0 < (double)reloc_permille * (double)n_map ||
           (reloc_lk_permille > 0 && succ * 1000.0 < (double)reloc_lk_permille * pairs);
    return VISO_OK;
}

// One attempt for the lost frame cur: every keyframe from its own pose and
// from the last good pose (only_kf >= 0, the attempt behind a seed stage: that
// keyframe alone, from its own pose and from `seed`).  The choice, cur's pose
// (the winner's, else the held one), its pose-log row and the last good pose
// are written on the device; the host reads the winner back.
int viso_ctx::reloc_attempt(int cur, int li, bool* won, int only_kf, const double* seed) {
    *won = false;
    const int all_kf = (int)kf_slots.size();
    if (all_kf < 1 || all_kf > kMaxKeyframes || n_map <= 0 || only_kf >= all_kf || (only_kf >= 0 && !seed))
        return VISO_ERR_STATE;
    const int n_kf = only_kf >= 0 ? 1 : all_kf, first = only_kf >= 0 ? only_kf : 0;
    KfAlignArgs a{};
    intrinsics(a.K);
    for (int j = 0; j < n_kf; ++j) a.kf[j] = frame(kf_slots[(size_t)(first + j)]);
    a.kf_poses = (const double*)kf_poses.ptr + 12 * (size_t)first;
    a.n_kf = n_kf;
    a.cur = frame(cur);
    for (int l = 0; l < kLevels; ++l) {
        a.w[l] = geom.w[l];
        a.h[l] = geom.h[l];
    }
    a.points = (const double*)map_pts.ptr;
    a.n = n_map;
    a.extra_seed = only_kf >= 0 ? seed : reloc_good();
    a.n_extra = 1;
    a.iterations = reloc_iterations;
    a.max_points = reloc_max_points;
    a.min_good_permille = reloc_permille;
    a.max_cost = reloc_max_cost;
    a.poses_out = reloc_poses();
    a.report = reloc_report();
    a.winner = reloc_winner();
    a.hold_pose = reloc_good();
    a.pose_dst = pose_of(cur);
    a.good_dst = reloc_good();
    a.log = li >= 0 ? (double*)pose_log.ptr : nullptr;
    a.log_host = log_host(li);
    a.flog = flog();
    a.log_index = li;
    const bool illum = reloc_illum_mode != 0;  // viso_set_reloc_illum: every attempt in the (T, g, o) form
    if (illum) {
        a.max_gain = reloc_illum_max_gain;
        a.gain_offset = (double*)reloc_illum_buf.ptr;
    }
    {
        TimedRegion t(timing, VISO_KERNEL_RELOC, stream);
        launch_kf_align(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(h_int + 40, a.winner, sizeof(int), hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    ++reloc_attempts;
    reloc_last_frame = frames;
    reloc_last_winner = h_int[40];
    reloc_last_cands = 2 * n_kf;
    if (illum) {
        ++reloc_illum_attempts;
        reloc_illum_last_winner = reloc_last_winner;
        reloc_illum_last_cands = reloc_last_cands;
    }
    *won = reloc_last_winner >= 0;
    return VISO_OK;
}

namespace {

bool gain_bound_ok(double max_gain) { return std::isfinite(max_gain) && max_gain > 1.0; }

// viso_kf_align, and viso_kf_align_illum (illum: max_gain and gain_offset are
// its two arguments): one attempt on host data through the frame path's launches.
int kf_align_host(viso_ctx* c, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf, const uint8_t* cur_pyr,
                  int32_t width, int32_t height, const double* points, int32_t n, const double* extra_seed12,
                  int32_t n_extra, int32_t iterations, int32_t max_points, double max_cost, int32_t min_good_permille,
                  bool illum, double max_gain, double* poses_out, double* report, double* gain_offset,
                  int32_t* winner) {
    if (!c || !kf_pyrs || !kf_poses || n_kf < 1 || n_kf > kMaxKeyframes || !cur_pyr || width < 64 || height < 64 ||
        width > kMaxWidth || height > kMaxWidth || n < 0 || n > kMaxMapPoints || (n > 0 && !points) || n_extra < 0 ||
        n_extra > 1 || (n_extra == 1 && !extra_seed12) || !align_params_ok(iterations, max_points, max_cost,
                                                                           min_good_permille) ||
        !poses_out || !report || !winner || (illum && (!gain_bound_ok(max_gain) || !gain_offset)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const PyrGeom g = make_geom(width, height);
    const int n_cand = n_kf * (1 + n_extra);
    Bump b;
    const size_t o_kf = b.take(g.bytes * (size_t)n_kf), o_kp = b.take(96 * (size_t)n_kf), o_c = b.take(g.bytes),
                 o_p = b.take(24 * (size_t)std::max(n, 1)), o_s = b.take(96), o_po = b.take(96 * (size_t)n_cand),
                 o_r = b.take(8 * (size_t)kAlignReport * n_cand), o_w = b.take(4),
                 o_go = b.take(illum ? 16 * (size_t)n_cand : 0);
    if (int rc = c->scratch_a.ensure(b.off)) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_kf, kf_pyrs, g.bytes * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_kp, kf_poses, 96 * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_c, cur_pyr, g.bytes, hipMemcpyHostToDevice, c->stream));
    if (n > 0) VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (n_extra) VISO_HIP_CHECK(hipMemcpyAsync(base + o_s, extra_seed12, 96, hipMemcpyHostToDevice, c->stream));
    KfAlignArgs a{};
    c->intrinsics(a.K);
    for (int j = 0; j < n_kf; ++j) a.kf[j] = frame_from_base((const uint8_t*)(base + o_kf + g.bytes * j), g);
    a.kf_poses = (const double*)(base + o_kp);
    a.n_kf = n_kf;
    a.cur = frame_from_base((const uint8_t*)(base + o_c), g);
    for (int l = 0; l < kLevels; ++l) {
        a.w[l] = g.w[l];
        a.h[l] = g.h[l];
    }
    a.points = (const double*)(base + o_p);
    a.n = n;
    a.extra_seed = n_extra ? (const double*)(base + o_s) : nullptr;
    a.n_extra = n_extra;
    a.iterations = iterations;
    a.max_points = max_points;
    a.min_good_permille = min_good_permille;
    a.max_cost = max_cost;
    a.poses_out = (double*)(base + o_po);
    a.report = (double*)(base + o_r);
    a.winner = (int*)(base + o_w);
    a.log_index = -1;
    if (illum) {
        a.max_gain = max_gain;
        a.gain_offset = (double*)(base + o_go);
    }
    {
        TimedRegion t(c->timing, VISO_KERNEL_RELOC, c->stream);
        launch_kf_align(a, c->stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(poses_out, a.poses_out, 96 * (size_t)n_cand, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(report, a.report, 8 * (size_t)kAlignReport * n_cand, hipMemcpyDeviceToHost,
                                  c->stream));
    if (illum)
        VISO_HIP_CHECK(hipMemcpyAsync(gain_offset, a.gain_offset, 16 * (size_t)n_cand, hipMemcpyDeviceToHost,
                                      c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_int + 40, a.winner, 4, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    *winner = c->h_int[40];
    return VISO_OK;
}

}  // namespace

extern "C" {

int viso_kf_align(viso_ctx* c, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf, const uint8_t* cur_pyr,
                  int32_t width, int32_t height, const double* points, int32_t n, const double* extra_seed12,
                  int32_t n_extra, int32_t iterations, int32_t max_points, double max_cost, int32_t min_good_permille,
                  double* poses_out, double* report, int32_t* winner) {
    return kf_align_host(c, kf_pyrs, kf_poses, n_kf, cur_pyr, width, height, points, n, extra_seed12, n_extra,
                         iterations, max_points, max_cost, min_good_permille, false, 0.0, poses_out, report, nullptr,
                         winner);
}

int viso_kf_align_illum(viso_ctx* c, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf,
                        const uint8_t* cur_pyr, int32_t width, int32_t height, const double* points, int32_t n,
                        const double* extra_seed12, int32_t n_extra, int32_t iterations, int32_t max_points,
                        double max_cost, int32_t min_good_permille, double max_gain, double* poses_out, double* report,
                        double* gain_offset, int32_t* winner) {
    return kf_align_host(c, kf_pyrs, kf_poses, n_kf, cur_pyr, width, height, points, n, extra_seed12, n_extra,
                         iterations, max_points, max_cost, min_good_permille, true, max_gain, poses_out, report,
                         gain_offset, winner);
}

// The illumination form in the frame path.  Takes effect while
// viso_set_relocalise is on; off, nothing is allocated for it.
int viso_set_reloc_illum(viso_ctx* c, int32_t mode, double max_gain) {
    if (!c || (mode != 0 && mode != 1) || (mode == 1 && !gain_bound_ok(max_gain))) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    if (mode == 1) {
        VISO_HIP_CHECK(hipSetDevice(c->device));
        if (!c->reloc_illum_buf.ptr) {
            const size_t bytes = 16 * (size_t)kMaxAlignCands;
            if (int rc = c->reloc_illum_buf.ensure(bytes)) return rc;
            VISO_HIP_CHECK(hipMemsetAsync(c->reloc_illum_buf.ptr, 0xff, bytes, c->stream));  // NaN until written
        }
        c->reloc_illum_max_gain = max_gain;
    }
    c->reloc_illum_mode = mode;
    return VISO_OK;
}

int viso_get_reloc_illum(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[0] = c->reloc_illum_mode;
    info[1] = c->reloc_illum_attempts;
    info[2] = c->reloc_illum_recoveries;
    info[3] = c->reloc_illum_last_winner;
    return VISO_OK;
}

int viso_get_reloc_illum_rows(viso_ctx* c, double* gain_offset2, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (!c->reloc_illum_mode) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    const size_t total = (size_t)c->reloc_illum_last_cands, m = std::min(cap, total);
    if (n) *n = total;
    if (m == 0 || !gain_offset2) return VISO_OK;
    VISO_HIP_CHECK(hipSetDevice(c->device));
    VISO_HIP_CHECK(hipMemcpyAsync(gain_offset2, c->reloc_illum_buf.ptr, 16 * m, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

int viso_set_relocalise(viso_ctx* c, int32_t lost_after, double max_cost, int32_t min_good_permille, int32_t lk_permille,
                        int32_t iterations, int32_t max_points) {
    if (!c || lost_after < 0 || lost_after > 1000) return VISO_ERR_ARG;
    if (lost_after > 0 && (!align_params_ok(iterations, max_points, max_cost, min_good_permille) || lk_permille < 0 ||
                           lk_permille > 1000))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    if (lost_after > 0) {
        VISO_HIP_CHECK(hipSetDevice(c->device));
        if (!c->reloc_buf.ptr) {
            const size_t bytes = 8 * (size_t)(16 + (12 + kAlignReport) * kMaxAlignCands + 2);
            if (int rc = c->reloc_buf.ensure(bytes)) return rc;
            VISO_HIP_CHECK(hipMemsetAsync(c->reloc_buf.ptr, 0xff, bytes, c->stream));  // NaN until written
        }
        c->reloc_max_cost = max_cost;
        c->reloc_permille = min_good_permille;
        c->reloc_lk_permille = lk_permille;
        c->reloc_iterations = iterations;
        c->reloc_max_points = max_points;
    } else {
        c->reloc_lost = false;
        c->reloc_bad_run = 0;
    }
    c->reloc_lost_after = lost_after;
    return VISO_OK;
}

int viso_get_relocalise(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    info[0] = c->reloc_lost_after;
    info[1] = c->reloc_lost ? 1 : 0;
    info[2] = c->reloc_losses;
    info[3] = c->reloc_attempts;
    info[4] = c->reloc_recoveries;
    info[5] = c->reloc_last_frame;
    info[6] = c->reloc_last_winner;
    info[7] = c->reloc_last_cands;
    return VISO_OK;
}

int viso_get_relocalise_report(viso_ctx* c, double* poses, double* report, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (!c->reloc_on()) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    const size_t total = (size_t)c->reloc_last_cands, m = std::min(cap, total);
    if (n) *n = total;
    if (m == 0 || !c->reloc_buf.ptr) return VISO_OK;
    VISO_HIP_CHECK(hipSetDevice(c->device));
    if (poses) VISO_HIP_CHECK(hipMemcpyAsync(poses, c->reloc_poses(), 96 * m, hipMemcpyDeviceToHost, c->stream));
    if (report)
        VISO_HIP_CHECK(hipMemcpyAsync(report, c->reloc_report(), 8 * (size_t)kAlignReport * m, hipMemcpyDeviceToHost,
                                      c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

int viso_get_frame_status(viso_ctx* c, uint8_t* status, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    const size_t total = (size_t)c->n_poses;
    if (n) *n = total;
    const size_t m = std::min(cap, total);
    if (status)
        for (size_t i = 0; i < m; ++i) status[i] = i < c->frame_status.size() ? c->frame_status[i] : 0;
    return VISO_OK;
}

}  // extern "C"
