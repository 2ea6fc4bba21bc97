// viso_amd — relocalisation seed (viso_reloc_seed, viso_set_reloc_seed;
// include/viso/viso_c.h).  The repo's own spec, restated in
// tests/reloc_seed_ref.py: a pose seed for the keyframe alignment (reloc.hip)
// that does not depend on where tracking stopped.
//
// Every map point is described in its host keyframe and every FAST corner of
// the current frame in the current frame by a 256-bit BRIEF on pyramid level 1
// (the offsets come from mix64, no table); the descriptors are matched both
// ways by Hamming distance (best, second best, ratio and mutual tests); three-
// point hypotheses from the start pose S are solved by ten unweighted
// Gauss-Newton passes each and scored against every match; the best one's
// inliers go, as an LK row, through refine_pose_kernel (§14).
//
// Launches, all on one stream, no host synchronisation between them:
//   corner_keep_kernel      1 workgroup: the corners with a valid descriptor, in order
//   brief_kernel<MAP>       4 lanes per descriptor, 64 descriptors per workgroup
//   brief_kernel<CUR>
//   brief_match_kernel<0>   a point per lane, the corners streamed through LDS
//   brief_match_kernel<1>   the roles swapped: every corner's best point
//   match_accept_kernel     1 workgroup: the three tests, ordered compaction
//   pnp_hyp_kernel          a thread per hypothesis
//   pnp_count_kernel        8 hypotheses per workgroup against every match
//   pnp_pick_kernel         1 workgroup: the best hypothesis, its inliers as an LK row
//   refine_pose_kernel      (refine.hip)
//   seed_final_kernel       the report's §14 columns and the seed pose
// Integer atomics only (a counter, eight LDS counters); no atomics on doubles,
// no inline assembly; fp64 in both precision modes, -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <limits>

#include "block_rank.hpp"
#include "context.hpp"
#include "device_math.hpp"

namespace viso {

namespace {

constexpr int kBriefBorder = 6;
constexpr int kBriefBits = 256;
constexpr int kDescPerGroup = 64;  // descriptors per brief workgroup (4 lanes each)
constexpr int kMatchLanes = 64;    // queries per match workgroup = streamed items per chunk
constexpr int kHypPerGroup = 8;    // hypotheses per count workgroup
constexpr int kCountLanes = 256;
constexpr int kOneLanes = 1024;    // the one-workgroup launches
constexpr int kGnPasses = 10;
constexpr int kSeedRefineIterations = 10;

__device__ inline bool brief_valid(int x1, int y1, int w1, int h1) {
    return x1 >= kBriefBorder && x1 < w1 - kBriefBorder && y1 >= kBriefBorder && y1 < h1 - kBriefBorder;
}

// ---- the corners with a valid descriptor, in the detector's order
__global__ __launch_bounds__(kOneLanes) void corner_keep_kernel(RelocSeedArgs a) {
    __shared__ int table[kOneLanes / 64];
    const int tid = threadIdx.x;
    const int n = std::min(std::max(a.n_corners[0], 0), a.cap_corners);
    int base = 0;
    for (int start = 0; start < n; start += kOneLanes) {
        const int i = start + tid;
        int4 c = make_int4(0, 0, 0, 0);
        bool keep = false;
        if (i < n) {
            c = a.corners[i];
            keep = brief_valid(c.x >> 1, c.y >> 1, a.w[1], a.h[1]);
        }
        const BlockRank r = block_rank<kOneLanes / 64>(keep, table);
        if (keep) a.kept_xy[base + r.rank] = make_int2(c.x, c.y);
        base += r.total;
    }
    if (tid == 0) a.counts[1] = base;
}

// ---- descriptors: lane q of a descriptor's four forms words 2 q and 2 q + 1
template <bool MAP>
__global__ __launch_bounds__(4 * kDescPerGroup) void brief_kernel(RelocSeedArgs a) {
    __shared__ int offs[kBriefBits];  // (ax, ay, bx, by) + 6, a byte each
    const int tid = threadIdx.x, q = tid & 3;
    {
        int pack = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) pack |= (int)(mix64((uint64_t)(4 * tid + c)) % 13) << (8 * c);
        offs[tid] = pack;
    }
    __syncthreads();
    const int count = MAP ? a.n : a.counts[1];
    const int i = blockIdx.x * kDescPerGroup + (tid >> 2);
    const int w1 = a.w[1], h1 = a.h[1];
    bool valid = false;
    int x1 = kBriefBorder, y1 = kBriefBorder;
    const uint8_t* img = a.cur.l[1];
    if (i < count) {
        if (MAP) {
            const int k = a.host[i];
            if (k >= 0 && k < a.n_kf) {
                const Intrinsics Kin{a.K[0], a.K[1], a.K[2], a.K[3]};
                double u, v;
                const double z = project_px_depth(a.kf_poses + 12 * (size_t)k, Kin, a.points + 3 * (size_t)i, u, v);
                if (z > 0 && inside_px(u, v, a.w[0], a.h[0])) {
                    x1 = (int)(u + 0.5) >> 1;
                    y1 = (int)(v + 0.5) >> 1;
                    valid = brief_valid(x1, y1, w1, h1);
                }
                img = a.kf[k].l[1];
            }
        } else {
            const int2 c = a.kept_xy[i];
            x1 = c.x >> 1;
            y1 = c.y >> 1;
            valid = brief_valid(x1, y1, w1, h1);
        }
    }
    if (!valid) {  // (the loads below stay inside the level)
        x1 = kBriefBorder;
        y1 = kBriefBorder;
    }
    uint32_t word[2] = {0u, 0u};
    const long long centre = (long long)y1 * w1 + x1;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        uint32_t bits = 0;
        for (int b = 0; b < 32; ++b) {
            const int o = offs[64 * q + 32 * half + b];
            const int ax = (o & 255) - 6, ay = ((o >> 8) & 255) - 6, bx = ((o >> 16) & 255) - 6, by = (o >> 24) - 6;
            const int pa = ld_global_u8(img, centre + (long long)ay * w1 + ax);
            const int pb = ld_global_u8(img, centre + (long long)by * w1 + bx);
            bits |= (pa < pb ? 1u : 0u) << b;
        }
        word[half] = valid ? bits : 0u;
    }
    if (i < count) {
        uint32_t* d = (MAP ? a.pdesc : a.cdesc) + 8 * (size_t)i + 2 * q;
        d[0] = word[0];
        d[1] = word[1];
        if (MAP && q == 0) a.pvalid[i] = valid ? 1 : 0;
    }
    if (MAP) {
        const unsigned long long m = __ballot(valid && q == 0);
        if ((tid & 63) == 0 && m) atomicAdd(a.counts, __popcll(m));
    }
}

// ---- matching: lane = one query, the other side streamed through LDS in
// chunks; SWAP = 0: queries the points, streamed the kept corners (best, second
// best, the corner); SWAP = 1: queries the kept corners, streamed the described
// points (the best point).  Ascending stream order and a strict < give the
// lowest index among equal distances.
template <bool SWAP>
__global__ __launch_bounds__(kMatchLanes) void brief_match_kernel(RelocSeedArgs a) {
    __shared__ uint4 s[kMatchLanes][2];
    __shared__ int sv[kMatchLanes];
    const int tid = threadIdx.x;
    const int n_kept = std::min(std::max(a.counts[1], 0), a.cap_corners);
    const int nq = SWAP ? n_kept : a.n, ns = SWAP ? a.n : n_kept;
    if (blockIdx.x * kMatchLanes >= nq) return;
    const uint4* qd = (const uint4*)(SWAP ? a.cdesc : a.pdesc);
    const uint4* sd = (const uint4*)(SWAP ? a.pdesc : a.cdesc);
    const int qi = blockIdx.x * kMatchLanes + tid;
    const bool qv = qi < nq && (SWAP || a.pvalid[qi] != 0);
    const uint4 zero = make_uint4(0, 0, 0, 0);
    const uint4 d0 = qv ? qd[2 * (size_t)qi] : zero, d1 = qv ? qd[2 * (size_t)qi + 1] : zero;
    int best = 257, second = 257, idx = -1;
    for (int c0 = 0; c0 < ns; c0 += kMatchLanes) {
        const int j = c0 + tid;
        const bool v = j < ns && (!SWAP || a.pvalid[j] != 0);
        s[tid][0] = v ? sd[2 * (size_t)j] : zero;
        s[tid][1] = v ? sd[2 * (size_t)j + 1] : zero;
        sv[tid] = v ? 1 : 0;
        __syncthreads();
        const int m = std::min(kMatchLanes, ns - c0);
        for (int t = 0; t < m; ++t) {
            if (SWAP && !sv[t]) continue;  // (the same for every lane)
            const uint4 e0 = s[t][0], e1 = s[t][1];
            const int d = (__popc(d0.x ^ e0.x) + __popc(d0.y ^ e0.y)) + (__popc(d0.z ^ e0.z) + __popc(d0.w ^ e0.w)) +
                          (__popc(d1.x ^ e1.x) + __popc(d1.y ^ e1.y)) + (__popc(d1.z ^ e1.z) + __popc(d1.w ^ e1.w));
            if (d < best) {
                second = best;
                best = d;
                idx = c0 + t;
            } else if (d < second) {
                second = d;
            }
        }
        __syncthreads();
    }
    if (qi < nq) {
        if (!qv) {
            best = second = 257;
            idx = -1;
        }
        if (SWAP) a.cbest[qi] = make_int2(best, idx);
        else a.pbest[qi] = make_int4(best, second, idx, 0);
    }
}

// ---- the three tests and the match list, in ascending point index
__global__ __launch_bounds__(kOneLanes) void match_accept_kernel(RelocSeedArgs a) {
    __shared__ int table[kOneLanes / 64];
    const int tid = threadIdx.x;
    int base = 0;
    for (int start = 0; start < a.n; start += kOneLanes) {
        const int i = start + tid;
        bool acc = false;
        int4 b = make_int4(257, 257, -1, 0);
        if (i < a.n && a.pvalid[i]) {
            b = a.pbest[i];
            acc = b.z >= 0 && b.x <= a.max_hamming && b.x * 1000 < a.ratio_permille * b.y && a.cbest[b.z].y == i;
        }
        const BlockRank r = block_rank<kOneLanes / 64>(acc, table);
        if (acc) a.matches[base + r.rank] = make_int4(i, b.z, b.x, 0);
        base += r.total;
    }
    if (tid == 0) a.counts[2] = base;
}

// ---- one match's residual and dPixeldXi at T (refine_pose_kernel's order);
// false when the depth is not positive
__device__ inline bool reproject(const double* T, const double* K, const double* P, double u, double v, double& r0,
                                 double& r1, double* J) {
    double Pc[3];
    mat3_vec(T, P, Pc);
    const double x = Pc[0] + T[9], y = Pc[1] + T[10], z = Pc[2] + T[11];
    if (!(z > 0)) return false;
    const double fx = K[0], fy = K[1];
    r0 = u - (fx * x / z + K[2]);
    r1 = v - (fy * y / z + K[3]);
    if (J) {
        const double zz = z * z, xy = x * y;
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
    }
    return true;
}

// ---- a thread per hypothesis: three draws, ten Gauss-Newton passes from S
__global__ __launch_bounds__(64) void pnp_hyp_kernel(RelocSeedArgs a) {
    const int h = blockIdx.x * 64 + threadIdx.x;
    const int M = a.counts[2];
    if (h >= a.hypotheses || M < 3) return;
    const uint64_t uM = (uint64_t)M;
    const uint64_t r0 = mix64(a.seed + 4ull * (uint64_t)h), r1 = mix64(a.seed + 4ull * (uint64_t)h + 1ull),
                   r2 = mix64(a.seed + 4ull * (uint64_t)h + 2ull);
    int pick[3];
    pick[0] = (int)(r0 % uM);
    pick[1] = (int)(r1 % (uM - 1));
    if (pick[1] >= pick[0]) pick[1] += 1;
    pick[2] = (int)(r2 % (uM - 2));
    const int lo = std::min(pick[0], pick[1]), hi = std::max(pick[0], pick[1]);
    if (pick[2] >= lo) pick[2] += 1;
    if (pick[2] >= hi) pick[2] += 1;
    double P[3][3], uv[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int4 m = a.matches[pick[k]];
        const int2 c = a.kept_xy[m.y];
#pragma unroll
        for (int q = 0; q < 3; ++q) P[k][q] = a.points[3 * (size_t)m.x + q];
        uv[k][0] = (double)c.x;
        uv[k][1] = (double)c.y;
    }
    double T[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = a.start[q];
    bool solved = true;
    for (int pass = 0; pass < kGnPasses && solved; ++pass) {
        double t[3][27];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double e0, e1, J[12];
            if (!reproject(T, a.K, P[k], uv[k][0], uv[k][1], e0, e1, J)) {
                solved = false;
#pragma unroll
                for (int s = 0; s < 27; ++s) t[k][s] = 0.0;
                continue;
            }
            int s = 0;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int q = p; q < 6; ++q, ++s) t[k][s] = J[p] * J[q] + J[6 + p] * J[6 + q];
#pragma unroll
            for (int p = 0; p < 6; ++p) t[k][21 + p] = J[p] * e0 + J[6 + p] * e1;
        }
        if (!solved) break;
        double S[27];
#pragma unroll
        for (int s = 0; s < 27; ++s) S[s] = (t[0][s] + t[1][s]) + t[2][s];
        double H[36], Hi[36];
        {
            int s = 0;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int q = p; q < 6; ++q, ++s) {
                    H[6 * p + q] = S[s];
                    H[6 * q + p] = S[s];
                }
        }
        inverse6(H, Hi);
        double xi[6];
        bool finite = true;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double v = Hi[6 * p] * S[21];
#pragma unroll
            for (int q = 1; q < 6; ++q) v = v + Hi[6 * p + q] * S[21 + q];
            xi[p] = v;
            finite = finite && finite_f64(v);
        }
        if (!finite) {
            solved = false;
            break;
        }
        SE3d t0;
        quat_from_matrix(T, t0.q);
        t0.t[0] = T[9];
        t0.t[1] = T[10];
        t0.t[2] = T[11];
        const SE3d t1 = se3_mul(se3_exp(xi), t0);
        se3_to_pose12(t1, T);
    }
    if (!solved) return;  // (hyp_score stays -1)
#pragma unroll
    for (int q = 0; q < 12; ++q) a.hyp_pose[12 * (size_t)h + q] = T[q];
    a.hyp_score[h] = 0;
}

__device__ inline bool is_inlier(const double* T, const double* K, const double* P, double u, double v, double px2) {
    double r0, r1;
    if (!reproject(T, K, P, u, v, r0, r1, nullptr)) return false;
    return r0 * r0 + r1 * r1 <= px2;
}

// ---- scores: a workgroup holds 8 hypotheses' poses, every lane loads its
// matches once and tests them against each; counts by ballot + popcount
__global__ __launch_bounds__(kCountLanes) void pnp_count_kernel(RelocSeedArgs a) {
    __shared__ double sp[kHypPerGroup][12];
    __shared__ int ss[kHypPerGroup];
    __shared__ int sc[kCountLanes / 64][kHypPerGroup];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int M = a.counts[2];
    if (M < 3) return;
    const int h0 = blockIdx.x * kHypPerGroup;
    if (tid < kHypPerGroup) ss[tid] = (h0 + tid < a.hypotheses && a.hyp_score[h0 + tid] >= 0) ? 1 : 0;
    __syncthreads();
    if (tid < 12 * kHypPerGroup) {
        const int g = tid / 12, q = tid - 12 * g;
        sp[g][q] = ss[g] ? a.hyp_pose[12 * (size_t)(h0 + g) + q] : 0.0;
    }
    __syncthreads();
    const double px2 = a.inlier_px * a.inlier_px;
    int cnt[kHypPerGroup];
#pragma unroll
    for (int g = 0; g < kHypPerGroup; ++g) cnt[g] = 0;
    for (int m0 = 0; m0 < M; m0 += kCountLanes) {
        const int m = m0 + tid;
        const bool active = m < M;
        double P[3] = {0.0, 0.0, 0.0}, u = 0.0, v = 0.0;
        if (active) {
            const int4 mt = a.matches[m];
            const int2 c = a.kept_xy[mt.y];
#pragma unroll
            for (int q = 0; q < 3; ++q) P[q] = a.points[3 * (size_t)mt.x + q];
            u = (double)c.x;
            v = (double)c.y;
        }
#pragma unroll
        for (int g = 0; g < kHypPerGroup; ++g) {
            const bool in = active && ss[g] && is_inlier(sp[g], a.K, P, u, v, px2);
            cnt[g] += __popcll(__ballot(in));
        }
    }
    if (lane == 0)
#pragma unroll
        for (int g = 0; g < kHypPerGroup; ++g) sc[wave][g] = cnt[g];
    __syncthreads();
    if (tid < kHypPerGroup && ss[tid]) {
        int c = 0;
        for (int w = 0; w < kCountLanes / 64; ++w) c += sc[w][tid];
        a.hyp_score[h0 + tid] = c;
    }
}

// ---- the best hypothesis (highest score, ties to the lowest h), the status,
// its inliers as an LK row over the map (uv_before = uv_after = the corner
// pixel), k* and the report's first columns
__global__ __launch_bounds__(kOneLanes) void pnp_pick_kernel(RelocSeedArgs a) {
    __shared__ int s_key[kOneLanes / 64], s_solved[kOneLanes / 64];
    __shared__ int s_kf[kMaxKeyframes];
    __shared__ int s_best, s_nsolved, s_status;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = a.counts[2];
    int key = -1, solved = 0;
    if (M >= 3)
        for (int h = tid; h < a.hypotheses; h += kOneLanes) {
            const int sc = a.hyp_score[h];
            if (sc >= 0) {
                solved += 1;
                key = std::max(key, sc * kSeedMaxHyp + (kSeedMaxHyp - 1 - h));
            }
        }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        key = std::max(key, __shfl_xor(key, off, 64));
        solved += __shfl_xor(solved, off, 64);
    }
    if (lane == 0) {
        s_key[wave] = key;
        s_solved[wave] = solved;
    }
    if (tid < kMaxKeyframes) s_kf[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        int k = -1, n = 0;
        for (int w = 0; w < kOneLanes / 64; ++w) {
            k = std::max(k, s_key[w]);
            n += s_solved[w];
        }
        const int score = k >= 0 ? k / kSeedMaxHyp : 0;
        s_best = k >= 0 ? kSeedMaxHyp - 1 - (k - score * kSeedMaxHyp) : -1;
        s_nsolved = n;
        s_status = M < 3 ? 1 : (k < 0 || score < a.min_inliers) ? 2 : 0;
        a.report[0] = (double)s_status;
        a.report[1] = (double)a.counts[0];
        a.report[2] = (double)a.counts[1];
        a.report[3] = (double)M;
        a.report[4] = (double)n;
        a.report[5] = (double)s_best;
        a.report[6] = (double)score;
        a.report[7] = -1.0;
        a.report[8] = std::numeric_limits<double>::quiet_NaN();
        a.report[9] = 0.0;
        a.report[10] = -1.0;
        a.report[11] = 0.0;
    }
    // the empty row
    for (int i = tid; i < a.n; i += kOneLanes) {
        a.pair_kf[i] = -1;
        a.success[i] = 0;
        a.uv[2 * (size_t)i] = 0.0;
        a.uv[2 * (size_t)i + 1] = 0.0;
    }
    __syncthreads();
    const int status = s_status, best = s_best;
    const double* src = status == 0 ? a.hyp_pose + 12 * (size_t)best : a.start;
    double T[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = src[q];
    if (tid < 12) a.hyp_best[tid] = T[tid];
    const double px2 = a.inlier_px * a.inlier_px;
    for (int m = tid; m < M; m += kOneLanes) {
        int4 mt = a.matches[m];
        bool in = false;
        if (status == 0) {
            const int2 c = a.kept_xy[mt.y];
            const double u = (double)c.x, v = (double)c.y;
            in = is_inlier(T, a.K, a.points + 3 * (size_t)mt.x, u, v, px2);
            if (in) {
                const int k = a.host[mt.x];
                a.pair_kf[mt.x] = k;
                a.success[mt.x] = 1;
                a.uv[2 * (size_t)mt.x] = u;
                a.uv[2 * (size_t)mt.x + 1] = v;
                if (k >= 0 && k < kMaxKeyframes) atomicAdd(&s_kf[k], 1);
            }
        }
        mt.w = in ? 1 : 0;
        a.matches[m] = mt;
    }
    __syncthreads();
    if (tid == 0 && status == 0) {
        int ks = 0;
        for (int k = 1; k < a.n_kf; ++k)
            if (s_kf[k] > s_kf[ks]) ks = k;
        a.report[10] = (double)ks;
    }
}

// ---- behind the refinement: the report's §14 columns and the seed pose
__global__ __launch_bounds__(64) void seed_final_kernel(RelocSeedArgs a) {
    if (threadIdx.x != 0) return;
    const double* src = a.hyp_best;
    if (a.report[0] == 0.0) {
        const double st = a.refine_rep[5];
        a.report[7] = st;
        a.report[8] = a.refine_rep[3];
        a.report[9] = a.refine_rep[4];
        if (st == 0.0 || st == 3.0) src = a.refine_pose;
    }
    double out[12];
    for (int q = 0; q < 12; ++q) out[q] = src[q];
    for (int q = 0; q < 12; ++q) a.pose_out[q] = out[q];
}

struct SeedLayout {
    size_t counts, kept, pdesc, pvalid, cdesc, pbest, cbest, matches, hyp_pose, hyp_score, pair, succ, uv, dbl, total;
};

SeedLayout seed_layout(int n, int cap, int hyp) {
    const size_t m = (size_t)std::max(n, 1), c = (size_t)std::max(cap, 1), h = (size_t)std::max(hyp, 1);
    Bump b;
    SeedLayout L;
    L.counts = b.take(16);
    L.hyp_score = b.take(4 * h);  // (behind counts: one memset pair)
    L.kept = b.take(8 * c);
    L.pdesc = b.take(32 * m);
    L.pvalid = b.take(m);
    L.cdesc = b.take(32 * c);
    L.pbest = b.take(16 * m);
    L.cbest = b.take(8 * c);
    L.matches = b.take(16 * m);
    L.hyp_pose = b.take(96 * h);
    L.pair = b.take(4 * m);
    L.succ = b.take(m);
    L.uv = b.take(16 * m);
    L.dbl = b.take(8 * (12 + 12 + 8 + kSeedReport + 12));
    L.total = b.off;
    return L;
}

}  // namespace

size_t reloc_seed_scratch_bytes(int n, int cap_corners, int hypotheses) {
    return seed_layout(n, cap_corners, hypotheses).total;
}

size_t reloc_seed_scratch_at(RelocSeedArgs& a, void* base, int n, int cap_corners, int hypotheses) {
    const SeedLayout L = seed_layout(n, cap_corners, hypotheses);
    char* p = (char*)base;
    a.counts = (int*)(p + L.counts);
    a.hyp_score = (int*)(p + L.hyp_score);
    a.kept_xy = (int2*)(p + L.kept);
    a.pdesc = (uint32_t*)(p + L.pdesc);
    a.pvalid = (uint8_t*)(p + L.pvalid);
    a.cdesc = (uint32_t*)(p + L.cdesc);
    a.pbest = (int4*)(p + L.pbest);
    a.cbest = (int2*)(p + L.cbest);
    a.matches = (int4*)(p + L.matches);
    a.hyp_pose = (double*)(p + L.hyp_pose);
    a.pair_kf = (int32_t*)(p + L.pair);
    a.success = (uint8_t*)(p + L.succ);
    a.uv = (double*)(p + L.uv);
    double* d = (double*)(p + L.dbl);
    a.hyp_best = d;
    a.refine_pose = d + 12;
    a.refine_rep = d + 24;
    a.report = d + 32;
    a.pose_out = d + 32 + kSeedReport;
    return L.total;
}

bool reloc_seed_params_ok(int hypotheses, int max_hamming, int ratio_permille, double inlier_px, int min_inliers) {
    return hypotheses >= 1 && hypotheses <= kSeedMaxHyp && max_hamming >= 1 && max_hamming <= 256 &&
           ratio_permille >= 1 && ratio_permille <= 1000 && inlier_px > 0 && std::isfinite(inlier_px) &&
           min_inliers >= 6;
}

void launch_reloc_seed(const RelocSeedArgs& a, hipStream_t stream) {
    (void)hipMemsetAsync(a.counts, 0, 16, stream);
    (void)hipMemsetAsync(a.hyp_score, 0xff, 4 * (size_t)a.hypotheses, stream);  // -1: unsolved
    const int cap = a.cap_corners;
    corner_keep_kernel<<<1, kOneLanes, 0, stream>>>(a);
    if (a.n > 0)
        brief_kernel<true><<<(a.n + kDescPerGroup - 1) / kDescPerGroup, 4 * kDescPerGroup, 0, stream>>>(a);
    brief_kernel<false><<<(cap + kDescPerGroup - 1) / kDescPerGroup, 4 * kDescPerGroup, 0, stream>>>(a);
    if (a.n > 0) {
        brief_match_kernel<false><<<(a.n + kMatchLanes - 1) / kMatchLanes, kMatchLanes, 0, stream>>>(a);
        brief_match_kernel<true><<<(cap + kMatchLanes - 1) / kMatchLanes, kMatchLanes, 0, stream>>>(a);
    }
    match_accept_kernel<<<1, kOneLanes, 0, stream>>>(a);
    pnp_hyp_kernel<<<(a.hypotheses + 63) / 64, 64, 0, stream>>>(a);
    pnp_count_kernel<<<(a.hypotheses + kHypPerGroup - 1) / kHypPerGroup, kCountLanes, 0, stream>>>(a);
    pnp_pick_kernel<<<1, kOneLanes, 0, stream>>>(a);
    RefineArgs r{};
    for (int k = 0; k < 4; ++k) r.K[k] = a.K[k];
    r.pts = a.points;
    r.pair_kf = a.pair_kf;
    r.success = a.success;
    r.uv_before = a.uv;
    r.uv_after = a.uv;
    r.n = a.n;
    r.iterations = kSeedRefineIterations;
    r.huber = a.inlier_px;
    r.max_shift = 1.0;
    r.pose_in = a.hyp_best;
    r.pose_out = a.refine_pose;
    r.log = nullptr;
    r.log_host = nullptr;
    r.log_index = -1;
    r.report = a.refine_rep;
    launch_refine_pose(r, stream);
    seed_final_kernel<<<1, 64, 0, stream>>>(a);
}

}  // namespace viso

using namespace viso;

// The seed stage of the lost frame cur in the frame path (reloc_lost_frame,
// behind an attempt without a winner): FAST on cur's level 0, the launches
// above from the last good pose, and one host sync for the status and k*.  The
// seed pose stays on the device (rseed_pose()).
int viso_ctx::reloc_seed_run(int cur, int* status, int* kstar) {
    *status = -1;
    *kstar = -1;
    const int n_kf = (int)kf_slots.size();
    if (n_kf < 1 || n_kf > kMaxKeyframes || n_map <= 0 || (int)point_host.size() != n_map || !rseed_buf.ptr)
        return VISO_ERR_STATE;
    if (int rc = point_host_dev.ensure(4 * (size_t)kMaxMapPoints)) return rc;
    VISO_HIP_CHECK(hipMemcpyAsync(point_host_dev.ptr, point_host.data(), 4 * (size_t)n_map, hipMemcpyHostToDevice,
                                  stream));
    RelocSeedArgs a{};
    intrinsics(a.K);
    for (int j = 0; j < n_kf; ++j) a.kf[j] = frame(kf_slots[(size_t)j]);
    a.kf_poses = (const double*)kf_poses.ptr;
    a.n_kf = n_kf;
    a.cur = frame(cur);
    for (int l = 0; l < kLevels; ++l) {
        a.w[l] = geom.w[l];
        a.h[l] = geom.h[l];
    }
    a.points = (const double*)map_pts.ptr;
    a.host = (const int*)point_host_dev.ptr;
    a.n = n_map;
    a.start = reloc_good();
    a.cap_corners = p.max_features;
    a.hypotheses = rseed_hyp;
    a.max_hamming = rseed_hamming;
    a.ratio_permille = rseed_ratio;
    a.min_inliers = rseed_min_inliers;
    a.inlier_px = rseed_px;
    a.seed = rseed_seed;
    char* base = (char*)rseed_buf.ptr;
    const size_t used = reloc_seed_scratch_at(a, base, kMaxMapPoints, p.max_features, kSeedMaxHyp);
    a.corners = (const int4*)(base + used);
    a.n_corners = (const int*)(base + used + 16 * (size_t)p.max_features);
    {
        TimedRegion t(timing, VISO_KERNEL_FAST, stream);
        launch_fast(a.cur.l[0], geom.w[0], geom.h[0], p.fast_thresh, fast, nullptr, (int4*)a.corners, a.cap_corners,
                    (int*)a.n_corners, stream);
    }
    {
        TimedRegion t(timing, VISO_KERNEL_RELOC_SEED, stream);
        launch_reloc_seed(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(h_dbl + 72, a.report, 8 * kSeedReport, hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    ++rseed_runs;
    *status = (int)h_dbl[72];
    *kstar = (int)h_dbl[72 + 10];
    if (*status == 0) ++rseed_ok;
    rseed_last[0] = (int64_t)h_dbl[72 + 3];
    rseed_last[1] = (int64_t)h_dbl[72 + 6];
    rseed_last[2] = *kstar;
    rseed_last[3] = *status;
    return VISO_OK;
}

double* viso_ctx::rseed_report() const {
    RelocSeedArgs a{};
    reloc_seed_scratch_at(a, rseed_buf.ptr, kMaxMapPoints, p.max_features, kSeedMaxHyp);
    return a.report;
}

extern "C" {

int viso_set_reloc_seed(viso_ctx* c, int32_t hypotheses, int32_t max_hamming, int32_t ratio_permille, double inlier_px,
                        int32_t min_inliers, uint64_t seed) {
    if (!c || (hypotheses != 0 && !reloc_seed_params_ok(hypotheses, max_hamming, ratio_permille, inlier_px,
                                                       min_inliers)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    if (hypotheses > 0) {
        VISO_HIP_CHECK(hipSetDevice(c->device));
        if (!c->rseed_buf.ptr) {
            const size_t used = reloc_seed_scratch_bytes(kMaxMapPoints, c->p.max_features, kSeedMaxHyp);
            const size_t bytes = used + 16 * (size_t)c->p.max_features + 256;
            if (int rc = c->rseed_buf.ensure(bytes)) return rc;
            VISO_HIP_CHECK(hipMemsetAsync(c->rseed_report(), 0xff, 8 * (kSeedReport + 12), c->stream));  // NaN until written
        }
        c->rseed_hamming = max_hamming;
        c->rseed_ratio = ratio_permille;
        c->rseed_px = inlier_px;
        c->rseed_min_inliers = min_inliers;
        c->rseed_seed = seed;
    }
    c->rseed_hyp = hypotheses;
    return VISO_OK;
}

int viso_get_reloc_seed(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    info[0] = c->rseed_on() ? 1 : 0;
    info[1] = c->rseed_runs;
    info[2] = c->rseed_ok;
    info[3] = c->rseed_recoveries;
    for (int k = 0; k < 4; ++k) info[4 + k] = c->rseed_last[k];
    return VISO_OK;
}

int viso_get_reloc_seed_report(viso_ctx* c, double report[12], double pose[12]) {
    if (!c || !report || !pose) return VISO_ERR_ARG;
    if (!c->rseed_on()) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_dbl + 72, c->rseed_report(), 8 * (kSeedReport + 12), hipMemcpyDeviceToHost,
                                  c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < kSeedReport; ++k) report[k] = c->h_dbl[72 + k];
    for (int k = 0; k < 12; ++k) pose[k] = c->h_dbl[72 + kSeedReport + k];
    return VISO_OK;
}

int viso_reloc_seed(viso_ctx* c, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf, const uint8_t* cur_pyr,
                    int32_t width, int32_t height, const double* points, const int32_t* hosts, int32_t n,
                    const double start12[12], int32_t hypotheses, int32_t max_hamming, int32_t ratio_permille,
                    double inlier_px, int32_t min_inliers, uint64_t seed, double report[12], double pose[12],
                    int32_t* matches, uint8_t* inliers, size_t cap, size_t* n_matches) {
    if (!c || !kf_pyrs || !kf_poses || n_kf < 1 || n_kf > kMaxKeyframes || !cur_pyr || width < 64 || height < 64 ||
        width > kMaxWidth || height > kMaxWidth || n < 0 || n > kMaxMapPoints || (n > 0 && (!points || !hosts)) ||
        !start12 || !reloc_seed_params_ok(hypotheses, max_hamming, ratio_permille, inlier_px, min_inliers) ||
        !report || !pose || !n_matches || (cap > 0 && (!matches || !inliers)))
        return VISO_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (hosts[i] < 0 || hosts[i] >= n_kf) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const PyrGeom g = make_geom(width, height);
    const int capc = c->p.max_features;
    Bump b;
    const size_t o_kf = b.take(g.bytes * (size_t)n_kf), o_kp = b.take(96 * (size_t)n_kf), o_c = b.take(g.bytes),
                 o_p = b.take(24 * (size_t)std::max(n, 1)), o_h = b.take(4 * (size_t)std::max(n, 1)), o_s = b.take(96),
                 o_cr = b.take(16 * (size_t)capc), o_nc = b.take(16),
                 o_x = b.take(reloc_seed_scratch_bytes(n, capc, hypotheses));
    int rc = c->scratch_a.ensure(b.off);
    if (!rc) rc = c->scratch_b.ensure(fast_scratch_bytes(width, height));
    if (rc) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_kf, kf_pyrs, g.bytes * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_kp, kf_poses, 96 * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_c, cur_pyr, g.bytes, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_h, hosts, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_s, start12, 96, hipMemcpyHostToDevice, c->stream));
    RelocSeedArgs a{};
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
    a.host = (const int*)(base + o_h);
    a.n = n;
    a.start = (const double*)(base + o_s);
    a.corners = (const int4*)(base + o_cr);
    a.n_corners = (const int*)(base + o_nc);
    a.cap_corners = capc;
    a.hypotheses = hypotheses;
    a.max_hamming = max_hamming;
    a.ratio_permille = ratio_permille;
    a.min_inliers = min_inliers;
    a.inlier_px = inlier_px;
    a.seed = seed;
    reloc_seed_scratch_at(a, base + o_x, n, capc, hypotheses);
    FastScratch fs = fast_scratch_at(c->scratch_b.ptr, width, height);
    {
        TimedRegion t(c->timing, VISO_KERNEL_FAST, c->stream);
        launch_fast(a.cur.l[0], g.w[0], g.h[0], c->p.fast_thresh, fs, nullptr, (int4*)a.corners, capc,
                    (int*)a.n_corners, c->stream);
    }
    {
        TimedRegion t(c->timing, VISO_KERNEL_RELOC_SEED, c->stream);
        launch_reloc_seed(a, c->stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(c->h_dbl + 72, a.report, 8 * (kSeedReport + 12), hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < kSeedReport; ++k) report[k] = c->h_dbl[72 + k];
    for (int k = 0; k < 12; ++k) pose[k] = c->h_dbl[72 + kSeedReport + k];
    const size_t M = (size_t)std::max(0.0, report[3]);
    *n_matches = M;
    const size_t m = std::min(cap, M);
    if (m > 0) {
        std::vector<int32_t> rows(4 * m);
        VISO_HIP_CHECK(hipMemcpy(rows.data(), a.matches, 16 * m, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < m; ++i) {
            matches[3 * i] = rows[4 * i];
            matches[3 * i + 1] = rows[4 * i + 1];
            matches[3 * i + 2] = rows[4 * i + 2];
            inliers[i] = (uint8_t)rows[4 * i + 3];
        }
    }
    return VISO_OK;
}

}  // extern "C"
