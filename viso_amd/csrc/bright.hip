// viso_amd — brightness-compensated tracking (viso_track_affine,
// viso_set_brightness; include/viso/viso_c.h).  The repo's own
// spec, restated in tests/bright_ref.py: the frame's pose together with an
// affine brightness map (g, o) from the last frame to the current one, an
// iterated photometric Gauss-Newton on levels 3..0 with the keyframe
// alignment's per-point arithmetic (reloc.hip) and decisions, its residual
// e = (g R + o) - C, and (g, o) eliminated by the Schur complement in front of
// the 6x6 solve.
//
// Mapping: one launch per pass, a fixed chain of 4 (iterations + 1) + 1
// launches.  A workgroup owns whole tiles of the direct pose's canonical map
// tree (tiles of map_tile(n, 256) consecutive points); a wave handles a point,
// a lane a patch pixel (x outer, y inner).  The 14 pixel sums are descending
// wave trees; lane t < 44 forms term t and stores it in the point's LDS row;
// the tile's tree runs in LDS and its 44 sums and its count go to HBM.  The
// prologue of the next launch adds the tile partials (the tree over tiles),
// decides and steps, redundantly in every workgroup; the state (level, pass,
// T, g, o, the previous pass, the report) goes through a double-buffered block
// of which only workgroup 0 writes the next one.  Once level 0 has exited,
// the launches that are left return behind their read of the state; the last
// launch writes the pose, its log rows, the level-0 stats and the report.  No
// grid-wide barrier, no atomics, no inline assembly, no host synchronisation
// inside the chain; fp64 in both precision modes, -ffp-contract=off.
//
// The robust form (viso_track_robust, viso_set_robust; DESIGN.md §23, restated
// in tests/robust_ref.py) is the same chain with a Huber weight per patch
// pixel: the kernel and the decision are templates on the form, the plain
// instantiation is the code above unchanged, the robust one carries 46 terms
// (sum w and the count of down-weighted pixels behind the 44) and writes every
// pass's weight mass per point.
#include <algorithm>
#include <cmath>
#include <limits>

#include "context.hpp"
#include "device_math.hpp"

namespace viso {

namespace {

constexpr int kBrWaves = 8;
constexpr int kBrLanes = 64 * kBrWaves;
// the two forms of the chain: the plain one (viso_track_affine) and the robust
// one (viso_track_robust), which weights every patch pixel by
// Huber's rule and carries two more terms (sum w, the down-weighted pixels)
template <bool kRobust>
struct BrForm;
template <>
struct BrForm<false> {
    using Args = BrightArgs;
    static constexpr int kTerms = kBrightTerms;  // 28 + B (12) + d00, d01, c0, c1
};
template <>
struct BrForm<true> {
    using Args = RobustArgs;
    static constexpr int kTerms = kRobustTerms;  // + sum w, the count of |e| > k
};
__device__ inline const BrightArgs& br_base(const BrightArgs& a) { return a; }
__device__ inline const BrightArgs& br_base(const RobustArgs& a) { return a.b; }
constexpr int kBrMaxTiles = 256;           // map_tile's groups
constexpr int kBrMaxTile = 64;             // points per tile at most
constexpr double kBrDeltaThresh = 0.005;   // the reference's delta_thresh

// the state block (doubles)
constexpr int kStLevel = 0;    // levels finished (4: the chain is done)
constexpr int kStPass = 1;     // j
constexpr int kStPending = 2;  // the previous launch left a pass's partials
constexpr int kStT = 3;        // T (12), g, o
constexpr int kStPrev = 17;    // pass j - 1: T (12), g, o, cost, n
constexpr int kStReport = 33;  // the report (24; the robust form's 28)
static_assert(kStReport + kBrightReport <= kBrightState && kStReport + kRobustReport <= kBrightState, "state block");

template <int kBrTerms>
struct BrightLds {
    double acc[kBrMaxTile][kBrTerms];  // a tile's point rows; the prologue's tile sums
    double st[kBrightState];
    double S[kBrTerms];
    int cnt[kBrWaves];
    int n;
};

__device__ inline int pow2_ge(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
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

// oracle_common.hpp tree_sum over the rows 0 .. m - 1 of L.acc (m a power of
// two, the padding rows zero), all columns at once; the sums end in row 0.
// Called by every thread of the workgroup.
template <int kBrTerms>
__device__ inline void lds_tree(BrightLds<kBrTerms>& L, int m, int tid) {
    for (int s = 1; s < m; s <<= 1) {
        __syncthreads();
        const int pairs = m / (2 * s);
        for (int e = tid; e < pairs * kBrTerms; e += kBrLanes) {
            const int i = (e / kBrTerms) * 2 * s, t = e % kBrTerms;
            L.acc[i][t] = L.acc[i][t] + L.acc[i + s][t];
        }
    }
    __syncthreads();
}

// device_math.hpp inverse6 (Eigen's PartialPivLU inverse, the same operations
// in the same order) with every index a constant: the row swaps are compares
// against the pivot row instead of indexed moves, so the matrices stay in
// registers.
__device__ inline void inverse6_regs(const double* Hin, double* x) {
    double lu[36];
    int tr[6];
#pragma unroll
    for (int i = 0; i < 36; ++i) {
        lu[i] = Hin[i];
        x[i] = (i % 7 == 0) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double best = fabs(lu[7 * k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double s = fabs(lu[6 * i + k]);
            if (s > best) {
                best = s;
                p = i;
            }
        }
        tr[k] = p;
        if (best != 0.0) {
#pragma unroll
            for (int i = k + 1; i < 6; ++i) {
                if (p == i) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        const double tmp = lu[6 * k + c];
                        lu[6 * k + c] = lu[6 * i + c];
                        lu[6 * i + c] = tmp;
                    }
                }
            }
            const double piv = lu[7 * k];
#pragma unroll
            for (int i = k + 1; i < 6; ++i) lu[6 * i + k] = lu[6 * i + k] / piv;
        }
#pragma unroll
        for (int i = k + 1; i < 6; ++i)
#pragma unroll
            for (int c = k + 1; c < 6; ++c) lu[6 * i + c] = lu[6 * i + c] - lu[6 * i + k] * lu[6 * k + c];
    }
    // X = P I, then unit-L forward and U backward substitution per column
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            if (tr[k] == i) {
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const double tmp = x[6 * k + c];
                    x[6 * k + c] = x[6 * i + c];
                    x[6 * i + c] = tmp;
                }
            }
        }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int i = j + 1; i < 6; ++i) x[6 * i + c] = x[6 * i + c] - lu[6 * i + j] * x[6 * j + c];
#pragma unroll
        for (int j = 5; j >= 0; --j) {
            x[6 * j + c] = x[6 * j + c] / lu[7 * j];
#pragma unroll
            for (int i = 0; i < j; ++i) x[6 * i + c] = x[6 * i + c] - lu[6 * i + j] * x[6 * j + c];
        }
    }
}

// The decisions of pass j and the step behind the pass's sums L.S / L.n: the
// level's result (its report row, the next level from pass 0) or the next
// state of this level.  One lane.  The robust form: d11 = S[44] (sum w) in
// place of 64 n, and level 0's exit keeps S[44] and S[45] of the pass it judged
// (the last pass whose sums were formed) in report columns 24 and 25.
template <bool kRobust>
__device__ void bright_decide(BrightLds<BrForm<kRobust>::kTerms>& L, int iterations) {
    double* st = L.st;
    const int q = (int)st[kStLevel], j = (int)st[kStPass];
    const int n = L.n;
    const double* S = L.S;
    const double cost = S[27] / (double)n;
    const double prev_cost = st[kStPrev + 14];
    int ex = -1;
    bool use_prev = false;
    if (n < 6 || !finite_f64(cost)) {
        ex = j == 0 ? 4 : 5;
        use_prev = j > 0;
    } else if (j >= 1 && cost >= prev_cost) {
        ex = 1;
        use_prev = true;
    } else if (j >= 1 && (1 - cost / prev_cost) < kBrDeltaThresh) {
        ex = 2;
    } else if (j == iterations) {
        ex = 0;
    }
    double xi[6], dg = 0.0, dof = 0.0;
    if (ex < 0) {
        // (g, o) eliminated: A' = A - B D^-1 B^T, b' = b - B D^-1 c
        const double d00 = S[40], d01 = S[41], c0 = S[42], c1 = S[43];
        double d11 = 64.0 * (double)n;
        if constexpr (kRobust) d11 = S[44];
        const double det = d00 * d11 - d01 * d01;
        const double q0 = (d11 * c0 - d01 * c1) / det;
        const double q1 = (d00 * c1 - d01 * c0) / det;
        double Y0[6], Y1[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            Y0[a] = (d11 * S[28 + a] - d01 * S[34 + a]) / det;
            Y1[a] = (d00 * S[34 + a] - d01 * S[28 + a]) / det;
        }
        double A[36], Ai[36], b[6];
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
        for (int a = 0; a < 6; ++a) b[a] = S[21 + a] - (S[28 + a] * q0 + S[34 + a] * q1);
        inverse6_regs(A, Ai);
        bool finite = true;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            double v = Ai[6 * r] * b[0];
#pragma unroll
            for (int c = 1; c < 6; ++c) v = v + Ai[6 * r + c] * b[c];
            xi[r] = v;
            finite = finite && finite_f64(v);
        }
        double s0 = Y0[0] * xi[0], s1 = Y1[0] * xi[0];
#pragma unroll
        for (int a = 1; a < 6; ++a) {
            s0 = s0 + Y0[a] * xi[a];
            s1 = s1 + Y1[a] * xi[a];
        }
        dg = q0 - s0;
        dof = q1 - s1;
        if (!(finite && finite_f64(dg) && finite_f64(dof))) ex = 3;
    }
    if (ex >= 0) {
        const double r_n = use_prev ? st[kStPrev + 15] : (double)n;
        const double r_cost = ex == 4 ? std::numeric_limits<double>::quiet_NaN() : use_prev ? prev_cost : cost;
        const double steps = (double)(use_prev ? j - 1 : ex == 4 ? 0 : j);
        if (use_prev)
            for (int e = 0; e < 14; ++e) st[kStT + e] = st[kStPrev + e];
        double* rep = st + kStReport;
        rep[4 + 4 * q] = (double)ex;
        rep[5 + 4 * q] = steps;
        rep[6 + 4 * q] = r_n;
        rep[7 + 4 * q] = r_cost;
        rep[22] = rep[22] + steps;
        if (q == kLevels - 1) {
            rep[0] = ex == 4 ? 2.0 : 0.0;
            rep[2] = r_n;
            rep[3] = r_cost;
            rep[20] = st[kStT + 12];
            rep[21] = st[kStT + 13];
            if constexpr (kRobust) {
                rep[24] = S[44];
                rep[25] = S[45];
            }
        }
        st[kStLevel] = (double)(q + 1);
        st[kStPass] = 0.0;
    } else {
        // T_{j+1} = exp(xi) T_j (Sophus left-multiplication)
        double T[12], nT[12];
        for (int e = 0; e < 12; ++e) T[e] = st[kStT + e];
        SE3d t0;
        quat_from_matrix(T, t0.q);
        t0.t[0] = T[9];
        t0.t[1] = T[10];
        t0.t[2] = T[11];
        const SE3d t1 = se3_mul(se3_exp(xi), t0);
        se3_to_pose12(t1, nT);
        for (int e = 0; e < 14; ++e) st[kStPrev + e] = st[kStT + e];
        st[kStPrev + 14] = cost;
        st[kStPrev + 15] = (double)n;
        for (int e = 0; e < 12; ++e) st[kStT + e] = nT[e];
        st[kStT + 12] = st[kStT + 12] + dg;
        st[kStT + 13] = st[kStT + 13] + dof;
        st[kStPass] = (double)(j + 1);
    }
}

// Launch k of the chain (last: the launch that writes the results).
template <bool kRobust>
__global__ __launch_bounds__(kBrLanes) void bright_pass_kernel(typename BrForm<kRobust>::Args args, int k,
                                                               int last) {
    constexpr int kBrTerms = BrForm<kRobust>::kTerms;
    const BrightArgs& a = br_base(args);
    __shared__ BrightLds<kBrTerms> L;
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int nt = a.n_tiles;
    const double* st_in = a.state + (size_t)(k & 1) * kBrightState;
    double* st_out = a.state + (size_t)((k + 1) & 1) * kBrightState;
    const double* part_in = a.part + (size_t)((k + 1) & 1) * kBrMaxTiles * kBrTerms;
    const int* good_in = a.good + ((k + 1) & 1) * kBrMaxTiles;
    double* part_out = a.part + (size_t)(k & 1) * kBrMaxTiles * kBrTerms;
    int* good_out = a.good + (k & 1) * kBrMaxTiles;

    // ---- the state: (seed, 1, 0) on level 3 in the first launch
    if (tid < kBrightState) {
        double v;
        if (k == 0) {
            v = 0.0;
            if (tid >= kStT && tid < kStT + 12) v = a.seed[tid - kStT];
            if (tid == kStT + 12) v = 1.0;
            if (tid == kStReport + 1) v = (double)a.n;
            if constexpr (kRobust)
                if (tid == kStReport + 23) v = args.huber_k;
        } else {
            v = st_in[tid];
        }
        L.st[tid] = v;
    }
    __syncthreads();
    if ((int)L.st[kStLevel] >= kLevels && !last) {
        // level 0 has exited: the state only moves on to the next launch
        if (blockIdx.x == 0 && tid < kBrightState) st_out[tid] = L.st[tid];
        return;
    }

    // ---- the prologue: the previous launch's pass — the tree over its tile
    // partials, the decisions, the step
    if (L.st[kStPending] != 0.0) {
        const int p = pow2_ge(nt), m = p >= 4 ? p / 4 : 1;
        // the tree's first two levels on the way into LDS (leaves past nt are +0.0)
        for (int e = tid; e < m * kBrTerms; e += kBrLanes) {
            const int i = e / kBrTerms, t = e % kBrTerms;
            double x[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = 4 * i + r < nt ? part_in[(size_t)(4 * i + r) * kBrTerms + t] : 0.0;
            L.acc[i][t] = p >= 4 ? (x[0] + x[1]) + (x[2] + x[3]) : p == 2 ? x[0] + x[1] : x[0];
        }
        if (wave == 1) {
            int c = 0;
            for (int i = lane; i < nt; i += 64) c += good_in[i];
            for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s);
            if (lane == 0) L.n = c;
        }
        lds_tree(L, m, tid);
        if (tid < kBrTerms) L.S[tid] = L.acc[0][tid];
        __syncthreads();
        if (tid == 0) {
            bright_decide<kRobust>(L, a.iterations);
            L.st[kStPending] = 0.0;
        }
        __syncthreads();
    }
    const int q = (int)L.st[kStLevel];
    if (q >= kLevels || last) {
        if (blockIdx.x != 0) return;
        if (tid < kBrightState) st_out[tid] = L.st[tid];
        if (!last) return;
        // ---- the results, where the direct chain's final solve writes them
        const double* T = L.st + kStT;
        const double* rep = L.st + kStReport;
        if (tid < 12) {
            a.pose_out[tid] = T[tid];
            if (a.log && a.log_index >= 0) {
                a.log[12 * (size_t)a.log_index + tid] = T[tid];
                if (a.log_host)
                    __hip_atomic_store(a.log_host + 12 * (size_t)a.log_index + tid, T[tid], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        if constexpr (kRobust) {
            // the plain report keeps its column 23 (0); the robust one has k there
            if (tid < kBrightReport && a.report) a.report[tid] = tid == 23 ? 0.0 : rep[tid];
            if (tid < kRobustReport) args.report[tid] = rep[tid];
            if (tid == 0) {
                if (args.rlog && a.log_index >= 0) {
                    double* row = args.rlog + 2 * (size_t)a.log_index;
                    row[0] = rep[24] / (64.0 * rep[2]);
                    row[1] = rep[25];
                }
                if (args.info) {
                    args.info[1] = args.info[1] + 1;
                    args.info[2] = (long long)rep[25];
                    args.info[3] = (long long)rep[2];
                }
            }
        } else {
            if (tid < kBrightReport) a.report[tid] = rep[tid];
        }
        if (tid == 0) {
            if (a.stats) {
                a.stats[0] = rep[2];
                a.stats[1] = rep[3];
            }
            if (a.log && a.log_index >= 0) {
                if (a.flog) {
                    a.flog[4 * (size_t)a.log_index + 0] = rep[2];
                    a.flog[4 * (size_t)a.log_index + 1] = rep[3];
                }
                if (a.blog) {
                    double* row = a.blog + 4 * (size_t)a.log_index;
                    row[0] = rep[20];
                    row[1] = rep[21];
                    row[2] = rep[16];
                    row[3] = rep[22];
                }
            }
            if (a.info) {
                a.info[1] = a.info[1] + 1;
                a.info[2] = a.info[2] + (long long)rep[22];
                a.info[3] = a.info[3] + (rep[0] == 2.0 ? 1 : 0);
                a.info[4] = (long long)rep[16];
                a.info[5] = (long long)rep[22];
                a.info[6] = (long long)rep[2];
            }
        }
        return;
    }

    // ---- the pass at (T, g, o) on this level: the workgroup's tiles
    const int level = kLevels - 1 - q;
    const double scale = kScale[level];
    const int w = a.w[level], h = a.h[level];
    const uint8_t* limg = a.last.l[level];
    const uint8_t* cimg = a.cur.l[level];
    const double fxs = a.K[0] * scale, fys = a.K[1] * scale;
    double T[12], Lp[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        T[e] = L.st[kStT + e];
        Lp[e] = a.pose_last[e];
    }
    const double g = L.st[kStT + 12], o = L.st[kStT + 13];
    // the term lane t forms: A entry (ta, tb) for t < 21; entry ta of b for
    // t < 27, of B's columns for 28 <= t < 40
    int ta = 0, tb = 0;
    {
        int t = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int r = p; r < 6; ++r, ++t)
                if (t == lane) {
                    ta = p;
                    tb = r;
                }
        if (lane >= 21 && lane < 27) ta = lane - 21;
        if (lane >= 28 && lane < 34) ta = lane - 28;
        if (lane >= 34 && lane < 40) ta = lane - 34;
    }
    const double px = (double)((lane >> 3) - kHalfPatch), py = (double)((lane & 7) - kHalfPatch);
    const double hp = 4.0;
    double hk = 0.0;  // Huber's k
    if constexpr (kRobust) hk = args.huber_k;
    if (blockIdx.x == 0 && tid < kBrightState) st_out[tid] = tid == kStPending ? 1.0 : L.st[tid];

    for (int tile = blockIdx.x; tile < nt; tile += gridDim.x) {
        const int first = tile * a.tile;
        const int c = a.n - first < a.tile ? a.n - first : a.tile;
        const int pc = pow2_ge(c);
        int cnt = 0;
        for (int p = wave; p < pc; p += kBrWaves) {
            double term = 0.0;  // the padding rows, and a point that is not good
            double mass = 0.0;  // (robust) the point's sum w
            bool good = false;
            double ur = 0, vr = 0, uc = 0, vc = 0, Pr[3], Pc[3] = {0, 0, 1};
            if (p < c) {
                const double* Pp = a.points + 3 * (size_t)(first + p);
                const double P[3] = {Pp[0], Pp[1], Pp[2]};
                const double zr = project_level(Lp, a.K, P, scale, ur, vr, Pr);
                const double zc = project_level(T, a.K, P, scale, uc, vc, Pc);
                good = inside_px(ur - hp, vr - hp, w, h) && inside_px(ur + hp, vr + hp, w, h) &&
                       inside_px(uc - hp, vc - hp, w, h) && inside_px(uc + hp, vc + hp, w, h) && zr > 0 && zc > 0;
            }
            if (__builtin_amdgcn_readfirstlane(good ? 1 : 0)) {
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
                const double R = sample_px(limg, w, h, ur + px, vr + py);
                const double C = sample_px(cimg, w, h, xc, yc);
                const double err = (g * R + o) - C;
                double g0, g1;
                gradient_px(cimg, w, h, xc, yc, g0, g1);
                double G[15];
                double n_out = 0.0;
                if constexpr (kRobust) {
                    // Huber's weight of the pixel: every leaf is w x, x the plain
                    // form's leaf; the cost's is twice the Huber function
                    const double r = fabs(err);
                    const bool out = r > hk;
                    const double wt = out ? hk / r : 1.0;
                    const double rho = out ? hk * (2.0 * r - hk) : err * err;
                    n_out = (double)__popcll(__ballot(out));
                    wave_tree_sum3_desc(wt * (g0 * g0), wt * (g0 * g1), wt * (g1 * g1), G[0], G[1], G[2]);
                    wave_tree_sum3_desc(wt * (err * g0), wt * (err * g1), rho, G[3], G[4], G[5]);
                    wave_tree_sum3_desc(wt * (g0 * R), wt * (g1 * R), wt * g0, G[6], G[7], G[8]);
                    wave_tree_sum3_desc(wt * g1, wt * (R * R), wt * R, G[9], G[10], G[11]);
                    wave_tree_sum3_desc(wt * (err * R), wt * err, wt, G[12], G[13], G[14]);
                    mass = G[14];
                } else {
                    wave_tree_sum3_desc(g0 * g0, g0 * g1, g1 * g1, G[0], G[1], G[2]);
                    wave_tree_sum3_desc(err * g0, err * g1, err * err, G[3], G[4], G[5]);
                    wave_tree_sum3_desc(g0 * R, g1 * R, g0, G[6], G[7], G[8]);
                    wave_tree_sum3_desc(g1, R * R, R, G[9], G[10], G[11]);
                    wave_tree_sum3_desc(err * R, err, 0.0, G[12], G[13], G[14]);
                }
                const double J0a = pick6(J0, ta), J0b = pick6(J0, tb), J1a = pick6(J1, ta), J1b = pick6(J1, tb);
                const double th = (G[0] * (J0a * J0b) + G[1] * (J0a * J1b + J1a * J0b)) + G[2] * (J1a * J1b);
                const double tbv = G[3] * J0a + G[4] * J1a;
                const double tB0 = -(G[6] * J0a + G[7] * J1a);
                const double tB1 = -(G[8] * J0a + G[9] * J1a);
                term = lane < 21   ? th
                       : lane < 27 ? tbv
                       : lane < 28 ? G[5]
                       : lane < 34 ? tB0
                       : lane < 40 ? tB1
                       : lane == 40 ? G[10]
                       : lane == 41 ? G[11]
                       : lane == 42 ? -G[12]
                                    : -G[13];
                if constexpr (kRobust) term = lane == 44 ? G[14] : lane == 45 ? n_out : term;
                cnt += 1;
            }
            if (lane < kBrTerms) L.acc[p][lane] = term;
            if constexpr (kRobust)
                if (lane == 0 && p < c) args.weights[first + p] = mass;
        }
        if (lane == 0) L.cnt[wave] = cnt;
        lds_tree(L, pc, tid);
        if (tid < kBrTerms) part_out[(size_t)tile * kBrTerms + tid] = L.acc[0][tid];
        if (tid == 64) {
            int v = 0;
            for (int i = 0; i < kBrWaves; ++i) v += L.cnt[i];
            good_out[tile] = v;
        }
        __syncthreads();  // (the rows and counts are free for the next tile)
    }
}

}  // namespace

size_t bright_scratch_bytes() {
    return 2 * (size_t)kBrMaxTiles * kBrightTerms * 8 + 2 * (size_t)kBrMaxTiles * 4 + 2 * (size_t)kBrightState * 8;
}

void bright_scratch_at(BrightArgs& a, void* base) {
    char* b = (char*)base;
    a.part = (double*)b;
    b += 2 * (size_t)kBrMaxTiles * kBrightTerms * 8;
    a.state = (double*)b;
    b += 2 * (size_t)kBrightState * 8;
    a.good = (int*)b;
}

int bright_launches(int iterations) { return kLevels * (iterations + 1) + 1; }

namespace {

// the canonical map tree's tiles; returns the grid
int bright_tiles(BrightArgs& a) {
    const int n = a.n > 0 ? a.n : 0;
    a.tile = std::max(1, std::min(kBrMaxTile, (n + kBrMaxTiles - 1) / kBrMaxTiles));  // oracle_common.hpp map_tile
    a.n_tiles = (n + a.tile - 1) / a.tile;
    return a.n_tiles > 0 ? a.n_tiles : 1;
}

}  // namespace

void launch_bright(BrightArgs a, hipStream_t stream) {
    const int grid = bright_tiles(a), chain = bright_launches(a.iterations);
    for (int k = 0; k < chain; ++k) {
        const int last = k == chain - 1;
        bright_pass_kernel<false><<<last ? 1 : grid, kBrLanes, 0, stream>>>(a, k, last);
    }
}

size_t robust_scratch_bytes() {
    return 2 * (size_t)kBrMaxTiles * kRobustTerms * 8 + 2 * (size_t)kBrMaxTiles * 4 + 2 * (size_t)kBrightState * 8;
}

void robust_scratch_at(RobustArgs& a, void* base) {
    char* b = (char*)base;
    a.b.part = (double*)b;
    b += 2 * (size_t)kBrMaxTiles * kRobustTerms * 8;
    a.b.state = (double*)b;
    b += 2 * (size_t)kBrightState * 8;
    a.b.good = (int*)b;
}

void launch_robust(RobustArgs a, hipStream_t stream) {
    const int grid = bright_tiles(a.b), chain = bright_launches(a.b.iterations);
    for (int k = 0; k < chain; ++k) {
        const int last = k == chain - 1;
        bright_pass_kernel<true><<<last ? 1 : grid, kBrLanes, 0, stream>>>(a, k, last);
    }
}

}  // namespace viso

using namespace viso;

// A tracking frame with the mode on (on_new_frame, in place of the direct
// chain): cur's pose from the last frame's, written with its log rows, the
// level-0 stats and the report by the chain's last launch.
int viso_ctx::bright_frame(int last, int cur, int li) {
    BrightArgs a{};
    intrinsics(a.K);
    a.last = frame(last);
    a.cur = frame(cur);
    for (int l = 0; l < kLevels; ++l) {
        a.w[l] = geom.w[l];
        a.h[l] = geom.h[l];
    }
    a.points = (const double*)map_pts.ptr;
    a.n = n_map;
    a.pose_last = pose_of(last);
    a.seed = pose_of(last);
    a.iterations = bright_iterations;
    bright_scratch_at(a, bright_buf.ptr);
    a.pose_out = pose_of(cur);
    a.log = li >= 0 ? (double*)pose_log.ptr : nullptr;
    a.log_host = log_host(li);
    a.flog = flog();
    a.blog = bright_log();
    a.log_index = li;
    a.stats = (double*)direct_stats.ptr;
    a.report = bright_report();
    a.info = bright_info();
    {
        TimedRegion t(timing, VISO_KERNEL_BRIGHT, stream);
        if (robust_on()) {
            // the robust form: its own scratch, report, weights, log and
            // counters; the brightness report, log and counters as ever
            RobustArgs r{};
            r.b = a;
            robust_scratch_at(r, robust_buf.ptr);
            r.huber_k = robust_k;
            r.weights = robust_weights();
            r.report = robust_report();
            r.rlog = robust_log();
            r.info = robust_info();
            robust_wn = n_map;
            launch_robust(r, stream);
        } else {
            launch_bright(a, stream);
        }
    }
    VISO_HIP_CHECK(hipGetLastError());
    return VISO_OK;
}

int viso_ctx::robust_ensure() {
    if (!bright_on() || !robust_on() || robust_buf.ptr) return VISO_OK;
    VISO_HIP_CHECK(hipSetDevice(device));
    const size_t head = robust_head() + 8 * (size_t)kMaxMapPoints;
    const size_t bytes = head + 16 * (size_t)std::max(p.max_poses, 1);
    if (int rc = robust_buf.ensure(bytes)) return rc;
    VISO_HIP_CHECK(hipMemsetAsync(robust_buf.ptr, 0, head, stream));
    VISO_HIP_CHECK(hipMemsetAsync((char*)robust_buf.ptr + head, 0xff, bytes - head, stream));  // NaN rows
    return VISO_OK;
}

namespace {

// viso_track_affine (huber_k = 0) and viso_track_robust behind their argument
// checks: the stage on host data through the frame path's launches.
int track_stage(viso_ctx* c, const uint8_t* last_pyr, const uint8_t* cur_pyr, int width, int height,
                const double* points, int n_points, const double* pose_last12, const double* seed12, int iterations,
                double huber_k, double* pose_out12, double* report, double* weights) {
    const bool robust = huber_k > 0.0;
    const int n_report = robust ? kRobustReport : kBrightReport;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const PyrGeom g = make_geom(width, height);
    Bump b;
    const size_t o_l = b.take(g.bytes), o_c = b.take(g.bytes), o_p = b.take(24 * (size_t)std::max(n_points, 1)),
                 o_pl = b.take(96), o_s = b.take(96), o_po = b.take(96), o_r = b.take(8 * n_report),
                 o_x = b.take(robust ? robust_scratch_bytes() : bright_scratch_bytes()),
                 o_w = b.take(robust ? 8 * (size_t)std::max(n_points, 1) : 0);
    if (int rc = c->scratch_a.ensure(b.off)) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_l, last_pyr, g.bytes, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_c, cur_pyr, g.bytes, hipMemcpyHostToDevice, c->stream));
    if (n_points > 0)
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n_points, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_pl, pose_last12, 96, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_s, seed12, 96, hipMemcpyHostToDevice, c->stream));
    BrightArgs a{};
    c->intrinsics(a.K);
    a.last = frame_from_base((const uint8_t*)(base + o_l), g);
    a.cur = frame_from_base((const uint8_t*)(base + o_c), g);
    for (int l = 0; l < kLevels; ++l) {
        a.w[l] = g.w[l];
        a.h[l] = g.h[l];
    }
    a.points = (const double*)(base + o_p);
    a.n = n_points;
    a.pose_last = (const double*)(base + o_pl);
    a.seed = (const double*)(base + o_s);
    a.iterations = iterations;
    a.pose_out = (double*)(base + o_po);
    a.log_index = -1;
    {
        TimedRegion t(c->timing, VISO_KERNEL_BRIGHT, c->stream);
        if (robust) {
            RobustArgs r{};
            r.b = a;
            robust_scratch_at(r, base + o_x);
            r.huber_k = huber_k;
            r.weights = (double*)(base + o_w);
            r.report = (double*)(base + o_r);
            launch_robust(r, c->stream);
        } else {
            bright_scratch_at(a, base + o_x);
            a.report = (double*)(base + o_r);
            launch_bright(a, c->stream);
        }
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(pose_out12, base + o_po, 96, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(report, base + o_r, 8 * (size_t)n_report, hipMemcpyDeviceToHost, c->stream));
    if (robust && weights && n_points > 0)
        VISO_HIP_CHECK(hipMemcpyAsync(weights, base + o_w, 8 * (size_t)n_points, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

bool track_args_ok(viso_ctx* c, const uint8_t* last_pyr, const uint8_t* cur_pyr, int width, int height,
                   const double* points, int n_points, const double* pose_last12, const double* seed12, int iterations,
                   double* pose_out12, double* report) {
    return c && last_pyr && cur_pyr && width >= 64 && height >= 64 && width <= kMaxWidth && height <= kMaxWidth &&
           n_points >= 0 && n_points <= kMaxMapPoints && (n_points == 0 || points) && pose_last12 && seed12 &&
           iterations >= 1 && iterations <= 20 && pose_out12 && report;
}

// viso_set_robust's and viso_track_robust's k: finite, 0 < k <= 1e300
bool huber_k_ok(double k) { return k > 0.0 && k <= 1e300; }

}  // namespace

extern "C" {

int viso_track_affine(viso_ctx* c, const uint8_t* last_pyr, const uint8_t* cur_pyr, int32_t width, int32_t height,
                      const double* points, int32_t n_points, const double* pose_last12, const double* seed12,
                      int32_t iterations, double* pose_out12, double* report24) {
    if (!track_args_ok(c, last_pyr, cur_pyr, width, height, points, n_points, pose_last12, seed12, iterations,
                       pose_out12, report24))
        return VISO_ERR_ARG;
    return track_stage(c, last_pyr, cur_pyr, width, height, points, n_points, pose_last12, seed12, iterations, 0.0,
                       pose_out12, report24, nullptr);
}

int viso_track_robust(viso_ctx* c, const uint8_t* last_pyr, const uint8_t* cur_pyr, int32_t width, int32_t height,
                      const double* points, int32_t n_points, const double* pose_last12, const double* seed12,
                      int32_t iterations, double huber_k, double* pose_out12, double* report28, double* weights) {
    if (!track_args_ok(c, last_pyr, cur_pyr, width, height, points, n_points, pose_last12, seed12, iterations,
                       pose_out12, report28) ||
        !huber_k_ok(huber_k))
        return VISO_ERR_ARG;
    return track_stage(c, last_pyr, cur_pyr, width, height, points, n_points, pose_last12, seed12, iterations, huber_k,
                       pose_out12, report28, weights);
}

int viso_set_robust(viso_ctx* c, double huber_k) {
    if (!c || !(huber_k == 0.0 || huber_k_ok(huber_k))) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    c->robust_k = huber_k;
    return c->robust_ensure();
}

int viso_get_robust(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    for (int k = 0; k < 8; ++k) info[k] = 0;
    if (c->robust_buf.ptr) {
        VISO_HIP_CHECK(hipSetDevice(c->device));
        VISO_HIP_CHECK(hipMemcpyAsync(info, c->robust_info(), 64, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    info[0] = c->robust_on() ? 1 : 0;
    for (int k = 4; k < 8; ++k) info[k] = 0;
    return VISO_OK;
}

int viso_get_robust_report(viso_ctx* c, double report[28]) {
    if (!c || !report) return VISO_ERR_ARG;
    if (!c->robust_buf.ptr) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    VISO_HIP_CHECK(hipMemcpyAsync(report, c->robust_report(), 8 * kRobustReport, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

int viso_get_robust_weights(viso_ctx* c, double* w, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (!c->robust_buf.ptr) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t total = (size_t)c->robust_wn;
    if (n) *n = total;
    const size_t m = std::min(cap, total);
    if (m > 0 && w) VISO_HIP_CHECK(hipMemcpyAsync(w, c->robust_weights(), 8 * m, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

int viso_get_robust_log(viso_ctx* c, double* rows, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (!c->robust_buf.ptr) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t total = std::min((size_t)c->n_poses, (size_t)std::max(c->p.max_poses, 0));
    if (n) *n = total;
    const size_t m = std::min(cap, total);
    if (m > 0 && rows) VISO_HIP_CHECK(hipMemcpyAsync(rows, c->robust_log(), 16 * m, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

int viso_set_brightness(viso_ctx* c, int32_t iterations) {
    if (!c || iterations < 0 || iterations > 20) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    if (iterations > 0 && !c->bright_buf.ptr) {
        VISO_HIP_CHECK(hipSetDevice(c->device));
        // the chain's scratch, then info (8 x int64), the last report, the log
        const size_t head = c->bright_head(), bytes = head + 32 * (size_t)std::max(c->p.max_poses, 1);
        if (int rc = c->bright_buf.ensure(bytes)) return rc;
        VISO_HIP_CHECK(hipMemsetAsync(c->bright_buf.ptr, 0, head, c->stream));
        VISO_HIP_CHECK(hipMemsetAsync((char*)c->bright_buf.ptr + head, 0xff, bytes - head, c->stream));  // NaN rows
    }
    c->bright_iterations = iterations;
    return c->robust_ensure();  // (viso_set_robust ahead of this call)
}

int viso_get_brightness(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    for (int k = 0; k < 8; ++k) info[k] = 0;
    if (c->bright_buf.ptr) {
        VISO_HIP_CHECK(hipSetDevice(c->device));
        VISO_HIP_CHECK(hipMemcpyAsync(info, c->bright_info(), 64, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    info[0] = c->bright_iterations;
    info[7] = 0;
    return VISO_OK;
}

int viso_get_brightness_log(viso_ctx* c, double* rows, size_t cap, size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (!c->bright_on()) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t total = std::min((size_t)c->n_poses, (size_t)std::max(c->p.max_poses, 0));
    if (n) *n = total;
    const size_t m = std::min(cap, total);
    if (m > 0 && rows)
        VISO_HIP_CHECK(hipMemcpyAsync(rows, c->bright_log(), 32 * m, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

int viso_get_brightness_report(viso_ctx* c, double report[24]) {
    if (!c || !report) return VISO_ERR_ARG;
    if (!c->bright_on()) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    VISO_HIP_CHECK(hipMemcpyAsync(report, c->bright_report(), 8 * kBrightReport, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

}  // extern "C"
