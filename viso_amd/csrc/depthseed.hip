// viso_amd — depth seeds: the map grows by an epipolar search over the frames
// after a keyframe (viso_set_depth_seeds, include/viso/viso_c.h; DESIGN.md
// §18).  The repo's own spec, restated in tests/depth_seed_ref.py; the
// reference has no counterpart.
//
// A seed is a corner of a keyframe h with an inverse depth mu (of z in h's
// camera) and its variance s2.  Creation: the cell winners of a new keyframe's
// FAST corners in the cells the map leaves unmarked (monokf.hip's occupancy,
// winner and compaction kernels) become seeds with the whole depth range.
// Update, once per tracking frame: the segment mu ± 2 sigma of the seed's
// epipolar line is searched in steps of one pixel of the level that holds it
// in max_steps steps, for the host patch warped by §17's affine map; the best
// step's depth is fused into (mu, s2).  Promotion: converged seeds become map
// points, failed ones are dropped, survivors compacted in order.
//
// Mapping: the update is one wave per seed, lane = patch pixel (the LK
// kernels' geometry); the per-seed scalars are computed once per wave with
// their divisions spread over the low lanes.  fp64 in both precision modes,
// in the operand order of the restatement, -ffp-contract=off; the 64-pixel
// sums are wave_tree_sum (the ascending tree).  No atomics, no scratch.
#include <algorithm>
#include <cmath>

#include "block_rank.hpp"
#include "context.hpp"
#include "device_math.hpp"

namespace viso {

namespace {

constexpr double kInf = __builtin_huge_val();

__device__ inline bool uni(bool b) { return __builtin_amdgcn_readfirstlane(b ? 1 : 0) != 0; }

// min over the wave (exact in any order)
__device__ inline double wave_min(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void seed_update_kernel(SeedUpdateArgs a) {
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (i >= a.n) return;
    const SeedUpdateArgs* ka = (const SeedUpdateArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63;
    const int px = (lane >> 3) - 4, py = (lane & 7) - 4;
    const bool odd = lane & 1;
    const Intrinsics K{a.K[0], a.K[1], a.K[2], a.K[3]};
    const int h = __builtin_amdgcn_readfirstlane(a.rows.h[i]);
    const double u = a.rows.uv[2 * (size_t)i], v = a.rows.uv[2 * (size_t)i + 1];
    const double mu = a.rows.mu[i], s2 = a.rows.s2[i];
    int4 cnt = a.rows.cnt[i];
    const double rho_min = a.p.rho_min, rho_max = a.p.rho_max;
    const double* hp = a.kf_poses + 12 * h;
    const double* cp = a.cur_pose;
    int st = 0, lvl = -1, jstar = -1;
    double mu_n = mu, s2_n = s2;
    do {
        // 1. the segment: R = R_c R_h^T, t = t_c - R t_h, q = R f
        double R[9], t[3], q[3];
        relative_motion(hp, cp, R, t);
        // f's two divisions on lanes 0 and 1
        const double fq = ((odd ? v : u) - (odd ? K.cy : K.cx)) / (odd ? K.fy : K.fx);
        const double f0 = readlane_f64(fq, 0), f1 = readlane_f64(fq, 1);
#pragma unroll
        for (int r = 0; r < 3; ++r) q[r] = (R[3 * r] * f0 + R[3 * r + 1] * f1) + R[3 * r + 2] * 1.0;
        const double sig = sqrt(s2);
        const double lo = mu - 2.0 * sig, hi = mu + 2.0 * sig;
        const double rlo = lo > rho_min ? lo : rho_min, rhi = hi < rho_max ? hi : rho_max;
        // the three pixels' six divisions on lanes 0 (rho_lo), 1 (rho_hi), 2 (mu)
        const int l3 = lane & 3;
        const double rho = l3 == 0 ? rlo : l3 == 1 ? rhi : mu;
        const double X0 = q[0] + rho * t[0], X1 = q[1] + rho * t[1], X2 = q[2] + rho * t[2];
        const double pu = X0 / X2 * K.fx + K.cx, pv = X1 / X2 * K.fy + K.cy;
        const double ax = readlane_f64(pu, 0), ay = readlane_f64(pv, 0), az = readlane_f64(X2, 0);
        const double bx = readlane_f64(pu, 1), by = readlane_f64(pv, 1), bz = readlane_f64(X2, 1);
        const double mx = readlane_f64(pu, 2), my = readlane_f64(pv, 2), mz = readlane_f64(X2, 2);
        if (!uni(az > 0 && bz > 0 && mz > 0 && inside_px(mx, my, a.g.w[0], a.g.h[0]))) {
            st = 1;
            break;
        }
        // 2. the level and the steps
        const double dx = bx - ax, dy = by - ay;
        const double adx = fabs(dx), ady = fabs(dy);
        const double Lm = adx >= ady ? adx : ady;
        const int k = __builtin_amdgcn_readfirstlane(adx >= ady ? 0 : 1);
        const double lim = (double)(a.p.max_steps - 1);
        int l = -1;
#pragma unroll
        for (int c = kLevels - 1; c >= 0; --c)
            if (Lm * kScale[c] <= lim) l = c;
        l = __builtin_amdgcn_readfirstlane(l);
        if (l < 0) {
            st = 3;
            break;
        }
        const double ks = l == 0 ? 1.0 : l == 1 ? 0.5 : l == 2 ? 0.25 : 0.125;
        const double Ls = Lm * ks;
        if (uni(Ls < 1)) {
            st = 4;
            break;
        }
        lvl = l;
        const int n = __builtin_amdgcn_readfirstlane(min((int)floor(Ls) + 1, 64));
        const double eq = (odd ? dy : dx) / Lm;
        const double ex = readlane_f64(eq, 0), ey = readlane_f64(eq, 1);
        // 3. the template: §17's affine map with anchor h, (bu, bv) = (u, v),
        // za = 1 / mu, (uc, vc) = the pixel of mu.  Even lanes carry Qu, odd
        // lanes Qv (lk_warp_kernel's arrangement).
        const double za = 1.0 / mu;
        const double qu = odd ? u : u + 4.0, qv = odd ? v + 4.0 : v;
        const double Ph[3] = {(qu - K.cx) / K.fx * za, (qv - K.cy) / K.fy * za, za};
        double Wp[3];
        camera_to_world(hp, Ph, Wp);
        double uq, vq;
        const double zq = project_px_depth(cp, K, Wp, uq, vq);
        const double au = (uq - mx) / 4.0, av = (vq - my) / 4.0;
        const double A00 = readlane_f64(au, 0), A10 = readlane_f64(av, 0);
        const double A01 = readlane_f64(au, 1), A11 = readlane_f64(av, 1);
        const double zu = readlane_f64(zq, 0), zv = readlane_f64(zq, 1);
        const double det = A00 * A11 - A01 * A10;
        double D = fabs(det);
        if (!uni(za > 0 && zu > 0 && zv > 0 && finite_f64(A00) && finite_f64(A01) && finite_f64(A10) && finite_f64(A11) &&
                 1.0 / kSeedAreaRatio <= D && D <= kSeedAreaRatio)) {
            st = 2;
            break;
        }
        const double num = l3 == 0 ? A11 : l3 == 1 ? -A01 : l3 == 2 ? -A10 : A00;
        const double qi = num / det;  // the inverse's four divisions on lanes 0..3
        const double Ai00 = readlane_f64(qi, 0), Ai01 = readlane_f64(qi, 1), Ai10 = readlane_f64(qi, 2),
                     Ai11 = readlane_f64(qi, 3);
        int shift = 0;
        if (D > 3.0) {
            while (D > 3.0 && shift > -3) {
                shift -= 1;
                D *= 0.25;
            }
        } else if (D < 1.0 / 3.0) {
            while (D < 1.0 / 3.0 && shift < 3) {
                shift += 1;
                D *= 4.0;
            }
        }
        shift = __builtin_amdgcn_readfirstlane(shift);
        const int r = min(max(l + shift, 0), kLevels - 1);
        const double sr = r == 0 ? 1.0 : r == 1 ? 0.5 : r == 2 ? 0.25 : 0.125;
        const double kk = sr / ks;  // an exact power of two
        const int wr = ka->g.w[r], hr = ka->g.h[r];
        const double x = u * sr + ((Ai00 * px + Ai01 * py) * kk);
        const double y = v * sr + ((Ai10 * px + Ai11 * py) * kk);
        if (__builtin_amdgcn_ballot_w64(0 <= x && x + 1 < wr && 0 <= y && y + 1 < hr) != ~0ull) {
            st = 5;
            break;
        }
        const double I1 = sample_px(ka->kf[h].l[r], wr, hr, x, y);
        const double tt = I1 - wave_tree_sum(I1) / 64.0;
        // 4. the scores: step j's score ends in lane j
        const int wl = ka->g.w[l], hl = ka->g.h[l];
        const uint8_t* curl = ka->cur.l[l];
        const double xmax = (double)(wl - 1), ymax = (double)(hl - 1);
        const double sx = ax * ks, sy = ay * ks;
        double Sj = kInf;
        unsigned long long valid = 0;
        for (int j = 0; j < n; ++j) {
            const double X = (sx + j * ex) + px, Y = (sy + j * ey) + py;
            if (__builtin_amdgcn_ballot_w64(0 <= X && X < xmax && 0 <= Y && Y < ymax) != ~0ull) continue;
            const double c = sample_px(curl, wl, hl, X, Y);
            const double cb = wave_tree_sum(c) / 64.0;
            const double e = (c - cb) - tt;
            const double S = wave_tree_sum(e * e);
            Sj = lane == j ? S : Sj;
            valid |= 1ull << j;
        }
        if (__popcll(valid) < 3) {
            st = 6;
            break;
        }
        // 5. the best step (the first of the least) and the best away from it
        const double Sst = wave_min(Sj);
        const int js = __builtin_amdgcn_readfirstlane(__ffsll((long long)__builtin_amdgcn_ballot_w64(Sj == Sst)) - 1);
        jstar = js;
        const int dj = lane - js;
        const double S2 = wave_min((dj > 1 || dj < -1) ? Sj : kInf);
        if (uni(Sst > a.p.max_score)) {
            st = 7;
            break;
        }
        if (uni(Sst * a.p.uniqueness > S2)) {
            st = 8;
            break;
        }
        // 6. the sub-step
        const bool both = js > 0 && js < 63 && ((valid >> (js - 1)) & 1ull) && ((valid >> (js + 1)) & 1ull);
        const double Sm = __shfl(Sj, max(js - 1, 0), 64), Sp = __shfl(Sj, min(js + 1, 63), 64);
        const double den = (Sm - 2.0 * Sst) + Sp;
        double delta = 0.0;
        if (both && den > 0) {
            delta = 0.5 * (Sm - Sp) / den;
            delta = delta > -0.5 ? delta : -0.5;
            delta = delta < 0.5 ? delta : 0.5;
        }
        const double pk = k == 0 ? sx + js * ex : sy + js * ey;
        const double ek = k == 0 ? ex : ey;
        const double m_k = (pk + delta * ek) / ks;
        // 7. the depth: rho_obs on lane 0, rho_1 (one step further) on lane 1
        const double c_k = k == 0 ? K.cx : K.cy, f_k = k == 0 ? K.fx : K.fy;
        const double q_k = k == 0 ? q[0] : q[1], t_k = k == 0 ? t[0] : t[1];
        const double mm = odd ? m_k + 1.0 / ks : m_k;
        const double n_k = (mm - c_k) / f_k;
        const double rq = (n_k * q[2] - q_k) / (t_k - n_k * t[2]);
        const double robs = readlane_f64(rq, 0), r1 = readlane_f64(rq, 1);
        if (!uni(finite_f64(robs) && finite_f64(r1) && rho_min <= robs && robs <= rho_max)) {
            st = 9;
            break;
        }
        const double dr = r1 - robs, fl = 1e-4 * (rho_max - rho_min);
        const double dr2 = dr * dr, fl2 = fl * fl;
        const double tau2 = dr2 > fl2 ? dr2 : fl2;
        // 8. the fusion: its two divisions on lanes 0 and 1
        const double vv = s2 + tau2;
        const double fz = (odd ? s2 * tau2 : tau2 * mu + s2 * robs) / vv;
        mu_n = readlane_f64(fz, 0);
        s2_n = readlane_f64(fz, 1);
        st = 0;
    } while (false);
    if (lane == 0) {
        // 1, 2, 5, 6 lose the seed once more; 3 and 4 change nothing; 0 and
        // 7..9 scored a search, so lost = 0
        if (st == 1 || st == 2 || st == 5 || st == 6) cnt.z += 1;
        if (st == 0 || st >= 7) cnt.z = 0;
        if (st >= 7) cnt.y += 1;
        if (st == 0) cnt.x += 1;
        cnt.w = st;
        a.rows.mu[i] = mu_n;
        a.rows.s2[i] = s2_n;
        a.rows.cnt[i] = cnt;
        if (a.diag) a.diag[i] = make_int2(lvl, jstar);
    }
}

// Promotion: one workgroup walks the seeds in chunks of 1024.  Per seed a
// class (converged first, then dropped); the converged ones of rank < room
// become points in seed order, every seed that is neither promoted nor dropped
// is kept, compacted in place in seed order (a chunk's rows are all read
// before the first block_rank call and written behind the second, to indices
// no later chunk reads; block_rank.hpp).
__global__ __launch_bounds__(1024) void seed_promote_kernel(SeedPromoteArgs a) {
    __shared__ int s_w[2 * 16], s_s[16];
    const int tid = threadIdx.x;
    int base_c = 0, base_s = 0, base_d = 0;
    for (int i0 = 0; i0 < a.n; i0 += 1024) {
        const int i = i0 + tid;
        const bool live = i < a.n;
        int h = 0;
        double u = 0.0, v = 0.0, mu = 1.0, s2 = 0.0;
        int4 cnt = make_int4(0, 0, 0, 0);
        if (live) {
            h = a.rows.h[i];
            u = a.rows.uv[2 * (size_t)i];
            v = a.rows.uv[2 * (size_t)i + 1];
            mu = a.rows.mu[i];
            s2 = a.rows.s2[i];
            cnt = a.rows.cnt[i];
        }
        const double lim = a.conv_rel * mu;
        const bool conv = live && cnt.x >= a.min_good && s2 <= lim * lim;
        const bool drop = live && !conv && (cnt.y >= a.max_bad || cnt.z >= a.max_lost);
        const bool cd[2] = {conv, drop};
        BlockRank r[2];  // (of the dropped only the count)
        block_rank<16>(cd, s_w, r);
        const int rank = base_c + r[0].rank;
        const bool prom = conv && rank < a.room;
        const bool surv = live && !prom && !drop;
        const BlockRank rs = block_rank<16>(surv, s_s);
        if (prom) {
            // R_h^T (f / mu - t_h)
            const double Ph[3] = {((u - a.K[2]) / a.K[0]) / mu, ((v - a.K[3]) / a.K[1]) / mu, 1.0 / mu};
            camera_to_world(a.kf_poses + 12 * h, Ph, a.out_pts + 3 * (size_t)rank);
            a.out_host[rank] = h;
        }
        if (surv) {
            const int j = base_s + rs.rank;
            a.rows.h[j] = h;
            a.rows.uv[2 * (size_t)j] = u;
            a.rows.uv[2 * (size_t)j + 1] = v;
            a.rows.mu[j] = mu;
            a.rows.s2[j] = s2;
            a.rows.cnt[j] = cnt;
        }
        base_c += r[0].total;
        base_s += rs.total;
        base_d += r[1].total;
    }
    if (tid == 0) {
        a.counts[0] = base_c;
        a.counts[1] = min(base_c, max(a.room, 0));
        a.counts[2] = base_d;
        a.counts[3] = base_s;
    }
}

// A retirement (viso_set_map_window): the seeds of keyframe 0 leave, the others
// move up in order with h - 1 (seed_promote_kernel's in-place compaction);
// counts[0] = survivors
__global__ __launch_bounds__(1024) void seed_retire_kernel(SeedRows rows, int n, int* counts) {
    __shared__ int s_s[16];
    const int tid = threadIdx.x;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        int h = 0;
        double u = 0.0, v = 0.0, mu = 0.0, s2 = 0.0;
        int4 cnt = make_int4(0, 0, 0, 0);
        if (i < n) {
            h = rows.h[i];
            u = rows.uv[2 * (size_t)i];
            v = rows.uv[2 * (size_t)i + 1];
            mu = rows.mu[i];
            s2 = rows.s2[i];
            cnt = rows.cnt[i];
        }
        const bool keep = i < n && h > 0;
        const BlockRank r = block_rank<16>(keep, s_s);
        if (keep) {
            const int j = base + r.rank;
            rows.h[j] = h - 1;
            rows.uv[2 * (size_t)j] = u;
            rows.uv[2 * (size_t)j + 1] = v;
            rows.mu[j] = mu;
            rows.s2[j] = s2;
            rows.cnt[j] = cnt;
        }
        base += r.total;
    }
    if (tid == 0) counts[0] = base;
}

// Creation: the compacted cell winners (monokf.hip) become fresh seed rows
// from row dst on, as many as kMaxSeeds leaves beside the n_live seeds there
// are; counts[0] = winners, counts[1] = seeds appended
__global__ __launch_bounds__(256) void seed_rows_kernel(SeedRows rows, const int2* win_xy, const int* n_win, int cap_win,
                                                        int n_live, int dst, int host, double mu0, double s20,
                                                        int* counts) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int nw = min(*n_win, cap_win);
    const int m = min(nw, max(kMaxSeeds - n_live, 0));
    if (j == 0) {
        counts[0] = nw;
        counts[1] = m;
    }
    if (j >= m) return;
    const int2 c = win_xy[j];
    const size_t o = (size_t)dst + j;
    rows.h[o] = host;
    rows.uv[2 * o] = (double)c.x;
    rows.uv[2 * o + 1] = (double)c.y;
    rows.mu[o] = mu0;
    rows.s2[o] = s20;
    rows.cnt[o] = make_int4(0, 0, 0, 0);
}

}  // namespace

size_t seed_rows_bytes(int n) {
    SeedRows r{};
    return seed_rows_at(r, nullptr, n);
}

size_t seed_rows_at(SeedRows& r, void* base, int n) {
    const size_t m = (size_t)std::max(n, 1);
    Bump b;
    const size_t o_h = b.take(4 * m), o_uv = b.take(16 * m), o_mu = b.take(8 * m), o_s2 = b.take(8 * m),
                 o_c = b.take(16 * m);
    if (base) {
        char* p = (char*)base;
        r.h = (int32_t*)(p + o_h);
        r.uv = (double*)(p + o_uv);
        r.mu = (double*)(p + o_mu);
        r.s2 = (double*)(p + o_s2);
        r.cnt = (int4*)(p + o_c);
    }
    return b.off;
}

bool seed_params_ok(int max_steps, double depth_min, double depth_max, double max_score, double uniqueness) {
    return max_steps >= 8 && max_steps <= 64 && std::isfinite(depth_min) && std::isfinite(depth_max) &&
           depth_min > 0 && depth_min < depth_max && std::isfinite(max_score) && max_score > 0 &&
           std::isfinite(uniqueness) && uniqueness >= 1;
}

bool seed_promote_params_ok(int min_good, double conv_rel, int max_bad, int max_lost) {
    return min_good >= 1 && min_good <= 1000 && std::isfinite(conv_rel) && conv_rel > 0 && conv_rel <= 1 &&
           max_bad >= 1 && max_bad <= 1000 && max_lost >= 1 && max_lost <= 1000;
}

void launch_seed_update(const SeedUpdateArgs& a, hipStream_t stream) {
    if (a.n <= 0) return;
    seed_update_kernel<<<(a.n + 3) / 4, 256, 0, stream>>>(a);
}

void launch_seed_promote(const SeedPromoteArgs& a, hipStream_t stream) {
    seed_promote_kernel<<<1, 1024, 0, stream>>>(a);
}

void launch_seed_retire(const SeedRows& rows, int n, int* counts, hipStream_t stream) {
    seed_retire_kernel<<<1, 1024, 0, stream>>>(rows, n, counts);
}

void launch_seed_rows(const SeedRows& rows, const MonoKfArgs& m, int n_live, int dst, int host, double depth_min,
                      double depth_max, int* counts, hipStream_t stream) {
    const double rho_min = 1.0 / depth_max, rho_max = 1.0 / depth_min;
    const double s = (rho_max - rho_min) / 4.0;
    const int room = std::min(std::max(kMaxSeeds - n_live, 0), m.cap_win);
    seed_rows_kernel<<<std::max((room + 255) / 256, 1), 256, 0, stream>>>(rows, m.win_xy, m.counts + 1, m.cap_win, n_live,
                                                                       dst, host, (rho_min + rho_max) / 2.0, s * s,
                                                                       counts);
}

}  // namespace viso

using namespace viso;

// The candidate launches of one seed set on the context stream (scratch:
// mono_kf_scratch_at bytes): FAST on c's level 0, the map's occupancy, the
// cell winners in corner order (a.win_xy, a.counts[1]).
int viso_ctx::seed_candidates(MonoKfArgs& a, const uint8_t* level0, const PyrGeom& g, FastScratch& fs,
                              const double* pose_c, const double* points, int n_points) {
    intrinsics(a.K);
    for (int k = 0; k < 9; ++k) a.Kinv[k] = Kinv[k];
    a.pose_c = pose_c;
    a.pose_k = pose_c;  // (the compaction's KLT seed is not used)
    a.map_pts = points;
    a.n_map = n_points;
    {
        TimedRegion t(timing, VISO_KERNEL_FAST, stream);
        launch_fast(level0, g.w[0], g.h[0], p.fast_thresh, fs, nullptr, (int4*)a.corners, a.cap_corners,
                    (int*)a.n_corners, stream);
    }
    launch_mono_candidates(a, stream);
    VISO_HIP_CHECK(hipGetLastError());
    return VISO_OK;
}

// ------------------------------------------------------------------ frame path
// seed_buf: the rows of kMaxSeeds seeds, 64 count words, kMaxSeeds promoted hosts
SeedRows viso_ctx::seed_rows() const {
    SeedRows r{};
    seed_rows_at(r, seed_buf.ptr, kMaxSeeds);
    return r;
}
int* viso_ctx::seed_counts() const { return (int*)((char*)seed_buf.ptr + seed_rows_bytes(kMaxSeeds)); }

// The seed set of the keyframe just created from frame cur (the last of
// kf_slots), behind that step's own points (on_new_frame: map creation;
// stereo_init; append_keyframe).  fresh: a new map, the seeds of the old one
// go.  One host sync: the appended count (n_seeds is host state).
int viso_ctx::create_seeds(int cur, bool fresh) {
    if (!seeds_on()) return VISO_OK;
    if (fresh) n_seeds = 0;
    const PyrGeom& g = geom;
    int rc = mono_buf.ensure(mono_kf_scratch_bytes(g.w[0], g.h[0], seed_cell, p.max_features));
    if (rc) return rc;
    MonoKfArgs a{};
    mono_kf_scratch_at(a, mono_buf.ptr, g.w[0], g.h[0], seed_cell, p.max_features);
    rc = seed_candidates(a, frame(cur).l[0], g, fast, pose_of(cur), (const double*)map_pts.ptr, n_map);
    if (rc) return rc;
    {
        TimedRegion t(timing, VISO_KERNEL_SEEDS, stream);
        launch_seed_rows(seed_rows(), a, n_seeds, n_seeds, (int)kf_slots.size() - 1, seed_dmin, seed_dmax, seed_counts(),
                         stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(h_int + 20, seed_counts(), 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    const int m = std::max(0, std::min(h_int[21], kMaxSeeds - n_seeds));
    n_seeds += m;
    seeds_created += m;
    return VISO_OK;
}

// One tracking frame's update (on_new_frame, behind finish_call and the pose
// refinement: cur's pose is final).  No host synchronisation.
int viso_ctx::update_seeds(int cur) {
    if (!seeds_on() || n_seeds <= 0) return VISO_OK;
    SeedUpdateArgs a{};
    a.n_kf = (int)kf_slots.size();
    for (int j = 0; j < a.n_kf; ++j) a.kf[j] = frame(kf_slots[(size_t)j]);
    a.kf_poses = (const double*)kf_poses.ptr;
    a.cur = frame(cur);
    a.cur_pose = pose_of(cur);
    for (int l = 0; l < kLevels; ++l) {
        a.g.w[l] = geom.w[l];
        a.g.h[l] = geom.h[l];
    }
    intrinsics(a.K);
    a.p.max_steps = seed_max_steps;
    a.p.rho_min = 1.0 / seed_dmax;
    a.p.rho_max = 1.0 / seed_dmin;
    a.p.max_score = seed_max_score;
    a.p.uniqueness = seed_uniqueness;
    a.rows = seed_rows();
    a.n = n_seeds;
    a.diag = nullptr;
    {
        TimedRegion t(timing, VISO_KERNEL_SEEDS, stream);
        launch_seed_update(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    seed_updates += 1;
    return VISO_OK;
}

// One promotion (on_new_frame, behind the frame's update and the point
// refinement, ahead of the cull and the insertion check).  The promoted points
// go straight behind the map.  One host sync for the counts; a promotion that
// appended points reads their hosts back too and rebuilds the LK templates:
// a map rewrite's entry (begin_map_rewrite, mapwin.hip; the hosts are not
// read on the device, so none are uploaded).
int viso_ctx::promote_seeds() {
    if (!seeds_on() || n_seeds <= 0) return VISO_OK;
    if ((int)point_host.size() != n_map) return VISO_ERR_STATE;
    const int room = std::min(kMaxMapPoints - n_map, n_seeds);
    if (int rc = begin_map_rewrite(false)) return rc;
    SeedPromoteArgs a{};
    a.rows = seed_rows();
    a.n = n_seeds;
    a.kf_poses = (const double*)kf_poses.ptr;
    intrinsics(a.K);
    a.min_good = seed_min_good;
    a.conv_rel = seed_conv_rel;
    a.max_bad = seed_max_bad;
    a.max_lost = seed_max_lost;
    a.room = room;
    a.out_pts = (double*)map_pts.ptr + 3 * (size_t)n_map;
    a.out_host = seed_counts() + 64;
    a.counts = seed_counts();
    {
        TimedRegion t(timing, VISO_KERNEL_SEEDS, stream);
        launch_seed_promote(a, stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(h_int + 20, a.counts, 4 * sizeof(int), hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    const int m = std::max(0, std::min(h_int[21], room));
    const int dropped = std::max(0, h_int[22]);
    n_seeds = std::max(0, std::min(h_int[23], n_seeds));
    seeds_promoted += m;
    seeds_dropped += dropped;
    seed_last[0] = frames;
    seed_last[1] = m;
    seed_last[2] = dropped;
    if (m == 0) return VISO_OK;
    std::vector<int32_t> hosts((size_t)m);
    VISO_HIP_CHECK(hipMemcpyAsync(hosts.data(), a.out_host, 4 * (size_t)m, hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    point_host.insert(point_host.end(), hosts.begin(), hosts.end());
    n_map += m;
    if (int rc = tracks_zero(n_map - m, m)) return rc;
    return build_lk_templates();
}

// A retirement's seeds (retire_keyframe, once keyframe 0 has left): its seeds
// go, the others' h moves down.  One host sync for the count.
int viso_ctx::retire_seeds() {
    if (!seeds_on() || n_seeds <= 0) return VISO_OK;
    {
        TimedRegion t(timing, VISO_KERNEL_SEEDS, stream);
        launch_seed_retire(seed_rows(), n_seeds, seed_counts(), stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(h_int + 20, seed_counts(), sizeof(int), hipMemcpyDeviceToHost, stream));
    VISO_HIP_CHECK(hipStreamSynchronize(stream));
    const int kept = std::max(0, std::min(h_int[20], n_seeds));
    seeds_retired += n_seeds - kept;
    n_seeds = kept;
    return VISO_OK;
}

extern "C" {

// The setter settles pending work first (frames queued with the mode as it
// was are finished with it), then allocates or frees the seed rows.
int viso_set_depth_seeds(viso_ctx* c, int32_t interval, int32_t cell, int32_t max_steps, double depth_min,
                         double depth_max, double max_score, double uniqueness, int32_t min_good, double conv_rel,
                         int32_t max_bad, int32_t max_lost) {
    if (!c || interval < 0) return VISO_ERR_ARG;
    if (interval > 0 && (cell < 8 || cell > 64 || !seed_params_ok(max_steps, depth_min, depth_max, max_score, uniqueness) ||
                         !seed_promote_params_ok(min_good, conv_rel, max_bad, max_lost)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    if (interval > 0) {
        if (!c->seeds_on()) {
            int rc = c->seed_buf.ensure(seed_rows_bytes(kMaxSeeds) + 4 * (64 + (size_t)kMaxSeeds));
            if (!rc) rc = c->point_host_dev.ensure(4 * (size_t)kMaxMapPoints);
            if (rc) return rc;
            c->n_seeds = 0;
            c->seeds_created = c->seeds_promoted = c->seeds_dropped = c->seeds_retired = c->seed_updates = 0;
            c->seed_last[0] = -1;
            c->seed_last[1] = c->seed_last[2] = 0;
        }
        c->seed_cell = cell;
        c->seed_max_steps = max_steps;
        c->seed_dmin = depth_min;
        c->seed_dmax = depth_max;
        c->seed_max_score = max_score;
        c->seed_uniqueness = uniqueness;
        c->seed_min_good = min_good;
        c->seed_conv_rel = conv_rel;
        c->seed_max_bad = max_bad;
        c->seed_max_lost = max_lost;
    } else if (c->seeds_on()) {
        VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
        c->seed_buf.release();
        c->n_seeds = 0;
    }
    c->seed_interval = interval;
    return VISO_OK;
}

int viso_get_depth_seed_rows(viso_ctx* c, int32_t* h, double* uv, double* mu, double* s2, int32_t* counters, size_t cap,
                             size_t* n) {
    if (!c) return VISO_ERR_ARG;
    if (!c->seeds_on()) return VISO_ERR_STATE;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t m = std::min(cap, (size_t)c->n_seeds);
    const SeedRows r = c->seed_rows();
    if (m > 0) {
        if (h) VISO_HIP_CHECK(hipMemcpyAsync(h, r.h, 4 * m, hipMemcpyDeviceToHost, c->stream));
        if (uv) VISO_HIP_CHECK(hipMemcpyAsync(uv, r.uv, 16 * m, hipMemcpyDeviceToHost, c->stream));
        if (mu) VISO_HIP_CHECK(hipMemcpyAsync(mu, r.mu, 8 * m, hipMemcpyDeviceToHost, c->stream));
        if (s2) VISO_HIP_CHECK(hipMemcpyAsync(s2, r.s2, 8 * m, hipMemcpyDeviceToHost, c->stream));
        if (counters) VISO_HIP_CHECK(hipMemcpyAsync(counters, r.cnt, 16 * m, hipMemcpyDeviceToHost, c->stream));
    }
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (n) *n = (size_t)c->n_seeds;
    return VISO_OK;
}

int viso_get_depth_seeds(viso_ctx* c, int64_t info[8]) {
    if (!c || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    for (int k = 0; k < 8; ++k) info[k] = 0;
    if (!c->seeds_on()) return VISO_OK;
    info[0] = c->seed_interval;
    info[1] = c->n_seeds;
    info[2] = c->seeds_created;
    info[3] = c->seeds_promoted;
    info[4] = c->seeds_dropped + c->seeds_retired;
    const size_t m = (size_t)c->n_seeds;
    if (m == 0 || c->seed_updates == 0) return VISO_OK;
    // the live rows' last statuses, counted on the host (integer counts of a
    // getter, as viso_get_lk_warp's); a seed no update has seen yet (status 0
    // and good 0) is not counted
    VISO_HIP_CHECK(hipSetDevice(c->device));
    std::vector<int32_t> cnt(4 * m);
    VISO_HIP_CHECK(hipMemcpyAsync(cnt.data(), c->seed_rows().cnt, 16 * m, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < m; ++i) {
        const int st = cnt[4 * i + 3];
        if (st == 0)
            info[5] += cnt[4 * i] > 0;
        else if (st >= 7)
            info[6] += 1;
        else
            info[7] += 1;
    }
    return VISO_OK;
}

int viso_depth_seeds_create(viso_ctx* c, const uint8_t* image, int32_t width, int32_t height, const double pose[12],
                            const double* points, int32_t n_points, int32_t cell, int32_t host, double depth_min,
                            double depth_max, int32_t n_live, int32_t* h, double* uv, double* mu, double* s2,
                            int32_t* counters, size_t cap, size_t* n, int32_t counts[2]) {
    if (!c || !image || !pose || width < 16 || height < 16 || width > kMaxWidth || n_points < 0 ||
        n_points > kMaxMapPoints || cell < 8 || cell > 64 || host < 0 || host >= kMaxKeyframes ||
        !(std::isfinite(depth_min) && std::isfinite(depth_max) && depth_min > 0 && depth_min < depth_max) ||
        n_live < 0 || n_live > kMaxSeeds || (n_points > 0 && !points) ||
        (cap > 0 && (!h || !uv || !mu || !s2 || !counters)))
        return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const PyrGeom g = make_geom(width, height);
    const size_t npx = (size_t)width * height;
    const int cells = mono_kf_cells(width, height, cell);
    const int room = std::min(kMaxSeeds - n_live, cells);
    Bump b;
    const size_t o_i = b.take(npx), o_pc = b.take(96), o_p = b.take(24 * (size_t)std::max(n_points, 1)),
                 o_cnt = b.take(16), o_rows = b.take(seed_rows_bytes(room));
    int rc = c->scratch_a.ensure(b.off);
    if (!rc) rc = c->scratch_b.ensure(fast_scratch_bytes(width, height));
    if (!rc) rc = c->scratch_c.ensure(mono_kf_scratch_bytes(width, height, cell, c->p.max_features));
    if (rc) return rc;
    char* base = (char*)c->scratch_a.ptr;
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_i, image, npx, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_pc, pose, 96, hipMemcpyHostToDevice, c->stream));
    if (n_points > 0)
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_p, points, 24 * (size_t)n_points, hipMemcpyHostToDevice, c->stream));
    FastScratch fs = fast_scratch_at(c->scratch_b.ptr, width, height);
    MonoKfArgs a{};
    mono_kf_scratch_at(a, c->scratch_c.ptr, width, height, cell, c->p.max_features);
    rc = c->seed_candidates(a, (const uint8_t*)(base + o_i), g, fs, (const double*)(base + o_pc),
                            (const double*)(base + o_p), n_points);
    if (rc) return rc;
    SeedRows rows{};
    seed_rows_at(rows, base + o_rows, room);
    {
        TimedRegion t(c->timing, VISO_KERNEL_SEEDS, c->stream);
        // (the rows of this call alone, from row 0, capped as beside n_live live seeds)
        launch_seed_rows(rows, a, n_live, 0, host, depth_min, depth_max, (int*)(base + o_cnt), c->stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    int32_t cnt[2] = {0, 0};
    VISO_HIP_CHECK(hipMemcpyAsync(cnt, base + o_cnt, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    const size_t m = std::min<size_t>((size_t)std::max(std::min(cnt[1], room), 0), cap);
    if (m > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(h, rows.h, 4 * m, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(uv, rows.uv, 16 * m, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(mu, rows.mu, 8 * m, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(s2, rows.s2, 8 * m, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(counters, rows.cnt, 16 * m, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    if (n) *n = (size_t)std::max(cnt[1], 0);
    if (counts) {
        counts[0] = cnt[0];
        counts[1] = cnt[1];
    }
    return VISO_OK;
}

int viso_depth_seeds_update(viso_ctx* c, const uint8_t* kf_pyrs, const double* kf_poses, int32_t n_kf,
                            const uint8_t* cur_pyr, const double cur_pose[12], int32_t width, int32_t height,
                            int32_t n, int32_t max_steps, double depth_min, double depth_max, double max_score,
                            double uniqueness, const int32_t* h, const double* uv, double* mu, double* s2,
                            int32_t* counters, int32_t* level_step) {
    if (!c || !kf_pyrs || !kf_poses || n_kf <= 0 || n_kf > kMaxKeyframes || !cur_pyr || !cur_pose || width < 16 ||
        height < 16 || width > kMaxWidth || n < 0 || n > kMaxSeeds ||
        !seed_params_ok(max_steps, depth_min, depth_max, max_score, uniqueness))
        return VISO_ERR_ARG;
    if (n > 0 && (!h || !uv || !mu || !s2 || !counters)) return VISO_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (h[i] < 0 || h[i] >= n_kf) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    if (n == 0) return VISO_OK;
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const PyrGeom g = make_geom(width, height);
    Bump b;
    const size_t o_kf = b.take(g.bytes * (size_t)n_kf), o_kp = b.take(96 * (size_t)n_kf), o_c = b.take(g.bytes),
                 o_cp = b.take(96), o_rows = b.take(seed_rows_bytes(n)), o_d = b.take(8 * (size_t)n);
    int rc = c->scratch_a.ensure(b.off);
    if (rc) return rc;
    char* base = (char*)c->scratch_a.ptr;
    SeedUpdateArgs a{};
    seed_rows_at(a.rows, base + o_rows, n);
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_kf, kf_pyrs, g.bytes * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_kp, kf_poses, 96 * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_c, cur_pyr, g.bytes, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_cp, cur_pose, 96, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(a.rows.h, h, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(a.rows.uv, uv, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(a.rows.mu, mu, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(a.rows.s2, s2, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(a.rows.cnt, counters, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    for (int j = 0; j < n_kf; ++j) a.kf[j] = frame_from_base((const uint8_t*)(base + o_kf + g.bytes * j), g);
    a.kf_poses = (const double*)(base + o_kp);
    a.n_kf = n_kf;
    a.cur = frame_from_base((const uint8_t*)(base + o_c), g);
    a.cur_pose = (const double*)(base + o_cp);
    for (int l = 0; l < kLevels; ++l) {
        a.g.w[l] = g.w[l];
        a.g.h[l] = g.h[l];
    }
    c->intrinsics(a.K);
    a.p.max_steps = max_steps;
    a.p.rho_min = 1.0 / depth_max;
    a.p.rho_max = 1.0 / depth_min;
    a.p.max_score = max_score;
    a.p.uniqueness = uniqueness;
    a.n = n;
    a.diag = (int2*)(base + o_d);
    {
        TimedRegion t(c->timing, VISO_KERNEL_SEEDS, c->stream);
        launch_seed_update(a, c->stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(mu, a.rows.mu, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(s2, a.rows.s2, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(counters, a.rows.cnt, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (level_step)
        VISO_HIP_CHECK(hipMemcpyAsync(level_step, a.diag, 8 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

int viso_depth_seeds_promote(viso_ctx* c, const double* kf_poses, int32_t n_kf, int32_t n, int32_t min_good,
                             double conv_rel, int32_t max_bad, int32_t max_lost, int32_t room, int32_t* h, double* uv,
                             double* mu, double* s2, int32_t* counters, double* points, int32_t* hosts,
                             int32_t counts[4]) {
    if (!c || !kf_poses || n_kf <= 0 || n_kf > kMaxKeyframes || n < 0 || n > kMaxSeeds || room < 0 ||
        room > kMaxMapPoints || !seed_promote_params_ok(min_good, conv_rel, max_bad, max_lost) || !counts)
        return VISO_ERR_ARG;
    if (n > 0 && (!h || !uv || !mu || !s2 || !counters)) return VISO_ERR_ARG;
    const int out_cap = std::min(room, n);
    if (out_cap > 0 && (!points || !hosts)) return VISO_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (h[i] < 0 || h[i] >= n_kf) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    Bump b;
    const size_t o_kp = b.take(96 * (size_t)n_kf), o_rows = b.take(seed_rows_bytes(n)),
                 o_p = b.take(24 * (size_t)std::max(out_cap, 1)), o_h = b.take(4 * (size_t)std::max(out_cap, 1)),
                 o_cnt = b.take(16);
    int rc = c->scratch_a.ensure(b.off);
    if (rc) return rc;
    char* base = (char*)c->scratch_a.ptr;
    SeedPromoteArgs a{};
    seed_rows_at(a.rows, base + o_rows, n);
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_kp, kf_poses, 96 * (size_t)n_kf, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(a.rows.h, h, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(a.rows.uv, uv, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(a.rows.mu, mu, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(a.rows.s2, s2, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(a.rows.cnt, counters, 16 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    a.n = n;
    a.kf_poses = (const double*)(base + o_kp);
    c->intrinsics(a.K);
    a.min_good = min_good;
    a.conv_rel = conv_rel;
    a.max_bad = max_bad;
    a.max_lost = max_lost;
    a.room = out_cap;
    a.out_pts = (double*)(base + o_p);
    a.out_host = (int32_t*)(base + o_h);
    a.counts = (int*)(base + o_cnt);
    {
        TimedRegion t(c->timing, VISO_KERNEL_SEEDS, c->stream);
        launch_seed_promote(a, c->stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    int32_t cnt[4] = {0, 0, 0, 0};
    VISO_HIP_CHECK(hipMemcpyAsync(cnt, a.counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    const size_t np = (size_t)std::max(0, std::min(cnt[1], out_cap)), ns = (size_t)std::max(0, std::min(cnt[3], n));
    if (np > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(points, a.out_pts, 24 * np, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(hosts, a.out_host, 4 * np, hipMemcpyDeviceToHost, c->stream));
    }
    if (ns > 0) {
        VISO_HIP_CHECK(hipMemcpyAsync(h, a.rows.h, 4 * ns, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(uv, a.rows.uv, 16 * ns, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(mu, a.rows.mu, 8 * ns, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(s2, a.rows.s2, 8 * ns, hipMemcpyDeviceToHost, c->stream));
        VISO_HIP_CHECK(hipMemcpyAsync(counters, a.rows.cnt, 16 * ns, hipMemcpyDeviceToHost, c->stream));
    }
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; ++k) counts[k] = cnt[k];
    return VISO_OK;
}

}  // extern "C"
