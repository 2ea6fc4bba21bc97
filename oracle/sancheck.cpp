// TEST INFRASTRUCTURE ONLY (see viso_oracle.h) — a driver for the
// AddressSanitizer / UndefinedBehaviorSanitizer build of the oracle
// (`make -C oracle sanitize`, run by tests/test_oracle_sanitize.py).
//
// The reference has two undefined behaviours on its hot path that the
// oracle restates as defined ones: the uninitialised
// `init_.frame_cnt` (include/viso.h:38; the oracle starts it at 0) and the
// unguarded `data[step + 1]` bilinear taps past the cv::Mat
// (include/common.h:35-41; the oracle reads 0 outside the level buffer).
// This driver runs every oracle path over a procedural scene whose camera
// drifts to the image border (so patches and taps leave the buffer) with the
// sanitizers armed: the monocular initialisation (FAST, KLT, 2D-2D RANSAC,
// SelectMotion), stereo initialisation and tracking (direct pose, LK
// alignment, keyframe insertion) in both summation orders, and the
// multi-camera rig; and the stereo VO spec's motion stage on its smallest
// inputs (0..12 matches, every exit).
// Exit status 0 and no sanitizer report = clean.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/viso/viso_svo.h"
#include "viso_oracle.h"

namespace {

constexpr int W = 320, H = 160;

// block-noise texture (8 px blocks) sampled bilinearly at a sub-pixel shift
struct Texture {
    int tw = 1024, th = 512;
    std::vector<uint8_t> t;
    Texture() : t((size_t)tw * th) {
        uint64_t s = 0x9E3779B97F4A7C15ULL;
        std::vector<uint8_t> blocks((size_t)(tw / 8) * (th / 8));
        for (auto& b : blocks) {
            s ^= s << 13;
            s ^= s >> 7;
            s ^= s << 17;
            b = (uint8_t)(s >> 56);
        }
        for (int y = 0; y < th; ++y)
            for (int x = 0; x < tw; ++x) t[(size_t)y * tw + x] = blocks[(size_t)(y / 8) * (tw / 8) + x / 8];
    }
    uint8_t at(double x, double y) const {
        const int ix = (int)std::floor(x), iy = (int)std::floor(y);
        const double fx = x - ix, fy = y - iy;
        auto p = [&](int a, int b) {
            a = std::min(std::max(a, 0), tw - 1);
            b = std::min(std::max(b, 0), th - 1);
            return (double)t[(size_t)b * tw + a];
        };
        const double v = (1 - fx) * (1 - fy) * p(ix, iy) + fx * (1 - fy) * p(ix + 1, iy) +
                         (1 - fx) * fy * p(ix, iy + 1) + fx * fy * p(ix + 1, iy + 1);
        return (uint8_t)std::lround(v);
    }
};

void render(const Texture& tex, double ox, double oy, double zoom, std::vector<uint8_t>& img) {
    img.resize((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) img[(size_t)y * W + x] = tex.at(ox + x * zoom, oy + y * zoom);
}

int run_viso(const Texture& tex, bool stereo, int literal) {
    oracle_set_sum_order(literal);
    oracle_params p;
    oracle_default_params(&p, 300.0, 300.0, W / 2.0, H / 2.0, W, H);
    p.enable_tracking = 1;
    oracle_viso* v = oracle_viso_create(&p);
    if (!v) return 1;
    if (stereo) {
        oracle_viso_set_stereo(v, 0.5, 64, 1);
        oracle_viso_set_keyframes(v, 2, 900);
    }
    std::vector<uint8_t> L, R;
    for (int f = 0; f < 10; ++f) {
        // the view drifts right and zooms in (forward motion), leaving the map
        const double ox = 40 + 9.0 * f, oy = 30 + 1.5 * f, zoom = 0.77 - 0.01 * f;
        render(tex, ox, oy, zoom, L);
        if (stereo) {
            render(tex, ox + 12.0, oy, zoom, R);
            oracle_viso_on_new_stereo(v, L.data(), R.data());
        } else {
            oracle_viso_on_new_frame(v, L.data());
        }
    }
    std::printf("%s%s: state %d, poses %d, points %d\n", stereo ? "stereo" : "mono", literal ? " (literal)" : "",
                oracle_viso_state(v), oracle_viso_num_poses(v), oracle_viso_num_points(v));
    oracle_viso_destroy(v);
    oracle_set_sum_order(0);
    return 0;
}

int run_rig(const Texture& tex) {
    const double E[24] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0,
                          0.9848077530, 0, -0.1736481777, 0, 1, 0, 0.1736481777, 0, 0.9848077530, -0.2, 0, 0};
    const double K[4] = {300.0, 300.0, W / 2.0, H / 2.0};
    oracle_rig* r = oracle_rig_create(2, W, H, K, 50, E, 0.5, 64, 1);
    if (!r) return 1;
    std::vector<uint8_t> L0, L1, R0, R1;
    for (int f = 0; f < 4; ++f) {
        render(tex, 40 + 3.0 * f, 30, 0.77, L0);
        render(tex, 400 + 3.0 * f, 60, 0.77, L1);
        render(tex, 52 + 3.0 * f, 30, 0.77, R0);
        render(tex, 412 + 3.0 * f, 60, 0.77, R1);
        const uint8_t* ls[2] = {L0.data(), L1.data()};
        const uint8_t* rs[2] = {R0.data(), R1.data()};
        oracle_rig_process(r, ls, f == 0 ? rs : nullptr);
    }
    std::printf("rig: state %d, poses %d, points %d + %d\n", oracle_rig_state(r), oracle_rig_num_poses(r),
                oracle_rig_num_points(r, 0), oracle_rig_num_points(r, 1));
    oracle_rig_destroy(r);
    return 0;
}

// Two of the late-failure inputs of tests/svo_cases.py (best hypothesis with 6
// inliers, 5 after the refinement): {n, noise, seed} = {8, 1.0, 5}, sampler
// frame 0, and {12, 1.5, 42}, frame 2.
const int32_t kLate8[8 * 8] = {
    990, 193, 978, 193, 983, 194, 971, 194, 74, 36, 54, 36, 96, 41, 74, 41, 1189, 321, 1170, 321, 1170, 316,
    1152, 316, 93, 206, 79, 206, 107, 205, 93, 205, 1064, 96, 1051, 96, 1054, 97, 1042, 97, 21, 189, 8, 189,
    35, 188, 23, 188, 400, 70, 388, 70, 404, 74, 394, 74, 404, 288, 375, 288, 417, 283, 387, 283};
const int32_t kLate12[12 * 8] = {
    547, 308, 535, 308, 551, 302, 536, 302, 963, 63, 951, 63, 955, 67, 946, 67, 1007, 169, 993, 169, 997, 170,
    983, 170, 778, 274, 767, 274, 775, 274, 765, 274, 254, 176, 242, 176, 263, 177, 251, 177, 1181, 129, 1169,
    129, 1169, 131, 1160, 131, 591, 96, 550, 96, 597, 103, 558, 103, 986, 150, 975, 150, 980, 152, 969, 152,
    29, 284, -3, 284, 64, 276, 33, 276, 702, 67, 684, 67, 703, 69, 685, 69, 938, 233, 922, 233, 931, 233,
    916, 233, 544, 92, 480, 92, 556, 100, 497, 100};

// one estimate on exactly-sized heap buffers (an overrun is a report); a
// failed estimate must leave the identity and a cleared mask
int svo_estimate_once(const int32_t* uv8, int n, int64_t frame, const viso_svo_params& p, int want_exit) {
    std::vector<int32_t> m(uv8, uv8 + (size_t)8 * n);
    std::vector<uint8_t> inl((size_t)n, 0xAA);
    std::vector<double> motion(12, -1.0);
    const int rc = oracle_svo_estimate(m.data(), n, frame, &p, motion.data(), inl.data());
    int32_t tr[5];
    oracle_svo_estimate_trace(tr);
    int cnt = 0;
    for (uint8_t f : inl) cnt += f;
    bool ok = rc == -1 ? cnt == 0 : (rc >= 6 && cnt == rc);
    if (rc == -1)
        for (int i = 0; i < 12; ++i) ok = ok && motion[(size_t)i] == ((i % 4 == 0 && i < 9) ? 1.0 : 0.0);
    ok = ok && (want_exit < 0 || tr[0] == want_exit) && (rc >= 6) == (tr[0] == ORACLE_SVO_EXIT_OK ||
                                                                      tr[0] == ORACLE_SVO_EXIT_REFINE_FAILED);
    std::printf("svo estimate: n %d frame %d -> %d, exit %d, best %d (%d), final %d%s\n", n, (int)frame, rc, tr[0],
                tr[1], tr[2], tr[4], ok ? "" : "  MISMATCH");
    return ok ? 0 : 1;
}

int run_svo() {
    viso_svo_params p;
    oracle_svo_default_params(&p, 1242, 375, 718.856, 718.856, 607.19, 185.22, 0.54);
    int rc = 0;
    rc |= svo_estimate_once(kLate8, 8, 0, p, ORACLE_SVO_EXIT_FINAL_FEW);
    rc |= svo_estimate_once(kLate12, 12, 2, p, ORACLE_SVO_EXIT_FINAL_FEW);
    for (int n = 0; n <= 5; n += 5) rc |= svo_estimate_once(kLate12, n, 1, p, ORACLE_SVO_EXIT_FEW_MATCHES);
    for (int n = 6; n <= 12; ++n) rc |= svo_estimate_once(kLate12, n, n, p, -1);
    // two distinct matches six times over: every hypothesis is rank-deficient
    std::vector<int32_t> two;
    for (int r = 0; r < 6; ++r) two.insert(two.end(), kLate8, kLate8 + 16);
    rc |= svo_estimate_once(two.data(), 12, 3, p, ORACLE_SVO_EXIT_NO_HYPOTHESIS);
    // three distinct matches three times over ("rep3", {9, 1.0, 2}, frame 2):
    // the best hypothesis keeps two of them, whose refinement is singular
    const int32_t three[3 * 8] = {378, 293, 351, 293, 389, 290, 366, 290, 86,  112, 52,  112,
                                  119, 117, 87,  117, 823, 162, 804, 162, 817, 163, 799, 163};
    std::vector<int32_t> rep;
    for (int r = 0; r < 3; ++r) rep.insert(rep.end(), three, three + 24);
    rc |= svo_estimate_once(rep.data(), 9, 2, p, ORACLE_SVO_EXIT_REFINE_FAILED);
    return rc;
}

}  // namespace

int main() {
    Texture tex;
    int rc = 0;
    rc |= run_viso(tex, false, 0);
    rc |= run_viso(tex, true, 0);
    rc |= run_viso(tex, true, 1);
    rc |= run_rig(tex);
    rc |= run_svo();
    std::printf(rc ? "FAILED\n" : "sancheck ok\n");
    return rc;
}
