// viso_amd — header-only C++ facade over the C ABI (viso_c.h) that keeps the
// reference's class names and call shapes, so code written against
// Seasandwpy/viso compiles with minimal changes:
//   Keyframe(mat)                     include/keyframe.h:28-46 (raw grey buffer
//                                     instead of cv::Mat)
//   FrameSequence::FrameHandler       include/frame_sequence.h:13-16
//   FrameSequence::RunOnce()          include/frame_sequence.h:25-38 (loader
//                                     callback instead of cv::imread)
//   Viso(fx, fy, cx, cy)              include/viso.h:47-52
//   Viso::OnNewFrame(Keyframe::Ptr)   src/viso.cpp:7-145
//   Viso::poses                       include/viso.h:54 (Tcw, R row-major + t)
//   Viso::GetPoints()                 include/viso.h:60-67
//   StereoViso::process(left, right, dims)   the reference path with the
//                                     stereo initialisation (viso_set_stereo)
// The north-star VisualOdometryStereo / Matcher (the SVO engine) are in
// viso_svo.hpp, the multi-camera photometric rig (VisoRig) in viso_rig.hpp.
// No Eigen / Sophus / OpenCV types: poses are std::array<double, 12>.
#ifndef VISO_HPP
#define VISO_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <mutex>
#include <vector>

#include "viso_c.h"

namespace viso {

inline void check(int rc, const char* what) {
    if (rc != VISO_OK) throw std::runtime_error(std::string(what) + " failed: " + std::to_string(rc));
}

using Pose = std::array<double, 12>;  // R (row-major 3x3) + t: Pc = R * Pw + t
using V3d = std::array<double, 3>;
using V2d = std::array<double, 2>;
using M3d = std::array<double, 9>;  // row-major

// cv::KeyPoint's fields (Keyframe::Keypoints / AddKeypoint)
struct KeyPoint {
    float x = 0.f, y = 0.f;  // pt
    float size = 0.f, angle = -1.f, response = 0.f;
    int octave = 0, class_id = -1;
};

// One pyramid level as the reference reads a cv::Mat: data, cols, rows, step
// (continuous: step == cols for levels 1..3, the caller's stride for level 0).
struct GreyView {
    const uint8_t* data = nullptr;
    int cols = 0, rows = 0;
    size_t step = 0;
};

namespace detail {
// A library context per image size that builds Keyframe pyramids with the
// same pyrDown kernels as the frame path (viso_pyramid).  Keyframe has no
// device argument (the reference's Keyframe(cv::Mat) has none), so these
// contexts live on device 0; they are created once per size, shared by every
// thread (the cache is guarded by a mutex) and released only at process exit.
inline viso_ctx* pyramid_ctx(int w, int h) {
    struct Entry {
        int w, h;
        viso_ctx* ctx;
    };
    static std::mutex mu;
    static std::vector<Entry> cache;
    std::lock_guard<std::mutex> lock(mu);
    for (const Entry& e : cache)
        if (e.w == w && e.h == h) return e.ctx;
    viso_params p;
    check(viso_default_params(&p, 1.0, 1.0, 0.0, 0.0, w, h), "viso_default_params");
    viso_ctx* c = nullptr;
    check(viso_create(&p, 0, &c), "viso_create");
    cache.push_back(Entry{w, h, c});
    return c;
}
}  // namespace detail

// include/keyframe.h:10-123.  The frame is a raw grey buffer instead of a
// cv::Mat; the accessors keep the reference's names, arguments and
// arithmetic (GetPixelValue's int() base with floor weights, :50-57;
// GetGradient's central differences, :59-64; Project, :82-89; IsInside,
// :71-80; ViewingAngle, :93-98), so a FrameHandler written against the
// reference compiles.  The pyramid (:37-45) is built on first use by the
// library's pyrDown kernels; taps outside a level's buffer read 0 (the
// reference reads past the cv::Mat there).  These are per-call host helpers
// for handler code: the tracking path never calls them.
class Keyframe {
public:
    using Ptr = std::shared_ptr<Keyframe>;
    Keyframe(const uint8_t* grey, int width, int height, int stride)
        : id_(next_id_++), w_(width), h_(height), data_(grey, grey + (size_t)stride * height),
          stride_(stride) {}
    long GetId() const { return id_; }
    static long GetNextId() { return next_id_; }
    const uint8_t* Data() const { return data_.data(); }
    int Width() const { return w_; }
    int Height() const { return h_; }
    int Stride() const { return stride_; }

    // include/keyframe.h:102
    GreyView Mat() const { return GreyView{data_.data(), w_, h_, (size_t)stride_}; }
    // include/keyframe.h:112: levels 0..3 (level 0 is the frame itself)
    const std::vector<GreyView>& Pyramids() const {
        if (pyr_views_.empty()) build_pyramid();
        return pyr_views_;
    }
    // include/keyframe.h:110
    double GetScale(int level) const { return kScales[level]; }

    // include/keyframe.h:50-57
    double GetPixelValue(const double& x, const double& y, int level = 0) const {
        const GreyView& m = Pyramids()[level];
        const long long n = (long long)m.step * m.rows;
        const long long base = (long long)(int)y * (long long)m.step + (long long)(int)x;
        auto tap = [&](long long i) -> double { return (i >= 0 && i < n) ? (double)m.data[i] : 0.0; };
        const double xx = x - std::floor(x);
        const double yy = y - std::floor(y);
        return double((1 - xx) * (1 - yy) * tap(base) + xx * (1 - yy) * tap(base + 1) +
                      (1 - xx) * yy * tap(base + (long long)m.step) + xx * yy * tap(base + (long long)m.step + 1));
    }
    // include/keyframe.h:59-64
    V2d GetGradient(const double& u, const double& v, int level = 0) const {
        const double dx = 0.5 * (GetPixelValue(u + 1, v, level) - GetPixelValue(u - 1, v, level));
        const double dy = 0.5 * (GetPixelValue(u, v + 1, level) - GetPixelValue(u, v - 1, level));
        return V2d{dx, dy};
    }
    // include/keyframe.h:82-89 (Pc = R Pw + T, then K at the level's scale)
    V2d Project(const V3d& point, int level) const {
        double uv1[3];
        for (int i = 0; i < 3; ++i)
            uv1[i] = (R_[3 * i] * point[0] + R_[3 * i + 1] * point[1]) + R_[3 * i + 2] * point[2] + T_[i];
        const double z = uv1[2];
        for (int i = 0; i < 3; ++i) uv1[i] /= z;
        const double u = kScales[level] * (uv1[0] * K_[0] + K_[2]);
        const double v = kScales[level] * (uv1[1] * K_[4] + K_[5]);
        return V2d{u, v};
    }
    // include/keyframe.h:71-80 (level sizes: Pyramids()[level])
    bool IsInside(const double& u, const double& v, int level = 0) const {
        const GreyView& m = Pyramids()[level];
        return u >= 0 && u < m.cols && v >= 0 && v < m.rows;
    }
    bool IsInside(const V3d& point, int level = 0) const {
        const V2d uv = Project(point, level);
        return IsInside(uv[0], uv[1], level);
    }
    // include/keyframe.h:93-98: angle between the ray to Pw and the camera's z axis
    double ViewingAngle(const V3d& Pw) const {
        double Pc[3];
        for (int i = 0; i < 3; ++i)
            Pc[i] = (R_[3 * i] * Pw[0] + R_[3 * i + 1] * Pw[1]) + R_[3 * i + 2] * Pw[2] + T_[i];
        const double norm = std::sqrt(Pc[0] * Pc[0] + Pc[1] * Pc[1] + Pc[2] * Pc[2]);
        return std::acos(Pc[2] / norm);
    }
    // include/keyframe.h:100-108 (R row-major, K row-major 3x3)
    std::vector<KeyPoint>& Keypoints() { return keypoints_; }
    int AddKeypoint(const KeyPoint& kp) {
        keypoints_.push_back(kp);
        return (int)keypoints_.size();
    }
    M3d GetR() const { return R_; }
    V3d GetT() const { return T_; }
    void SetR(const M3d& R) { R_ = R; }
    void SetT(const V3d& T) { T_ = T; }
    M3d GetK() const { return K_; }
    void SetK(const M3d& K) { K_ = K; }

private:
    static constexpr double kScales[4] = {1.0, 0.5, 0.25, 0.125};  // include/keyframe.h:22
    void build_pyramid() const {
        // level 0 continuous for viso_pyramid, then levels 1..3 from the device
        std::vector<uint8_t> l0((size_t)w_ * h_);
        for (int y = 0; y < h_; ++y)
            std::copy(data_.begin() + (size_t)y * stride_, data_.begin() + (size_t)y * stride_ + w_,
                      l0.begin() + (size_t)y * w_);
        int32_t dims[8];
        size_t total = 0;
        check(viso_pyramid_dims(w_, h_, dims, &total), "viso_pyramid_dims");
        pyr_.resize(total);
        check(viso_pyramid(detail::pyramid_ctx(w_, h_), l0.data(), 1, w_, h_, pyr_.data()), "viso_pyramid");
        pyr_views_.clear();
        pyr_views_.push_back(Mat());
        size_t off = (size_t)dims[0] * dims[1];
        for (int l = 1; l < 4; ++l) {
            pyr_views_.push_back(GreyView{pyr_.data() + off, dims[2 * l], dims[2 * l + 1], (size_t)dims[2 * l]});
            off += (size_t)dims[2 * l] * dims[2 * l + 1];
        }
    }
    static inline long next_id_ = 0;
    long id_;
    int w_, h_;
    std::vector<uint8_t> data_;
    int stride_;
    M3d R_{1, 0, 0, 0, 1, 0, 0, 0, 1};  // include/keyframe.h:34-35
    V3d T_{0, 0, 0};
    M3d K_{0, 0, 0, 0, 0, 0, 0, 0, 1};
    std::vector<KeyPoint> keypoints_;
    mutable std::vector<uint8_t> pyr_;
    mutable std::vector<GreyView> pyr_views_;
};

class FrameSequence {
public:
    class FrameHandler {
    public:
        virtual ~FrameHandler() = default;
        virtual void OnNewFrame(Keyframe::Ptr keyframe) = 0;
    };
    // loader(path, &grey, &w, &h) -> false when the file does not exist
    using Loader = std::function<bool(const std::string&, std::vector<uint8_t>*, int*, int*)>;
    FrameSequence(std::string location, FrameHandler* handler, Loader loader)
        : location_(std::move(location)), handler_(handler), loader_(std::move(loader)) {}
    void RunOnce() {
        const std::string file = location_ + std::to_string(Keyframe::GetNextId() + 1) + ".png";
        std::vector<uint8_t> grey;
        int w = 0, h = 0;
        if (loader_(file, &grey, &w, &h))
            handler_->OnNewFrame(std::make_shared<Keyframe>(grey.data(), w, h, w));
    }

private:
    std::string location_;
    FrameHandler* handler_;
    Loader loader_;
};

class Viso : public FrameSequence::FrameHandler {
public:
    Viso(double fx, double fy, double cx, double cy, int width, int height, int device = 0,
         bool enable_tracking = false) {
        viso_params p;
        check(viso_default_params(&p, fx, fy, cx, cy, width, height), "viso_default_params");
        p.enable_tracking = enable_tracking ? 1 : 0;
        check(viso_create(&p, device, &ctx_), "viso_create");
    }
    explicit Viso(const viso_params& p, int device = 0) { check(viso_create(&p, device, &ctx_), "viso_create"); }
    ~Viso() override {
        if (ctx_) viso_destroy(ctx_);
    }
    Viso(const Viso&) = delete;
    Viso& operator=(const Viso&) = delete;

    void OnNewFrame(Keyframe::Ptr cur) override {
        check(viso_process_frame(ctx_, cur->Data(), cur->Width(), cur->Height(), cur->Stride()),
              "viso_process_frame");
    }

    // The pose log.  The reference exposes it as a public field
    // (`std::vector<Sophus::SE3d> poses`, include/viso.h:54; src/main.cpp:50
    // passes `viso.poses` to DrawMap and iterates it), so `poses` is a member
    // that reads like that field -- `viso.poses.size()`, `viso.poses[i]`,
    // `for (auto& Tcw : viso.poses)`, `const std::vector<Pose>& p =
    // viso.poses` -- and also keeps the call form `viso.poses()`.  size()
    // asks the library for the count only (no copy); indexing and iteration
    // read a host snapshot that is re-downloaded only when the count has
    // changed since it was taken (entries below the count are final once the
    // library reports them), so `for (i < poses.size()) poses[i]` costs one
    // download per new frame, not one per call.
    class PoseLog {
       public:
        explicit PoseLog(const Viso* v) : v_(v) {}
        PoseLog(const PoseLog&) = delete;
        PoseLog& operator=(const PoseLog&) = delete;
        std::vector<Pose> operator()() const { return v_->fetch_poses(); }
        operator std::vector<Pose>() const { return v_->fetch_poses(); }
        size_t size() const { return v_->num_poses(); }
        bool empty() const { return size() == 0; }
        const Pose& operator[](size_t i) const { return current()[i]; }
        std::vector<Pose>::const_iterator begin() const { return current().begin(); }
        // both iterators come from the same snapshot whichever is evaluated first
        std::vector<Pose>::const_iterator end() const { return current().end(); }

       private:
        const std::vector<Pose>& current() const {
            if (cache_.size() != v_->num_poses()) cache_ = v_->fetch_poses();
            return cache_;
        }
        const Viso* v_;
        mutable std::vector<Pose> cache_;
    };
    PoseLog poses{this};

    std::vector<V3d> GetPoints() const {
        size_t n = 0;
        check(viso_get_points(ctx_, nullptr, 0, &n), "viso_get_points");
        std::vector<V3d> out(n);
        if (n) check(viso_get_points(ctx_, out.front().data(), n, &n), "viso_get_points");
        return out;
    }

    size_t num_poses() const {
        size_t n = 0;
        check(viso_get_poses(ctx_, nullptr, 0, &n), "viso_get_poses");
        return n;
    }

    std::vector<Pose> fetch_poses() const {
        size_t n = 0;
        check(viso_get_poses(ctx_, nullptr, 0, &n), "viso_get_poses");
        std::vector<Pose> out(n);
        if (n) check(viso_get_poses(ctx_, out.front().data(), n, &n), "viso_get_poses");
        return out;
    }

    int state() const {
        int32_t s = 0;
        check(viso_get_state(ctx_, &s), "viso_get_state");
        return s;
    }

    // viso_direct_solve: the faithful solve of one direct-pose level on given
    // sums (28), nGood and T21 (7) -> {stats[50], the new T21}
    std::pair<std::array<double, 50>, std::array<double, 7>> DirectSolve(const std::array<double, 28>& sums,
                                                                         int n_good,
                                                                         const std::array<double, 7>& state) const {
        std::pair<std::array<double, 50>, std::array<double, 7>> out{};
        check(viso_direct_solve(ctx_, sums.data(), n_good, state.data(), out.first.data(), out.second.data()),
              "viso_direct_solve");
        return out;
    }

    // Map growth for the monocular path (viso_set_mono_keyframes: the
    // triangulation Viso::Reconstruct, src/viso.cpp:434-501, sketches), and
    // the photometric BA after each insertion (viso_set_bundle_adjust).
    void SetMonoKeyframes(int interval, int ngood_permille = 500, int cell = 16, double min_parallax_deg = 0.25) {
        check(viso_set_mono_keyframes(ctx_, interval, ngood_permille, cell, min_parallax_deg),
              "viso_set_mono_keyframes");
    }
    void SetBundleAdjust(int iterations) { check(viso_set_bundle_adjust(ctx_, iterations), "viso_set_bundle_adjust"); }

    // Sliding-window map (viso_set_map_window): at most `window` keyframes;
    // an insertion into a full window first retires the oldest keyframe and
    // culls the points it hosts.  0 = off.
    void SetMapWindow(int window, int cell = 16) { check(viso_set_map_window(ctx_, window, cell), "viso_set_map_window"); }
    // viso_get_map_window's info[8]
    std::array<int64_t, 8> MapWindow() const {
        std::array<int64_t, 8> info{};
        check(viso_get_map_window(ctx_, info.data()), "viso_get_map_window");
        return info;
    }
    // every map point's host keyframe index
    std::vector<int32_t> GetPointHosts() const {
        size_t n = 0;
        check(viso_get_point_hosts(ctx_, nullptr, 0, &n), "viso_get_point_hosts");
        std::vector<int32_t> out(n);
        if (n) check(viso_get_point_hosts(ctx_, out.data(), n, &n), "viso_get_point_hosts");
        return out;
    }

    // Pose refinement (viso_set_pose_refine): every tracking frame's direct
    // pose is refined on its LK-aligned features (Huber-weighted
    // Gauss-Newton on the reprojection error).  0 iterations = off.
    void SetPoseRefine(int iterations, double huber_px = 1.0, double max_shift_px = 8.0) {
        check(viso_set_pose_refine(ctx_, iterations, huber_px, max_shift_px), "viso_set_pose_refine");
    }
    // viso_get_pose_refine's report[8] (NaN before the first refinement)
    std::array<double, 8> PoseRefine() const {
        std::array<double, 8> report{};
        check(viso_get_pose_refine(ctx_, report.data()), "viso_get_pose_refine");
        return report;
    }

    // Map point culling (viso_set_point_cull): every map point keeps a track
    // record {age, seen, found, fail_run} of its LK alignments; every
    // interval-th tracking frame the points that failed max_fail_run frames
    // in a row leave the map.  0 = off.
    void SetPointCull(int interval, int max_fail_run = 3, double reproj_px = 2.0, int min_points = 50) {
        check(viso_set_point_cull(ctx_, interval, max_fail_run, reproj_px, min_points), "viso_set_point_cull");
    }
    // viso_get_point_cull's info[8]
    std::array<int64_t, 8> PointCull() const {
        std::array<int64_t, 8> info{};
        check(viso_get_point_cull(ctx_, info.data()), "viso_get_point_cull");
        return info;
    }
    // every map point's track record {age, seen, found, fail_run}
    std::vector<std::array<int32_t, 4>> PointTracks() const {
        size_t n = 0;
        check(viso_get_point_tracks(ctx_, nullptr, 0, &n), "viso_get_point_tracks");
        std::vector<std::array<int32_t, 4>> out(n);
        if (n) check(viso_get_point_tracks(ctx_, out.data()->data(), n, &n), "viso_get_point_tracks");
        return out;
    }

    // Point refinement (viso_set_point_refine): every tracking frame's final
    // pose and LK-aligned positions go into a ring of `window` frames; every
    // interval-th tracking frame each map point's depth along its anchor
    // keyframe's ray is refined on them.  0 = off.
    void SetPointRefine(int interval, int window = 5, int iterations = 3, double huber_px = 1.0,
                        double max_shift_px = 8.0, int min_obs = 3, double max_rel_sigma = 0.05) {
        check(viso_set_point_refine(ctx_, interval, window, iterations, huber_px, max_shift_px, min_obs,
                                    max_rel_sigma),
              "viso_set_point_refine");
    }
    // viso_get_point_refine's info[8]
    std::array<int64_t, 8> PointRefine() const {
        std::array<int64_t, 8> info{};
        check(viso_get_point_refine(ctx_, info.data()), "viso_get_point_refine");
        return info;
    }
    // the last refinement's {status, steps} per point (empty before the first)
    std::vector<std::array<uint8_t, 2>> PointRefineStatus() const {
        size_t n = 0;
        check(viso_get_point_refine_status(ctx_, nullptr, nullptr, 0, &n), "viso_get_point_refine_status");
        std::vector<uint8_t> status(n), steps(n);
        if (n)
            check(viso_get_point_refine_status(ctx_, status.data(), steps.data(), n, &n),
                  "viso_get_point_refine_status");
        std::vector<std::array<uint8_t, 2>> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = {status[i], steps[i]};
        return out;
    }

    // Warped LK alignment (viso_set_lk_warp): every keyframe patch is warped
    // into the current view by the affine map its point's depth and the two
    // poses imply and taken from the pyramid level that matches its scale.
    // mode 0 = off.
    void SetLkWarp(int mode, double max_area_ratio = 64.0) {
        check(viso_set_lk_warp(ctx_, mode, max_area_ratio), "viso_set_lk_warp");
    }
    // viso_get_lk_warp's info[8]
    std::array<int64_t, 8> LkWarp() const {
        std::array<int64_t, 8> info{};
        check(viso_get_lk_warp(ctx_, info.data()), "viso_get_lk_warp");
        return info;
    }
    // the last frame's warp rows: A (4 per point), shift, status
    struct LkWarpRows {
        std::vector<double> A;
        std::vector<int8_t> shift;
        std::vector<uint8_t> status;
    };
    LkWarpRows LkWarpRowsLast() const {
        size_t n = 0;
        check(viso_get_lk_warp_rows(ctx_, nullptr, nullptr, nullptr, 0, &n), "viso_get_lk_warp_rows");
        LkWarpRows r{std::vector<double>(4 * n), std::vector<int8_t>(n), std::vector<uint8_t>(n)};
        if (n)
            check(viso_get_lk_warp_rows(ctx_, r.A.data(), r.shift.data(), r.status.data(), n, &n),
                  "viso_get_lk_warp_rows");
        return r;
    }

    // Illumination-invariant LK alignment (viso_set_lk_illum): a per-patch
    // gain and offset are projected out of the warped alignment; runs while
    // SetLkWarp is on.  mode 0 = off.
    void SetLkIllum(int mode, double max_gain = 4.0) {
        check(viso_set_lk_illum(ctx_, mode, max_gain), "viso_set_lk_illum");
    }
    // viso_get_lk_illum's info[8]
    std::array<int64_t, 8> LkIllum() const {
        std::array<int64_t, 8> info{};
        check(viso_get_lk_illum(ctx_, info.data()), "viso_get_lk_illum");
        return info;
    }
    // the last frame's (gain, offset) rows, 2 per point
    std::vector<double> LkIllumRows() const {
        size_t n = 0;
        check(viso_get_lk_illum_rows(ctx_, nullptr, 0, &n), "viso_get_lk_illum_rows");
        std::vector<double> go(2 * n);
        if (n) check(viso_get_lk_illum_rows(ctx_, go.data(), n, &n), "viso_get_lk_illum_rows");
        return go;
    }

    // Depth seeds (viso_set_depth_seeds): every corner of a new keyframe that
    // the map does not cover becomes a seed; every tracking frame searches the
    // seed's epipolar segment and narrows its inverse depth; every
    // interval-th frame the converged seeds become map points.  interval 0 =
    // off.
    void SetDepthSeeds(int interval, int cell = 16, int max_steps = 32, double depth_min = 2.0,
                       double depth_max = 60.0, double max_score = 57600.0, double uniqueness = 1.5,
                       int min_good = 3, double conv_rel = 0.15, int max_bad = 4, int max_lost = 4) {
        check(viso_set_depth_seeds(ctx_, interval, cell, max_steps, depth_min, depth_max, max_score, uniqueness,
                                   min_good, conv_rel, max_bad, max_lost),
              "viso_set_depth_seeds");
    }
    // viso_get_depth_seeds' info[8]
    std::array<int64_t, 8> GetDepthSeeds() const {
        std::array<int64_t, 8> info{};
        check(viso_get_depth_seeds(ctx_, info.data()), "viso_get_depth_seeds");
        return info;
    }
    // the live seeds' rows: host keyframe, corner (2 per seed), inverse depth,
    // its variance, counters (4 per seed: good, bad, lost, status)
    struct DepthSeedRows {
        std::vector<int32_t> h;
        std::vector<double> uv, mu, s2;
        std::vector<int32_t> counters;
    };
    DepthSeedRows GetDepthSeedRows() const {
        size_t n = 0;
        check(viso_get_depth_seed_rows(ctx_, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n),
              "viso_get_depth_seed_rows");
        DepthSeedRows r{std::vector<int32_t>(n), std::vector<double>(2 * n), std::vector<double>(n),
                        std::vector<double>(n), std::vector<int32_t>(4 * n)};
        if (n)
            check(viso_get_depth_seed_rows(ctx_, r.h.data(), r.uv.data(), r.mu.data(), r.s2.data(),
                                           r.counters.data(), n, &n),
                  "viso_get_depth_seed_rows");
        return r;
    }

    // Relocalisation (viso_set_relocalise): lost_after consecutive bad
    // tracking frames lose the context; every lost frame then aligns the
    // keyframes to itself until one alignment is accepted.  lost_after 0 = off.
    void SetRelocalise(int lost_after, double max_cost = 57600.0, int min_good_permille = 500, int lk_permille = 0,
                       int iterations = 10, int max_points = 512) {
        check(viso_set_relocalise(ctx_, lost_after, max_cost, min_good_permille, lk_permille, iterations, max_points),
              "viso_set_relocalise");
    }
    // viso_get_relocalise's info[8]
    std::array<int64_t, 8> GetRelocalise() const {
        std::array<int64_t, 8> info{};
        check(viso_get_relocalise(ctx_, info.data()), "viso_get_relocalise");
        return info;
    }
    // the last attempt's candidate rows: poses (12 per candidate), report (20)
    struct RelocaliseReport {
        std::vector<double> poses, report;
    };
    RelocaliseReport GetRelocaliseReport() const {
        size_t n = 0;
        check(viso_get_relocalise_report(ctx_, nullptr, nullptr, 0, &n), "viso_get_relocalise_report");
        RelocaliseReport r{std::vector<double>(12 * n), std::vector<double>(20 * n)};
        if (n) check(viso_get_relocalise_report(ctx_, r.poses.data(), r.report.data(), n, &n), "viso_get_relocalise_report");
        return r;
    }
    // Brightness-compensated tracking (viso_set_brightness): every tracking
    // frame's pose is estimated together with an affine brightness map (g, o)
    // from the last frame to it, in place of the direct pose.  iterations 0 =
    // off.
    void SetBrightness(int iterations = 10) { check(viso_set_brightness(ctx_, iterations), "viso_set_brightness"); }
    // viso_get_brightness's info[8]
    std::array<int64_t, 8> GetBrightness() const {
        std::array<int64_t, 8> info{};
        check(viso_get_brightness(ctx_, info.data()), "viso_get_brightness");
        return info;
    }
    // one row per pose: g, o, level-0 exit, steps over all levels
    std::vector<double> GetBrightnessLog() const {
        size_t n = 0;
        check(viso_get_brightness_log(ctx_, nullptr, 0, &n), "viso_get_brightness_log");
        std::vector<double> rows(4 * n);
        if (n) check(viso_get_brightness_log(ctx_, rows.data(), n, &n), "viso_get_brightness_log");
        return rows;
    }
    // the last frame's report, as viso_track_affine returns it
    std::array<double, 24> GetBrightnessReport() const {
        std::array<double, 24> r{};
        check(viso_get_brightness_report(ctx_, r.data()), "viso_get_brightness_report");
        return r;
    }
    // Robust tracking (viso_set_robust): every frame the brightness chain
    // tracks weights each patch pixel by Huber's rule with this k (grey
    // levels).  0 = off; no effect while SetBrightness is off.
    void SetRobust(double huber_k = 9.0) { check(viso_set_robust(ctx_, huber_k), "viso_set_robust"); }
    // viso_get_robust's info[8]
    std::array<int64_t, 8> GetRobust() const {
        std::array<int64_t, 8> info{};
        check(viso_get_robust(ctx_, info.data()), "viso_get_robust");
        return info;
    }
    // the last robust frame's report, as viso_track_robust returns it
    std::array<double, 28> GetRobustReport() const {
        std::array<double, 28> r{};
        check(viso_get_robust_report(ctx_, r.data()), "viso_get_robust_report");
        return r;
    }
    // the last robust frame's weight mass per map point, in the map's order
    // when that frame was tracked
    std::vector<double> GetRobustWeights() const {
        size_t n = 0;
        check(viso_get_robust_weights(ctx_, nullptr, 0, &n), "viso_get_robust_weights");
        std::vector<double> w(n);
        if (n) check(viso_get_robust_weights(ctx_, w.data(), n, &n), "viso_get_robust_weights");
        return w;
    }
    // one row per pose: mean weight, down-weighted pixels
    std::vector<double> GetRobustLog() const {
        size_t n = 0;
        check(viso_get_robust_log(ctx_, nullptr, 0, &n), "viso_get_robust_log");
        std::vector<double> rows(2 * n);
        if (n) check(viso_get_robust_log(ctx_, rows.data(), n, &n), "viso_get_robust_log");
        return rows;
    }
    // Relocalisation seed (viso_set_reloc_seed; effective while SetRelocalise
    // is on): a lost frame whose attempt has no winner gets a pose seed from
    // descriptor matches and a second attempt from it.  hypotheses 0 = off.
    void SetRelocSeed(int hypotheses = 256, int max_hamming = 48, int ratio_permille = 800, double inlier_px = 2.0,
                      int min_inliers = 30, uint64_t seed = 0) {
        check(viso_set_reloc_seed(ctx_, hypotheses, max_hamming, ratio_permille, inlier_px, min_inliers, seed),
              "viso_set_reloc_seed");
    }
    // viso_get_reloc_seed's info[8]
    std::array<int64_t, 8> GetRelocSeed() const {
        std::array<int64_t, 8> info{};
        check(viso_get_reloc_seed(ctx_, info.data()), "viso_get_reloc_seed");
        return info;
    }
    // the last seed stage's report (12) and seed pose (12)
    struct RelocSeedReport {
        std::array<double, 12> report, pose;
    };
    RelocSeedReport GetRelocSeedReport() const {
        RelocSeedReport r{};
        check(viso_get_reloc_seed_report(ctx_, r.report.data(), r.pose.data()), "viso_get_reloc_seed_report");
        return r;
    }
    // Affine brightness per candidate in the relocalisation attempts
    // (viso_set_reloc_illum; effective while SetRelocalise is on): every
    // attempt of a lost frame estimates (pose, gain, offset) and rejects a
    // gain outside [1 / max_gain, max_gain].  mode 0 = off.
    void SetRelocIllum(int mode, double max_gain = 4.0) {
        check(viso_set_reloc_illum(ctx_, mode, max_gain), "viso_set_reloc_illum");
    }
    // viso_get_reloc_illum's info[8]
    std::array<int64_t, 8> GetRelocIllum() const {
        std::array<int64_t, 8> info{};
        check(viso_get_reloc_illum(ctx_, info.data()), "viso_get_reloc_illum");
        return info;
    }
    // the last such attempt's (gain, offset) rows, 2 per candidate
    std::vector<double> RelocIllumRows() const {
        size_t n = 0;
        check(viso_get_reloc_illum_rows(ctx_, nullptr, 0, &n), "viso_get_reloc_illum_rows");
        std::vector<double> go(2 * n);
        if (n) check(viso_get_reloc_illum_rows(ctx_, go.data(), n, &n), "viso_get_reloc_illum_rows");
        return go;
    }
    // one byte per pose: 0 tracked, 1 bad verdict, 2 lost, 3 recovered
    std::vector<uint8_t> GetFrameStatus() const {
        size_t n = 0;
        check(viso_get_frame_status(ctx_, nullptr, 0, &n), "viso_get_frame_status");
        std::vector<uint8_t> st(n);
        if (n) check(viso_get_frame_status(ctx_, st.data(), n, &n), "viso_get_frame_status");
        return st;
    }

    // Rectification (viso_set_rectify): camera `cam` (0 left or mono, 1
    // right) delivers raw frames, undistorted and rectified on the device
    // ahead of the pyramid.  p.R takes rays of the rectified camera into the
    // raw camera (the transpose of OpenCV's R1 / R2).  nullptr or model 0 =
    // off.  Only before the first frame.
    void set_rectify(int cam, const viso_rectify_params* p) { check(viso_set_rectify(ctx_, cam, p), "viso_set_rectify"); }
    // viso_get_rectify's info[8]
    std::array<int64_t, 8> get_rectify(int cam = 0) const {
        std::array<int64_t, 8> info{};
        check(viso_get_rectify(ctx_, cam, info.data()), "viso_get_rectify");
        return info;
    }
    // viso_rectify (stage entry): n raw images -> n rectified width x height
    // images with the output intrinsics K; counts = {outside, clipped}
    std::vector<uint8_t> Rectify(const viso_rectify_params& p, const std::array<double, 4>& K, int width, int height,
                                 const uint8_t* raw, int n, std::array<int64_t, 2>* counts = nullptr) const {
        std::vector<uint8_t> out((size_t)width * height * (size_t)std::max(n, 0));
        check(viso_rectify(ctx_, &p, K.data(), width, height, raw, n, out.data(), counts ? counts->data() : nullptr),
              "viso_rectify");
        return out;
    }

    viso_ctx* handle() const { return ctx_; }

protected:
    viso_ctx* ctx_ = nullptr;
};

// The reference path fed with stereo pairs: the left image drives
// OnNewFrame; while initialising, the right image gives the metric stereo
// initialisation (viso_set_stereo, enabled with SetStereo) in place of the
// 2D-2D one (src/viso.cpp:178-256).
class StereoViso : public Viso {
public:
    using Viso::Viso;
    void SetStereo(double baseline, int max_disp = 128, int min_disp = 1) {
        check(viso_set_stereo(ctx_, baseline, max_disp, min_disp), "viso_set_stereo");
    }
    bool process(const uint8_t* left, const uint8_t* right, const int32_t* dims) {
        return viso_process_stereo(ctx_, left, right, dims) == VISO_OK;
    }
};

}  // namespace viso

#endif
