// viso_amd — rectification: undistort and rectify raw camera frames at ingest
// (viso_set_rectify, viso_rectify; include/viso/viso_c.h).  The
// repo's own spec, restated in tests/rectify_ref.py: per output pixel the
// coordinates (u, v) in the raw image — the radial-tangential model through
// the rotation R, in fp64, or a caller's table — quantised to 1/32 pixel and
// sampled bilinearly in integers.
//
// Mapping: one launch for all images of a chunk (left and right, a camera
// index per image).  A workgroup is a tile of 128 x 8 output pixels: a lane
// produces the 4 bytes of one aligned dword of its output row and stores it
// once; the 32 lanes of a row write 128 contiguous bytes.  A row that does not
// start on a dword (w not a multiple of 4) shifts its lanes left by the
// misalignment, so only a row's first and last dword are partial (byte
// stores).  The taps of neighbouring lanes and rows fall on the same raw
// lines: the gather is served from L1 / L2.  Every tap is tested against the
// raw image (never a read outside [0, rw * rh)).  No LDS, no inline assembly;
// atomics only in the one-off count launch.  -ffp-contract=off.
#include <algorithm>
#include <cmath>

#include "context.hpp"

namespace viso {

namespace {

constexpr int kRtW = 128, kRtH = 8;  // output pixels of a tile (32 x 8 lanes)

// (u, v) of output pixel (x, y); false: the pixel is outside (Z <= 0)
template <int MODEL>
__device__ __forceinline__ bool rect_uv(const RectCam& c, const double* K, int w, int x, int y, double& u, double& v) {
    if (MODEL == VISO_RECTIFY_TABLE) {
        const float2 m = reinterpret_cast<const float2*>(c.map)[(size_t)y * w + x];
        u = (double)m.x;
        v = (double)m.y;
        return true;
    }
    const double a = ((double)x - K[2]) / K[0];
    const double b = ((double)y - K[3]) / K[1];
    const double X = (c.R[0] * a + c.R[1] * b) + c.R[2];
    const double Y = (c.R[3] * a + c.R[4] * b) + c.R[5];
    const double Z = (c.R[6] * a + c.R[7] * b) + c.R[8];
    if (!(Z > 0.0)) return false;
    const double xn = X / Z, yn = Y / Z;
    const double r2 = xn * xn + yn * yn, xy = xn * yn;
    const double rad = 1.0 + r2 * (c.k[0] + r2 * (c.k[1] + r2 * c.k[4]));
    const double xd = xn * rad + ((2.0 * c.k[2]) * xy + c.k[3] * (r2 + 2.0 * (xn * xn)));
    const double yd = yn * rad + (c.k[2] * (r2 + 2.0 * (yn * yn)) + (2.0 * c.k[3]) * xy);
    u = c.Kr[0] * xd + c.Kr[2];
    v = c.Kr[1] * yd + c.Kr[3];
    return true;
}

// The output byte at (u, v).  flags: bit 0 outside, bit 1 clipped.  COUNT:
// the flags only (src is not read).
template <bool COUNT>
__device__ __forceinline__ int rect_sample(const uint8_t* __restrict__ src, int rw, int rh, int fill, bool front,
                                           double u, double v, int& flags) {
    if (!(front && u > -1.0 && u < (double)rw && v > -1.0 && v < (double)rh)) {
        flags = 3;
        return fill;
    }
    const int qu = (int)floor(u * 32.0 + 0.5), qv = (int)floor(v * 32.0 + 0.5);
    const int x0 = qu >> 5, ax = qu & 31, y0 = qv >> 5, ay = qv & 31;
    if (COUNT) {
        // a tap of non-zero weight outside: column x0 and row y0 always
        // weigh, column x0 + 1 with ax > 0, row y0 + 1 with ay > 0
        const bool clip = x0 < 0 || x0 >= rw || (ax > 0 && x0 + 1 >= rw) || y0 < 0 || y0 >= rh ||
                          (ay > 0 && y0 + 1 >= rh);
        flags = clip ? 2 : 0;
        return 0;
    }
    flags = 0;
    int t00, t01, t10, t11;
    if (x0 >= 0 && x0 + 1 < rw && y0 >= 0 && y0 + 1 < rh) {
        // all four taps inside (rw * rh < 2^25): the two bytes of a raw line
        // in one load each, at a 32-bit offset from the image's base
        const uint32_t o = (uint32_t)(y0 * rw + x0);
        uint16_t r0, r1;
        __builtin_memcpy(&r0, src + o, 2);
        __builtin_memcpy(&r1, src + o + (uint32_t)rw, 2);
        t00 = r0 & 255;
        t01 = r0 >> 8;
        t10 = r1 & 255;
        t11 = r1 >> 8;
    } else {
        auto tap = [&](int xx, int yy) -> int {
            return (xx >= 0 && xx < rw && yy >= 0 && yy < rh) ? (int)src[(uint32_t)(yy * rw + xx)] : fill;
        };
        t00 = tap(x0, y0), t01 = tap(x0 + 1, y0), t10 = tap(x0, y0 + 1), t11 = tap(x0 + 1, y0 + 1);
    }
    return (t00 * (32 - ax) * (32 - ay) + t01 * ax * (32 - ay) + t10 * (32 - ax) * ay + t11 * ax * ay + 512) >> 10;
}

// grid: (tiles across, tiles down, images).  COUNT: one image of camera
// a.cam[0], nothing stored, counts[0] += outside, counts[1] += clipped.
template <int MODEL, bool COUNT>
__global__ __launch_bounds__(256) void rectify_kernel(RectifyArgs a, int* __restrict__ counts) {
    const int img = blockIdx.z;
    const RectCam& c = a.cams[a.cam[img]];
    const int w = a.w, h = a.h;
    const int lx = threadIdx.x & 31, y = blockIdx.y * kRtH + (threadIdx.x >> 5);
    int n_out = 0, n_clip = 0;
    if (y < h) {
        uint8_t* __restrict__ row = COUNT ? nullptr : a.dst[img] + (size_t)y * w;
        // the lane's dword is aligned in memory: the row's lanes start
        // `mis` bytes ahead of the row
        const int mis = COUNT ? 0 : (int)((uintptr_t)row & 3);
        const int x = blockIdx.x * kRtW + 4 * lx - mis;
        const uint8_t* __restrict__ src = a.src[img];
        const int rw = c.rw, rh = c.rh, fill = c.fill;
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xx = x + k;
            if (xx < 0 || xx >= w) continue;
            double u = 0.0, v = 0.0;
            const bool front = rect_uv<MODEL>(c, a.K, w, xx, y, u, v);
            int flags;
            const int px = rect_sample<COUNT>(src, rw, rh, fill, front, u, v, flags);
            word |= (uint32_t)px << (8 * k);
            n_out += flags & 1;
            n_clip += flags >> 1;
        }
        if (!COUNT) {
            if (x >= 0 && x + 4 <= w) {
                *reinterpret_cast<uint32_t*>(row + x) = word;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k >= 0 && x + k < w) row[x + k] = (uint8_t)(word >> (8 * k));
            }
        }
    }
    if (COUNT) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            n_out += __shfl_down(n_out, d, 64);
            n_clip += __shfl_down(n_clip, d, 64);
        }
        if ((threadIdx.x & 63) == 0 && (n_out | n_clip)) {
            atomicAdd(counts, n_out);
            atomicAdd(counts + 1, n_clip);
        }
    }
}

dim3 rect_grid(int w, int h, int n) {
    // (a misaligned row starts up to 3 bytes ahead of its first pixel)
    return dim3((unsigned)((w + 3 + kRtW - 1) / kRtW), (unsigned)((h + kRtH - 1) / kRtH), (unsigned)n);
}

bool finite_all(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// viso_set_rectify's argument rules for an `on` camera (sizes in [min_dim, kMaxWidth])
bool rect_params_ok(const viso_rectify_params* p, int min_dim) {
    if (p->model != VISO_RECTIFY_RADTAN && p->model != VISO_RECTIFY_TABLE) return false;
    if (p->raw_width < min_dim || p->raw_height < min_dim || p->raw_width > kMaxWidth || p->raw_height > kMaxWidth)
        return false;
    if (p->fill < 0 || p->fill > 255) return false;
    if (p->model == VISO_RECTIFY_TABLE) return p->map != nullptr;
    const double num[9] = {p->fx, p->fy, p->cx, p->cy, p->k1, p->k2, p->p1, p->p2, p->k3};
    return finite_all(num, 9) && finite_all(p->R, 9) && p->fx > 0 && p->fy > 0;
}

RectCam rect_cam(const viso_rectify_params* p, const float* map_dev) {
    RectCam c;
    c.model = p->model;
    c.rw = p->raw_width;
    c.rh = p->raw_height;
    c.fill = p->fill;
    if (p->model == VISO_RECTIFY_RADTAN) {
        const double Kr[4] = {p->fx, p->fy, p->cx, p->cy}, k[5] = {p->k1, p->k2, p->p1, p->p2, p->k3};
        std::copy(Kr, Kr + 4, c.Kr);
        std::copy(k, k + 5, c.k);
        std::copy(p->R, p->R + 9, c.R);
    }
    c.map = map_dev;
    return c;
}

// the counts of one image of `cam` -> out[2], through two device ints at d_counts (one host sync)
int rect_counts(const RectCam& cam, const double K[4], int w, int h, int* d_counts, hipStream_t st, int64_t out[2]) {
    VISO_HIP_CHECK(hipMemsetAsync(d_counts, 0, 8, st));
    launch_rectify_count(cam, K, w, h, d_counts, st);
    VISO_HIP_CHECK(hipGetLastError());
    int host[2] = {0, 0};
    VISO_HIP_CHECK(hipMemcpyAsync(host, d_counts, 8, hipMemcpyDeviceToHost, st));
    VISO_HIP_CHECK(hipStreamSynchronize(st));
    out[0] = host[0];
    out[1] = host[1];
    return VISO_OK;
}

}  // namespace

void launch_rectify(const RectCam cams[2], const double K[4], int w, int h, const uint8_t* const* src,
                    uint8_t* const* dst, const uint8_t* cam, int n, hipStream_t stream) {
    for (int model = VISO_RECTIFY_RADTAN; model <= VISO_RECTIFY_TABLE; ++model) {
        RectifyArgs a;
        a.cams[0] = cams[0];
        a.cams[1] = cams[1];
        std::copy(K, K + 4, a.K);
        a.w = w;
        a.h = h;
        int nb = 0;
        auto flush = [&] {
            if (nb == 0) return;
            if (model == VISO_RECTIFY_RADTAN)
                rectify_kernel<VISO_RECTIFY_RADTAN, false><<<rect_grid(w, h, nb), 256, 0, stream>>>(a, nullptr);
            else
                rectify_kernel<VISO_RECTIFY_TABLE, false><<<rect_grid(w, h, nb), 256, 0, stream>>>(a, nullptr);
            nb = 0;
        };
        for (int i = 0; i < n; ++i) {
            if (cams[cam[i]].model != model) continue;
            a.src[nb] = src[i];
            a.dst[nb] = dst[i];
            a.cam[nb] = cam[i];
            if (++nb == kRectBatch) flush();
        }
        flush();
    }
}

void launch_rectify_count(const RectCam& cam, const double K[4], int w, int h, int* counts, hipStream_t stream) {
    RectifyArgs a;
    a.cams[0] = cam;
    a.cam[0] = 0;
    a.src[0] = nullptr;
    a.dst[0] = nullptr;
    std::copy(K, K + 4, a.K);
    a.w = w;
    a.h = h;
    if (cam.model == VISO_RECTIFY_RADTAN)
        rectify_kernel<VISO_RECTIFY_RADTAN, true><<<rect_grid(w, h, 1), 256, 0, stream>>>(a, counts);
    else
        rectify_kernel<VISO_RECTIFY_TABLE, true><<<rect_grid(w, h, 1), 256, 0, stream>>>(a, counts);
}

}  // namespace viso

using namespace viso;

int viso_ctx::rectify_launch(const uint8_t* const* src, uint8_t* const* dst, const uint8_t* cam, int n,
                             hipStream_t st) {
    if (n <= 0) return VISO_OK;
    double K[4];
    intrinsics(K);
    {
        TimedRegion t(timing, VISO_KERNEL_RECTIFY, st);
        launch_rectify(rect, K, p.width, p.height, src, dst, cam, n, st);
    }
    VISO_HIP_CHECK(hipGetLastError());
    bool seen[2] = {false, false};
    for (int i = 0; i < n; ++i) {
        seen[cam[i]] = true;
        rect_info[cam[i]][3] += 1;
    }
    for (int k = 0; k < 2; ++k) rect_info[k][2] += seen[k] ? 1 : 0;
    return VISO_OK;
}

extern "C" {

int viso_set_rectify(viso_ctx* c, int32_t cam, const viso_rectify_params* p) {
    if (!c || cam < 0 || cam > 1) return VISO_ERR_ARG;
    const bool on = p && p->model != VISO_RECTIFY_OFF;
    if (on && !rect_params_ok(p, 16)) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    if (c->frames > 0) return VISO_ERR_STATE;
    VISO_HIP_CHECK(hipSetDevice(c->device));
    for (int k = 0; k < 4; ++k) c->rect_info[cam][k] = 0;
    if (!on) {
        c->rect[cam] = RectCam{};
        c->rect_map[cam].release();
        c->rect_raw[cam].release();
        if (cam == 1) c->rect_right.release();
        return VISO_OK;
    }
    const size_t px = (size_t)c->p.width * c->p.height;
    const float* map_dev = nullptr;
    if (p->model == VISO_RECTIFY_TABLE) {
        if (int rc = c->rect_map[cam].ensure(8 * px)) return rc;
        VISO_HIP_CHECK(hipMemcpyAsync(c->rect_map[cam].ptr, p->map, 8 * px, hipMemcpyHostToDevice, c->stream));
        VISO_HIP_CHECK(hipStreamSynchronize(c->stream));  // (the caller's map is copied when the call returns)
        map_dev = (const float*)c->rect_map[cam].ptr;
    } else {
        c->rect_map[cam].release();
    }
    // the camera's raw host frame (and the two count words of this call)
    if (int rc = c->rect_raw[cam].ensure(std::max<size_t>((size_t)p->raw_width * p->raw_height, 256))) return rc;
    if (cam == 1)
        if (int rc = c->rect_right.ensure(px * (size_t)c->p.batch_frames)) return rc;
    c->rect[cam] = rect_cam(p, map_dev);
    double K[4];
    c->intrinsics(K);
    int64_t counts[2];
    if (int rc = rect_counts(c->rect[cam], K, c->p.width, c->p.height, (int*)c->rect_raw[cam].ptr, c->stream, counts)) {
        c->rect[cam] = RectCam{};
        return rc;
    }
    c->rect_info[cam][0] = counts[0];
    c->rect_info[cam][1] = counts[1];
    return VISO_OK;
}

int viso_get_rectify(viso_ctx* c, int32_t cam, int64_t info[8]) {
    if (!c || cam < 0 || cam > 1 || !info) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    const RectCam& r = c->rect[cam];
    info[0] = r.model;
    info[1] = r.rw;
    info[2] = r.rh;
    info[3] = r.fill;
    for (int k = 0; k < 4; ++k) info[4 + k] = c->rect_info[cam][k];
    return VISO_OK;
}

int viso_rectify(viso_ctx* c, const viso_rectify_params* p, const double K[4], int32_t width, int32_t height,
                 const uint8_t* raw, int32_t n, uint8_t* out, int64_t counts[2]) {
    if (!c || !p || !K || !raw || !out || n < 1 || width < 1 || height < 1 || width > kMaxWidth || height > kMaxWidth)
        return VISO_ERR_ARG;
    if (!rect_params_ok(p, 1) || !finite_all(K, 4)) return VISO_ERR_ARG;
    if (int rc = c->settle()) return rc;  // (host-frame work left pending)
    VISO_HIP_CHECK(hipSetDevice(c->device));
    const size_t px = (size_t)width * height, rpx = (size_t)p->raw_width * p->raw_height;
    Bump b;
    // (images packed as the caller's: an odd size leaves rows and images off the dword grid)
    const size_t o_map = b.take(p->model == VISO_RECTIFY_TABLE ? 8 * px : 0), o_cnt = b.take(8),
                 o_raw = b.take(rpx * (size_t)n), o_out = b.take(px * (size_t)n);
    if (int rc = c->scratch_a.ensure(b.off)) return rc;
    char* base = (char*)c->scratch_a.ptr;
    if (p->model == VISO_RECTIFY_TABLE)
        VISO_HIP_CHECK(hipMemcpyAsync(base + o_map, p->map, 8 * px, hipMemcpyHostToDevice, c->stream));
    VISO_HIP_CHECK(hipMemcpyAsync(base + o_raw, raw, rpx * (size_t)n, hipMemcpyHostToDevice, c->stream));
    RectCam cams[2];
    cams[0] = rect_cam(p, (const float*)(base + o_map));
    std::vector<const uint8_t*> src((size_t)n);
    std::vector<uint8_t*> dst((size_t)n);
    for (int i = 0; i < n; ++i) {
        src[(size_t)i] = (const uint8_t*)(base + o_raw) + rpx * (size_t)i;
        dst[(size_t)i] = (uint8_t*)(base + o_out) + px * (size_t)i;
    }
    const std::vector<uint8_t> cam((size_t)n, 0);
    {
        TimedRegion t(c->timing, VISO_KERNEL_RECTIFY, c->stream);
        launch_rectify(cams, K, width, height, src.data(), dst.data(), cam.data(), n, c->stream);
    }
    VISO_HIP_CHECK(hipGetLastError());
    VISO_HIP_CHECK(hipMemcpyAsync(out, base + o_out, px * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (counts) return rect_counts(cams[0], K, width, height, (int*)(base + o_cnt), c->stream, counts);
    VISO_HIP_CHECK(hipStreamSynchronize(c->stream));
    return VISO_OK;
}

}  // extern "C"
