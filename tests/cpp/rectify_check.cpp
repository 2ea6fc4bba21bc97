// Compile/link check of the rectification methods of the C++ facade
// (include/viso/viso.hpp: set_rectify, get_rectify, Rectify) against the C
// ABI.  Without an argument nothing is run (no GPU needed); with one, a context
// is created, the mode is set and read back and the stage entry is called.
#include <cstdio>

#include "viso/viso.hpp"

int main(int argc, char**) {
    void (viso::Viso::*set)(int, const viso_rectify_params*) = &viso::Viso::set_rectify;
    std::array<int64_t, 8> (viso::Viso::*get)(int) const = &viso::Viso::get_rectify;
    if (!set || !get) return 1;
    if (argc > 1) {
        const int w = 61, h = 17;
        // (power-of-two focal lengths: (x - cx) / fx * fx + cx is exact)
        const std::array<double, 4> K{64.0, 32.0, 30.0, 8.0};
        viso::Viso v(K[0], K[1], K[2], K[3], w, h);
        viso_rectify_params p{};
        p.model = VISO_RECTIFY_RADTAN;
        p.raw_width = w;
        p.raw_height = h;
        p.fill = 7;
        p.fx = K[0], p.fy = K[1], p.cx = K[2], p.cy = K[3];
        p.R[0] = p.R[4] = p.R[8] = 1.0;
        v.set_rectify(0, &p);
        const auto info = v.get_rectify(0);
        // identity: nothing outside, nothing clipped, nothing rectified yet
        if (info[0] != VISO_RECTIFY_RADTAN || info[1] != w || info[2] != h || info[3] != 7 || info[4] != 0 ||
            info[5] != 0 || info[6] != 0 || info[7] != 0)
            return 2;
        if (v.get_rectify(1)[0] != VISO_RECTIFY_OFF) return 3;
        v.set_rectify(0, nullptr);
        if (v.get_rectify(0)[0] != VISO_RECTIFY_OFF) return 4;
        // the stage entry: identity returns the image, cx + 3 shifts it by 3
        // pixels (fill past the raw image's right edge)
        std::vector<uint8_t> raw((size_t)w * h * 2);
        for (size_t i = 0; i < raw.size(); ++i) raw[i] = (uint8_t)((i * 37u + (i >> 5) * 11u) & 255u);
        std::array<int64_t, 2> counts{-1, -1};
        const auto same = v.Rectify(p, K, w, h, raw.data(), 2, &counts);
        if (same != raw || counts[0] != 0 || counts[1] != 0) return 5;
        p.cx = K[2] + 3.0;
        const auto sh = v.Rectify(p, K, w, h, raw.data(), 2, &counts);
        for (int i = 0; i < 2; ++i)
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const uint8_t want = x + 3 < w ? raw[((size_t)i * h + y) * w + x + 3] : (uint8_t)7;
                    if (sh[((size_t)i * h + y) * w + x] != want) return 6;
                }
        // u = x + 3 < rw only for x < w - 3: the last 3 columns are outside
        if (counts[0] != 3 * h || counts[1] != 3 * h) return 7;
    }
    std::printf("rectify facade ok\n");
    return 0;
}
