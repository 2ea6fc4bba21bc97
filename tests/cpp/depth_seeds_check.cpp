// Compile/link check of the depth-seed methods of the C++ facade
// (include/viso/viso.hpp: SetDepthSeeds, GetDepthSeeds, GetDepthSeedRows)
// against the C ABI.  Without an argument nothing is run (no GPU needed); with
// one, a context is created and the three methods are called.
#include <cstdio>

#include "viso/viso.hpp"

int main(int argc, char**) {
    void (viso::Viso::*set)(int, int, int, double, double, double, double, int, double, int, int) =
        &viso::Viso::SetDepthSeeds;
    std::array<int64_t, 8> (viso::Viso::*get)() const = &viso::Viso::GetDepthSeeds;
    viso::Viso::DepthSeedRows (viso::Viso::*rows)() const = &viso::Viso::GetDepthSeedRows;
    if (!set || !get || !rows) return 1;
    if (argc > 1) {
        viso::Viso v(300.0, 300.0, 160.0, 48.0, 320, 96);
        v.SetDepthSeeds(4);
        const auto info = v.GetDepthSeeds();
        const auto r = v.GetDepthSeedRows();
        if (info[0] != 4 || info[1] != 0 || !r.h.empty() || !r.counters.empty()) return 2;
        v.SetDepthSeeds(0);
        if (v.GetDepthSeeds()[0] != 0) return 3;
    }
    std::printf("depth seeds facade ok\n");
    return 0;
}
