//  gfhip_flux_volumes_host on the planted map of tests/flux_volume_model.py (psi = (R - 2)^2 + z^2), for a run of the
//  host code under the address and undefined-behaviour sanitizers; no device is touched.  From graph_framework_amd/csrc:
//
//      hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I../../include \
//          -o /tmp/volumes_host_check ../../profiles/diag/volumes_host_check.cpp gf_hip.cpp cells_rays.cpp cells_particles.cpp \
//          reduce.hip deposition.hip flux_profile.hip flux_spectrum.hip phase_bins.hip moment_bins.hip confinement.hip \
//          particle_source.hip hand_over.hip cli_distribution.cpp -lhiprtc && /tmp/volumes_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gf_hip.h"

int main() {
    const size_t numr = 8, numz = 8, table = numr*numz, limbs = 67;
    std::vector<double> coefficients(16*table, 0.0);
    const struct { int a, b; double value; } planted[] = {{0, 0, 2.0}, {1, 0, -0.5}, {2, 0, 0.0625}, {0, 1, -0.5}, {0, 2, 0.0625}};
    for (const auto &c : planted) {
        for (size_t at = 0; at < table; at++) coefficients[(c.a*4 + c.b)*table + at] = c.value;
    }
    const gfhip_flux_map map = {1.0, 0.25, -1.0, 0.25, numr, numz, coefficients.data(), 0.0, 1.0, 0u, 0u};
    const double edges[3] = {0.04, 0.25, 0.64};
    const double pi = 3.14159265358979323846;
    int failures = 0;
    for (uint32_t sub : {1u, 3u, 32u, 256u}) {
        const uint64_t total = numr*sub*numz*sub;
        std::vector<int64_t> state(2*limbs, 0);
        uint64_t counters[3] = {0, 0, 0};
//  in three pieces, the cuts inside a row, the last piece through a window that holds everything
        const gfhip_flux_window window = {0.5, INFINITY, -INFINITY, 1.0};
        const uint64_t cuts[4] = {0, total/3 + 1, total/2 + 5 < total ? total/2 + 5 : total, total};
        for (int p = 0; p < 3; p++) {
            if (gfhip_flux_volumes_host(&map, edges, 2, sub, p == 2 ? &window : nullptr, cuts[p], cuts[p + 1] - cuts[p], state.data(), counters)) {
                std::printf("sub %u piece %d: %s\n", sub, p, gfhip_last_error(nullptr));
                failures++;
            }
        }
        double sum[2];
        for (int cell = 0; cell < 2; cell++) {                  // the leading digits are enough for a look
            long double value = 0.0L;
            for (size_t k = limbs; k-- > 0;) value = value*4294967296.0L + static_cast<long double> (state[cell*limbs + k]);
            sum[cell] = static_cast<double> (std::ldexp(value, -1074));
        }
        std::printf("sub %3u: %llu points, %llu outside; volumes %.6f %.6f (exact %.6f %.6f)\n", sub,
                    static_cast<unsigned long long> (counters[0]), static_cast<unsigned long long> (counters[1]),
                    2.0*pi*sum[0], 2.0*pi*sum[1], 4.0*pi*pi*0.21, 4.0*pi*pi*0.39);
        if (counters[0] != total) failures++;
    }
    const gfhip_flux_window empty = {2.0, 2.0, 0.0, 1.0};
    std::vector<int64_t> state(2*limbs, 0);
    uint64_t counters[3] = {0, 0, 0};
    const int refused = gfhip_flux_volumes_host(&map, edges, 2, 0, nullptr, 0, 1, state.data(), counters) +
                        gfhip_flux_volumes_host(&map, edges, 2, 4, &empty, 0, 1, state.data(), counters) +
                        gfhip_flux_volumes_host(&map, edges, 2, 4, nullptr, UINT64_MAX, 2, state.data(), counters);
    std::printf("refused %d of 3: %s\n", refused, gfhip_last_error(nullptr));
    return failures || refused != 3;
}
