//  gfhip_spectrum_npar_host on a planted map (psi = (R - 2)^2 + z^2, fpol = 2 + tp/8 over 4 intervals), for a run of the
//  host code under the address and undefined-behaviour sanitizers; no device is touched.  From graph_framework_amd/csrc:
//
//      hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I../../include \
//          -o /tmp/spectrum_host_check ../../profiles/diag/spectrum_host_check.cpp gf_hip.cpp cells_rays.cpp cells_particles.cpp \
//          reduce.hip deposition.hip flux_profile.hip flux_spectrum.hip phase_bins.hip moment_bins.hip confinement.hip \
//          particle_source.hip hand_over.hip cli_distribution.cpp -lhiprtc && /tmp/spectrum_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gf_hip.h"

int main() {
    const size_t numr = 8, numz = 8, table = numr*numz, numpsi = 4;
    std::vector<double> coefficients(16*table, 0.0);
    const struct { int a, b; double value; } planted[] = {{0, 0, 2.0}, {1, 0, -0.5}, {2, 0, 0.0625}, {0, 1, -0.5}, {0, 2, 0.0625}};
    for (const auto &c : planted) {
        for (size_t at = 0; at < table; at++) coefficients[(c.a*4 + c.b)*table + at] = c.value;
    }
    const gfhip_flux_map map = {1.0, 0.25, -1.0, 0.25, numr, numz, coefficients.data(), 0.0, 1.0, 0u, 0u};
    const std::vector<double> c0(numpsi, 2.0), c1(numpsi, 0.125), c2(numpsi, 0.0), c3(numpsi, 0.0);
//  psi runs from 0 to 2 on this map and the table covers [0.25, 1.25): intervals below 0 and above the last are clamped
    gfhip_spectrum_field field = {0.25, 0.25, numpsi, {c0.data(), c1.data(), c2.data(), c3.data()}, 1.0, 0};

    std::vector<double> columns[7];
    const double nan = std::nan(""), inf = INFINITY;
    const double rows[][7] = {{2.5, 0.0, 0.25, 1.0, 0.0, 0.0, 1.0},           // k along R
                              {0.0, 2.5, 0.25, 0.0, 0.0, 1.0, 1.0},           // k along z
                              {1.5, 1.5, -0.5, 0.3, -0.2, 0.1, 2.0},
                              {1.0, 0.0, -1.0, 1.0, 1.0, 1.0, 1.0},           // tr = tz = 0
                              {3.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0},            // tr = numr: off the map
                              {2.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0},            // the axis: psi = 0, below the fpol table
                              {2.9, 0.0, 0.9, 1.0, 1.0, 1.0, 1.0},            // psi above the fpol table
                              {2.5, 0.0, 0.25, 1.0, 0.0, 0.0, 0.0},           // w = 0
                              {2.5, 0.0, 0.25, 0.0, 0.0, 0.0, 1.0},           // k = 0
                              {nan, 0.0, 0.25, 1.0, 0.0, 0.0, 1.0},
                              {2.5, 0.0, inf, 1.0, 0.0, 0.0, 1.0},
                              {2.5, 0.0, 0.25, inf, nan, -inf, 1.0},
                              {1.0e200, 1.0e200, 0.0, 1.0, 0.0, 0.0, 1.0}};
    for (const auto &row : rows) {
        for (int k = 0; k < 7; k++) columns[k].push_back(row[k]);
    }
    const size_t count = columns[0].size();
    const double *pointers[7];
    for (int k = 0; k < 7; k++) pointers[k] = columns[k].data();
    std::vector<double> label(count), npar(count);
    int failures = 0;
    if (gfhip_spectrum_npar_host(&map, &field, pointers, count, label.data(), npar.data())) {
        std::printf("refused: %s\n", gfhip_last_error(nullptr));
        return 1;
    }
    for (size_t s = 0; s < count; s++) std::printf("sample %2zu: label %.6f  N %.6f\n", s, label[s], npar[s]);
//  The values are the numpy model's business (tests/test_spectrum.py); here: the samples off the map are NaN, those inside
//  are numbers with |N| <= c |k|/w
    if (!std::isnan(label[4]) || !std::isnan(npar[4]) || !std::isnan(label[9]) || !std::isnan(label[10])) failures++;
    for (const size_t s : {0, 1, 2, 3, 5, 6, 8}) {
        const double k = std::sqrt(columns[3][s]*columns[3][s] + columns[4][s]*columns[4][s] + columns[5][s]*columns[5][s]);
        if (!(std::fabs(npar[s]) <= k/columns[6][s]*(1.0 + 1.0e-15))) failures++;
    }
    if (!std::isinf(npar[7]) || npar[8] != 0.0) failures++;
    if (gfhip_spectrum_npar_host(&map, &field, pointers, 0, nullptr, nullptr)) failures++;      // nothing to do is no error

    int refused = 0;
    field.numpsi = 0;
    refused += gfhip_spectrum_npar_host(&map, &field, pointers, count, label.data(), npar.data());
    field.numpsi = numpsi;
    field.c = 0.0;
    refused += gfhip_spectrum_npar_host(&map, &field, pointers, count, label.data(), npar.data());
    field.c = 1.0;
    field.fpol[3] = nullptr;
    refused += gfhip_spectrum_npar_host(&map, &field, pointers, count, label.data(), npar.data());
    field.fpol[3] = c3.data();
    refused += gfhip_spectrum_npar_host(&map, &field, pointers, count, nullptr, npar.data());
    refused += gfhip_spectrum_npar_host(nullptr, &field, pointers, count, label.data(), npar.data());
    std::printf("refused %d of 5: %s; %d failures\n", refused, gfhip_last_error(nullptr), failures);
    return failures || refused != 5;
}
