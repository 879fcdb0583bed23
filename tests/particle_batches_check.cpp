//  The plain C++ pieces of the batches of particles, for a run under the address and undefined-behaviour sanitizers:
//  moments_host.hpp's and phase_host.hpp's add_particles_host on the planted map of moments_host_check.cpp,
//  psi = (R - 2)^2 + z^2 and fpol = 2 + tp/8 over 4 intervals, as float and as double columns, with and without weights,
//  over G in {1, 2, 3, 16, 64}, n in {1, 63, 64, 65, 64G - 1, 64G, 64G + 1, 4099} and first in {0, 1, 63, 65, 2^40 + 5},
//  held to a plain restatement: per batch a linear scan over all particles for those whose index says so, the cell by a
//  linear scan of the edges, the sums by long double additions of the values the headers themselves hand out.  No
//  device, no library.
//
//      g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I graph_framework_amd/csrc -o particle_batches_check tests/particle_batches_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <vector>

#include "moments_host.hpp"
#include "phase_host.hpp"

using namespace gfhip;

static int scan_cell(const std::vector<double> &e, const double c) {
    for (size_t i = 0; i + 1 < e.size(); i++) {
        if (e[i] <= c && c < e[i + 1]) return static_cast<int> (i);
    }
    return -1;
}

static long cases = 0, failures = 0;

static void expect(const bool ok, const char *what, const size_t at) {
    cases++;
    if (!ok) {
        std::printf("%s fails at %zu\n", what, at);
        failures++;
    }
}

static bool sums_agree(const int64_t *limbs, const long double want, const size_t n) {
    const double got = superacc::round(limbs);
    const double scale = std::fabs(static_cast<double> (want)) + 1.0e-3;
    return std::fabs(got - static_cast<double> (want)) <= 1.0e-9*scale*static_cast<double> (n);
}

struct axes_of {
    std::vector<double> label, pitch, gamma;
};

template<typename T>
static void run(const flux::map &m, const flux::field &f, const moments::host_tables &t, const std::vector<double> &surfaces,
                const axes_of &axes, const std::vector<std::vector<double>> &rows, const size_t n, const unsigned int batch_count,
                const uint64_t first, const bool weighted) {
    std::vector<std::vector<T>> typed(8, std::vector<T> (n));
    for (size_t s = 0; s < n; s++) {
        for (size_t k = 0; k < 8; k++) typed[k][s] = static_cast<T> (rows[s][k]);
    }
    const void *columns[8];
    for (size_t k = 0; k < 8; k++) columns[k] = typed[k].data();
    if (!weighted) columns[7] = nullptr;
    std::vector<double> label(n), values(4*n);
    moments::values_host<T> (m, f, t, columns, n, label.data(), values.data());

//  The moments: two adds in a row into the same limbs, cut at an odd place.
    const size_t ns = surfaces.size() - 1, cut = n/3;
    std::vector<int64_t> limbs(static_cast<size_t> (batch_count)*ns*4*superacc::limbs, 0);
    uint64_t counters[3] = {0, 0, 0};
    const void *later[8];
    for (size_t k = 0; k < 8; k++) later[k] = columns[k] ? static_cast<const T *> (columns[k]) + cut : nullptr;
    moments::add_particles_host<T> (m, f, t, surfaces.data(), ns, batch_count, first, columns, cut, limbs.data(), counters);
    moments::add_particles_host<T> (m, f, t, surfaces.data(), ns, batch_count, first + cut, later, n - cut, limbs.data(), counters);
    uint64_t outside = 0, skipped = 0;
    for (unsigned int g = 0; g < batch_count; g++) {
        std::vector<long double> want(ns*4, 0.0L);
        for (size_t s = 0; s < n; s++) {
            if (((first + s)/64)%batch_count != g) continue;
            const int is = scan_cell(surfaces, label[s]);
            if (is < 0) {
                outside++;
                continue;
            }
            const double w = weighted ? static_cast<double> (typed[7][s]) : 1.0;
            const double *v = values.data() + 4*s;
            const double d[4] = {w, w*v[1], w*v[2], w*v[3]};
            if (!(std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) && std::isfinite(d[3]))) {
                skipped++;
                continue;
            }
            for (size_t k = 0; k < 4; k++) want[static_cast<size_t> (is)*4 + k] += d[k];
        }
        bool agree = true;
        for (size_t cell = 0; cell < ns*4; cell++) {
            agree = agree && sums_agree(limbs.data() + (static_cast<size_t> (g)*ns*4 + cell)*superacc::limbs, want[cell], n);
        }
        expect(agree, "moment sums of a batch", g);
    }
    expect(counters[0] == n && counters[1] == outside && counters[2] == skipped, "moment counters", n);

//  The distribution.
    const size_t shape[3] = {axes.label.size() - 1, axes.pitch.size() - 1, axes.gamma.size() - 1};
    const size_t cells = shape[0]*shape[1]*shape[2];
    const double *edges[3] = {axes.label.data(), axes.pitch.data(), axes.gamma.data()};
    std::vector<int64_t> grid(static_cast<size_t> (batch_count)*cells*superacc::limbs, 0);
    uint64_t seen[3] = {0, 0, 0};
    phase::add_particles_host<T> (m, f, t, edges, shape, batch_count, first, columns, cut, grid.data(), seen);
    phase::add_particles_host<T> (m, f, t, edges, shape, batch_count, first + cut, later, n - cut, grid.data(), seen);
    outside = skipped = 0;
    for (unsigned int g = 0; g < batch_count; g++) {
        std::vector<long double> want(cells, 0.0L);
        for (size_t s = 0; s < n; s++) {
            if (((first + s)/64)%batch_count != g) continue;
            double s_label, xi;
            phase::host_point(m, f, t, typed[0][s], typed[1][s], typed[2][s], typed[3][s], typed[4][s], typed[5][s], s_label, xi);
            const int is = scan_cell(axes.label, s_label), ip = scan_cell(axes.pitch, xi);
            const int ig = scan_cell(axes.gamma, static_cast<double> (typed[6][s]));
            if (is < 0 || ip < 0 || ig < 0) {
                outside++;
                continue;
            }
            const double w = weighted ? static_cast<double> (typed[7][s]) : 1.0;
            if (!std::isfinite(w)) {
                skipped++;
                continue;
            }
            want[(static_cast<size_t> (is)*shape[1] + static_cast<size_t> (ip))*shape[2] + static_cast<size_t> (ig)] += w;
        }
        bool agree = true;
        for (size_t cell = 0; cell < cells; cell++) {
            agree = agree && sums_agree(grid.data() + (static_cast<size_t> (g)*cells + cell)*superacc::limbs, want[cell], n);
        }
        expect(agree, "distribution sums of a batch", g);
    }
    expect(seen[0] == n && seen[1] == outside && seen[2] == skipped, "distribution counters", n);
}

int main() {
    flux::map m = {1.0, 0.25, -1.0, 0.25, 8.0, 8.0, 8ull, 0.0, 1.0, 0u};
    flux::field f = {0.25, 0.25, 4.0, 3, 1.0};
//  Every table cell holds the same polynomial, c[a][b] at [4*a + b]: psi = 2 - tr/2 + tr^2/16 - tz/2 + tz^2/16.
    const size_t table = 64;
    std::vector<double> coefficients(16*table, 0.0), fpol[4];
    for (size_t at = 0; at < table; at++) {
        coefficients[0*table + at] = 2.0;
        coefficients[4*table + at] = -0.5;
        coefficients[8*table + at] = 0.0625;
        coefficients[1*table + at] = -0.5;
        coefficients[2*table + at] = 0.0625;
    }
    for (size_t k = 0; k < 4; k++) fpol[k].assign(4, k == 0 ? 2.0 : k == 1 ? 0.125 : 0.0);
    const moments::host_tables t = {coefficients.data(), table, {fpol[0].data(), fpol[1].data(), fpol[2].data(), fpol[3].data()}};

    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const std::vector<double> three = {0.0, 0.015625, 0.25, 0.75};
    std::vector<double> uniform;
    for (int i = 0; i <= 64; i++) uniform.push_back(0.015625*i);
    const axes_of axes = {three, {-1.0, 0.0, std::nextafter(1.0, 2.0)}, {1.0, 2.0, 50.0}};

//  x, y, z, ux, uy, uz, gamma, weight: 4099 particles all over the map and a little beyond it, a sixth of them off it;
//  gamma = 0, NaN and infinite weights, zero and negative weights planted among them.
    const size_t most = 4099;
    std::vector<std::vector<double>> rows;
    for (size_t s = 0; s < most; s++) {
        const double radius = 0.9 + 2.3*std::fmod(0.61803398875*static_cast<double> (s), 1.0);
        const double z = -1.1 + 2.2*std::fmod(0.41421356237*static_cast<double> (s), 1.0), angle = 0.1*static_cast<double> (s);
        const double ux = 3.0*std::sin(1.7*static_cast<double> (s)), uy = 2.0*std::cos(0.3*static_cast<double> (s)), uz = -0.7 + 0.001*static_cast<double> (s);
        double gamma = std::sqrt(1.0 + ux*ux + uy*uy + uz*uz), weight = 1.0 + 0.25*static_cast<double> (s % 7) - 1.5*static_cast<double> (s % 3 == 0);
        if (s % 97 == 5) gamma = 0.0;
        if (s % 101 == 7) weight = nan;
        if (s % 103 == 9) weight = s % 2 ? inf : -inf;
        if (s % 53 == 11) weight = s % 2 ? 0.0 : -0.0;
        rows.push_back({radius*std::cos(angle), radius*std::sin(angle), z, ux, uy, uz, gamma, weight});
    }

    const uint64_t firsts[5] = {0, 1, 63, 65, (1ull << 40) + 5};
    for (const unsigned int batch_count : {1u, 2u, 3u, 16u, 64u}) {
        const std::set<size_t> sizes = {1, 63, 64, 65, 64u*batch_count - 1, 64u*batch_count, 64u*batch_count + 1, most};
        size_t turn = batch_count;
        for (const size_t n : sizes) {
            for (const uint64_t first : firsts) {
//  Every size meets every first; the two label axes, the types and the weights take turns, and the largest size all.
                for (int variant = 0; variant < 8; variant++) {
                    if (n != most && static_cast<size_t> (variant) != turn % 8) continue;
                    const std::vector<double> &surfaces = variant & 1 ? uniform : three;
                    if (variant & 2) {
                        run<float> (m, f, t, surfaces, axes, rows, n, batch_count, first, (variant & 4) != 0);
                    } else {
                        run<double> (m, f, t, surfaces, axes, rows, n, batch_count, first, (variant & 4) != 0);
                    }
                }
                turn++;
            }
        }
    }
    std::printf("cases %ld failures %ld\n", cases, failures);
    return failures != 0;
}
