//  The first-exit rule on the host (csrc/confinement_host.hpp, what gfhip_confine_check_host runs), for a run under the
//  address and undefined-behaviour sanitizers: three checks in a row over planted particles and every edge's neighbours on
//  a planted map, psi = (R - 2)^2 + z^2, as float and as double columns, with and without weights and exit arrays, held to
//  a plain restatement: a loop per particle with a linear scan of the edges and sums of small integers in a double.
//  No device, no library.
//
//      g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I graph_framework_amd/csrc -o confinement_host_check tests/confinement_host_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "confinement_host.hpp"

using namespace gfhip;

static const double nan_value = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

static int scan_cell(const std::vector<double> &e, const double c) {
    for (size_t i = 0; i + 1 < e.size(); i++) {
        if (e[i] <= c && c < e[i + 1]) return static_cast<int> (i);
    }
    return -1;
}

static bool same_bits(const double a, const double b) {
    return std::memcmp(&a, &b, sizeof(double)) == 0;
}

struct particle {
    double x, y, z, gamma;
};

static long cases = 0, failures = 0;

static void expect(const bool holds, const char *what, const size_t s, const int check) {
    cases++;
    if (!holds) {
        std::printf("%s: particle %zu at check %d\n", what, s, check);
        failures++;
    }
}

//  Three checks of `states` (one state of all particles per check) with the type T against the restatement.
template<typename T>
static void run(const flux::map &m, const std::vector<double> &table, const double limit, const std::vector<std::vector<double>> &edges,
                const std::vector<std::vector<particle>> &states, const bool weighted, const bool with_exit, const bool with_cells) {
    const size_t count = states[0].size(), cells_per_table = table.size()/16;
    const size_t n[3] = {edges[0].size() - 1, edges[1].size() - 1, edges[2].size() - 1};
    const double *axes[3] = {edges[0].data(), edges[1].data(), edges[2].data()};
    const size_t cells = n[0]*n[1]*n[2];
    std::vector<uint32_t> lost_step(count, confine::confined), want_step(count, confine::confined);
    std::vector<T> alive(count, static_cast<T> (1)), weight(count);
    std::vector<double> exit_r(count, nan_value), exit_z(count, nan_value), want_r(count, nan_value), want_z(count, nan_value);
    std::vector<int64_t> limbs(cells*superacc::limbs, 0);
    std::vector<double> want_sum(cells, 0.0);
    uint64_t counters[3] = {0, 0, 0}, want_counters[3] = {0, 0, 0};
    for (size_t s = 0; s < count; s++) {
        weight[s] = static_cast<T> (static_cast<double> (s%7) - 3.0);          // small integers: a double sums them exactly
        if (s%31 == 5) weight[s] = static_cast<T> (nan_value);
        if (s%31 == 6) weight[s] = static_cast<T> (s%2 ? inf : -inf);
    }
    const uint32_t steps[3] = {7u, 7u, 4000000000u};
    for (int check = 0; check < 3; check++) {
        std::vector<T> x(count), y(count), z(count), gamma(count);
        for (size_t s = 0; s < count; s++) {
            x[s] = static_cast<T> (states[check][s].x);
            y[s] = static_cast<T> (states[check][s].y);
            z[s] = static_cast<T> (states[check][s].z);
            gamma[s] = static_cast<T> (states[check][s].gamma);
        }
        const void *columns[8] = {x.data(), y.data(), z.data(), nullptr, nullptr, nullptr, gamma.data(), weighted ? weight.data() : nullptr};
        uint64_t newly = 100, want_newly = 100;
        confine::check_host<T> (m, table.data(), cells_per_table, limit, axes, n, columns, count, steps[check], lost_step.data(),
                                alive.data(), with_exit ? exit_r.data() : nullptr, with_exit ? exit_z.data() : nullptr, &newly,
                                with_cells ? limbs.data() : nullptr, counters);
        for (size_t s = 0; s < count; s++) {
            const double px = static_cast<double> (x[s]), py = static_cast<double> (y[s]), pz = static_cast<double> (z[s]);
            if (want_step[s] == confine::confined) {
                const double label = confine::host_label(m, table.data(), cells_per_table, px, py, pz);
                const bool stays = label < limit;                            // a NaN label does not
                if (!stays) {
                    want_step[s] = steps[check];
                    want_newly++;
                    const double r = std::sqrt(px*px + py*py);
                    want_r[s] = r;
                    want_z[s] = pz;
                    want_counters[0]++;
                    const int ir = scan_cell(edges[0], r), iz = scan_cell(edges[1], pz), ig = scan_cell(edges[2], static_cast<double> (gamma[s]));
                    const double w = weighted ? static_cast<double> (weight[s]) : 1.0;
                    if (ir < 0 || iz < 0 || ig < 0) {
                        want_counters[1]++;
                    } else if (!std::isfinite(w)) {
                        want_counters[2]++;
                    } else {
                        want_sum[(static_cast<size_t> (ir)*n[1] + static_cast<size_t> (iz))*n[2] + static_cast<size_t> (ig)] += w;
                    }
                }
            }
            expect(lost_step[s] == want_step[s], "lost_step", s, check);
            expect(alive[s] == static_cast<T> (want_step[s] == confine::confined ? 1 : 0), "alive", s, check);
            if (with_exit) {
                expect((std::isnan(want_r[s]) ? std::isnan(exit_r[s]) : same_bits(exit_r[s], want_r[s])) &&
                       (std::isnan(want_z[s]) ? std::isnan(exit_z[s]) : same_bits(exit_z[s], want_z[s])), "exit", s, check);
            }
        }
        expect(newly == want_newly, "newly_lost", 0, check);
        if (with_cells) {
            for (size_t cell = 0; cell < cells; cell++) {
                expect(same_bits(superacc::round(limbs.data() + cell*superacc::limbs), want_sum[cell] == 0.0 ? 0.0 : want_sum[cell]), "cell", cell, check);
            }
            for (int k = 0; k < 3; k++) expect(counters[k] == want_counters[k], "counter", static_cast<size_t> (k), check);
        } else {
            for (int k = 0; k < 3; k++) expect(counters[k] == 0, "untouched counter", static_cast<size_t> (k), check);
        }
    }
    size_t confined_at_the_end = 0;
    for (size_t s = 0; s < count; s++) {
        if (want_step[s] == confine::confined) confined_at_the_end++;
    }
    expect(want_counters[0] + confined_at_the_end == count, "every particle is confined or lost once", 0, 3);
}

int main() {
    const flux::map m = {1.0, 0.25, -1.0, 0.25, 8.0, 8.0, 8ull, 0.0, 1.0, 0u};
    double c[16] = {0.0};
    c[0] = 2.0;                                         // c[a][b] at c[4*a + b]: psi = 2 - tr/2 + tr^2/16 - tz/2 + tz^2/16
    c[4] = -0.5;
    c[8] = 0.0625;
    c[1] = -0.5;
    c[2] = 0.0625;
    std::vector<double> table(16*64);                   // [k][table cell]: every cell holds the same polynomial
    for (size_t k = 0; k < 16; k++) {
        for (size_t cell = 0; cell < 64; cell++) table[k*64 + cell] = c[k];
    }
    const std::vector<std::vector<double>> edges = {{1.0, 1.5, 2.0, 2.5, 3.0}, {-1.0, -0.999, -0.5, 0.0, 1.0e-300, 0.75, 1.0},
                                                    {1.0, 1.5, 2.0, 2.5, 3.0}};

//  The planted particles: on the axis; R < rmin; a NaN, +inf and -inf in x, y and z in turn; one whose label is the
//  limit, and its neighbours in z, 40 units either way.
    const particle axis = {2.0, 0.0, 0.0, 1.8}, rim = {2.5, 0.125, 0.25, 1.8};
    const double limit = confine::host_label(m, table.data(), 64, rim.x, rim.y, rim.z);
    if (!(limit > 0.2 && limit < 0.4)) return 2;
    std::vector<particle> first = {axis, {0.5, 0.0, 0.0, 1.8}};
    for (int column = 0; column < 3; column++) {
        for (const double value : {nan_value, inf, -inf}) {
            particle p = axis;
            (column == 0 ? p.x : column == 1 ? p.y : p.z) = value;
            first.push_back(p);
        }
    }
    first.push_back(rim);
    double up = rim.z, down = rim.z;
    for (int k = 0; k < 40; k++) {
        up = std::nextafter(up, inf);
        down = std::nextafter(down, -inf);
        first.push_back({rim.x, rim.y, up, 1.8});
        first.push_back({rim.x, rim.y, down, 1.8});
    }
//  Every edge of every axis, its neighbours and beyond, off the plasma so that they deposit (label >= limit).
    for (const double edge : edges[0]) {
        for (const double r : {edge, std::nextafter(edge, -inf), std::nextafter(edge, inf), edge - 0.1, edge + 0.1}) {
            first.push_back({r, 0.0, 0.9, 1.25});
            first.push_back({0.0, -r, 0.9, 2.75});
        }
    }
    for (const double edge : edges[1]) {
        for (const double z : {edge, std::nextafter(edge, -inf), std::nextafter(edge, inf), edge - 0.1, edge + 0.1}) {
            first.push_back({2.9, 0.0, z, 1.25});
        }
    }
    for (const double edge : edges[2]) {
        for (const double gamma : {edge, std::nextafter(edge, -inf), std::nextafter(edge, inf), edge - 0.1, edge + 0.1, nan_value, inf}) {
            first.push_back({2.9, 0.0, 0.5, gamma});
        }
    }
    for (int i = 0; i < 12; i++) {                      // a coarse sweep of the map and beyond
        for (int j = 0; j < 12; j++) first.push_back({0.9 + 0.2*i, 0.01*j, -1.15 + 0.2*j, 1.0 + 0.17*(i + j)});
    }
//  Check 2: everybody on the axis but every third, who stays where he was; check 3: every second off the map.
    std::vector<particle> second = first, third = first;
    for (size_t s = 0; s < first.size(); s++) {
        if (s%3) second[s] = axis;
        third[s] = s%2 ? particle{3.5, 0.0, 0.0, 2.2} : axis;
    }
    second[1] = axis;                                   // the one below rmin is inside at checks 2 and 3
    third[1] = axis;
    const std::vector<std::vector<particle>> states = {first, second, third};
    for (const bool weighted : {false, true}) {
        for (const bool with_exit : {false, true}) {
            for (const bool with_cells : {false, true}) {
                run<double> (m, table, limit, edges, states, weighted, with_exit, with_cells);
                run<float> (m, table, limit, edges, states, weighted, with_exit, with_cells);
            }
        }
    }
    run<double> (m, table, -inf, edges, states, true, true, true);          // nobody stays
    run<double> (m, table, inf, edges, states, true, true, true);           // only a NaN label leaves
    std::printf("%zu particles\ncases %ld failures %ld\n", first.size(), cases, failures);
    return failures != 0;
}
