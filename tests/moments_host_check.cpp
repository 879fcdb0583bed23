//  The plain C++ pieces of the moment profile, for a run under the address and undefined-behaviour sanitizers:
//  moments_host.hpp's values_host and add_host (flux_label.hpp's moments_of behind them) on a planted map,
//  psi = (R - 2)^2 + z^2 and fpol = 2 + tp/8 over 4 intervals, as float and as double columns, with and without weights,
//  held to a plain restatement: the moments from the analytic field within a tolerance, the surface by a linear scan of
//  the edges, the sums by long double additions of the values the header itself hands out.  No device, no library.
//
//      g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I graph_framework_amd/csrc -o moments_host_check tests/moments_host_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "moments_host.hpp"

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

static bool close_to(const double got, const double want, const double scale) {
    return std::fabs(got - want) <= 1.0e-12*scale;
}

template<typename T>
static void run(const flux::map &m, const flux::field &f, const moments::host_tables &t, const std::vector<double> &edges,
                const std::vector<std::vector<double>> &rows, const bool weighted) {
    const size_t n = rows.size(), ns = edges.size() - 1;
    std::vector<std::vector<T>> typed(8, std::vector<T> (n));
    for (size_t s = 0; s < n; s++) {
        for (size_t k = 0; k < 8; k++) typed[k][s] = static_cast<T> (rows[s][k]);
    }
    const void *columns[8];
    for (size_t k = 0; k < 8; k++) columns[k] = typed[k].data();
    if (!weighted) columns[7] = nullptr;
    std::vector<double> label(n), values(4*n);
    moments::values_host<T> (m, f, t, columns, n, label.data(), values.data());

    std::vector<long double> want(ns*4, 0.0L);
    uint64_t outside = 0, skipped = 0;
    for (size_t s = 0; s < n; s++) {
        const double x = typed[0][s], y = typed[1][s], z = typed[2][s], ux = typed[3][s], uy = typed[4][s], uz = typed[5][s],
                     gamma = typed[6][s];
        const double r = std::sqrt(x*x + y*y);
        const bool on_map = r >= 1.0 && r < 3.0 && z >= -1.0 && z < 1.0;
        const double *v = values.data() + 4*s;
        if (!on_map) {
            expect(std::isnan(label[s]) && std::isnan(v[0]) && std::isnan(v[1]) && std::isnan(v[2]) && std::isnan(v[3]), "off the map", s);
        } else {
//  The analytic field: psi_R = 2 (R - 2), psi_z = 2 z, fpol = 2 + tp/8 with tp = (psi - 1/4)*4: R B = (psi_z, fpol, -psi_R).
            const double psi = (r - 2.0)*(r - 2.0) + z*z, br = 2.0*z, bz = -2.0*(r - 2.0), bp = 2.0 + (psi - 0.25)*4.0/8.0;
            const double size = std::sqrt(br*br + bp*bp + bz*bz);
            const double ur = (ux*x + uy*y)/r, up = (uy*x - ux*y)/r;
            const double upar = (ur*br + up*bp + uz*bz)/size, uu = ux*ux + uy*uy + uz*uz;
            const double perp = uu - upar*upar, bsq = size*size/(r*r);
            expect(close_to(label[s], psi, 1.0 + std::fabs(psi)), "label", s);
            expect(v[0] == 1.0, "density", s);
            if (std::isfinite(upar) && std::isfinite(gamma) && gamma != 0.0) expect(close_to(v[1], upar/gamma, 1.0 + std::fabs(upar/gamma)), "current", s);
            if (std::isfinite(gamma)) expect(v[2] == gamma - 1.0, "energy", s);
            if (std::isfinite(uu)) {
                expect(close_to(v[3], perp > 0.0 ? perp*bsq : 0.0, (1.0 + uu)*bsq), "radiation", s);
                expect(v[3] >= 0.0 && !std::signbit(v[3]), "radiation is not negative", s);
            }
        }
        const int is = scan_cell(edges, label[s]);
        if (is < 0) {
            outside++;
            continue;
        }
        const double w = weighted ? static_cast<double> (typed[7][s]) : 1.0;
        const double d[4] = {w, w*v[1], w*v[2], w*v[3]};
        if (!(std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]) && std::isfinite(d[3]))) {
            skipped++;
            continue;
        }
        for (size_t k = 0; k < 4; k++) want[static_cast<size_t> (is)*4 + k] += d[k];
    }

//  Three adds in a row into the same limbs, the middle one empty.
    std::vector<int64_t> limbs(ns*4*superacc::limbs, 0);
    uint64_t counters[3] = {0, 0, 0};
    const size_t cut = n/3;
    const void *later[8];
    for (size_t k = 0; k < 8; k++) later[k] = columns[k] ? static_cast<const T *> (columns[k]) + cut : nullptr;
    moments::add_host<T> (m, f, t, edges.data(), ns, columns, cut, limbs.data(), counters);
    moments::add_host<T> (m, f, t, edges.data(), ns, later, 0, limbs.data(), counters);
    moments::add_host<T> (m, f, t, edges.data(), ns, later, n - cut, limbs.data(), counters);
    expect(counters[0] == n && counters[1] == outside && counters[2] == skipped, "counters", n);
    for (size_t cell = 0; cell < ns*4; cell++) {
        const double got = superacc::round(limbs.data() + cell*superacc::limbs);
        const double scale = std::fabs(static_cast<double> (want[cell])) + 1.0e-3;
        expect(std::fabs(got - static_cast<double> (want[cell])) <= 1.0e-9*scale*static_cast<double> (n), "sum", cell);
    }
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
    const std::vector<double> uneven = {0.0, 0.015625, 0.25, 0.5, 0.75, 1.5, 2.0};
    std::vector<double> uniform;
    for (int i = 0; i <= 64; i++) uniform.push_back(0.03125*i);
    const std::vector<double> *axes[2] = {&uneven, &uniform};

//  x, y, z, ux, uy, uz, gamma, weight: a good particle; u = 0; gamma = 0 and inf; every column in turn NaN, +inf, -inf;
//  weights that are zero, negative, NaN and infinite.
    const double good[8] = {2.5, 0.3, 0.25, 0.4, -1.25, 0.75, 1.8, 2.5};
    std::vector<std::vector<double>> rows = {{good, good + 8}};
    rows.push_back({good, good + 8});
    rows.back()[3] = rows.back()[4] = rows.back()[5] = 0.0;
    for (const double gamma : {0.0, inf}) {
        rows.push_back({good, good + 8});
        rows.back()[6] = gamma;
    }
    for (int column = 0; column < 8; column++) {
        for (const double value : {nan, inf, -inf}) {
            rows.push_back({good, good + 8});
            rows.back()[column] = value;
        }
    }
    for (const double weight : {0.0, -0.0, -3.0, 1.0e-300, 1.0e300}) {
        rows.push_back({good, good + 8});
        rows.back()[7] = weight;
    }
//  Every edge's neighbours: psi = (R - 2)^2 on z = 0, so R = 2 + sqrt(edge) lies on the edge up to rounding, and its
//  neighbours in R on either side of it.
    for (const std::vector<double> *edges : axes) {
        for (const double edge : *edges) {
            const double at = 2.0 + std::sqrt(edge);
            for (const double radius : {at, std::nextafter(at, 0.0), std::nextafter(at, 9.0), at - 1.0e-9, at + 1.0e-9, 4.0 - at}) {
                rows.push_back({good, good + 8});
                rows.back()[0] = radius;
                rows.back()[1] = 0.0;
                rows.back()[2] = 0.0;
            }
        }
    }
//  u = +-t B all over the map, where uu - upup cancels, and a general u beside it.
    for (int i = 0; i < 24; i++) {
        for (int j = 0; j < 24; j++) {
            const double radius = 1.0 + 2.0*(i + 0.37)/24.0, z = -1.0 + 2.0*(j + 0.61)/24.0, angle = 0.1*(i*24 + j);
            const double x = radius*std::cos(angle), y = radius*std::sin(angle);
            const double psi = (radius - 2.0)*(radius - 2.0) + z*z, br = 2.0*z, bz = -2.0*(radius - 2.0), bp = 2.0 + (psi - 0.25)*0.5;
            for (const double scale : {0.37, -11.0}) {
                const double ur = scale*br, up = scale*bp, uz = scale*bz;
                const double ux = (ur*x - up*y)/radius, uy = (ur*y + up*x)/radius;
                rows.push_back({x, y, z, ux, uy, uz, std::sqrt(1.0 + ux*ux + uy*uy + uz*uz), 0.5*scale});
            }
            rows.push_back({x, y, z, 0.3*i - 2.0, 0.1*j, -0.7, 1.0 + 0.05*(i + j), 1.0 + i});
        }
    }

    for (const std::vector<double> *edges : axes) {
        for (const bool weighted : {false, true}) {
            run<double> (m, f, t, *edges, rows, weighted);
            run<float> (m, f, t, *edges, rows, weighted);
        }
    }
    std::printf("cases %ld failures %ld\n", cases, failures);
    return failures != 0;
}
