//  The plain C++ pieces of the particle distribution, for a run under the address and undefined-behaviour sanitizers:
//  flux_label.hpp's pitch_of (with locate, psi_gradient, fpol_interval and fpol_of in front of it) on a planted map,
//  psi = (R - 2)^2 + z^2 and fpol = 2 + tp/8 over 4 intervals, and a host cell finder that follows cell_deposit.hpp's
//  find_cell line by line, held to a linear scan of the edges.  No device, no library.
//
//      g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I graph_framework_amd/csrc -o phase_host_check tests/phase_host_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "flux_label.hpp"

using namespace gfhip;

//  cell_deposit.hpp's find_cell on the host.
static int find_cell(const double *e, const int n, const double scale, const double c) {
    if (!(c >= e[0] && c < e[n])) return -1;
    const double t = (c - e[0])*scale;
    int g = t >= 0.0 && t < static_cast<double> (n) ? static_cast<int> (t) : 0;
    if (c >= e[g] && c < e[g + 1]) return g;
    if (g + 1 < n && c >= e[g + 1] && c < e[g + 2]) return g + 1;
    if (g > 0 && c >= e[g - 1] && c < e[g]) return g - 1;
    int low = 0, high = n;
    while (high - low > 1) {
        const int middle = (low + high)/2;
        if (c >= e[middle]) {
            low = middle;
        } else {
            high = middle;
        }
    }
    return low;
}

static int scan_cell(const std::vector<double> &e, const double c) {
    for (size_t i = 0; i + 1 < e.size(); i++) {
        if (e[i] <= c && c < e[i + 1]) return static_cast<int> (i);
    }
    return -1;
}

struct planted_map {
    flux::map m;
    flux::field f;
    double c[16], cubic[4];
};

//  The label and xi of a particle as gf_hip.cpp's host entry point forms them.
static void coordinates(const planted_map &p, const double x, const double y, const double z, const double ux, const double uy,
                        const double uz, double &label, double &xi) {
    double tr, tz, tp, gr, gz;
    if (flux::locate(p.m, x, y, z, tr, tz) < 0) {
        label = xi = std::numeric_limits<double>::quiet_NaN();
        return;
    }
    const double psi = flux::psi_gradient(p.m, p.c, tr, tz, gr, gz);          // every table cell holds the same polynomial
    label = flux::canonical(flux::label_of(p.m, psi));
    const int q = flux::fpol_interval(p.f, psi, tp);
    if (q < 0 || q > p.f.last) std::abort();
    xi = flux::pitch_of(x, y, flux::radius_of(x, y), ux, uy, uz, gr, gz, flux::fpol_of(p.cubic, tp));
}

int main() {
    planted_map p = {};
    p.m = {1.0, 0.25, -1.0, 0.25, 8.0, 8.0, 8ull, 0.0, 1.0, 0u};
    p.f = {0.25, 0.25, 4.0, 3, 1.0};
    p.c[0] = 2.0;                                       // c[a][b] at c[4*a + b]: psi = 2 - tr/2 + tr^2/16 - tz/2 + tz^2/16
    p.c[4] = -0.5;
    p.c[8] = 0.0625;
    p.c[1] = -0.5;
    p.c[2] = 0.0625;
    p.cubic[0] = 2.0;
    p.cubic[1] = 0.125;

    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    std::vector<double> pedges;                         // distribution.pitch_edges(8)
    for (int i = 0; i <= 8; i++) pedges.push_back(-1.0 + 0.25*i);
    pedges[8] = std::nextafter(1.0, 2.0);
    const std::vector<double> gedges = {1.0, 1.5, 2.0, 2.5, 3.0};
    const std::vector<double> uneven = {-1.0, -0.999, -0.5, 0.0, 1.0e-300, 0.75, 1.0};
    long cases = 0, failures = 0;

    auto finder_agrees = [&](const std::vector<double> &e, const double c) {
        const int n = static_cast<int> (e.size()) - 1;
        cases++;
        if (find_cell(e.data(), n, static_cast<double> (n)/(e[n] - e[0]), c) != scan_cell(e, c)) {
            std::printf("find_cell(%a) disagrees with the scan\n", c);
            failures++;
        }
    };

//  The planted particles of tests/test_phase.py: a good one; u = 0; every column in turn NaN, +inf, -inf; gamma on edges.
    const double good[7] = {2.5, 0.3, 0.25, 0.4, -1.25, 0.75, 1.8};
    std::vector<std::vector<double>> rows = {{good, good + 7}};
    rows.push_back({good, good + 7});
    rows.back()[3] = rows.back()[4] = rows.back()[5] = 0.0;
    for (int column = 0; column < 7; column++) {
        for (const double value : {nan, inf, -inf}) {
            rows.push_back({good, good + 7});
            rows.back()[column] = value;
        }
    }
    for (const double gamma : {1.0, 2.0, 3.0}) {
        rows.push_back({good, good + 7});
        rows.back()[6] = gamma;
    }
    double first_xi = 0.0;
    for (size_t s = 0; s < rows.size(); s++) {
        const std::vector<double> &r = rows[s];
        double label, xi;
        coordinates(p, r[0], r[1], r[2], r[3], r[4], r[5], label, xi);
        if (s == 0) first_xi = xi;
        cases++;
        const bool position_bad = s >= 2 && s < 11, momentum_bad = s == 1 || (s >= 11 && s < 20);
        if (position_bad ? !(std::isnan(label) && std::isnan(xi)) : !std::isfinite(label)) failures++;
        if (momentum_bad && !std::isnan(xi)) failures++;
        if (!position_bad && !momentum_bad && !(xi == first_xi && std::fabs(xi) < 1.0)) failures++;
        finder_agrees(pedges, xi);
        finder_agrees(gedges, r[6]);
        finder_agrees(uneven, xi);
    }
    if (scan_cell(gedges, 1.0) != 0 || scan_cell(gedges, 2.0) != 2 || scan_cell(gedges, 3.0) != -1) failures++;

//  u = +-t B all over the map: R B = (gZ, fpol, -gR).  The clamp holds xi within [-1, 1], in the last or the first cell.
    long above = 0;
    for (int i = 0; i < 40; i++) {
        for (int j = 0; j < 40; j++) {
            const double radius = 1.0 + 2.0*(i + 0.37)/40.0, z = -1.0 + 2.0*(j + 0.61)/40.0, angle = 0.1*(i*40 + j);
            const double x = radius*std::cos(angle), y = radius*std::sin(angle);
            double tr, tz, tp, gr, gz;
            if (flux::locate(p.m, x, y, z, tr, tz) < 0) continue;
            const double psi = flux::psi_gradient(p.m, p.c, tr, tz, gr, gz);
            flux::fpol_interval(p.f, psi, tp);
            const double fpol = flux::fpol_of(p.cubic, tp), r = flux::radius_of(x, y);
            for (const double t : {0.37, -0.37, 11.0, -1.0e3}) {
                const double ur = t*gz, up = t*fpol, uz = -t*gr;
                double label, xi;
                coordinates(p, x, y, z, (ur*x - up*y)/r, (ur*y + up*x)/r, uz, label, xi);
                cases++;
                if (!(std::fabs(xi) <= 1.0 && std::fabs(xi) > 1.0 - 1.0e-12 && (xi > 0.0) == (t > 0.0))) failures++;
                if (std::fabs(xi) == 1.0) above++;
                if (find_cell(pedges.data(), 8, 8.0/(pedges[8] - pedges[0]), xi) != (t > 0.0 ? 7 : 0)) failures++;
                finder_agrees(uneven, xi);
            }
        }
    }
//  The finder on every edge, its neighbours and beyond.
    const std::vector<double> *axes[3] = {&pedges, &gedges, &uneven};
    for (const std::vector<double> *e : axes) {
        for (const double edge : *e) {
            for (const double c : {edge, std::nextafter(edge, -inf), std::nextafter(edge, inf), edge - 0.1, edge + 0.1}) finder_agrees(*e, c);
        }
        for (const double c : {nan, inf, -inf, 0.0, -0.0, 1.0e300, -1.0e300}) finder_agrees(*e, c);
    }
    std::printf("%ld particles reached |xi| = 1 exactly\ncases %ld failures %ld\n", above, cases, failures);
    return failures != 0;
}
