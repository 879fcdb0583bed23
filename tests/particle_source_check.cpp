//  source_host.hpp on its own under the sanitizers: an analytic map (psi = (R - 1.7)^2 + z^2 as exact bicubic cells, fpol
//  constant), fills of fp32 and fp64 columns with and without a profile, counts around a wave and particle indices whose
//  low word wraps, against a plain restatement of what a fill promises: the known answers of the generator; placed +
//  unplaced = count; a placed particle's stored position has its label in the range (recomputed here from the analytic
//  psi), finite columns and |u| in the speed range; an unplaced one is all NaN with placed = 0; two shards are one fill.
//  Prints "cases N failures M".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "source_host.hpp"

using namespace gfhip;

namespace {

long cases = 0, failures = 0;

void expect(const bool ok, const char *what) {
    cases++;
    if (!ok) {
        failures++;
        if (failures < 20) std::printf("FAILED: %s\n", what);
    }
}

constexpr size_t numr = 24, numz = 32;
constexpr double rmin = 1.0, dr = 0.0625, zmin = -1.0, dz = 0.0625, axis = 1.7;

//  psi = (rmin + dr*tr - axis)^2 + (zmin + dz*tz)^2 in the global normalised coordinates: c[a][b] multiplies tr^a tz^b.
std::vector<double> coefficients() {
    std::vector<double> c(16*numr*numz, 0.0);
    const size_t table = numr*numz;
    for (size_t at = 0; at < table; at++) {
        c[0*table + at] = (rmin - axis)*(rmin - axis) + zmin*zmin;        // c00
        c[1*table + at] = 2.0*zmin*dz;                                     // c01
        c[2*table + at] = dz*dz;                                           // c02
        c[4*table + at] = 2.0*(rmin - axis)*dr;                            // c10
        c[8*table + at] = dr*dr;                                           // c20
    }
    return c;
}

template<typename T>
struct filled {
    std::vector<T> column[8];
    uint64_t counters[4] = {0, 0, 0, 0};
};

template<typename T>
filled<T> fill(const flux::map &m, const flux::field &f, const draw::parameters &par, const draw::host_tables &tables,
               const uint64_t first, const size_t count, const bool with_placed) {
    filled<T> out;
    void *pointers[8];
    for (int k = 0; k < 8; k++) {
        out.column[k].assign(count, static_cast<T> (7));
        pointers[k] = out.column[k].data();
    }
    draw::fill_host<T> (m, f, par, tables, pointers, with_placed ? pointers[7] : nullptr, first, count, out.counters);
    return out;
}

template<typename T>
void check(const char *kind, const bool with_profile) {
    const std::vector<double> c = coefficients();
    const std::vector<double> fpol[4] = {std::vector<double> (8, 2.5), std::vector<double> (8, 0.0), std::vector<double> (8, 0.0),
                                         std::vector<double> (8, 0.0)};
    const flux::map m = {rmin, dr, zmin, dz, static_cast<double> (numr), static_cast<double> (numz), numz, 0.0, 0.25, 0u};
    const flux::field f = {0.0, 0.05, 8.0, 7, 1.0};
    const double sedges[4] = {0.1, 0.3, 0.5, 0.8}, accept[3] = {1.0, 0.0, 0.5};
    const double box[4] = {1.05, 2.4, -0.9, 0.9};
    const double slo = 0.05, shi = 0.9, blo = 0.2, bhi = 0.95;
    const draw::host_tables tables = {c.data(), numr*numz, {fpol[0].data(), fpol[1].data(), fpol[2].data(), fpol[3].data()},
                                      with_profile ? sedges : nullptr, with_profile ? accept : nullptr, with_profile ? 3u : 0u};
    const size_t counts[] = {1, 63, 64, 65, 257, 600};
    const uint64_t firsts[] = {0, 1, 0xfffffffdull, 1ull << 40};
    const uint32_t attempts[] = {1, 2, 64};
    int turn = 0;
    for (const size_t count : counts) {
        for (const uint64_t first : firsts) {
            const uint32_t tries = attempts[turn++ % 3];
            const draw::parameters par = draw::parameters_of(box, slo, shi, blo, bhi, -1.0, 1.0, 0x1234567887654321ull + turn, tries,
                                                             with_profile ? 3 : 0);
            const filled<T> whole = fill<T> (m, f, par, tables, first, count, true);
            expect(whole.counters[0] + whole.counters[1] == count, "placed + unplaced = count");
            expect(whole.counters[2] <= static_cast<uint64_t> (count)*tries && whole.counters[3] <= static_cast<uint64_t> (count)*tries,
                   "no more tries than attempts");
            uint64_t placed = 0;
            for (size_t s = 0; s < count; s++) {
                const T *v[8];
                for (int k = 0; k < 8; k++) v[k] = &whole.column[k][s];
                if (*v[7] == static_cast<T> (1)) {
                    placed++;
                    const double x = *v[0], y = *v[1], z = *v[2], r = std::sqrt(x*x + y*y);
                    const double label = ((r - axis)*(r - axis) + z*z)/0.25;
                    expect(label > slo - 1.0e-6 && label < shi + 1.0e-6, "a placed particle lies in the label range");
                    expect(!with_profile || (label > 0.1 - 1.0e-6 && label < 0.8 + 1.0e-6 && !(label > 0.3 + 1.0e-6 && label < 0.5 - 1.0e-6)),
                           "a placed particle lies in a cell of the profile that accepts");
                    const double size = std::sqrt(double(*v[3])*double(*v[3]) + double(*v[4])*double(*v[4]) + double(*v[5])*double(*v[5]));
                    expect(size > blo - 1.0e-6 && size < bhi + 1.0e-6 && *v[6] == static_cast<T> (0), "the speed is in its range, gamma is 0");
                } else {
                    bool all_nan = *v[7] == static_cast<T> (0);
                    for (int k = 0; k < 7; k++) all_nan = all_nan && *v[k] != *v[k];
                    expect(all_nan, "an unplaced particle is all NaN with placed = 0");
                }
            }
            expect(placed == whole.counters[0], "the placed column sums to the counter");
//  two shards, and no placed column: the same bytes, the eighth array untouched
            const size_t cut = count/3;
            const filled<T> low = fill<T> (m, f, par, tables, first, cut, false);
            const filled<T> high = fill<T> (m, f, par, tables, first + cut, count - cut, false);
            bool same = true;
            for (int k = 0; k < 7; k++) {
                same = same && (cut == 0 || !std::memcmp(low.column[k].data(), whole.column[k].data(), cut*sizeof(T)));
                same = same && !std::memcmp(high.column[k].data(), whole.column[k].data() + cut, (count - cut)*sizeof(T));
            }
            for (int k = 0; k < 4; k++) same = same && low.counters[k] + high.counters[k] == whole.counters[k];
            for (const T value : high.column[7]) same = same && value == static_cast<T> (7);
            expect(same, "two shards are one fill");
        }
    }
    std::printf("%s%s done\n", kind, with_profile ? " with a profile" : "");
}

}  // namespace

int main() {
    const uint32_t counter[3][4] = {{0, 0, 0, 0}, {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                    {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}};
    const uint32_t key[3][2] = {{0, 0}, {0xffffffffu, 0xffffffffu}, {0xa4093822u, 0x299f31d0u}};
    const uint32_t answer[3][4] = {{0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
                                   {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
    for (int k = 0; k < 3; k++) {
        uint32_t out[4];
        draw::philox(counter[k], key[k], out);
        expect(!std::memcmp(out, answer[k], sizeof(out)), "a known answer of Philox4x32-10");
    }
    expect(draw::uniform_of(0xffffffffu, 0xffffffffu) < 1.0 && draw::uniform_of(0, 0) == 0.0, "U lies in [0, 1)");
    check<double> ("fp64", false);
    check<double> ("fp64", true);
    check<float> ("fp32", false);
    check<float> ("fp32", true);
    std::printf("cases %ld failures %ld\n", cases, failures);
    return failures ? 1 : 0;
}
