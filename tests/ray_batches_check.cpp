//  csrc/ray_batches.hpp on the host: the walk of the batched deposit kernels driven as the kernels drive it, one call
//  per (workgroup, wave), over a grid of ranges, batch counts and launch shapes, and batch_rays against a count ray by
//  ray.  Built by tests/test_ray_batches.py with -fsanitize=address,undefined.  Prints one line per property and
//  returns 0, or says which case failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../graph_framework_amd/csrc/ray_batches.hpp"

using namespace gfhip::batches;

namespace {

struct shape {
    uint64_t first, count;
    unsigned int batches, workgroups, waves;
};

int failures = 0;

void fail(const shape &s, const char *what) {
    if (failures++ < 20) {
        std::printf("FAILED %s: first_ray %llu count %llu batches %u workgroups %u waves %u\n", what,
                    static_cast<unsigned long long> (s.first), static_cast<unsigned long long> (s.count), s.batches,
                    s.workgroups, s.waves);
    }
}

//  Every (workgroup, wave) of the launch walks; what the lanes of its chunks and its close() calls see is recorded.
void drive(const shape &s, unsigned long long &chunks) {
    std::vector<unsigned char> visits(s.count, 0);
    bool own_batch = true, whole_batches = true, uniform = true, in_range = true;
    for (unsigned int workgroup = 0; workgroup < s.workgroups; workgroup++) {
        std::vector<unsigned int> first_wave;                               // the batches wave 0 closes, in order
        for (unsigned int wave = 0; wave < s.waves; wave++) {
            std::vector<unsigned int> closed, open;                         // open: the batches of the chunks since the last close
            walk(s.first, s.count, s.batches, s.workgroups, s.waves, workgroup, wave,
                 [&](const unsigned int g, const uint64_t chunk_ray) {
                     chunks++;
                     open.push_back(g);
                     if (chunk_ray % chunk_rays) in_range = false;
                     bool any = false;
                     for (unsigned int lane = 0; lane < chunk_rays; lane++) {
                         uint64_t at;
                         if (!sample_of(s.first, s.count, chunk_ray, lane, at)) continue;
                         any = true;
                         if (at >= s.count) {
                             in_range = false;
                             continue;
                         }
                         if (visits[at] < 255) visits[at]++;
                         if (batch_of(s.first + at, s.batches) != g) own_batch = false;
                     }
                     if (!any) in_range = false;                            // a chunk handed out holds a sample
                 },
                 [&](const unsigned int g) {
                     for (const unsigned int was : open) {
                         if (was != g) whole_batches = false;
                     }
                     open.clear();
                     closed.push_back(g);
                 });
            if (!open.empty()) whole_batches = false;                       // chunks after the last close
            if (wave == 0) {
                first_wave = closed;
            } else if (closed != first_wave) {
                uniform = false;
            }
        }
    }
    for (uint64_t at = 0; at < s.count; at++) {
        if (visits[at] != 1) {
            fail(s, "every sample exactly once");
            break;
        }
    }
    if (!own_batch) fail(s, "a sample is visited by a unit of its own batch");
    if (!whole_batches) fail(s, "a workgroup closes a batch after that batch's chunks alone");
    if (!uniform) fail(s, "the close() calls are the same for every wave of a workgroup");
    if (!in_range) fail(s, "chunks start on a multiple of 64 and hold a sample of the range");
}

}  // namespace

int main() {
    const uint64_t firsts[] = {0, 1, 63, 64, 65, (1ull << 40) + 5};
    const unsigned int batch_counts[] = {1, 2, 3, 16, 64, 256};
    const unsigned int workgroup_counts[] = {1, 2, 300};
    const unsigned int wave_counts[] = {1, 4, 16};
    unsigned long long cases = 0, chunks = 0, counted = 0;
    for (const uint64_t first : firsts) {
        for (const unsigned int batches : batch_counts) {
            const uint64_t counts[] = {1, 63, 64, 65, 64ull*batches - 1, 64ull*batches, 64ull*batches + 1, 4099};
            for (const uint64_t count : counts) {
                const shape range = {first, count, batches, 0, 0};
//  batch_rays against a count ray by ray
                std::vector<uint64_t> brute(batches, 0);
                for (uint64_t at = 0; at < count; at++) brute[batch_of(first + at, batches)]++;
                uint64_t sum = 0;
                for (unsigned int g = 0; g < batches; g++) {
                    const uint64_t rays = batch_rays(first, count, batches, g);
                    sum += rays;
                    if (rays != brute[g]) fail(range, "batch_rays is the count ray by ray");
                    counted++;
                }
                if (sum != count) fail(range, "the batches' rays add up to the range");
                for (const unsigned int workgroups : workgroup_counts) {
                    const unsigned int whole = whole_teams(workgroups, batches);
                    if (whole > workgroups || whole == 0 || (whole > batches && whole % batches)) fail(range, "whole_teams");
                    for (const unsigned int waves : wave_counts) {
                        drive({first, count, batches, workgroups, waves}, chunks);
                        if (whole != workgroups) drive({first, count, batches, whole, waves}, chunks);
                        cases++;
                    }
                }
            }
        }
    }
    if (batch_rays(5, 0, 3, 1) != 0) failures++;
    std::printf("cases %llu chunks %llu batch_rays %llu failures %d\n", cases, chunks, counted, failures);
    return failures ? 1 : 0;
}
