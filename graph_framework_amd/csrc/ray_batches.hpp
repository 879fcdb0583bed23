//------------------------------------------------------------------------------
///  @file ray_batches.hpp
///  @brief The batch of a ray, written once: which of G fixed batches a ray of the ensemble belongs to, how many rays of
///  a range a batch holds, and the walk by which a deposit launch hands the chunks of one batch at a time to the waves
///  of a workgroup.
///
///  Ray r is the ray's index in the whole ensemble, over all ranks and files.  64 consecutive rays are a chunk, r >> 6,
///  and chunk c belongs to batch c % G: a wave reads one chunk, 512 contiguous bytes per column, and all its lanes have
///  one batch.
///
///  Shared by the deposit kernels (flux_profile.hip, flux_spectrum.hip), the host runtime (gf_hip.cpp) and a host-only
///  test (tests/ray_batches_check.cpp): no HIP header, plain C++17.
//------------------------------------------------------------------------------
#ifndef gfhip_ray_batches_hpp
#define gfhip_ray_batches_hpp

#include <stdint.h>

#ifndef GFHIP_HD                    // (superacc.hpp has the same)
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GFHIP_HD __host__ __device__ inline
#else
#define GFHIP_HD inline
#endif
#endif

namespace gfhip {
namespace batches {

constexpr unsigned int chunk_shift = 6;
constexpr unsigned int chunk_rays = 1u << chunk_shift;
constexpr unsigned int max_batches = 256;

GFHIP_HD unsigned int batch_of(const uint64_t ray, const unsigned int batches) {
    return static_cast<unsigned int> ((ray >> chunk_shift) % batches);
}

//  The chunks below `chunk` that belong to batch g.
GFHIP_HD uint64_t chunks_below(const uint64_t chunk, const unsigned int batches, const unsigned int g) {
    return chunk/batches + (chunk % batches > g ? 1u : 0u);
}

//  The first chunk at or above `chunk` that belongs to batch g.
GFHIP_HD uint64_t first_chunk_of(const uint64_t chunk, const unsigned int batches, const unsigned int g) {
    return chunk + (g + batches - static_cast<unsigned int> (chunk % batches)) % batches;
}

//  The rays of [first, first + count) that belong to batch g; first + count does not wrap.
GFHIP_HD uint64_t batch_rays(const uint64_t first, const uint64_t count, const unsigned int batches, const unsigned int g) {
    if (count == 0) return 0;
    const uint64_t last = first + (count - 1);                              // the last ray itself
    const uint64_t low = first >> chunk_shift, high = last >> chunk_shift;
    uint64_t rays = (chunks_below(high + 1, batches, g) - chunks_below(low, batches, g)) << chunk_shift;
    if (low % batches == g) rays -= first & (chunk_rays - 1u);             // the partial first chunk
    if (high % batches == g) rays -= (chunk_rays - 1u) - (last & (chunk_rays - 1u));    // and the partial last one
    return rays;
}

//  Lane `lane` of the wave that holds the chunk whose first ray is `chunk_ray`: whether its ray is one of the add's
//  [first_ray, first_ray + count), and then which sample it is: sample i of an add is ray first_ray + i.
GFHIP_HD bool sample_of(const uint64_t first_ray, const uint64_t count, const uint64_t chunk_ray, const unsigned int lane,
                        uint64_t &sample) {
    const uint64_t ray = chunk_ray + lane;
    sample = ray - first_ray;
    return ray >= first_ray && sample < count;
}

//  The workgroups a launch of `wanted` should have: with more workgroups than batches, a whole number per batch, so that
//  none is idle.
GFHIP_HD unsigned int whole_teams(const unsigned int wanted, const unsigned int batches) {
    return wanted > batches ? wanted - wanted % batches : wanted;
}

//  The walk of wave `wave` of workgroup `workgroup`, in a launch of `workgroups` workgroups of `waves` waves each, over
//  the rays [first_ray, first_ray + count), count >= 1.
//
//  The work is cut into units (batch g, team t): T = max(1, workgroups/batches) teams share a batch, unit v = t*batches
//  + g.  Workgroup b takes the units b, b + workgroups, ... below batches*T, one after the other: with fewer workgroups
//  than batches it works through several batches, with more, T workgroups share one (and workgroups % batches of them
//  have no unit, see whole_teams).  In a unit the T*waves waves of the batch's teams take the batch's chunks in turn:
//  wave w of team t the chunks number t*waves + w, then every T*waves-th, of those of batch g in the range.
//
//  chunk(g, chunk_ray): one chunk of batch g, its first ray (a multiple of 64) — the first and the last chunk of the
//  range may be partial, sample_of says which lanes hold a sample.  close(g): the unit of batch g is done.  The
//  sequence of close() calls depends on the workgroup alone, not on the wave: a barrier belongs there, and nowhere else.
template<typename CHUNK, typename CLOSE>
GFHIP_HD void walk(const uint64_t first_ray, const uint64_t count, const unsigned int batches, const unsigned int workgroups,
                   const unsigned int waves, const unsigned int workgroup, const unsigned int wave, CHUNK chunk, CLOSE close) {
    const uint64_t low = first_ray >> chunk_shift, end = ((first_ray + (count - 1)) >> chunk_shift) + 1;
    const unsigned int teams = workgroups > batches ? workgroups/batches : 1u;
    const unsigned int units = batches*teams;
    const uint64_t step = static_cast<uint64_t> (teams)*waves*batches;
    for (unsigned int v = workgroup; v < units; v += workgroups) {          // uniform over the workgroup
        const unsigned int g = v % batches, team = v/batches;
        const uint64_t mine = first_chunk_of(low, batches, g) + static_cast<uint64_t> (team*waves + wave)*batches;
        for (uint64_t c = mine; c < end; c += step) chunk(g, c << chunk_shift);
        close(g);
    }
}

}  // namespace batches
}  // namespace gfhip

#endif /* gfhip_ray_batches_hpp */
