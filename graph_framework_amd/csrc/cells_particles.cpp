//------------------------------------------------------------------------------
///  @file cells_particles.cpp
///  @brief libgf_hip.so: the particle-side objects on the shared host pieces of cells.hpp: distributions (gfhip_phase_*),
///  moment profiles (gfhip_moments_*), first-exit trackers (gfhip_confine_*) and particle sources (gfhip_source_*).
//------------------------------------------------------------------------------
#include <cmath>
#include <limits>

#include "cells.hpp"
#include "confinement_host.hpp"
#include "moments_host.hpp"
#include "phase_host.hpp"
#include "ray_batches.hpp"
#include "source_host.hpp"

using namespace gfhip::cells;
namespace flux = gfhip::flux;

//  The particles of a call: the seven columns and the weight (null without one), all of one type.
struct particle_input {
    const void *columns[8] = {};
    bool is_f32 = false;
};

//  `used` real buffers of ONE type, fp32 or fp64, of at least `count` elements, or the message; nothing is enqueued.
static int particle_columns(gfhip_context *ctx, const uint64_t *keys, const size_t used, const size_t count, const char *noun,
                            particle_input &in) {
    uint32_t dtype = 0;
    for (size_t c = 0; c < used; c++) {
        const buffer *found = find_buffer(ctx, keys[c]);
        if (!found) return 1;
        if (found->dtype != GFIR_F64 && found->dtype != GFIR_F32) return ctx->fail(std::string(noun) + " takes fp32 or fp64 buffers");
        if (c && found->dtype != dtype) return ctx->fail(std::string(noun) + " takes buffers of one type, all fp32 or all fp64");
        if (found->count < count) return ctx->fail(std::string(noun) + " buffer is shorter than the particle count");
        dtype = found->dtype;
        in.columns[c] = found->pointer;
    }
    in.is_f32 = dtype == GFIR_F32;
    return 0;
}

//  The same of the seven keys and the weight's, which is looked at only with has_weight.
static int weighted_particles(gfhip_context *ctx, const uint64_t *keys, const uint64_t weight_key, const int has_weight,
                              const size_t count, const char *noun, particle_input &in) {
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], weight_key};
    return particle_columns(ctx, all, has_weight ? 8 : 7, count, noun, in);
}

//  Whether a host call has its seven columns (needed only with particles).
static bool seven_columns(const void *const *columns, const size_t count) {
    for (int k = 0; columns && k < 7; k++) {
        if (!columns[k] && count) return false;
    }
    return columns != nullptr;
}

//  The batches and the particle range of a host call, or why they are refused.
static const char *host_batches_refused(const size_t batches, const uint64_t first_particle, const size_t count) {
    if (batches < 1 || batches > gfhip::batches::max_batches) return "a batched object has 1 to 256 batches";
    if (first_particle + static_cast<uint64_t> (count) < first_particle) return "first_particle + count overflows 64 bits";
    return nullptr;
}

//  with(float()) or with(double()): the type of a host call's columns.
template<typename WITH>
static void with_type(const int is_f32, WITH with) {
    if (is_f32) {
        with(float());
    } else {
        with(double());
    }
}

//  Distributions of particles over the flux label, the pitch cosine and gamma (phase_bins.hip, flux_label.hpp): cell
//  (is*np + ip)*ng + ig; the three axes' edges one after the other, staged in LDS on both paths.
static const axis_rules phase_rules = {flux_cell_limit, phase_cell_limit, "a distribution has 1 to 4096 cells per axis (at least two edges)",
                                       "the edges of a distribution must be finite and strictly increasing",
                                       "a distribution has at most 2^20 cells (536 B each)"};

struct gfhip_phase : flux_cells {};

//  batch_count: 0 for gfhip_phase_create.
static gfhip_phase *phase_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                 const double *sedges, size_t ns, const double *pedges, size_t np,
                                 const double *gedges, size_t ng, const size_t batch_count, const bool batched) {
    if (!map || !field || !sedges || !pedges || !gedges) {
        ctx->fail("a distribution needs a map, a field and three edge arrays");
        return nullptr;
    }
    const double *axes[3] = {sedges, pedges, gedges};
    const size_t n[3] = {ns, np, ng};
    std::unique_ptr<gfhip_phase> p(new gfhip_phase);
    p->noun = "a distribution";
    p->rank = 3;
    std::copy(n, n + 3, p->n);
    std::vector<double> edges;
    size_t cells = 0;
    const char *refused = axes_of(phase_rules, 3, axes, n, edges, cells, p->scale);
    if (!refused && batched) refused = batches_refused(batch_count, cells);
    if (refused) {
        ctx->fail(refused);
        return nullptr;
    }
    if (p->create(ctx, map, field, phase_field_of, cells, edges, gfhip::phase_prepare, batch_count)) return nullptr;
    return adopt(ctx, p);
}

extern "C" gfhip_phase *gfhip_phase_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                           const double *sedges, size_t ns, const double *pedges, size_t np,
                                           const double *gedges, size_t ng) {
    return ctx ? phase_create(ctx, map, field, sedges, ns, pedges, np, gedges, ng, 0, false) : nullptr;
}

extern "C" gfhip_phase *gfhip_phase_create_batched(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                                   const double *sedges, size_t ns, const double *pedges, size_t np,
                                                   const double *gedges, size_t ng, size_t batches) {
    return ctx ? phase_create(ctx, map, field, sedges, ns, pedges, np, gedges, ng, batches, true) : nullptr;
}

extern "C" void gfhip_phase_destroy(gfhip_phase *p) {
    destroy(p);
}

extern "C" int gfhip_phase_add(gfhip_phase *p, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count) {
    if (!p) return 1;
    if (!keys) return p->ctx->fail("gfhip_phase_add needs its 7 keys");
    if (p->batches) return p->ctx->fail("a batched distribution takes its particles with their index: gfhip_phase_add_particles");
    particle_input in;
    if (weighted_particles(p->ctx, keys, weight_key, has_weight, count, p->noun, in)) return 1;
    return p->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_phase_deposit(in.columns, in.is_f32, first, piece, p->tables(), p->edges.get(), p->n, p->scale, p->shape,
                                    p->target());
    });
}

extern "C" int gfhip_phase_add_particles(gfhip_phase *p, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count,
                                         uint64_t first_particle) {
    if (!p) return 1;
    if (!keys) return p->ctx->fail("gfhip_phase_add_particles needs its 7 keys");
    if (const char *refused = p->index_refused(true, first_particle, count)) return p->ctx->fail(refused);
    particle_input in;
    if (weighted_particles(p->ctx, keys, weight_key, has_weight, count, p->noun, in)) return 1;
    return p->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_phase_deposit_particles(in.columns, in.is_f32, first, piece, first_particle + first, p->batches, p->tables(),
                                              p->edges.get(), p->n, p->scale, p->shape, p->target());
    });
}

extern "C" int gfhip_phase_coordinates(gfhip_phase *p, const uint64_t keys[7], uint64_t label_key, uint64_t pitch_key, size_t count) {
    if (!p) return 1;
    gfhip_context *ctx = p->ctx;
    if (!keys) return ctx->fail("gfhip_phase_coordinates needs its 7 keys");
    particle_input in;
    if (particle_columns(ctx, keys, 7, count, p->noun, in)) return 1;
    double *out[2];
    if (fp64_columns(ctx, "a distribution's label and pitch", {label_key, pitch_key}, count, out)) return 1;
    if (enter(ctx)) return 1;
    gfhip::launch_phase_coordinates(in.columns, in.is_f32, count, p->tables(), out[0], out[1], ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "phase coordinates launch");
    return 0;
}

extern "C" int gfhip_phase_counts(gfhip_phase *p, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return counts_of(p, samples, outside, skipped);
}

extern "C" int gfhip_phase_state(gfhip_phase *p, int64_t *limbs) {
    return state_of(p, "gfhip_phase_state", limbs);
}

extern "C" int gfhip_phase_merge(gfhip_phase *p, const int64_t *limbs, size_t ns, size_t np, size_t ng, uint64_t samples,
                                 uint64_t outside, uint64_t skipped) {
    return merge_of(p, "gfhip_phase_merge", limbs, false, 0, {ns, np, ng}, samples, outside, skipped);
}

extern "C" int gfhip_phase_merge_batches(gfhip_phase *p, const int64_t *limbs, size_t batches, size_t ns, size_t np, size_t ng,
                                         uint64_t samples, uint64_t outside, uint64_t skipped) {
    return merge_of(p, "gfhip_phase_merge_batches", limbs, true, batches, {ns, np, ng}, samples, outside, skipped);
}

extern "C" int gfhip_phase_read(gfhip_phase *p, double divisor, double *values) {
    return read_of(p, "gfhip_phase_read", divisor, values);
}

extern "C" int gfhip_phase_info(gfhip_phase *p, struct gfhip_flux_info *info) {
    return info_of(p, "gfhip_phase_info", info);
}

//  Host side, no device: flux_label.hpp on the caller's 16 + 4 tables (phase_host.hpp).
extern "C" int gfhip_phase_coordinates_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                            const void *const columns[7], int is_f32, size_t count, double *label, double *pitch) {
    if (!(map && field && ((label && pitch) || !count) && seven_columns(columns, count))) {
        return refuse("gfhip_phase_coordinates_host needs a map, a field, seven columns and two destinations");
    }
    flux::map m;
    flux::field f;
    flux::host_tables t;
    if (const char *refused = host_tables_of(map, field, m, f, t)) return refuse(refused);
    with_type(is_f32, [&](auto type) {
        const auto *const *in = reinterpret_cast<const decltype(type) *const *> (columns);
        for (size_t s = 0; s < count; s++) {
            gfhip::phase::host_point(m, f, t, static_cast<double> (in[0][s]), static_cast<double> (in[1][s]),
                                     static_cast<double> (in[2][s]), static_cast<double> (in[3][s]), static_cast<double> (in[4][s]),
                                     static_cast<double> (in[5][s]), label[s], pitch[s]);
        }
    });
    return 0;
}

//  limbs: [batches][ns][np][ng][67] (phase_host.hpp's add_particles_host).
extern "C" int gfhip_phase_add_particles_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *sedges,
                                              size_t ns, const double *pedges, size_t np, const double *gedges, size_t ng,
                                              size_t batches, const void *const columns[8], int is_f32, size_t count,
                                              uint64_t first_particle, int64_t *limbs, uint64_t counters[3]) {
    if (!(map && field && sedges && pedges && gedges && limbs && counters && seven_columns(columns, count))) {
        return refuse("gfhip_phase_add_particles_host needs a map, a field, three edge arrays, seven columns, limbs and counters");
    }
    const double *axes[3] = {sedges, pedges, gedges};
    const size_t n[3] = {ns, np, ng};
    flux::map m;
    flux::field f;
    flux::host_tables t;
    std::vector<double> edges;
    size_t cells = 0;
    double scale[3];
    const char *refused = axes_of(phase_rules, 3, axes, n, edges, cells, scale);
    if (!refused) refused = host_batches_refused(batches, first_particle, count);
    if (!refused) refused = host_tables_of(map, field, m, f, t);
    if (refused) return refuse(refused);
    with_type(is_f32, [&](auto type) {
        gfhip::phase::add_particles_host<decltype(type)> (m, f, t, axes, n, static_cast<unsigned int> (batches), first_particle, columns,
                                                          count, limbs, counters);
    });
    return 0;
}

//  Moment profiles (moment_bins.hip, flux_label.hpp): four cells per flux surface, cell is*4 + k, k = density, current,
//  energy, radiation.  The surfaces are an axis of a distribution, 1 to 4096, so the 2^20 cells are never reached by an
//  accepted axis; the check stands first for callers that ask for more.
static const size_t moment_count = gfhip::moments::count;
static const axis_rules moments_rules = {flux_cell_limit, phase_cell_limit/moment_count,
                                         "a moment profile has 1 to 4096 surfaces (at least two edges)",
                                         "the edges of a moment profile must be finite and strictly increasing",
                                         "a moment profile has at most 2^20 cells (four per surface, 536 B each)"};

//  n = {surfaces, 4}: what a merge names.
struct gfhip_moments : flux_cells {};

//  The label axis checked, or why it is refused.
static const char *moments_axis_of(const double *sedges, const size_t ns, std::vector<double> &edges, double *scale) {
    if (ns > moments_rules.in_all) return moments_rules.cells_refused;
    size_t surfaces = 0;
    return axes_of(moments_rules, 1, &sedges, &ns, edges, surfaces, scale);
}

//  batch_count: 0 for gfhip_moments_create.
static gfhip_moments *moments_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                     const double *sedges, size_t ns, const size_t batch_count, const bool batched) {
    if (!map || !field || !sedges) {
        ctx->fail("a moment profile needs a map, a field and the label edges");
        return nullptr;
    }
    std::unique_ptr<gfhip_moments> p(new gfhip_moments);
    p->noun = "a moment profile";
    p->rank = 2;
    p->n[0] = ns;
    p->n[1] = moment_count;
    std::vector<double> edges;
    const char *refused = moments_axis_of(sedges, ns, edges, p->scale);
    if (!refused && batched) refused = batches_refused(batch_count, ns*moment_count);
    if (refused) {
        ctx->fail(refused);
        return nullptr;
    }
    if (p->create(ctx, map, field, phase_field_of, ns*moment_count, edges, gfhip::moments_prepare, batch_count)) return nullptr;
    return adopt(ctx, p);
}

extern "C" gfhip_moments *gfhip_moments_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                               const double *sedges, size_t ns) {
    return ctx ? moments_create(ctx, map, field, sedges, ns, 0, false) : nullptr;
}

extern "C" gfhip_moments *gfhip_moments_create_batched(gfhip_context *ctx, const gfhip_flux_map *map,
                                                       const gfhip_spectrum_field *field, const double *sedges, size_t ns,
                                                       size_t batches) {
    return ctx ? moments_create(ctx, map, field, sedges, ns, batches, true) : nullptr;
}

extern "C" void gfhip_moments_destroy(gfhip_moments *p) {
    destroy(p);
}

extern "C" int gfhip_moments_add(gfhip_moments *p, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count) {
    if (!p) return 1;
    if (!keys) return p->ctx->fail("gfhip_moments_add needs its 7 keys");
    if (p->batches) return p->ctx->fail("a batched moment profile takes its particles with their index: gfhip_moments_add_particles");
    if (count == 0) return p->ctx->fail("a moment profile takes at least one particle");
    particle_input in;
    if (weighted_particles(p->ctx, keys, weight_key, has_weight, count, p->noun, in)) return 1;
    return p->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_moment_deposit(in.columns, in.is_f32, first, piece, p->tables(), p->edges.get(), p->n[0], p->scale[0],
                                     p->shape, p->target());
    });
}

extern "C" int gfhip_moments_add_particles(gfhip_moments *p, const uint64_t keys[7], uint64_t weight_key, int has_weight,
                                           size_t count, uint64_t first_particle) {
    if (!p) return 1;
    if (!keys) return p->ctx->fail("gfhip_moments_add_particles needs its 7 keys");
    if (const char *refused = p->index_refused(true, first_particle, count)) return p->ctx->fail(refused);
    if (count == 0) return p->ctx->fail("a moment profile takes at least one particle");
    particle_input in;
    if (weighted_particles(p->ctx, keys, weight_key, has_weight, count, p->noun, in)) return 1;
    return p->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_moment_deposit_particles(in.columns, in.is_f32, first, piece, first_particle + first, p->batches, p->tables(),
                                               p->edges.get(), p->n[0], p->scale[0], p->shape, p->target());
    });
}

extern "C" int gfhip_moments_values(gfhip_moments *p, const uint64_t keys[7], uint64_t label_key, uint64_t values_key, size_t count) {
    if (!p) return 1;
    gfhip_context *ctx = p->ctx;
    if (!keys) return ctx->fail("gfhip_moments_values needs its 7 keys");
    if (count == 0) return ctx->fail("a moment profile takes at least one particle");
    if (count > std::numeric_limits<size_t>::max()/moment_count) return ctx->fail("a moment profile's values buffer is shorter than 4 x the particle count");
    particle_input in;
    if (particle_columns(ctx, keys, 7, count, p->noun, in)) return 1;
    double *label = nullptr, *values = nullptr;
    if (fp64_columns(ctx, "a moment profile's label", {label_key}, count, &label) ||
        fp64_columns(ctx, "a moment profile's values (4 per particle)", {values_key}, count*moment_count, &values)) {
        return 1;
    }
    if (enter(ctx)) return 1;
    gfhip::launch_moment_values(in.columns, in.is_f32, count, p->tables(), label, values, ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "moment values launch");
    return 0;
}

extern "C" int gfhip_moments_counts(gfhip_moments *p, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return counts_of(p, samples, outside, skipped);
}

extern "C" int gfhip_moments_state(gfhip_moments *p, int64_t *limbs) {
    return state_of(p, "gfhip_moments_state", limbs);
}

extern "C" int gfhip_moments_merge(gfhip_moments *p, const int64_t *limbs, size_t ns, size_t nm, uint64_t samples,
                                   uint64_t outside, uint64_t skipped) {
    return merge_of(p, "gfhip_moments_merge", limbs, false, 0, {ns, nm}, samples, outside, skipped);
}

extern "C" int gfhip_moments_merge_batches(gfhip_moments *p, const int64_t *limbs, size_t batches, size_t ns, size_t nm,
                                           uint64_t samples, uint64_t outside, uint64_t skipped) {
    return merge_of(p, "gfhip_moments_merge_batches", limbs, true, batches, {ns, nm}, samples, outside, skipped);
}

extern "C" int gfhip_moments_read(gfhip_moments *p, double divisor, double *values) {
    return read_of(p, "gfhip_moments_read", divisor, values);
}

extern "C" int gfhip_moments_info(gfhip_moments *p, struct gfhip_flux_info *info) {
    return info_of(p, "gfhip_moments_info", info);
}

//  Host side, no device: flux_label.hpp on the caller's 16 + 4 tables (moments_host.hpp).
extern "C" int gfhip_moments_values_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const void *const columns[7],
                                         int is_f32, size_t count, double *label, double *values) {
    if (!(map && field && ((label && values) || !count) && seven_columns(columns, count))) {
        return refuse("gfhip_moments_values_host needs a map, a field, seven columns and two destinations");
    }
    flux::map m;
    flux::field f;
    flux::host_tables t;
    if (const char *refused = host_tables_of(map, field, m, f, t)) return refuse(refused);
    with_type(is_f32, [&](auto type) {
        gfhip::moments::values_host<decltype(type)> (m, f, t, columns, count, label, values);
    });
    return 0;
}

//  The deposits of a host call: batches = 0 for gfhip_moments_add_host; limbs: [batches][ns][4][67].
static int moments_add_host(const char *entry, const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *sedges,
                            const size_t ns, const bool batched, const size_t batches, const void *const *columns,
                            const int is_f32, const size_t count, const uint64_t first_particle, int64_t *limbs,
                            uint64_t *counters) {
    if (!(map && field && sedges && limbs && counters && seven_columns(columns, count))) {
        creation_error = std::string(entry) + " needs a map, a field, the label edges, seven columns, limbs and counters";
        return 1;
    }
    flux::map m;
    flux::field f;
    flux::host_tables t;
    std::vector<double> edges;
    double scale = 0.0;
    const char *refused = moments_axis_of(sedges, ns, edges, &scale);
    if (!refused && batched) refused = host_batches_refused(batches, first_particle, count);
    if (!refused) refused = host_tables_of(map, field, m, f, t);
    if (refused) return refuse(refused);
    with_type(is_f32, [&](auto type) {
        using T = decltype(type);
        if (batched) {
            gfhip::moments::add_particles_host<T> (m, f, t, sedges, ns, static_cast<unsigned int> (batches), first_particle, columns,
                                                   count, limbs, counters);
        } else {
            gfhip::moments::add_host<T> (m, f, t, sedges, ns, columns, count, limbs, counters);
        }
    });
    return 0;
}

extern "C" int gfhip_moments_add_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *sedges, size_t ns,
                                      const void *const columns[8], int is_f32, size_t count, int64_t *limbs, uint64_t counters[3]) {
    return moments_add_host("gfhip_moments_add_host", map, field, sedges, ns, false, 0, columns, is_f32, count, 0, limbs, counters);
}

extern "C" int gfhip_moments_add_particles_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *sedges,
                                                size_t ns, size_t batches, const void *const columns[8], int is_f32, size_t count,
                                                uint64_t first_particle, int64_t *limbs, uint64_t counters[3]) {
    return moments_add_host("gfhip_moments_add_particles_host", map, field, sedges, ns, true, batches, columns, is_f32, count,
                            first_particle, limbs, counters);
}

//  First-exit trackers (confinement.hip, flux_label.hpp).  The axes and the cells are a distribution's; deposits always
//  go to the global state, so the launch shape is the global path's whatever the map's flags say.
static const axis_rules confine_rules = {flux_cell_limit, phase_cell_limit,
                                         "a loss footprint has 1 to 4096 cells per axis (at least two edges)",
                                         "the edges of a loss footprint must be finite and strictly increasing",
                                         "a loss footprint has at most 2^20 cells (536 B each)"};

//  A first-exit tracker of the particles of one push: per particle lost_step and the context buffer `alive_key`; per
//  check its step (here) and the number of particles it found lost (on the device); the footprint of the losses, cell
//  (ir*nz + iz)*ng + ig, the three axes' edges one after the other.
struct gfhip_confine : flux_cells {
    double limit = 0.0;
    size_t count = 0, capacity = 0;
    bool is_f32 = false;
    uint64_t alive_key = 0;
    device_ptr<uint32_t> lost_step;
    device_ptr<unsigned long long> newly_lost;         // [capacity]
    std::vector<uint32_t> steps;                       // the checks made
    bool exit_ready = false;                           // the exit buffers of `exit_keys` hold NaN for every confined particle
    uint64_t exit_keys[2] = {0, 0};
};

extern "C" gfhip_confine *gfhip_confine_create(gfhip_context *ctx, const gfhip_flux_map *map, double limit, const double *redges,
                                               size_t nr, const double *zedges, size_t nz, const double *gedges, size_t ng,
                                               size_t count, int is_f32, uint64_t alive_key, size_t capacity) {
    if (!ctx) return nullptr;
    if (!map || !redges || !zedges || !gedges) {
        ctx->fail("a confinement tracker needs a map and three edge arrays");
        return nullptr;
    }
    const double *axes[3] = {redges, zedges, gedges};
    const size_t n[3] = {nr, nz, ng};
    std::unique_ptr<gfhip_confine> c(new gfhip_confine);
    c->noun = "a loss footprint";
    c->rank = 3;
    std::copy(n, n + 3, c->n);
    std::vector<double> edges;
    size_t cells = 0;
    const char *refused = axes_of(confine_rules, 3, axes, n, edges, cells, c->scale);
    if (!refused && limit != limit) refused = "the limit of a confinement tracker must not be NaN";
    if (!refused && (count == 0 || capacity == 0)) refused = "a confinement tracker needs at least one particle and room for at least one check";
    if (refused) {
        ctx->fail(refused);
        return nullptr;
    }
    gfhip_flux_map global = *map;
    global.flags |= flux::flag_no_private_sums;
    c->limit = limit;
    c->count = count;
    c->capacity = capacity;
    c->is_f32 = is_f32 != 0;
    c->alive_key = alive_key;
    if (c->create(ctx, &global, nullptr, nullptr, cells, edges, nullptr) || enter(ctx) ||
        ensure_buffer(ctx, alive_key, count, c->is_f32 ? GFIR_F32 : GFIR_F64, nullptr) ||
        ctx->check(allocate(c->lost_step, count*sizeof(uint32_t)), "hipMalloc(lost steps)") ||
        ctx->check(allocate(c->newly_lost, capacity*sizeof(unsigned long long)), "hipMalloc(newly lost)") ||
        ctx->check(hipMemsetAsync(c->newly_lost.get(), 0, capacity*sizeof(unsigned long long), ctx->stream), "hipMemset(newly lost)")) {
        return nullptr;
    }
    gfhip::launch_confinement_reset(count, c->lost_step.get(), find_buffer(ctx, alive_key)->pointer, c->is_f32, nullptr, nullptr,
                                    ctx->stream);
    if (ctx->check(hipGetLastError(), "confinement reset launch")) return nullptr;
    return adopt(ctx, c);
}

extern "C" void gfhip_confine_destroy(gfhip_confine *c) {
    destroy(c);
}

extern "C" int gfhip_confine_check(gfhip_confine *c, const uint64_t keys[7], uint64_t weight_key, int has_weight,
                                   uint64_t exit_r_key, uint64_t exit_z_key, int has_exit, uint32_t step) {
    if (!c) return 1;
    gfhip_context *ctx = c->ctx;
    if (!keys) return ctx->fail("gfhip_confine_check needs its 7 keys");
    particle_input in;
    if (weighted_particles(ctx, keys, weight_key, has_weight, c->count, "a confinement tracker", in)) return 1;
    if (in.is_f32 != c->is_f32) return ctx->fail("the columns are not of the confinement tracker's type");
    const buffer *alive = find_buffer(ctx, c->alive_key);
    if (!alive) return 1;
    if (alive->dtype != (c->is_f32 ? GFIR_F32 : GFIR_F64) || alive->count < c->count) {
        return ctx->fail("the alive buffer of a confinement tracker has been replaced by one of another type or length");
    }
    double *exits[2] = {nullptr, nullptr};
    if (has_exit && fp64_columns(ctx, "a confinement tracker's exit", {exit_r_key, exit_z_key}, c->count, exits)) return 1;
    if (step == GFHIP_CONFINED) return ctx->fail("step 0xFFFFFFFF means confined: a check cannot have it");
    if (!c->steps.empty() && step < c->steps.back()) return ctx->fail("a check's step is below the previous check's");
    if (c->steps.size() >= c->capacity) return ctx->fail("more checks than the confinement tracker's capacity");
    if (enter(ctx)) return 1;
    if (has_exit && !(c->exit_ready && c->exit_keys[0] == exit_r_key && c->exit_keys[1] == exit_z_key)) {
        gfhip::launch_confinement_reset(c->count, nullptr, nullptr, c->is_f32, exits[0], exits[1], ctx->stream);
        GFHIP_TRY(ctx, hipGetLastError(), "confinement reset launch");
        c->exit_ready = true;
        c->exit_keys[0] = exit_r_key;
        c->exit_keys[1] = exit_z_key;
    }
    unsigned long long *entry = c->newly_lost.get() + c->steps.size();
    if (c->add(c->count, [&](const size_t first, const size_t piece) {
            gfhip::launch_confinement_check(in.columns, alive->pointer, c->is_f32, first, piece, c->tables(), c->limit, c->edges.get(),
                                            c->n, c->scale, step, c->lost_step.get(), exits[0], exits[1], entry, c->shape,
                                            c->target());
        })) {
        return 1;
    }
    c->steps.push_back(step);
    return 0;
}

extern "C" int gfhip_confine_lost_steps(gfhip_confine *c, uint32_t *lost_step) {
    if (!c) return 1;
    gfhip_context *ctx = c->ctx;
    if (!lost_step) return ctx->fail("gfhip_confine_lost_steps needs a destination");
    if (enter(ctx)) return 1;
    GFHIP_TRY(ctx, hipMemcpyAsync(lost_step, c->lost_step.get(), c->count*sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream),
              "hipMemcpyAsync(lost steps)");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return 0;
}

extern "C" int gfhip_confine_history(gfhip_confine *c, uint32_t *steps, uint64_t *newly_lost, size_t *checks) {
    if (!c) return 1;
    gfhip_context *ctx = c->ctx;
    if (!checks) return ctx->fail("gfhip_confine_history needs a destination for the number of checks");
    *checks = c->steps.size();
    if (steps) std::copy(c->steps.begin(), c->steps.end(), steps);
    if (newly_lost && !c->steps.empty()) {
        if (enter(ctx)) return 1;
        GFHIP_TRY(ctx, hipMemcpyAsync(newly_lost, c->newly_lost.get(), c->steps.size()*sizeof(uint64_t), hipMemcpyDeviceToHost,
                                      ctx->stream), "hipMemcpyAsync(newly lost)");
        GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    return 0;
}

extern "C" int gfhip_confine_counts(gfhip_confine *c, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return counts_of(c, samples, outside, skipped);
}

extern "C" int gfhip_confine_state(gfhip_confine *c, int64_t *limbs) {
    return state_of(c, "gfhip_confine_state", limbs);
}

extern "C" int gfhip_confine_merge(gfhip_confine *c, const int64_t *limbs, size_t nr, size_t nz, size_t ng, uint64_t samples,
                                   uint64_t outside, uint64_t skipped) {
    return merge_of(c, "gfhip_confine_merge", limbs, false, 0, {nr, nz, ng}, samples, outside, skipped);
}

extern "C" int gfhip_confine_read(gfhip_confine *c, double divisor, double *values) {
    return read_of(c, "gfhip_confine_read", divisor, values);
}

extern "C" int gfhip_confine_info(gfhip_confine *c, struct gfhip_flux_info *info) {
    return info_of(c, "gfhip_confine_info", info);
}

extern "C" int gfhip_confine_check_host(const gfhip_flux_map *map, double limit, const double *redges, size_t nr,
                                        const double *zedges, size_t nz, const double *gedges, size_t ng,
                                        const void *const columns[8], int is_f32, size_t count, uint32_t step, uint32_t *lost_step,
                                        void *alive, double *exit_r, double *exit_z, uint64_t *newly_lost, int64_t *limbs,
                                        uint64_t counters[3]) {
    bool complete = map && columns && newly_lost && ((lost_step && alive) || !count) && !exit_r == !exit_z &&
                    (!limbs || (redges && zedges && gedges && counters));
    for (int k = 0; complete && k < 7; k++) complete = columns[k] || !count || (k >= 3 && k <= 5) || (k == 6 && !limbs);
    if (!complete) {
        return refuse("gfhip_confine_check_host needs a map, the columns x, y, z and gamma, lost_step, alive and newly_lost, "
                      "both exit arrays or neither, and with limbs the three edge arrays and the counters");
    }
    flux::map m;
    const double *axes[3] = {redges, zedges, gedges};
    const size_t n[3] = {nr, nz, ng};
    std::vector<double> edges;
    size_t cells = 0;
    double scale[3];
    const char *refused = flux_map_of(map, m);
    if (!refused && limbs) refused = axes_of(confine_rules, 3, axes, n, edges, cells, scale);
    if (!refused && limit != limit) refused = "the limit of a confinement tracker must not be NaN";
    if (!refused && step == GFHIP_CONFINED) refused = "step 0xFFFFFFFF means confined: a check cannot have it";
    if (refused) return refuse(refused);
    const size_t table = static_cast<size_t> (map->numr*map->numz);
    with_type(is_f32, [&](auto type) {
        using T = decltype(type);
        gfhip::confine::check_host<T> (m, map->coefficients, table, limit, axes, n, columns, count, step, lost_step,
                                       static_cast<T *> (alive), exit_r, exit_z, newly_lost, limbs, counters);
    });
    return 0;
}

//  Particle sources (particle_source.hip, particle_draw.hpp).

//  The route of a source made with neither route flag.
static const bool source_refill_by_default = true;

//  A particle source: the map and the field as a distribution holds them, the profile's edges and then its
//  probabilities, and the counters placed, unplaced, position_tries, gyro_tries.
struct gfhip_source : context_object {
    flux::map map = {};
    flux::field field = {};
    gfhip::draw::parameters par = {};
    device_ptr<double> packed, fpol, profile;
    double scale = 0.0;                                // ns/(last edge - first edge)
    bool is_f32 = false, refill = false;
    size_t max_workgroups = 0;
    device_ptr<unsigned long long> counters;
};

//  What the rule needs beside the map and the field, or why a source is refused.
static const char *source_parameters_of(const double *box, const double slo, const double shi, const double blo, const double bhi,
                                        const double xlo, const double xhi, const double *sedges, const double *accept,
                                        const size_t ns, const uint64_t seed, const uint32_t attempts, const uint32_t flags,
                                        gfhip::draw::parameters &par) {
    if (!box) return "a particle source needs its box {rlo, rhi, zlo, zhi}";
    for (int k = 0; k < 4; k++) {
        if (!std::isfinite(box[k])) return "the box of a particle source must be finite";
    }
    if (!(box[0] < box[1]) || !(box[2] < box[3]) || box[0] < 0.0) return "the box of a particle source needs 0 <= rlo < rhi and zlo < zhi";
    if (!(slo < shi)) return "the label range of a particle source must not be empty or NaN";
    if (!(blo < bhi) || !(blo >= 0.0) || !(bhi < 1.0)) return "the speed range of a particle source needs 0 <= blo < bhi < 1";
    if (!(xlo < xhi) || !(xlo >= -1.0) || !(xhi <= 1.0)) return "the pitch range of a particle source needs -1 <= xlo < xhi <= 1";
    if (attempts == 0 || attempts > gfhip::draw::max_attempts) return "a particle source makes 1 to 4096 attempts";
    if (ns > static_cast<size_t> (gfhip::draw::max_profile_cells)) return "the profile of a particle source has at most 256 cells";
    if ((ns != 0) != (sedges != nullptr) || (ns != 0) != (accept != nullptr)) {
        return "the profile of a particle source is ns + 1 edges and ns probabilities, or neither with ns = 0";
    }
    for (size_t i = 0; ns && i <= ns; i++) {
        if (!std::isfinite(sedges[i]) || (i && !(sedges[i - 1] < sedges[i]))) {
            return "the edges of a particle source's profile must be finite and strictly increasing";
        }
    }
    for (size_t k = 0; k < ns; k++) {
        if (!(accept[k] >= 0.0 && accept[k] <= 1.0)) return "the probabilities of a particle source's profile lie in [0, 1]";
    }
    if (flags & ~gfhip::draw::known_flags) return "unknown flag bits for a particle source";
    if ((flags & gfhip::draw::known_flags) == gfhip::draw::known_flags) return "a particle source takes one route, plain or refill";
    par = gfhip::draw::parameters_of(box, slo, shi, blo, bhi, xlo, xhi, seed, attempts, static_cast<int> (ns));
    return nullptr;
}

extern "C" gfhip_source *gfhip_source_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                             const double box[4], double slo, double shi, double blo, double bhi, double xlo,
                                             double xhi, const double *sedges, const double *accept, size_t ns, uint64_t seed,
                                             uint32_t attempts, int is_f32, uint32_t flags, size_t max_workgroups) {
    if (!ctx) return nullptr;
    if (!map || !field) {
        ctx->fail("a particle source needs a map and a field");
        return nullptr;
    }
    std::unique_ptr<gfhip_source> s(new gfhip_source);
    const char *refused = flux_map_of(map, s->map);
    if (!refused) refused = phase_field_of(field, s->field);
    if (!refused) refused = source_parameters_of(box, slo, shi, blo, bhi, xlo, xhi, sedges, accept, ns, seed, attempts, flags, s->par);
    if (refused) {
        ctx->fail(refused);
        return nullptr;
    }
    s->ctx = ctx;
    s->is_f32 = is_f32 != 0;
    s->refill = flags & gfhip::draw::known_flags ? (flags & gfhip::draw::flag_refill) != 0 : source_refill_by_default;
    s->max_workgroups = max_workgroups ? max_workgroups : static_cast<size_t> (ctx->num_cus)*8u;
    std::vector<double> profile(1, 0.0);
    if (ns) {
        profile.assign(sedges, sedges + ns + 1);
        profile.insert(profile.end(), accept, accept + ns);
        s->scale = static_cast<double> (ns)/(sedges[ns] - sedges[0]);
    }
    const char *no_memory = "a particle source's tables do not fit the host's memory";
    if (enter(ctx) || upload_tables(ctx, map, field, no_memory, no_memory, s->packed, s->fpol) ||
        ctx->check(allocate(s->profile, profile.size()*sizeof(double)), "hipMalloc(profile)") ||
        ctx->check(hipMemcpy(s->profile.get(), profile.data(), profile.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(profile)") ||
        ctx->check(allocate(s->counters, 4*sizeof(unsigned long long)), "hipMalloc(counters)") ||
        ctx->check(hipMemsetAsync(s->counters.get(), 0, 4*sizeof(unsigned long long), ctx->stream), "hipMemset(counters)") ||
        ctx->check(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
        return nullptr;
    }
    return adopt(ctx, s);
}

extern "C" void gfhip_source_destroy(gfhip_source *s) {
    destroy(s);
}

extern "C" int gfhip_source_fill(gfhip_source *s, const uint64_t keys[7], uint64_t placed_key, int has_placed,
                                 uint64_t first_particle, size_t count) {
    if (!s) return 1;
    gfhip_context *ctx = s->ctx;
    if (!keys) return ctx->fail("gfhip_source_fill needs its 7 keys");
    if (count == 0) return ctx->fail("a particle source fills at least one particle");
    if (first_particle + static_cast<uint64_t> (count) < first_particle) return ctx->fail("first_particle + count overflows 64 bits");
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], placed_key};
    const size_t used = has_placed ? 8 : 7;
    const uint32_t dtype = s->is_f32 ? GFIR_F32 : GFIR_F64;
//  Everything is looked at before anything is allocated.
    for (size_t c = 0; c < used; c++) {
        for (size_t other = 0; other < c; other++) {
            if (all[other] == all[c]) return ctx->fail("a particle source fills eight different buffers: a key is given twice");
        }
        const auto found = ctx->buffers.find(all[c]);
        if (found == ctx->buffers.end()) continue;
        if (found->second.dtype != dtype) return ctx->fail("a buffer is not of the particle source's type");
        if (found->second.count < count) return ctx->fail("a particle source's buffer is shorter than the particle count");
    }
    if (enter(ctx)) return 1;
    void *columns[8] = {};
    for (size_t c = 0; c < used; c++) {
        if (ensure_buffer(ctx, all[c], count, dtype, nullptr)) return 1;
        columns[c] = find_buffer(ctx, all[c])->pointer;
    }
    gfhip::launch_particle_source(columns, columns[7], s->is_f32, count, first_particle, s->map, s->field, s->par, s->packed.get(),
                                  s->fpol.get(), s->profile.get(), s->scale, s->refill, s->max_workgroups, s->counters.get(),
                                  ctx->stream);
    return ctx->check(hipGetLastError(), "particle source launch");
}

extern "C" int gfhip_source_counts(gfhip_source *s, uint64_t counters[4]) {
    if (!s) return 1;
    gfhip_context *ctx = s->ctx;
    if (!counters) return ctx->fail("gfhip_source_counts needs a destination");
    if (enter(ctx)) return 1;
    unsigned long long host[4] = {0, 0, 0, 0};
    GFHIP_TRY(ctx, hipMemcpyAsync(host, s->counters.get(), sizeof(host), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(counters)");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (int k = 0; k < 4; k++) counters[k] = host[k];
    return 0;
}

//  Not through enter(): as gfhip_flux_info.
extern "C" int gfhip_source_info(gfhip_source *s, struct gfhip_flux_info *info) {
    if (!s) return 1;
    if (!info) return s->ctx->fail("gfhip_source_info needs a destination");
    info->private_sums = s->refill ? 1u : 0u;
    info->workgroup_size = 256;
    info->cap_cells = 0;
    info->max_workgroups = s->max_workgroups;
    info->lds_bytes = s->par.ns ? (2*static_cast<size_t> (s->par.ns) + 1)*sizeof(double) : 0;
    return 0;
}

extern "C" int gfhip_source_fill_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double box[4], double slo,
                                      double shi, double blo, double bhi, double xlo, double xhi, const double *sedges,
                                      const double *accept, size_t ns, uint64_t seed, uint32_t attempts, uint32_t flags,
                                      void *const columns[8], int is_f32, uint64_t first_particle, size_t count,
                                      uint64_t counters[4]) {
    if (!(map && field && counters && seven_columns(columns, count))) {
        return refuse("gfhip_source_fill_host needs a map, a field, the seven columns and the counters");
    }
    flux::map m;
    flux::field f;
    gfhip::draw::parameters par;
    const char *refused = flux_map_of(map, m);
    if (!refused) refused = phase_field_of(field, f);
    if (!refused) refused = source_parameters_of(box, slo, shi, blo, bhi, xlo, xhi, sedges, accept, ns, seed, attempts, flags, par);
    if (!refused && first_particle + static_cast<uint64_t> (count) < first_particle) refused = "first_particle + count overflows 64 bits";
    if (refused) return refuse(refused);
    const gfhip::draw::host_tables tables = {map->coefficients, static_cast<size_t> (map->numr*map->numz),
                                             {field->fpol[0], field->fpol[1], field->fpol[2], field->fpol[3]}, sedges, accept, ns};
    with_type(is_f32, [&](auto type) {
        gfhip::draw::fill_host<decltype(type)> (m, f, par, tables, columns, columns[7], first_particle, count, counters);
    });
    return 0;
}

extern "C" void gfhip_source_block_host(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    gfhip::draw::philox(counter, key, out);
}
