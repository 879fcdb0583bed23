//------------------------------------------------------------------------------
///  @file cells.hpp
///  @brief The host objects behind the exact-sum diagnostics (not installed): what cells_rays.cpp (deposition grids, flux
///  profiles, volumes, spectra) and cells_particles.cpp (distributions, moment profiles, first-exit trackers, particle
///  sources) share.  Each piece is written once here: the store of exact sums, the object with a map, a noun and a
///  shape, the one with a field, the checks of maps, fields, axes and buffers, and the bodies of the entry points that
///  every family has (counts, state, merge, merge_batches, read, info, destroy).
//------------------------------------------------------------------------------
#ifndef GFHIP_CELLS_HPP
#define GFHIP_CELLS_HPP

#include <algorithm>
#include <string>
#include <vector>

#include "cell_launch.hpp"
#include "flux_label.hpp"
#include "point_host.hpp"
#include "runtime.hpp"
#include "superacc.hpp"

namespace gfhip {
namespace cells {

using namespace runtime;

//  A store of exact sums, what every object here is: per cell the 67 limbs of superacc.hpp, [cell][limb], and what
//  became of the samples.  The entry points check their own arguments and call these.
struct exact_cells : context_object {
    size_t cells = 0;
    device_ptr<> state;
    device_ptr<unsigned long long> counters;           // samples, outside, skipped
    device_ptr<double> rounded;                        // what read() copies out (allocated by the first read)
    uint64_t pending = 0;                              // deposits since the state was last canonical

    int create(gfhip_context *context, size_t count);  // allocated and zero
    int normalise();
    template<typename LAUNCH> int add(size_t count, LAUNCH launch);
    int counts(uint64_t *samples, uint64_t *outside, uint64_t *skipped);
    int state_to(int64_t *limbs);
    int merge(const int64_t *limbs, uint64_t samples, uint64_t outside, uint64_t skipped);
    int read(double divisor, double *values);
    cell_target target() const { return {state.get(), counters.get(), ctx->stream}; }
};

//  `count` deposits, `launch(first, piece)` enqueueing those of the samples first .. first + piece: at most 2^30
//  between two normalisations (superacc.hpp); a workgroup-private limb sees fewer than its launch.
template<typename LAUNCH>
int exact_cells::add(const size_t count, LAUNCH launch) {
    if (enter(ctx)) return 1;
    for (size_t first = 0; first < count;) {
        const size_t piece = std::min<size_t> (count - first, superacc::deposits_per_normalise);
        if (pending + piece > superacc::deposits_per_normalise && normalise()) return 1;
        launch(first, piece);
        GFHIP_TRY(ctx, hipGetLastError(), "deposit launch");
        pending += piece;
        first += piece;
    }
    return 0;
}

//  The limits of the axes of one kind of object and what it says when they are broken.
struct axis_rules {
    size_t per_axis, in_all;
    const char *count_refused, *order_refused, *cells_refused;
};
//  At most 4096 cells per axis (the edges are staged in LDS on both paths) and 2^20 in all (536 B each).
constexpr size_t flux_cell_limit = 4096, phase_cell_limit = static_cast<size_t> (1) << 20;

//  The `rank` axes checked one after the other (count, then finite and strictly increasing), then the cells in all; the
//  edges laid one after the other into `edges` and scale[a] = n[a]/(last edge - first edge).  Null, or why refused.
const char *axes_of(const axis_rules &rules, int rank, const double *const *axes, const size_t *n, std::vector<double> &edges,
                    size_t &cells, double *scale);

//  The scalars of a caller's map or field, or why it is refused; phase_field_of: a field whose c takes no part.
const char *flux_map_of(const gfhip_flux_map *given, flux::map &m);
const char *spectrum_field_of(const gfhip_spectrum_field *given, flux::field &f);
const char *phase_field_of(const gfhip_spectrum_field *given, flux::field &f);
//  The map, the field and the tables of a host call, or why they are refused.
const char *host_tables_of(const gfhip_flux_map *map, const gfhip_spectrum_field *field, flux::map &m, flux::field &f,
                           flux::host_tables &t);
//  The batches of a batched object, or why they are refused: 1 to 256, and at most 2^20 cells in all.
const char *batches_refused(size_t batch_count, size_t count);

//  The psi tables as [table cell][16] and the fpol tables as [interval][4] on the device (`field` null: no fpol).
//  psi_refused, fpol_refused: what to say when the host has no memory to repack them.
int upload_tables(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field, const std::string &psi_refused,
                  const std::string &fpol_refused, device_ptr<double> &packed, device_ptr<double> &fpol);

//  What the objects with a map share: the psi tables on the device, the edges the deposit kernel stages in LDS, the
//  shape of its launches, what the object is called in messages and the shape of its cells.
struct flux_cells : exact_cells {
    const char *noun = "";
    int rank = 0;                                      // the axes a merge names: n[0] .. n[rank - 1]
    size_t n[3] = {0, 0, 0};
    double scale[3] = {0.0, 0.0, 0.0};                 // n/(last edge - first edge): the kernel's first guess of a cell
    flux::map map = {};
    flux::field field = {};                            // of a field_cells
    device_ptr<double> packed, fpol, edges;
    launch_shape shape = {};
//  Batches of rays or particles (ray_batches.hpp): 0 for a plain object; otherwise the state is [batch][cell][limb],
//  `cells` counts all of them and `slab` those of one batch, which the launch shape is decided by.
    size_t batches = 0, slab = 0;

//  The field (field_of null: the object has none) and the map checked and uploaded with the edges, the launch shape
//  decided and the `count` cells allocated.  field_of: spectrum_field_of or phase_field_of.  prepare: the deposit kernels'
//  request for large dynamic LDS, made on the private path.
    int create(gfhip_context *context, const gfhip_flux_map *given, const gfhip_spectrum_field *given_field,
               const char *(*field_of)(const gfhip_spectrum_field *, flux::field &), size_t count,
               const std::vector<double> &all_edges, hipError_t (*prepare)(), size_t batch_count = 0);
    cell_tables tables() const { return {map, field, packed.get(), fpol.get()}; }
//  Why an add with an index (a ray's, or a particle's) is refused: only a batched object takes one, and first + count
//  fits 64 bits.
    const char *index_refused(bool of_particles, uint64_t first, size_t count) const;
};

//  N fp64 buffers of at least `count` elements, or the message about `noun`; nothing is enqueued.
template<size_t N>
int fp64_columns(gfhip_context *ctx, const char *noun, const uint64_t (&keys)[N], const size_t count, double **columns) {
    for (size_t c = 0; c < N; c++) {
        const buffer *found = find_buffer(ctx, keys[c]);
        if (!found) return 1;
        if (found->dtype != GFIR_F64) return ctx->fail(std::string(noun) + " takes fp64 buffers");
        if (found->count < count) return ctx->fail(std::string(noun) + " buffer is shorter than the sample count");
        columns[c] = static_cast<double *> (found->pointer);
    }
    return 0;
}

//  The object into its context's list / behind everything the context has queued, out of the list.
template<typename T>
T *adopt(gfhip_context *ctx, std::unique_ptr<T> &object) {
    T *raw = object.get();
    ctx->objects.push_back(std::move(object));
    return raw;
}
void destroy(context_object *object);

//  The bodies of the entry points every family has.  `entry`: the function's name, for its message.
int counts_of(exact_cells *c, uint64_t *samples, uint64_t *outside, uint64_t *skipped);
int state_of(exact_cells *c, const char *entry, int64_t *limbs);
int read_of(exact_cells *c, const char *entry, double divisor, double *values);
int merge_of(exact_cells *c, const char *entry, const int64_t *limbs, uint64_t samples, uint64_t outside, uint64_t skipped);
//  shape: the caller's n[0] .. n[rank - 1]; batched: gfhip_*_merge_batches with `batch_count`.
int merge_of(flux_cells *c, const char *entry, const int64_t *limbs, bool batched, size_t batch_count,
             std::initializer_list<size_t> shape, uint64_t samples, uint64_t outside, uint64_t skipped);
//  Not through enter(): it reads what create decided on the host and touches neither the device nor the stream.
int info_of(flux_cells *c, const char *entry, struct gfhip_flux_info *info);
//  Where an entry point without a context leaves `message`; returns 1.
int refuse(const char *message);

}  // namespace cells
}  // namespace gfhip

#endif
