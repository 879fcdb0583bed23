//------------------------------------------------------------------------------
///  @file cells_rays.cpp
///  @brief libgf_hip.so: the shared host pieces of cells.hpp and the ray-side objects on top of them: deposition grids
///  (gfhip_bins_*), flux profiles with their volumes (gfhip_flux_*), spectra (gfhip_spectrum_*) and gfhip_exact_sum.
//------------------------------------------------------------------------------
#include <cmath>
#include <cstring>
#include <limits>
#include <new>

#include "cells.hpp"
#include "ray_batches.hpp"

using namespace gfhip::cells;
namespace flux = gfhip::flux;
namespace superacc = gfhip::superacc;

//  Stores of exact sums (cell_launch.hpp, superacc.hpp).
int exact_cells::create(gfhip_context *context, const size_t count) {
    ctx = context;
    cells = count;
    const size_t bytes = cells*superacc::limbs*sizeof(int64_t);
    return ctx->check(allocate(state, bytes), "hipMalloc(cells)") ||
           ctx->check(hipMemset(state.get(), 0, bytes), "hipMemset(cells)") ||
           ctx->check(allocate(counters, 3*sizeof(unsigned long long)), "hipMalloc(counters)") ||
           ctx->check(hipMemset(counters.get(), 0, 3*sizeof(unsigned long long)), "hipMemset(counters)");
}

//  The state canonical in place: before the deposits since the last time could reach 2^30 (a limb takes 2^31),
//  before the state is handed out and before it is rounded.  Later deposits add to the canonical digits.
int exact_cells::normalise() {
    gfhip::launch_cells_normalise(state.get(), cells, ctx->stream);
    pending = 0;
    return ctx->check(hipGetLastError(), "normalise launch");
}

int exact_cells::counts(uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    if (enter(ctx)) return 1;
    unsigned long long host[3] = {0, 0, 0};
    GFHIP_TRY(ctx, hipMemcpyAsync(host, counters.get(), sizeof(host), hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(counters)");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (samples) *samples = host[0];
    if (outside) *outside = host[1];
    if (skipped) *skipped = host[2];
    return 0;
}

int exact_cells::state_to(int64_t *limbs) {
    if (enter(ctx) || normalise()) return 1;
    GFHIP_TRY(ctx, hipMemcpyAsync(limbs, state.get(), cells*superacc::limbs*sizeof(int64_t), hipMemcpyDeviceToHost,
                                  ctx->stream), "hipMemcpyAsync(cells)");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return 0;
}

int exact_cells::merge(const int64_t *limbs, const uint64_t samples, const uint64_t outside, const uint64_t skipped) {
    if (enter(ctx)) return 1;
    const size_t words = cells*superacc::limbs;
    const unsigned long long incoming[3] = {samples, outside, skipped};
    device_ptr<> other;                                // the incoming limbs, then the three counts
    GFHIP_TRY(ctx, allocate(other, (words + 3)*sizeof(int64_t)), "hipMalloc(merge)");
    char *counts_at = static_cast<char *> (other.get()) + words*sizeof(int64_t);
    GFHIP_TRY(ctx, hipMemcpyAsync(other.get(), limbs, words*sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(merge)");
    GFHIP_TRY(ctx, hipMemcpyAsync(counts_at, incoming, sizeof(incoming), hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(merge)");
//  Canonical digits (below 2^32) on top of a state that 2^30 deposits may have reached: still inside a limb.
    gfhip::launch_cells_merge(state.get(), other.get(), words, ctx->stream);
    gfhip::launch_cells_merge(counters.get(), counts_at, 3, ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "merge launch");
    if (normalise()) return 1;
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");      // `other` is freed on return
    return 0;
}

int exact_cells::read(const double divisor, double *values) {
    if (enter(ctx)) return 1;
    if (!rounded) GFHIP_TRY(ctx, allocate(rounded, cells*sizeof(double)), "hipMalloc(rounded cells)");
    if (normalise()) return 1;
    gfhip::launch_cells_round(state.get(), cells, divisor, rounded.get(), ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "round launch");
    GFHIP_TRY(ctx, hipMemcpyAsync(values, rounded.get(), cells*sizeof(double), hipMemcpyDeviceToHost, ctx->stream),
              "hipMemcpyAsync(rounded cells)");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return 0;
}

//  What the entry points share.
void gfhip::cells::destroy(context_object *object) {
    if (!object) return;
    gfhip_context *ctx = object->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    auto &owned = ctx->objects;
    for (auto it = owned.begin(); it != owned.end(); ++it) {
        if (it->get() == object) {
            owned.erase(it);
            return;
        }
    }
}

int gfhip::cells::counts_of(exact_cells *c, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return c ? c->counts(samples, outside, skipped) : 1;
}

int gfhip::cells::state_of(exact_cells *c, const char *entry, int64_t *limbs) {
    if (!c) return 1;
    if (!limbs) return c->ctx->fail(std::string(entry) + " needs a destination");
    return c->state_to(limbs);
}

int gfhip::cells::read_of(exact_cells *c, const char *entry, const double divisor, double *values) {
    if (!c) return 1;
    if (!values) return c->ctx->fail(std::string(entry) + " needs a destination");
    return c->read(divisor, values);
}

int gfhip::cells::merge_of(exact_cells *c, const char *entry, const int64_t *limbs, const uint64_t samples, const uint64_t outside,
                           const uint64_t skipped) {
    if (!c) return 1;
    if (!limbs) return c->ctx->fail(std::string(entry) + " needs a state");
    return c->merge(limbs, samples, outside, skipped);
}

int gfhip::cells::merge_of(flux_cells *c, const char *entry, const int64_t *limbs, const bool batched, const size_t batch_count,
                           const std::initializer_list<size_t> shape, const uint64_t samples, const uint64_t outside,
                           const uint64_t skipped) {
    if (!c) return 1;
    if (!limbs) return c->ctx->fail(std::string(entry) + " needs a state");
    bool same = batched ? c->batches && batch_count == c->batches : !c->batches;
    same = same && shape.size() == static_cast<size_t> (c->rank) && std::equal(shape.begin(), shape.end(), c->n);
    if (!same) return c->ctx->fail(std::string("merge: ") + c->noun + " of another shape");
    return c->merge(limbs, samples, outside, skipped);
}

int gfhip::cells::info_of(flux_cells *c, const char *entry, struct gfhip_flux_info *info) {
    if (!c) return 1;
    if (!info) return c->ctx->fail(std::string(entry) + " needs a destination");
    info->private_sums = c->shape.is_private ? 1u : 0u;
    info->workgroup_size = c->shape.block;
    info->cap_cells = c->shape.cap;
    info->max_workgroups = c->shape.max_workgroups;
    info->lds_bytes = c->shape.lds_bytes;
    return 0;
}

int gfhip::cells::refuse(const char *message) {
    creation_error = message;
    return 1;
}

const char *gfhip::cells::axes_of(const axis_rules &rules, const int rank, const double *const *axes, const size_t *n,
                                  std::vector<double> &edges, size_t &cells, double *scale) {
    cells = 1;
    for (int a = 0; a < rank; a++) {
        if (!axes[a] || n[a] < 1 || n[a] > rules.per_axis) return rules.count_refused;
        for (size_t i = 0; i <= n[a]; i++) {
            if (!std::isfinite(axes[a][i]) || (i && !(axes[a][i - 1] < axes[a][i]))) return rules.order_refused;
        }
        edges.insert(edges.end(), axes[a], axes[a] + n[a] + 1);
        cells *= n[a];                                 // at most 2^36
        scale[a] = static_cast<double> (n[a])/(axes[a][n[a]] - axes[a][0]);
    }
    return cells > rules.in_all ? rules.cells_refused : nullptr;
}

const char *gfhip::cells::flux_map_of(const gfhip_flux_map *given, flux::map &m) {
    if (!given->coefficients) return "a flux map needs its 16 coefficient tables";
    if (given->numr == 0 || given->numz == 0) return "a flux map needs numr >= 1 and numz >= 1";
    const uint64_t table_limit = 1ull << 31;
    if (given->numr > table_limit || given->numz > table_limit || given->numr*given->numz > table_limit) {
        return "a flux map's table has at most 2^31 cells";
    }
    if (!std::isfinite(given->dr) || given->dr == 0.0 || !std::isfinite(given->dz) || given->dz == 0.0 ||
        !std::isfinite(given->span) || given->span == 0.0) {
        return "dr, dz and span of a flux map must be finite and non-zero";
    }
    if (!std::isfinite(given->rmin) || !std::isfinite(given->zmin) || !std::isfinite(given->psi0)) {
        return "rmin, zmin and psi0 of a flux map must be finite";
    }
    if (given->flags & ~flux::known_flags) return "unknown flag bits in a flux map";
    if (given->reserved != 0) return "the reserved field of a flux map must be 0";
    m.rmin = given->rmin;
    m.dr = given->dr;
    m.zmin = given->zmin;
    m.dz = given->dz;
    m.numr = static_cast<double> (given->numr);
    m.numz = static_cast<double> (given->numz);
    m.columns = given->numz;
    m.psi0 = given->psi0;
    m.span = given->span;
    m.flags = given->flags;
    return nullptr;
}

const char *gfhip::cells::spectrum_field_of(const gfhip_spectrum_field *given, flux::field &f) {
    for (const double *table : given->fpol) {
        if (!table) return "a spectrum's field needs its four fpol tables";
    }
    if (given->numpsi == 0 || given->numpsi > 0x7fffffffull) return "a spectrum's field needs 1 <= numpsi <= 2^31 - 1";
    if (!std::isfinite(given->dpsi) || given->dpsi == 0.0 || !std::isfinite(given->c) || given->c == 0.0) {
        return "dpsi and c of a spectrum's field must be finite and non-zero";
    }
    if (!std::isfinite(given->psimin)) return "psimin of a spectrum's field must be finite";
    if (given->reserved != 0) return "the reserved field of a spectrum's field must be 0";
    f.psimin = given->psimin;
    f.dpsi = given->dpsi;
    f.numpsi = static_cast<double> (given->numpsi);
    f.last = static_cast<int> (given->numpsi - 1);
    f.c = given->c;
    return nullptr;
}

const char *gfhip::cells::phase_field_of(const gfhip_spectrum_field *given, flux::field &f) {
    gfhip_spectrum_field without_c = *given;
    without_c.c = 1.0;
    return spectrum_field_of(&without_c, f);
}

const char *gfhip::cells::host_tables_of(const gfhip_flux_map *map, const gfhip_spectrum_field *field, flux::map &m,
                                         flux::field &f, flux::host_tables &t) {
    if (const char *refused = flux_map_of(map, m)) return refused;
    if (const char *refused = field ? phase_field_of(field, f) : nullptr) return refused;
    t.coefficients = map->coefficients;
    t.table = static_cast<size_t> (map->numr*map->numz);
    for (size_t k = 0; k < 4; k++) t.fpol[k] = field ? field->fpol[k] : nullptr;
    return nullptr;
}

const char *gfhip::cells::batches_refused(const size_t batch_count, const size_t count) {
    if (batch_count < 1 || batch_count > gfhip::batches::max_batches) return "a batched object has 1 to 256 batches";
    if (batch_count*count > (static_cast<size_t> (1) << 20)) return "batches x cells is at most 2^20 (536 B each)";
    return nullptr;
}

//  `tables` tables of `length` elements, [k][element], as [element][k] on the device: a lane's coefficients are one line
//  (128 bytes of psi, 32 of fpol).  what: "flux tables" or "fpol tables"; refused: what to say without host memory.
static int upload_lines(gfhip_context *ctx, const double *const *from, const size_t tables, const size_t length, const char *what,
                        const std::string &refused, device_ptr<double> &to) {
    std::vector<double> lines;
    try {
        lines.resize(length*tables);
    } catch (const std::bad_alloc &) {
        return ctx->fail(refused);
    }
    for (size_t k = 0; k < tables; k++) {
        for (size_t at = 0; at < length; at++) lines[at*tables + k] = from[k][at];
    }
    const std::string name = std::string("(") + what + ")";
    return ctx->check(allocate(to, lines.size()*sizeof(double)), ("hipMalloc" + name).c_str()) ||
           ctx->check(hipMemcpy(to.get(), lines.data(), lines.size()*sizeof(double), hipMemcpyHostToDevice), ("hipMemcpy" + name).c_str());
}

int gfhip::cells::upload_tables(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                const std::string &psi_refused, const std::string &fpol_refused, device_ptr<double> &packed,
                                device_ptr<double> &fpol) {
    const size_t table = static_cast<size_t> (map->numr*map->numz);
    const double *psi[16];
    for (size_t k = 0; k < 16; k++) psi[k] = map->coefficients + k*table;
    return upload_lines(ctx, psi, 16, table, "flux tables", psi_refused, packed) ||
           (field && upload_lines(ctx, field->fpol, 4, static_cast<size_t> (field->numpsi), "fpol tables", fpol_refused, fpol));
}

int flux_cells::create(gfhip_context *context, const gfhip_flux_map *given, const gfhip_spectrum_field *given_field,
                       const char *(*field_of)(const gfhip_spectrum_field *, flux::field &), const size_t count,
                       const std::vector<double> &all_edges, hipError_t (*prepare)(), const size_t batch_count) {
    if (const char *refused = field_of ? field_of(given_field, field) : nullptr) return context->fail(refused);
    if (const char *refused = flux_map_of(given, map)) return context->fail(refused);
    if (context->check(hipSetDevice(context->device), "hipSetDevice")) return 1;
    batches = batch_count;
    slab = count;
    shape = gfhip::flux_launch_shape(count, all_edges.size(), !(given->flags & flux::flag_no_private_sums), context->num_cus);
    return upload_tables(context, given, field_of ? given_field : nullptr, "a flux map's tables do not fit the host's memory",
                         std::string(noun) + "'s fpol tables do not fit the host's memory", packed, fpol) ||
           context->check(allocate(edges, all_edges.size()*sizeof(double)), "hipMalloc(edges)") ||
           context->check(hipMemcpy(edges.get(), all_edges.data(), all_edges.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(edges)") ||
           exact_cells::create(context, batch_count ? batch_count*count : count) ||
           (shape.is_private && context->check(prepare(), "hipFuncSetAttribute(flux deposit)"));
}

const char *flux_cells::index_refused(const bool of_particles, const uint64_t first, const size_t count) const {
    if (!batches) {
        return of_particles ? "only a batched object (gfhip_phase_create_batched, gfhip_moments_create_batched) takes particles with their index"
                            : "only a batched object (gfhip_flux_create_batched, gfhip_spectrum_create_batched) takes samples with a ray index";
    }
    if (first + static_cast<uint64_t> (count) < first) {
        return of_particles ? "first_particle + count overflows 64 bits" : "first_ray + count overflows 64 bits";
    }
    return nullptr;
}

//  Deposition grids (deposition.hip).  The limits of a grid: at most 2047 cells per axis, so that the
//  three axes' edges (3 x 2048 doubles, 48 KiB) fit the LDS a workgroup gets without asking; at most 2^25 cells
//  (536 B each: 16.8 GiB of state), so that cell*64 + limb fits the 32-bit key the deposit kernel compares.
static const axis_rules bins_rules = {2047, static_cast<size_t> (1) << 25, "a deposition grid has 1 to 2047 cells per axis",
                                      "the edges of a deposition grid must be finite and strictly increasing",
                                      "a deposition grid has at most 2^25 cells (536 B each)"};

//  A 3-D deposition grid.
struct gfhip_bins : exact_cells {
    int n[3] = {0, 0, 0};
    double scale[3] = {0.0, 0.0, 0.0};                 // n/(last edge - first edge): the kernel's first guess of a cell
    device_ptr<double> edges;                          // the three axes' edges one after the other
};

extern "C" gfhip_bins *gfhip_bins_create(gfhip_context *ctx, const double *xedges, size_t nx,
                                         const double *yedges, size_t ny, const double *zedges, size_t nz) {
    if (!ctx) return nullptr;
    const double *axes[3] = {xedges, yedges, zedges};
    const size_t n[3] = {nx, ny, nz};
    std::vector<double> edges;
    size_t cells = 0;
    std::unique_ptr<gfhip_bins> b(new gfhip_bins);
    if (const char *refused = axes_of(bins_rules, 3, axes, n, edges, cells, b->scale)) {
        ctx->fail(refused);
        return nullptr;
    }
    if (ctx->check(hipSetDevice(ctx->device), "hipSetDevice")) return nullptr;
    for (int a = 0; a < 3; a++) b->n[a] = static_cast<int> (n[a]);
    if (ctx->check(allocate(b->edges, edges.size()*sizeof(double)), "hipMalloc(edges)") ||
        ctx->check(hipMemcpy(b->edges.get(), edges.data(), edges.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(edges)") ||
        b->create(ctx, cells)) {
        return nullptr;
    }
    return adopt(ctx, b);
}

extern "C" void gfhip_bins_destroy(gfhip_bins *b) {
    destroy(b);
}

extern "C" int gfhip_bins_add(gfhip_bins *b, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t value_key, size_t count) {
    if (!b) return 1;
    double *columns[4];
    if (fp64_columns(b->ctx, "a deposition grid", {x_key, y_key, z_key, value_key}, count, columns)) return 1;
    return b->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_deposit(columns[0] + first, columns[1] + first, columns[2] + first, columns[3] + first, piece,
                              b->edges.get(), b->n[0], b->n[1], b->n[2], b->scale, b->state.get(), b->counters.get(),
                              b->ctx->num_cus, b->ctx->stream);
    });
}

extern "C" int gfhip_bins_counts(gfhip_bins *b, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return counts_of(b, samples, outside, skipped);
}

extern "C" int gfhip_bins_state(gfhip_bins *b, int64_t *limbs) {
    return state_of(b, "gfhip_bins_state", limbs);
}

extern "C" int gfhip_bins_merge(gfhip_bins *b, const int64_t *limbs, uint64_t samples, uint64_t outside, uint64_t skipped) {
    return merge_of(b, "gfhip_bins_merge", limbs, samples, outside, skipped);
}

extern "C" int gfhip_bins_read(gfhip_bins *b, double divisor, double *bins) {
    return read_of(b, "gfhip_bins_read", divisor, bins);
}

//  Flux profiles (flux_profile.hip, flux_label.hpp).  At most 4096 cells: the edges are staged in LDS on both paths.
static const axis_rules flux_rules = {flux_cell_limit, flux_cell_limit, "a flux profile has 1 to 4096 cells",
                                      "the edges of a flux profile must be finite and strictly increasing", ""};

//  A flux-surface profile: n[0] cells, scale[0] = cells/(last edge - first edge).
struct gfhip_flux : flux_cells {};

//  batch_count: 0 for gfhip_flux_create.
static gfhip_flux *flux_create(gfhip_context *ctx, const gfhip_flux_map *map, const double *edges, const size_t cells,
                               const size_t batch_count) {
    if (!map || !edges) {
        ctx->fail("a flux profile needs a map and edges");
        return nullptr;
    }
    std::unique_ptr<gfhip_flux> f(new gfhip_flux);
    f->noun = "a flux profile";
    f->rank = 1;
    f->n[0] = cells;
    std::vector<double> staged;
    size_t total = 0;
    if (const char *refused = axes_of(flux_rules, 1, &edges, &cells, staged, total, f->scale)) {
        ctx->fail(refused);
        return nullptr;
    }
    if (f->create(ctx, map, nullptr, nullptr, cells, staged, gfhip::flux_prepare, batch_count)) return nullptr;
    return adopt(ctx, f);
}

extern "C" gfhip_flux *gfhip_flux_create(gfhip_context *ctx, const gfhip_flux_map *map, const double *edges, size_t cells) {
    return ctx ? flux_create(ctx, map, edges, cells, 0) : nullptr;
}

extern "C" gfhip_flux *gfhip_flux_create_batched(gfhip_context *ctx, const gfhip_flux_map *map, const double *edges, size_t cells,
                                                 size_t batches) {
    if (!ctx) return nullptr;
    if (const char *refused = batches_refused(batches, cells)) {
        ctx->fail(refused);
        return nullptr;
    }
    return flux_create(ctx, map, edges, cells, batches);
}

extern "C" void gfhip_flux_destroy(gfhip_flux *f) {
    destroy(f);
}

extern "C" int gfhip_flux_add(gfhip_flux *f, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t value_key, size_t count) {
    if (!f) return 1;
    if (f->batches) return f->ctx->fail("a batched flux profile takes its samples with their ray index: gfhip_flux_add_rays");
    double *columns[4];
    if (fp64_columns(f->ctx, "a flux profile", {x_key, y_key, z_key, value_key}, count, columns)) return 1;
    return f->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_flux_deposit(columns[0] + first, columns[1] + first, columns[2] + first, columns[3] + first, piece,
                                   f->tables(), f->edges.get(), f->cells, f->scale[0], f->shape, f->target());
    });
}

extern "C" int gfhip_flux_add_rays(gfhip_flux *f, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t value_key, size_t count,
                                   uint64_t first_ray) {
    if (!f) return 1;
    if (const char *refused = f->index_refused(false, first_ray, count)) return f->ctx->fail(refused);
    double *columns[4];
    if (fp64_columns(f->ctx, "a flux profile", {x_key, y_key, z_key, value_key}, count, columns)) return 1;
    return f->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_flux_deposit_rays(columns[0] + first, columns[1] + first, columns[2] + first, columns[3] + first, piece,
                                        first_ray + first, f->batches, f->tables(), f->edges.get(), f->slab, f->scale[0],
                                        f->shape, f->target());
    });
}

extern "C" int gfhip_flux_label(gfhip_flux *f, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t label_key, size_t count) {
    if (!f) return 1;
    gfhip_context *ctx = f->ctx;
    double *columns[4];
    if (fp64_columns(ctx, "a flux profile", {x_key, y_key, z_key, label_key}, count, columns)) return 1;
    if (enter(ctx)) return 1;
    gfhip::launch_flux_label(columns[0], columns[1], columns[2], count, f->tables(), columns[3], ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "flux label launch");
    return 0;
}

extern "C" int gfhip_flux_counts(gfhip_flux *f, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return counts_of(f, samples, outside, skipped);
}

extern "C" int gfhip_flux_state(gfhip_flux *f, int64_t *limbs) {
    return state_of(f, "gfhip_flux_state", limbs);
}

extern "C" int gfhip_flux_merge(gfhip_flux *f, const int64_t *limbs, size_t cells, uint64_t samples, uint64_t outside, uint64_t skipped) {
    return merge_of(f, "gfhip_flux_merge", limbs, false, 0, {cells}, samples, outside, skipped);
}

extern "C" int gfhip_flux_merge_batches(gfhip_flux *f, const int64_t *limbs, size_t batches, size_t cells, uint64_t samples,
                                        uint64_t outside, uint64_t skipped) {
    return merge_of(f, "gfhip_flux_merge_batches", limbs, true, batches, {cells}, samples, outside, skipped);
}

extern "C" int gfhip_flux_read(gfhip_flux *f, double divisor, double *values) {
    return read_of(f, "gfhip_flux_read", divisor, values);
}

extern "C" int gfhip_flux_info(gfhip_flux *f, struct gfhip_flux_info *info) {
    return info_of(f, "gfhip_flux_info", info);
}

//  Host side, no device: flux_label.hpp on the caller's 16 tables.
extern "C" int gfhip_flux_label_host(const gfhip_flux_map *map, const double *x, const double *y, const double *z,
                                     size_t count, double *label) {
    if (!map || ((!x || !y || !z || !label) && count)) {
        return refuse("gfhip_flux_label_host needs a map, three coordinate arrays and a destination");
    }
    flux::map m;
    flux::field unused;
    flux::host_tables t;
    if (const char *refused = host_tables_of(map, nullptr, m, unused, t)) return refuse(refused);
    for (size_t s = 0; s < count; s++) label[s] = flux::host_label(m, t, x[s], y[s], z[s]);
    return 0;
}

//  What a run of quadrature points needs beside the map (flux_label.hpp), or why it is refused.
struct volume_points {
    unsigned long long row = 0;                        // numz*sub: the sub-cells along z
    double twice_sub = 0.0, area = 0.0;
    flux::window window = {};
};

static const char *volume_points_of(const flux::map &m, const uint32_t sub, const gfhip_flux_window *window,
                                    const uint64_t first, const uint64_t count, volume_points &p) {
    if (sub < 1 || sub > 256) return "flux volumes: sub must be 1 to 256";
    if (!(m.dr > 0.0) || !(m.dz > 0.0) || !(m.rmin >= 0.0)) return "flux volumes need a map with dr > 0, dz > 0 and rmin >= 0";
//  numr*numz <= 2^31 and sub*sub <= 2^16: the total fits 64 bits with room to spare.
    p.row = m.columns*sub;
    const uint64_t total = static_cast<uint64_t> (m.numr)*sub*p.row;
    if (first + count < first || first + count > total) return "flux volumes: first + count exceeds the numr*sub*numz*sub points of the map";
    const double inf = std::numeric_limits<double>::infinity();
    p.window = window ? flux::window{window->rlo, window->rhi, window->zlo, window->zhi} : flux::window{-inf, inf, -inf, inf};
    if (!(p.window.rlo < p.window.rhi) || !(p.window.zlo < p.window.zhi)) return "flux volumes: a window needs rlo < rhi and zlo < zhi, no NaN";
    p.twice_sub = static_cast<double> (2u*sub);
    p.area = flux::sub_area(m, sub);
    return nullptr;
}

extern "C" int gfhip_flux_add_volumes(gfhip_flux *f, uint32_t sub, const gfhip_flux_window *window, uint64_t first, uint64_t count) {
    if (!f) return 1;
    if (f->batches) return f->ctx->fail("flux volumes have no rays: a batched flux profile does not take them");
    volume_points p;
    if (const char *refused = volume_points_of(f->map, sub, window, first, count, p)) return f->ctx->fail(refused);
    return f->add(count, [&](const size_t done, const size_t piece) {
        gfhip::launch_flux_volumes(first + done, piece, p.row, p.twice_sub, p.area, p.window, f->tables(), f->edges.get(),
                                   f->cells, f->scale[0], f->shape, f->target());
    });
}

//  Host side, no device: the quadrature and the label of flux_label.hpp and superacc.hpp's deposit on the CPU.
extern "C" int gfhip_flux_volumes_host(const gfhip_flux_map *map, const double *edges, size_t cells, uint32_t sub,
                                       const gfhip_flux_window *window, uint64_t first, uint64_t count,
                                       int64_t *limbs, uint64_t counters[3]) {
    if (!map || !edges || !limbs || !counters) return refuse("gfhip_flux_volumes_host needs a map, edges, limbs and counters");
    std::vector<double> staged;
    size_t total = 0;
    double scale = 0.0;
    if (const char *refused = axes_of(flux_rules, 1, &edges, &cells, staged, total, &scale)) return refuse(refused);
    flux::map m;
    flux::field unused;
    flux::host_tables t;
    volume_points p;
    const char *refused = host_tables_of(map, nullptr, m, unused, t);
    if (!refused) refused = volume_points_of(m, sub, window, first, count, p);
    if (refused) return refuse(refused);
    const auto normalise_all = [&]() {
        for (size_t cell = 0; cell < cells; cell++) superacc::normalise(limbs + cell*superacc::limbs);
    };
    uint64_t pending = 0, outside = 0, skipped = 0;
    unsigned long long gr = first/p.row, gz = first%p.row;
    for (uint64_t done = 0; done < count; done++) {
        const double r = flux::sub_centre(m.rmin, m.dr, gr, p.twice_sub);
        const double z = flux::sub_centre(m.zmin, m.dz, gz, p.twice_sub);
        if (++gz == p.row) {
            gz = 0;
            gr++;
        }
        const double label = flux::in_window(p.window, r, z) ? flux::host_label(m, t, r, 0.0, z) : std::numeric_limits<double>::quiet_NaN();
        if (!(label >= edges[0] && label < edges[cells])) {            // off the window, off the map or in no cell
            outside++;
            continue;
        }
        const size_t cell = static_cast<size_t> (std::upper_bound(edges, edges + cells + 1, label) - edges) - 1;
        const double w = flux::sub_weight(r, p.area);
        if (!superacc::is_finite(w)) {
            skipped++;
            continue;
        }
        if (++pending > superacc::deposits_per_normalise) {
            normalise_all();
            pending = 1;
        }
        superacc::deposit(limbs + cell*superacc::limbs, w);
    }
    normalise_all();
    counters[0] += count;
    counters[1] += outside;
    counters[2] += skipped;
    return 0;
}

//  Spectra over the flux label and N (flux_spectrum.hip, flux_label.hpp).  At most 4096 cells per axis and 2^16 in all
//  (536 B each: 35 MB of state); the two axes' edges are staged in LDS on both paths.
static const axis_rules spectrum_rules = {flux_cell_limit, static_cast<size_t> (1) << 16, "a spectrum has 1 to 4096 cells per axis",
                                          "the edges of a spectrum must be finite and strictly increasing",
                                          "a spectrum has at most 65536 cells (536 B each)"};

//  A spectrum over the flux label and N: cell is*nn + in; the edges of the label, then those of N.
struct gfhip_spectrum : flux_cells {};

//  batch_count: 0 for gfhip_spectrum_create.
static gfhip_spectrum *spectrum_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                       const double *sedges, const size_t ns, const double *nedges, const size_t nn,
                                       const size_t batch_count) {
    if (!map || !field || !sedges || !nedges) {
        ctx->fail("a spectrum needs a map, a field and two edge arrays");
        return nullptr;
    }
    const double *axes[2] = {sedges, nedges};
    const size_t n[2] = {ns, nn};
    std::unique_ptr<gfhip_spectrum> s(new gfhip_spectrum);
    s->noun = "a spectrum";
    s->rank = 2;
    std::copy(n, n + 2, s->n);
    std::vector<double> edges;
    size_t cells = 0;
//  Both counts and their product before either axis' order: what a spectrum has always said first.
    const char *refused = ns < 1 || ns > flux_cell_limit || nn < 1 || nn > flux_cell_limit ? spectrum_rules.count_refused
                        : ns*nn > spectrum_rules.in_all ? spectrum_rules.cells_refused
                        : axes_of(spectrum_rules, 2, axes, n, edges, cells, s->scale);
    if (refused) {
        ctx->fail(refused);
        return nullptr;
    }
    if (s->create(ctx, map, field, spectrum_field_of, cells, edges, gfhip::spectrum_prepare, batch_count)) return nullptr;
    return adopt(ctx, s);
}

extern "C" gfhip_spectrum *gfhip_spectrum_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                                 const double *sedges, size_t ns, const double *nedges, size_t nn) {
    return ctx ? spectrum_create(ctx, map, field, sedges, ns, nedges, nn, 0) : nullptr;
}

extern "C" gfhip_spectrum *gfhip_spectrum_create_batched(gfhip_context *ctx, const gfhip_flux_map *map,
                                                         const gfhip_spectrum_field *field, const double *sedges, size_t ns,
                                                         const double *nedges, size_t nn, size_t batches) {
    if (!ctx) return nullptr;
//  Either axis has at most 4096 cells (checked below): the product cannot wrap here.
    if (const char *refused = batches_refused(batches, ns <= flux_cell_limit && nn <= flux_cell_limit ? ns*nn : 0)) {
        ctx->fail(refused);
        return nullptr;
    }
    return spectrum_create(ctx, map, field, sedges, ns, nedges, nn, batches);
}

extern "C" void gfhip_spectrum_destroy(gfhip_spectrum *s) {
    destroy(s);
}

//  The eight fp64 columns of a spectrum's samples, or the message.
static int spectrum_columns(gfhip_spectrum *s, const uint64_t *keys, const size_t count, double **columns) {
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], keys[7]};
    return fp64_columns(s->ctx, "a spectrum", all, count, columns);
}

extern "C" int gfhip_spectrum_add(gfhip_spectrum *s, const uint64_t keys[8], size_t count) {
    if (!s) return 1;
    if (!keys) return s->ctx->fail("gfhip_spectrum_add needs its 8 keys");
    if (s->batches) return s->ctx->fail("a batched spectrum takes its samples with their ray index: gfhip_spectrum_add_rays");
    double *columns[8];
    if (spectrum_columns(s, keys, count, columns)) return 1;
    return s->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_spectrum_deposit(columns, first, piece, s->tables(), s->edges.get(), s->n, s->scale, s->shape, s->target());
    });
}

extern "C" int gfhip_spectrum_add_rays(gfhip_spectrum *s, const uint64_t keys[8], size_t count, uint64_t first_ray) {
    if (!s) return 1;
    if (!keys) return s->ctx->fail("gfhip_spectrum_add_rays needs its 8 keys");
    if (const char *refused = s->index_refused(false, first_ray, count)) return s->ctx->fail(refused);
    double *columns[8];
    if (spectrum_columns(s, keys, count, columns)) return 1;
    return s->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_spectrum_deposit_rays(columns, first, piece, first_ray + first, s->batches, s->tables(), s->edges.get(),
                                            s->n, s->scale, s->shape, s->target());
    });
}

extern "C" int gfhip_spectrum_npar(gfhip_spectrum *s, const uint64_t keys[7], uint64_t label_key, uint64_t npar_key, size_t count) {
    if (!s) return 1;
    gfhip_context *ctx = s->ctx;
    if (!keys) return ctx->fail("gfhip_spectrum_npar needs its 7 keys");
    const uint64_t all[9] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], label_key, npar_key};
    double *columns[9];
    if (fp64_columns(ctx, "a spectrum", all, count, columns)) return 1;
    if (enter(ctx)) return 1;
    gfhip::launch_spectrum_npar(columns, count, s->tables(), columns[7], columns[8], ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "spectrum npar launch");
    return 0;
}

extern "C" int gfhip_spectrum_counts(gfhip_spectrum *s, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return counts_of(s, samples, outside, skipped);
}

extern "C" int gfhip_spectrum_state(gfhip_spectrum *s, int64_t *limbs) {
    return state_of(s, "gfhip_spectrum_state", limbs);
}

extern "C" int gfhip_spectrum_merge(gfhip_spectrum *s, const int64_t *limbs, size_t ns, size_t nn, uint64_t samples, uint64_t outside,
                                    uint64_t skipped) {
    return merge_of(s, "gfhip_spectrum_merge", limbs, false, 0, {ns, nn}, samples, outside, skipped);
}

extern "C" int gfhip_spectrum_merge_batches(gfhip_spectrum *s, const int64_t *limbs, size_t batches, size_t ns, size_t nn,
                                            uint64_t samples, uint64_t outside, uint64_t skipped) {
    return merge_of(s, "gfhip_spectrum_merge_batches", limbs, true, batches, {ns, nn}, samples, outside, skipped);
}

extern "C" int gfhip_spectrum_read(gfhip_spectrum *s, double divisor, double *values) {
    return read_of(s, "gfhip_spectrum_read", divisor, values);
}

extern "C" int gfhip_spectrum_info(gfhip_spectrum *s, struct gfhip_flux_info *info) {
    return info_of(s, "gfhip_spectrum_info", info);
}

//  Host side, no device: flux_label.hpp on the caller's 16 + 4 tables.
extern "C" int gfhip_spectrum_npar_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *const columns[7],
                                        size_t count, double *label, double *npar) {
    bool complete = map && field && columns && ((label && npar) || !count);
    for (int k = 0; complete && k < 7; k++) complete = columns[k] || !count;
    if (!complete) return refuse("gfhip_spectrum_npar_host needs a map, a field, seven columns and two destinations");
    flux::map m;
    flux::field f;
    flux::host_tables t;
    const char *refused = host_tables_of(map, nullptr, m, f, t);
    if (!refused) refused = spectrum_field_of(field, f);
    if (refused) return refuse(refused);
    for (size_t k = 0; k < 4; k++) t.fpol[k] = field->fpol[k];
    for (size_t s = 0; s < count; s++) {
        const double x = columns[0][s], y = columns[1][s];
        flux::host_point_values p;
        if (!flux::host_point(m, f, t, x, y, columns[2][s], p)) {
            label[s] = npar[s] = std::numeric_limits<double>::quiet_NaN();
            continue;
        }
        label[s] = p.label;
        npar[s] = flux::npar_of(f, x, y, flux::radius_of(x, y), columns[3][s], columns[4][s], columns[5][s], columns[6][s], p.gr,
                                p.gz, p.fpol);
    }
    return 0;
}

//  Host side, no device: the functions of superacc.hpp that the kernels run, on one accumulator.
extern "C" int gfhip_exact_sum(const double *values, size_t count, double *sum, int64_t *limbs) {
    if ((!values && count) || !sum) return 1;
    int64_t acc[superacc::limbs] = {0};
    uint64_t pending = 0;
    for (size_t i = 0; i < count; i++) {
        if (!superacc::is_finite(values[i])) return refuse("gfhip_exact_sum takes finite values");
        if (++pending > superacc::deposits_per_normalise) {
            superacc::normalise(acc);
            pending = 1;
        }
        superacc::deposit(acc, values[i]);
    }
    superacc::normalise(acc);
    *sum = superacc::round(acc);
    if (limbs) std::memcpy(limbs, acc, sizeof(acc));
    return 0;
}
