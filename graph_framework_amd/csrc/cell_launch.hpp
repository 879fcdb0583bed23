//------------------------------------------------------------------------------
///  @file cell_launch.hpp
///  @brief What the host objects (cells_rays.cpp, cells_particles.cpp) launch of deposition.hip, flux_profile.hip,
///  flux_spectrum.hip, phase_bins.hip, moment_bins.hip, confinement.hip and particle_source.hip, and the three small
///  structs every deposit launch takes: the tables it reads, the shape it was decided to have and where its sums go.
//------------------------------------------------------------------------------
#ifndef GFHIP_CELL_LAUNCH_HPP
#define GFHIP_CELL_LAUNCH_HPP

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "flux_label.hpp"
#include "particle_draw.hpp"

namespace gfhip {

//  What a deposit reads beside its samples: the map, the field (unused by a profile and a tracker, whose fpol is null),
//  the psi tables as [table cell][16] and fpol as [interval][4], both on the device.
struct cell_tables {
    flux::map map;
    flux::field field;
    const double *packed, *fpol;
};

//  The shape of an object's deposit launches, decided once (flux_launch_shape); cap: the most cells the private path takes.
struct launch_shape {
    bool is_private;
    unsigned int block;
    size_t max_workgroups, lds_bytes, cap;
};

//  Where a launch deposits: cells x 67 limbs, the counters samples, outside, skipped, and the stream it runs on.
struct cell_target {
    void *state;
    unsigned long long *counters;
    hipStream_t stream;
};

//  deposition.hip.  A store of exact sums, cells x 67 limbs: canonical in place, rounded and divided into `values`,
//  and `words` limbs (or counters) of another one added in.
void launch_cells_normalise(void *state, const size_t cells, hipStream_t stream);
void launch_cells_round(const void *state, const size_t cells, const double divisor, double *values, hipStream_t stream);
void launch_cells_merge(void *state, const void *other, const size_t words, hipStream_t stream);
//  The deposits of a 3-D grid.  edges: the three axes' one after the other; scale: n/(last edge - first edge) per axis.
void launch_deposit(const double *x, const double *y, const double *z, const double *value, const size_t count,
                    const double *edges, const int nx, const int ny, const int nz, const double *scale,
                    void *state, unsigned long long *counters, const unsigned int num_cus, hipStream_t stream);

//  flux_profile.hip.  The shape of the deposit launches of an object of `cells` cells; edge_count: the edges staged in
//  LDS (a profile's cells + 1, a spectrum's two axes, ...).
launch_shape flux_launch_shape(const size_t cells, const size_t edge_count, const bool allow_private, const unsigned int num_cus);
hipError_t flux_prepare();
void launch_flux_deposit(const double *x, const double *y, const double *z, const double *value, const size_t count,
                         const cell_tables &t, const double *edges, const size_t cells, const double scale,
                         const launch_shape &shape, const cell_target &to);
//  The same with the samples' rays (ray_batches.hpp): sample i is ray first_ray + i; state: [batch][cell][limb]; the
//  launch shape is that of `cells`, the cells of ONE batch.
void launch_flux_deposit_rays(const double *x, const double *y, const double *z, const double *value, const size_t count,
                              const unsigned long long first_ray, const size_t batch_count, const cell_tables &t,
                              const double *edges, const size_t cells, const double scale, const launch_shape &shape,
                              const cell_target &to);
//  The quadrature points first .. first + count of flux_label.hpp; row = numz*sub, twice_sub = (double)(2*sub).
void launch_flux_volumes(const unsigned long long first, const size_t count, const unsigned long long row, const double twice_sub,
                         const double area, const flux::window &window, const cell_tables &t, const double *edges,
                         const size_t cells, const double scale, const launch_shape &shape, const cell_target &to);
void launch_flux_label(const double *x, const double *y, const double *z, const size_t count, const cell_tables &t,
                       double *label, hipStream_t stream);

//  flux_spectrum.hip.  columns: x, y, z, kx, ky, kz, w (and the value, for the deposit); edges: the n[0] + 1 of the
//  label, then the n[1] + 1 of N, scale[a] = n[a]/(last edge - first edge); the cell of (is, in) is is*n[1] + in.
hipError_t spectrum_prepare();
void launch_spectrum_deposit(const double *const *columns, const size_t first, const size_t count, const cell_tables &t,
                             const double *edges, const size_t *n, const double *scale, const launch_shape &shape,
                             const cell_target &to);
//  The same with the samples' rays: sample first + i of the columns is ray first_ray + i; state: [batch][is][in][limb].
void launch_spectrum_deposit_rays(const double *const *columns, const size_t first, const size_t count,
                                  const unsigned long long first_ray, const size_t batch_count, const cell_tables &t,
                                  const double *edges, const size_t *n, const double *scale, const launch_shape &shape,
                                  const cell_target &to);
void launch_spectrum_npar(const double *const *columns, const size_t count, const cell_tables &t, double *label, double *npar,
                          hipStream_t stream);

//  phase_bins.hip.  columns: x, y, z, ux, uy, uz, gamma and the weight (null: every particle deposits 1.0), all float
//  when is_f32 and all double otherwise; edges: the n[0] + 1 of the label, the n[1] + 1 of xi, the n[2] + 1 of gamma,
//  scale[a] = n[a]/(last edge - first edge); the cell of (is, ip, ig) is (is*n[1] + ip)*n[2] + ig.
hipError_t phase_prepare();
void launch_phase_deposit(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                          const cell_tables &t, const double *edges, const size_t *n, const double *scale,
                          const launch_shape &shape, const cell_target &to);
//  The same with the particles' indices in the ensemble (ray_batches.hpp's rule): particle first + i of the columns is
//  particle first_particle + i; state: [batch][is][ip][ig][limb]; the launch shape is that of the cells of ONE batch.
void launch_phase_deposit_particles(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                                    const unsigned long long first_particle, const size_t batch_count, const cell_tables &t,
                                    const double *edges, const size_t *n, const double *scale, const launch_shape &shape,
                                    const cell_target &to);
void launch_phase_coordinates(const void *const *columns, const bool is_f32, const size_t count, const cell_tables &t,
                              double *label, double *pitch, hipStream_t stream);

//  moment_bins.hip.  columns: as launch_phase_deposit's; edges: the ns + 1 of the label, sscale = ns/(last edge - first
//  edge); the cell of (is, k) is is*4 + k, k = density, current, energy, radiation.  values: [particle][4].
hipError_t moments_prepare();
void launch_moment_deposit(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                           const cell_tables &t, const double *edges, const size_t ns, const double sscale,
                           const launch_shape &shape, const cell_target &to);
//  The same per batch of particles: state [batch][surface][moment][limb].
void launch_moment_deposit_particles(const void *const *columns, const bool is_f32, const size_t first, const size_t count,
                                     const unsigned long long first_particle, const size_t batch_count, const cell_tables &t,
                                     const double *edges, const size_t ns, const double sscale, const launch_shape &shape,
                                     const cell_target &to);
void launch_moment_values(const void *const *columns, const bool is_f32, const size_t count, const cell_tables &t,
                          double *label, double *values, hipStream_t stream);

//  confinement.hip.  columns: as launch_phase_deposit's, of which x, y, z, gamma and the weight are read; alive: the
//  tracker's own column of the same type; edges: the n[0] + 1 of R, the n[1] + 1 of z, the n[2] + 1 of gamma; the cell of
//  (ir, iz, ig) is (ir*n[1] + iz)*n[2] + ig.  lost_step, alive and the exit buffers (both null without them) are indexed
//  by particle, first .. first + count; newly_lost is the entry of this check.  Always the global path's launch shape.
void launch_confinement_check(const void *const *columns, void *alive, const bool is_f32, const size_t first, const size_t count,
                              const cell_tables &t, const double limit, const double *edges, const size_t *n,
                              const double *scale, const uint32_t step, uint32_t *lost_step, double *exit_r, double *exit_z,
                              unsigned long long *newly_lost, const launch_shape &shape, const cell_target &to);
//  The sentinel into lost_step and 1 into alive (both null: left alone), NaN into the exit buffers (both null: none).
void launch_confinement_reset(const size_t count, uint32_t *lost_step, void *alive, const bool is_f32, double *exit_r,
                              double *exit_z, hipStream_t stream);

//  particle_source.hip.  columns: x, y, z, ux, uy, uz, gamma, all float when is_f32 and all double otherwise, and `placed`
//  of the same type (null: none): element i receives particle first_particle + i.  profile: the par.ns + 1 edges, then the
//  par.ns probabilities (unread when par.ns = 0), scale = ns/(last edge - first edge).  counters: placed, unplaced,
//  position_tries, gyro_tries.  max_workgroups: of 256 lanes.
void launch_particle_source(void *const *columns, void *placed, const bool is_f32, const size_t count,
                            const unsigned long long first_particle, const flux::map &m, const flux::field &f,
                            const draw::parameters &par, const double *packed, const double *fpol, const double *profile,
                            const double scale, const bool refill, const size_t max_workgroups, unsigned long long *counters,
                            hipStream_t stream);

}  // namespace gfhip

#endif
