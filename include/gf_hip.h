/* ---------------------------------------------------------------------------
 * gf_hip.h — C ABI of libgf_hip.so, the MI355X (gfx950) backend for
 * graph_framework work items.
 *
 * This is the drop-in boundary.  Every entry point replaces one member of the
 * reference's duck-typed backend context (the thing jit::context<T,SAFE_MATH>
 * forwards to: graph_framework/jit.hpp:63-74, :87-338; models
 * gpu::cpu_context cpu_context.hpp:82-611 and gpu::cuda_context
 * cuda_context.hpp:73-1005).  graph_framework_amd/hip_context.hpp is the thin
 * C++ class with the reference's member names that calls these functions; it
 * is what a maintainer adds next to cuda_context.hpp.
 *
 * The reference hands its backend a work item as generated C++ text plus the
 * node lists; this backend takes the node DAG itself, serialized as GFIR
 * (include/gfir.h), and lowers it to a CDNA4 kernel: one wavefront lane per
 * ray/particle, SoA state, spline coefficient tables re-laid-out AoS per cell
 * and staged through LDS where they fit.
 *
 * Conventions: plain pointers and sizes only.  Functions returning int return
 * 0 on success, non-zero on failure with a message in gfhip_last_error().
 * A context is bound to one device and one stream and is not thread safe
 * (one context per host thread/rank, as in the reference).  Buffers are keyed
 * by an opaque 64-bit value chosen by the caller (the reference keys them by
 * leaf_node*, cpu_context.hpp:87-89, cuda_context.hpp:78-80) and are shared by
 * all kernels of the context.
 * ------------------------------------------------------------------------- */
#ifndef GF_HIP_H
#define GF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gfhip_context gfhip_context;
typedef struct gfhip_kernel gfhip_kernel;
typedef struct gfhip_bins gfhip_bins;

/* Number of devices = number of host threads/ranks a driver should start.
 * Replaces  static size_t max_concurrency()   (cuda_context.hpp:121-125, jit.hpp:87). */
int gfhip_max_concurrency(void);

/* Replaces  static std::string device_type()  (cuda_context.hpp:130-132, jit.hpp:92). */
const char *gfhip_device_type(void);

/* Host side, no device: the contiguous split every reference driver applies to its ensemble, one
 * shard per device thread:  batch = total/shards, extra = total%shards, shard `index` holds
 * batch + (extra > index ? 1 : 0) elements  (graph_benchmark/xrays_bench.cpp:38-51,
 * graph_driver/xrays.cpp:423-432, graph_korc/xkorc.cpp:20-25).  Writes [*begin, *end) of the
 * shard; returns 1 if shards == 0 or index >= shards. */
int gfhip_shard_bounds(size_t total, size_t shards, size_t index, size_t *begin, size_t *end);

/* Bind device `index`.  `stream` is a hipStream_t to launch on, or NULL to
 * create a private one.  Replaces the context constructor  ctx(const size_t index)
 * (cuda_context.hpp:137-148, jit.hpp:101).  Returns NULL on failure
 * (gfhip_last_error(NULL) has the reason). */
gfhip_context *gfhip_create_context(int index, void *stream);

/* Frees every buffer, module and stream the context owns.
 * Replaces ~cuda_context (cuda_context.hpp:153-185). */
void gfhip_destroy_context(gfhip_context *ctx);

/* Message of the last failure on this context (ctx may be NULL for creation errors). */
const char *gfhip_last_error(const gfhip_context *ctx);

/* Register one work item.  `gfir`/`bytes` is the serialized item (include/gfir.h);
 * `num_rays` is the ensemble size it runs over.
 * Replaces jit::context::add_kernel (jit.hpp:118-194) together with the
 * backend's create_kernel_prefix/create_kernel_postfix
 * (cuda_context.hpp:713-946, cpu_context.hpp:428-584). */
gfhip_kernel *gfhip_add_kernel(gfhip_context *ctx, const void *gfir, size_t bytes, size_t num_rays);

/* The same at a lowering level the caller chooses; gfhip_add_kernel is level 0.
 *   0  the lowering as it has always been;
 *   1  the assembly statement of a large fp64 item (the RK4 step) also folds what is exact for every operand but a NaN:
 *      multiplications by -1.0 become sign modifiers, records that differ in operand order and equal square roots are
 *      computed once.  Lanes that store a NaN are computed again by the unchanged redo kernel, so the stored bits are
 *      those of level 0.  Items whose pass is compiled have the same text at both levels.
 * GFHIP_LEVEL=0|1 in the environment overrides `level`; gfhip_kernel_get_info reports the level in force. */
gfhip_kernel *gfhip_add_kernel_at(gfhip_context *ctx, const void *gfir, size_t bytes, size_t num_rays, uint32_t level);

/* Lower and build every kernel added so far (pre-built code objects are looked
 * up by source hash in the kernel cache directories, otherwise hipRTC).
 * Replaces  void compile(source, names, add_reduction)  (cuda_context.hpp:194-302, jit.hpp:238-244). */
int gfhip_compile(gfhip_context *ctx);

/* Bind the kernel's arguments to buffers.  input_keys[i] / output_keys[o] name
 * the buffers; on first sight of a key the buffer is allocated with num_rays
 * elements (zero-filled) and, for inputs with a non-NULL input_init[i], its first
 * input_counts[i] elements (num_rays if input_counts is NULL) are filled from
 * that host array.  Replaces  create_kernel_call(name, inputs, outputs, state,
 * num_rays, ...)  (cuda_context.hpp:316-531, cpu_context.hpp:233-298). */
int gfhip_create_kernel_call(gfhip_kernel *kernel,
                             const uint64_t *input_keys, const void *const *input_init,
                             const size_t *input_counts, const uint64_t *output_keys);

/* Asynchronous launch of the kernel on the context's stream (the closure
 * create_kernel_call returns in the reference).  `steps` > 1 repeats the item
 * inside one launch, keeping the state in registers between passes. */
int gfhip_run(gfhip_kernel *kernel, uint32_t steps);

/* Run the kernel, reduce max over its LAST output on the device, synchronise and
 * return the scalar.  Items of up to 1500 nodes reduce inside the launch
 * (`<name>_max`: wave shuffle + one atomic per workgroup); larger ones run the
 * separate reduction kernel over the output buffer.  Replaces
 * create_max_call(arg, run)  (cuda_context.hpp:540-576, cpu_context.hpp:306-322).
 * Called again and again with no other entry point in between — which is what the
 * reference's converge_item::run (workflow.hpp:179-205) does through that closure — it
 * runs ahead: from the second call of the streak on, one `<name>_batch` launch runs
 * the asked pass and the next ones, each with its own max, the following calls are
 * answered from those without a launch or a synchronisation, and the next entry point
 * of any kind first takes back the passes nobody asked for (state of the beginning of
 * the batch restored, the asked passes run again).  Same values, same state, fewer
 * launches (10 instead of 25 for the benchmark's Newton solve); GFHIP_RUN_AHEAD=0
 * keeps one launch per call. */
int gfhip_run_max(gfhip_kernel *kernel, double *max_value);

/* The same for items of a complex type (enum gfir_dtype GFIR_C32 / GFIR_C64): value[0] + i value[1] =
 * the element of largest modulus of the last output, the first of equals, as
 * cpu_context.hpp:314-318 selects it (std::max_element on std::abs). */
int gfhip_run_max_complex(gfhip_kernel *kernel, double *value);

/* Reduce a BUFFER, whatever wrote it: value[0] (+ i value[1] for a complex buffer) = the max of its
 * elements as cpu_context takes it (std::max_element, cpu_context.hpp:306-322: a NaN only if it is
 * element 0; complex: the element of largest modulus, the first of equals), after everything queued on
 * the context's stream; synchronises.  This is the general form of  create_max_call(arg, run)
 * (jit.hpp:274-277): the caller runs `run` and then reduces `arg`'s buffer, which need not be the last
 * output of the kernel that `run` launches. */
int gfhip_reduce_max(gfhip_context *ctx, uint64_t key, double *value);

/* The loop of workflow::converge_item::run (workflow.hpp:179-205) around
 * gfhip_run_max: repeat until |max| <= tol, or max stalls against the previous
 * or the previous-but-one value, or max_iterations.  The loop's test runs on the
 * device after each pass and passes are queued ahead of the host, so the host
 * synchronises once per batch of passes; the passes that run, the iteration
 * count and the results are identical to calling gfhip_run_max from that loop. */
int gfhip_converge(gfhip_kernel *kernel, double tolerance, size_t max_iterations,
                   size_t *iterations, double *last_max);

/* The same stall loop run PER RAY inside one launch: each lane iterates on its own residual
 * and a wavefront leaves the loop when the ballot of active lanes is empty.  This is the
 * reference loop applied to every ray as its own shard: identical to gfhip_converge when the
 * rays are identical (the benchmark), otherwise rays stop as soon as they have stalled
 * instead of iterating until the slowest ray of the shard has.  `iterations` receives the
 * maximum over rays, `last_max` the maximum final residual. */
int gfhip_converge_per_ray(gfhip_kernel *kernel, double tolerance, size_t max_iterations,
                           size_t *iterations, double *last_max);

/* Drain the stream.  Replaces  void wait()  (cuda_context.hpp:581-584). */
int gfhip_wait(gfhip_context *ctx);

/* Status bits raised by kernels since the context was created (after a drain);
 * informational: the lanes concerned redid their pass with the compiler's IEEE
 * division, results are the IEEE ones either way.
 * Bit 0: a lane failed a check of the shared-reciprocal division (fp64: a
 *        denominator outside [2^-500, 2^500], a non-finite result or gather index
 *        quotient; fp32: a zero, infinite or NaN denominator).
 * Bit 1: fp64 only: a lane stored a zero computed from a quotient (its sign is only
 *        the IEEE one through v_div_fixup). */
int gfhip_get_flags(gfhip_context *ctx, unsigned int *flags);

/* Whole-buffer copies, synchronous on return.  Replace copy_to_device /
 * copy_to_host (cuda_context.hpp:625-643; callers read host data right after,
 * dispersion.hpp:1472). */
int gfhip_copy_to_device(gfhip_context *ctx, uint64_t key, const void *host);
int gfhip_copy_to_host(gfhip_context *ctx, uint64_t key, void *host);

/* Read one element after draining the stream.  Replaces  T check_value(index, node)
 * (cuda_context.hpp:602-607).  gfhip_check_value returns it as a double (the real part of a
 * complex element); gfhip_read_element copies the element itself (4, 8 or 16 bytes). */
int gfhip_check_value(gfhip_context *ctx, uint64_t key, size_t index, double *value);
int gfhip_read_element(gfhip_context *ctx, uint64_t key, size_t index, void *element);

/* Bind the MT19937 states of the item's random_state node (random.hpp:24-130): `states` are
 * the node's 1024 mt_state structures (state->data(), 2500 bytes each), uploaded on first
 * sight of `key` and shared by every kernel bound to that key, as create_kernel_call does
 * (cuda_context.hpp:367-380).  No-op for items without a random node. */
int gfhip_set_random_state(gfhip_kernel *kernel, uint64_t key, const void *states, size_t bytes);

/* Device pointer and element count of a buffer (NULL if the key is unknown).
 * The reference's get_buffer (cuda_context.hpp:650-652) returns the managed
 * pointer; here it is device memory. */
void *gfhip_get_buffer(gfhip_context *ctx, uint64_t key, size_t *count);

/* Allocate (zero-filled) the buffer for `key` if it does not exist yet: the
 * buffer side of create_kernel_call for nodes the kernel itself never stores
 * (an output that is a variable or equals a setter's expression,
 * cpu_context.hpp:551-553, still gets its buffer at cuda_context.hpp:364-383). */
int gfhip_allocate_buffer(gfhip_context *ctx, uint64_t key, size_t count, uint32_t dtype);

/* Element count and dtype (enum gfir_dtype) of a buffer; non-zero if the key is unknown. */
int gfhip_get_buffer_info(gfhip_context *ctx, uint64_t key, size_t *count, uint32_t *dtype);

/* A stable, pinned HOST copy of the buffer for `key`, valid for the life of the
 * context and refreshed by every gfhip_wait() (all mirrors are copied behind
 * the queued kernels, then one synchronisation).  This is what the reference's
 *   T *get_buffer(node)   (jit.hpp:336, cuda_context.hpp:1002-1004; managed
 * memory there) means to its caller output.hpp:271: a pointer the NetCDF
 * writer thread reads after wait(). */
void *gfhip_get_host_buffer(gfhip_context *ctx, uint64_t key, size_t *count);

/* Adopt caller-owned device memory (e.g. a shard of a larger allocation) as the
 * buffer for `key`; the context will not free it. */
int gfhip_set_buffer(gfhip_context *ctx, uint64_t key, void *device_pointer, size_t count, uint32_t dtype);

/* Hand arrays over from the buffers of one context to those of another (or of the same one) on the device, in
 * one launch of a hand-written streaming kernel (csrc/hand_over.hip): element i of `from_key`'s buffer in `from`
 * becomes element i of `to_key`'s buffer in `to`, for every entry.  This is what lets the stages of a pipeline,
 * each with a context of its own because the same variable is real in one item and complex in the next
 * (absorption.hpp:411-422 against solver.hpp:304-313), feed each other without a file or the host in between.
 * Values move bit for bit, never through arithmetic (NaN payloads, -0.0, infinities, subnormals unchanged):
 *   F64->F64, F32->F32, C64->C64, C32->C32   copied;
 *   F64->C64, F32->C32                       real part = source, imaginary part = +0.0 (what output.hpp:305,
 *                                            :425-428 does when a complex data_set reads a real variable);
 *   C64->F64, C32->F32                       the real parts (part = 0) or the imaginary parts (part = 1,
 *                                            reference_imag_variable).
 * Everything else fails with a message in gfhip_last_error of both contexts and launches NOTHING, whatever the
 * other entries are: a change of precision, part > 1, part = 1 where the source is not complex or the
 * destination not real, reserved != 0, an unknown key, buffers of different element counts, contexts on different
 * devices, a null context or a null `entries` with count > 0 (the message is also in gfhip_last_error(NULL)).
 * Ordering: both contexts are entered first, so passes that ran ahead of gfhip_run_max's caller are taken back
 * before anything is handed over.  The launch goes on `from`'s stream, behind the kernels that wrote the sources
 * and before the ones that overwrite them.  If `to` has another stream, `from`'s stream first waits for what
 * `to`'s has queued (it may still read the destinations) and `to`'s stream then waits for the launch; with one
 * shared stream no event is involved.  The call does not synchronise the host.  More than 16 entries (the
 * kernel's pointer table) take one launch per 16; entries of zero elements take none.  `to` == `from` is allowed
 * (x -> x_last).  Buffers adopted with gfhip_set_buffer need only the alignment of their elements: the 16-byte
 * accesses are chosen per entry from the pointers. */
struct gfhip_hand_over_entry {
    uint64_t to_key;      /* buffer of `to`   */
    uint64_t from_key;    /* buffer of `from` */
    uint32_t part;        /* complex -> real only: 0 = real parts, 1 = imaginary parts; else 0 */
    uint32_t reserved;    /* 0 */
};
int gfhip_hand_over(gfhip_context *to, gfhip_context *from,
                    const struct gfhip_hand_over_entry *entries, size_t count);

/* Introspection used by hosts, tests and the benchmark. */
struct gfhip_kernel_info {
    uint32_t dtype;                 /* enum gfir_dtype */
    uint32_t num_inputs, num_outputs, num_setters, num_tables, num_instructions;
    uint32_t vgprs, agprs, sgprs, lds_bytes, scratch_bytes;   /* from the code object, after compile */
    uint32_t block_size, grid_size; /* launch geometry for num_rays */
    uint32_t from_cache;            /* 1 if the code object came from the kernel cache */
    uint32_t segments;              /* kernels the item runs as when it was cut into segments, else 0 */
    uint32_t converge_batch;        /* passes per launch of gfhip_converge's loop (`<name>_batch`), 0 or 1: one launch per pass */
    uint32_t level;                 /* lowering level the kernel was planned at (gfhip_add_kernel_at, GFHIP_LEVEL) */
    uint64_t source_hash;
    char     name[64];
};
int gfhip_kernel_get_info(const gfhip_kernel *kernel, struct gfhip_kernel_info *info);

/* Lowering without a device: returns the generated HIP source of one item in a
 * malloc'ed, NUL-terminated string (free with gfhip_free_string) and its hash.
 * Used by __graft_entry__.build() to pre-build code objects with hipcc. */
char *gfhip_generate_source(const void *gfir, size_t bytes, uint64_t *source_hash);

/* The same for an item that runs as several kernels: items above GFHIP_SEGMENT_NODES records (default
 * 6000; e.g. a ray step on the 86-mode VMEC equilibrium, equilibrium.hpp:1868-2330: 54 k records) are
 * cut into consecutive segments, each lowered and cached as a translation unit of its own.  *source =
 * the text of piece `index` (free with gfhip_free_string), or NULL past the last piece; an item that
 * runs as one kernel has exactly one piece.  Returns non-zero on a malformed item. */
int gfhip_generate_piece_source(const void *gfir, size_t bytes, uint32_t index, char **source, uint64_t *source_hash);

/* Piece `index` of a segmented item as data, for checking the split without a device: *piece = a
 * malloc'ed block (free with gfhip_free_string) of int32 words
 *   { symbols S, outputs O, hand-over slots, pieces,
 *     S x state input it reads (-1: none), S x hand-over slot it reads (-1: none),
 *     O x hand-over slot it writes (-1: none), O x output of the item it is (-1: none) }
 * followed by the piece as a GFIR item (include/gfir.h).  *piece stays NULL past the last piece and
 * for items that run as one kernel. */
int gfhip_export_piece(const void *gfir, size_t bytes, uint32_t index, void **piece, size_t *piece_bytes);
/* The three above at a lowering level (gfhip_add_kernel_at); the plain names are level 0. */
char *gfhip_generate_source_at(const void *gfir, size_t bytes, uint64_t *source_hash, uint32_t level);
int gfhip_generate_piece_source_at(const void *gfir, size_t bytes, uint32_t index, char **source, uint64_t *source_hash, uint32_t level);
int gfhip_export_piece_at(const void *gfir, size_t bytes, uint32_t index, void **piece, size_t *piece_bytes, uint32_t level);
void gfhip_free_string(char *text);

/* Host side, no device: the initial conditions of the xrays command line for one shard, sample
 * for sample (graph_driver/xrays.cpp:397-453: std::mt19937_64(seed = shard index), libstdc++'s
 * std::normal_distribution per variable, drawn in the order omega, kx, ky, kz, z, (x, y)).
 * means/sigmas: 7 doubles each in that order with (radius, phi) last, sigma <= 0 = the mean, no
 * draw; columns: 8 arrays of n doubles, t, w, x, y, z, kx, ky, kz. */
void gfhip_cli_distribution(uint64_t seed, size_t n, const double *means, const double *sigmas, double *const *columns);

/* Average duration in milliseconds of the launches of `kernel` recorded since
 * the last call: HIP events on the context's stream around every `enable`-th
 * launch of each kernel (1 = every launch, 0 = off; a pair of event records
 * costs the stream 2-8 us, so a benchmark samples).  Used by bench.py for the
 * roofline line. */
int gfhip_enable_timing(gfhip_context *ctx, int enable);
int gfhip_kernel_timing(gfhip_kernel *kernel, double *average_ms, uint64_t *launches);
/* The individual durations (ms, launch order) behind the last gfhip_kernel_timing
 * (which this call performs first if launches are pending): up to `capacity`
 * values into `ms`, the number available into `count`. */
int gfhip_kernel_timing_samples(gfhip_kernel *kernel, double *ms, size_t capacity, size_t *count);

/* Deposition: per-sample values binned on a 3-D grid, every cell the EXACT sum of its samples, correctly
 * rounded once when it is read.  This is the device form of utilities/bin.py (which sums d_power over
 * nx*ny*nz boolean masks): a sample (x, y, z, value) belongs to cell (i, j, k) iff
 * edge[i] <= c && c < edge[i+1] on each axis (bin.py:54-56), cells are stored bins[nx][ny][nz].  A cell is
 * an integer superaccumulator (csrc/superacc.hpp: 67 limbs of 64 bits, limb k of weight 2^(32k - 1074)),
 * fed with 64-bit integer atomics, so the result does not depend on the order of the samples, on how they
 * are split into records, files or ranks, or on the run.
 *
 * gfhip_bins_create: each axis has n + 1 finite, strictly increasing edges.  Limits: 1 <= n <= 2047 per
 *   axis (the edges are staged in 48 KiB of LDS) and nx*ny*nz <= 2^25 cells (536 B each).  Returns NULL on
 *   failure (gfhip_last_error(ctx)).  The grid belongs to the context and is freed with it at the latest.
 * gfhip_bins_add: `count` samples from four fp64 context buffers (gfhip_allocate_buffer,
 *   gfhip_copy_to_device, or a kernel's outputs), asynchronous on the context's stream.  A sample with a
 *   coordinate outside [edge[0], edge[n]) or NaN on any axis lands nowhere and counts as `outside`; a
 *   sample inside the grid whose value is NaN or +-inf is not added and counts as `skipped`
 *   (utilities/fix_NaN.py:55 drops NaNs the same way).  Buffers that are unknown, not fp64 or shorter than
 *   `count` are refused before anything is launched.
 * gfhip_bins_counts: samples seen, and of those the ones outside and skipped; synchronises.
 * gfhip_bins_state: the canonical limbs, nx*ny*nz*67 (digits in [0, 2^32) in limbs 0-65, the sign in limb
 *   66): byte-identical for the same multiset of samples whatever their order; synchronises.
 * gfhip_bins_merge: add another grid's canonical limbs and counts (same edges: the caller's business).
 * gfhip_bins_read: bins[cell] = round_to_nearest_even(exact sum)/divisor, the division being IEEE: two
 *   roundings, as bin.py's power_bins/total; synchronises. */
gfhip_bins *gfhip_bins_create(gfhip_context *ctx, const double *xedges, size_t nx,
                              const double *yedges, size_t ny, const double *zedges, size_t nz);
int gfhip_bins_add(gfhip_bins *bins, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t value_key, size_t count);
int gfhip_bins_counts(gfhip_bins *bins, uint64_t *samples, uint64_t *outside, uint64_t *skipped);
int gfhip_bins_state(gfhip_bins *bins, int64_t *limbs);
int gfhip_bins_merge(gfhip_bins *bins, const int64_t *limbs, uint64_t samples, uint64_t outside, uint64_t skipped);
int gfhip_bins_read(gfhip_bins *bins, double divisor, double *values);
void gfhip_bins_destroy(gfhip_bins *bins);

/* Flux-surface profile: per-sample values binned on the flux label of their position, every cell the EXACT sum
 * of its samples (the superaccumulator of the deposition grids, state shape (cells, 67)).
 *
 * The label (csrc/flux_label.hpp) comes from the EFIT psi spline: the 16 tables psi_c<a><b> (numr x numz,
 * row-major, table a*4 + b at coefficients + (a*4 + b)*numr*numz) with rmin, dr, zmin, dz, evaluated in the
 * tracer's own representation, every operation one IEEE fp64 operation in this order, nothing fused:
 *     R = sqrt(x*x + y*y);  tr = (R - rmin)/dr;  tz = (z - zmin)/dz
 *     inside the map iff tr >= 0 && tr < numr && tz >= 0 && tz < numz   (a NaN is outside; no clamping)
 *     i = (int)tr, j = (int)tz, c[a][b] = psi_c<a><b>[i][j]
 *     col_a = ((c[a][3]*tz + c[a][2])*tz + c[a][1])*tz + c[a][0];  psi = ((col_3*tr + col_2)*tr + col_1)*tr + col_0
 *     s = (psi - psi0)/span;  label = s, or sqrt(s) with GFHIP_FLUX_SQRT_LABEL (s < 0: NaN, outside)
 * A sample belongs to cell i iff edges[i] <= label < edges[i+1]; the edges need not be uniform.
 *
 * gfhip_flux_create: copies the map (the tables are repacked on the device) and the cells + 1 finite, strictly
 *   increasing edges.  1 <= cells <= 4096; numr, numz >= 1 and numr*numz <= 2^31; dr, dz, span finite and
 *   non-zero; rmin, zmin, psi0 finite; no flag bits beyond the two below; reserved = 0.  Up to the cap of
 *   gfhip_flux_info (256 cells) every workgroup sums its deposits in LDS before they reach memory, unless
 *   GFHIP_FLUX_NO_PRIVATE_SUMS is set; the state is the same bytes either way.  NULL on failure
 *   (gfhip_last_error(ctx)).  The profile belongs to the context and is freed with it at the latest.
 * gfhip_flux_add: as gfhip_bins_add.  `outside`: off the map, off the edges or a NaN label; `skipped`: inside
 *   with a NaN or infinite value.
 * gfhip_flux_label: the labels of `count` points into a fourth fp64 buffer, NaN where outside the map.
 * gfhip_flux_counts / _state / _merge / _read / _destroy: as the deposition grids'; _merge takes the number of
 *   cells of the incoming state and refuses another shape.
 * gfhip_flux_info: how the deposits are launched.
 * gfhip_flux_label_host: no device; flux_label.hpp on the CPU, NaN where outside the map.  Errors:
 *   gfhip_last_error(NULL).
 *
 * Flux volumes: the power density dP/dV needs the volume between a cell's two flux surfaces.  It is one more
 * deposit into the same cells, of quadrature weights that the kernel generates itself.  The numr x numz table
 * cells are cut into sub x sub sub-cells each, 1 <= sub <= 256; point t of the total = numr*sub * numz*sub has
 * the sub-indices gr = t / (numz*sub) and gz = t % (numz*sub), and, every line one IEEE fp64 operation, nothing
 * fused:
 *     R = rmin + dr*((double)(2*gr + 1)/(double)(2*sub));  z = zmin + dz*((double)(2*gz + 1)/(double)(2*sub))
 *     area = (dr/sub)*(dz/sub)   (once, on the host);  w = R*area
 *     label = the label above of (x = R, y = 0, z)
 * With a window the point takes part iff rlo <= R < rhi && zlo <= z < zhi; NULL is the whole map.  A point that
 * takes part and whose label lies in cell i adds w to that cell.  Every point counts as a sample; one outside
 * the window, the map or the edges, or with a NaN label, as `outside`.  The state then holds the sum of
 * R dR dz per cell, exactly, and the volume in m^3 is 2 pi times the value read (rounded once).  That number
 * is the volume of the part of the map (or window) whose label lies in the cell: the shell between two closed
 * surfaces that lie inside the window; for cells beyond the last closed surface what it says and no more (a
 * label range that covers a whole rectangular map puts the map's corners into the outer cells).
 *
 * gfhip_flux_add_volumes: the points first .. first + count into the profile, asynchronous; launches of at
 *   most 2^30 points, normalised by the rule of gfhip_flux_add.  A volume profile is an ordinary profile with
 *   the same map and edges: _state, _merge, _read and _counts as above, and shards of the point range merge.
 *   Refused before any launch: sub outside 1-256; first + count beyond the total (or overflowing); a window
 *   with a NaN or lo >= hi (+-inf is allowed); a map with dr <= 0, dz <= 0 or rmin < 0.
 * gfhip_flux_volumes_host: no device, no context; the same points on the CPU with the same refusals, added to
 *   the cells*67 `limbs` (which are then canonical) and to the three counters.  Errors: gfhip_last_error(NULL).
 *
 * Batches of rays: a cell of a profile is a Monte-Carlo estimate, the mean over rays of what each ray left in it, and
 * the spread of the same tally kept per batch of rays gives its standard error.  The batch rule
 * (csrc/ray_batches.hpp): ray r is the ray's index in the whole ensemble over all ranks and files; 64 consecutive
 * rays are a chunk, r >> 6, and with G batches ray r belongs to batch (r >> 6) % G.  A batched profile has the state
 * (G, cells, 67), batch-major: slab g is the state an ordinary profile has after the samples of batch g's rays, so
 * the sum of the slabs is the ordinary profile to the last bit, and batched states of shards merge exactly.
 *
 * gfhip_flux_create_batched: gfhip_flux_create with 1 <= batches <= 256 and batches*cells <= 2^20 (536 B each).
 *   A workgroup sums one batch at a time, so the LDS path is taken up to 256 cells PER BATCH; gfhip_flux_info
 *   describes that launch.
 * gfhip_flux_add_rays: gfhip_flux_add for a batched profile: sample i is ray first_ray + i.  Refused: a profile
 *   without batches; first_ray + count overflowing 64 bits.  gfhip_flux_add (no ray index) and
 *   gfhip_flux_add_volumes (no rays) refuse a batched profile.
 * gfhip_flux_counts / _state / _read / _info / _destroy serve a batched profile, _state and _read in the batch-major
 *   shape (batches*cells*67 limbs, batches*cells values).  The counters are those of all samples.
 * gfhip_flux_merge_batches: gfhip_flux_merge for a batched profile; it takes the number of batches and of cells per
 *   batch of the incoming state and refuses another shape, as it refuses a profile without batches;
 *   gfhip_flux_merge refuses a batched profile. */
typedef struct gfhip_flux gfhip_flux;

#define GFHIP_FLUX_SQRT_LABEL 1u
#define GFHIP_FLUX_NO_PRIVATE_SUMS 2u

struct gfhip_flux_map {
    double rmin, dr, zmin, dz;
    uint64_t numr, numz;
    const double *coefficients;
    double psi0, span;
    uint32_t flags, reserved;
};

struct gfhip_flux_info {
    uint32_t private_sums;       /* 1: deposits are summed in LDS per workgroup */
    uint32_t workgroup_size;
    uint64_t cap_cells;          /* the most cells the private path takes */
    uint64_t max_workgroups;     /* the most workgroups of one launch */
    uint64_t lds_bytes;          /* dynamic LDS per workgroup */
};

gfhip_flux *gfhip_flux_create(gfhip_context *ctx, const struct gfhip_flux_map *map, const double *edges, size_t cells);
int gfhip_flux_add(gfhip_flux *flux, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t value_key, size_t count);
int gfhip_flux_label(gfhip_flux *flux, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t label_key, size_t count);
int gfhip_flux_counts(gfhip_flux *flux, uint64_t *samples, uint64_t *outside, uint64_t *skipped);
int gfhip_flux_state(gfhip_flux *flux, int64_t *limbs);
int gfhip_flux_merge(gfhip_flux *flux, const int64_t *limbs, size_t cells, uint64_t samples, uint64_t outside, uint64_t skipped);
int gfhip_flux_read(gfhip_flux *flux, double divisor, double *values);
int gfhip_flux_info(gfhip_flux *flux, struct gfhip_flux_info *info);
void gfhip_flux_destroy(gfhip_flux *flux);
int gfhip_flux_label_host(const struct gfhip_flux_map *map, const double *x, const double *y, const double *z,
                          size_t count, double *label);

struct gfhip_flux_window {
    double rlo, rhi, zlo, zhi;
};

int gfhip_flux_add_volumes(gfhip_flux *flux, uint32_t sub, const struct gfhip_flux_window *window, uint64_t first, uint64_t count);
int gfhip_flux_volumes_host(const struct gfhip_flux_map *map, const double *edges, size_t cells, uint32_t sub,
                            const struct gfhip_flux_window *window, uint64_t first, uint64_t count,
                            int64_t *limbs, uint64_t counters[3]);

gfhip_flux *gfhip_flux_create_batched(gfhip_context *ctx, const struct gfhip_flux_map *map, const double *edges, size_t cells,
                                      size_t batches);
int gfhip_flux_add_rays(gfhip_flux *flux, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t value_key, size_t count,
                        uint64_t first_ray);
int gfhip_flux_merge_batches(gfhip_flux *flux, const int64_t *limbs, size_t batches, size_t cells, uint64_t samples,
                             uint64_t outside, uint64_t skipped);

/* Power spectrum over the flux label and the parallel refractive index: per-sample values binned on the label
 * above AND on N = c (k.B)/(|B| w) at the sample's position, every cell the EXACT sum of its samples (state shape
 * (ns, nn, 67), cell (is, in) at is*nn + in).
 *
 * The field direction (csrc/flux_label.hpp) is B = (psi_z/R, fpol/R, -psi_R/R) in (R, phi, z) with the common 1/R
 * dropped.  fpol comes from the four tables fpol_c0 .. fpol_c3 (numpsi intervals of width dpsi from psimin), a cubic
 * in the GLOBAL normalised tp, the interval clamped to the table.  R, tr, tz, the inside test, c[a][b], col_a, psi and
 * the label are those of the flux profile; every line one IEEE fp64 operation in this order, nothing fused:
 *     dcol_a = ((c[a][3]*3.0)*tz + c[a][2]*2.0)*tz + c[a][1]
 *     psi_tz = ((dcol_3*tr + dcol_2)*tr + dcol_1)*tr + dcol_0;  psi_tr = ((col_3*3.0)*tr + col_2*2.0)*tr + col_1
 *     gR = psi_tr/dr;  gZ = psi_tz/dz;  tp = (psi - psimin)/dpsi
 *     q = 0 unless tp >= 0 (a NaN gives 0); numpsi - 1 if tp >= numpsi; else (int)tp
 *     f = ((fpol_c3[q]*tp + fpol_c2[q])*tp + fpol_c1[q])*tp + fpol_c0[q]
 *     a = kx*x + ky*y;  b = ky*x - kx*y
 *     num = (a*gZ + b*f)/R - kz*gR;  den = sqrt((gZ*gZ + f*f) + gR*gR);  npar = (c*(num/den))/w
 * A NaN label or npar is handed out as the quiet NaN without payload (0x7ff8000000000000).
 * A sample belongs to cell (is, in) iff sedges[is] <= label < sedges[is+1] and nedges[in] <= npar < nedges[in+1].
 * `outside`: off the map, off either axis, or a NaN or infinite label or npar (w = 0, R = 0, a zero field);
 * `skipped`: inside with a NaN or infinite value.
 *
 * gfhip_spectrum_create: as gfhip_flux_create, with the field and two edge arrays.  Refused: what
 *   gfhip_flux_create refuses for the map; either axis outside 1-4096 cells; ns*nn > 65536; edges not finite or
 *   not strictly increasing; dpsi or c zero or not finite; psimin not finite; numpsi zero or above 2^31 - 1; a
 *   missing fpol table; reserved != 0.  Up to 256 cells (ns*nn) every workgroup sums its deposits in LDS, unless
 *   the map sets GFHIP_FLUX_NO_PRIVATE_SUMS; the state is the same bytes either way.
 * gfhip_spectrum_add: keys = x, y, z, kx, ky, kz, w, value; fp64 buffers of at least `count` elements.
 * gfhip_spectrum_npar: keys = x, y, z, kx, ky, kz, w; the label and npar of `count` points into two more fp64
 *   buffers, both NaN outside the map, otherwise what the lines above give.
 * gfhip_spectrum_counts / _state / _read / _info / _destroy: as the flux profile's; _merge takes both cell counts of
 *   the incoming state and refuses another shape.
 * gfhip_spectrum_npar_host: no device, no context; the same lines on the CPU from the caller's tables.  Errors:
 *   gfhip_last_error(NULL).
 * gfhip_spectrum_create_batched / _add_rays / _merge_batches: the batches of rays of the flux profile (above) for a
 *   spectrum, state (G, ns, nn, 67); batches*ns*nn <= 2^20, the LDS path up to ns*nn = 256 per batch; the same
 *   refusals, and _merge_batches takes the batches and both cell counts of the incoming state. */
typedef struct gfhip_spectrum gfhip_spectrum;

struct gfhip_spectrum_field {
    double psimin, dpsi;
    uint64_t numpsi;
    const double *fpol[4];       /* fpol_c0 .. fpol_c3, numpsi doubles each */
    double c;                    /* the speed of light in the units of w/k */
    uint64_t reserved;
};

gfhip_spectrum *gfhip_spectrum_create(gfhip_context *ctx, const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                                      const double *sedges, size_t ns, const double *nedges, size_t nn);
int gfhip_spectrum_add(gfhip_spectrum *spectrum, const uint64_t keys[8], size_t count);
int gfhip_spectrum_npar(gfhip_spectrum *spectrum, const uint64_t keys[7], uint64_t label_key, uint64_t npar_key, size_t count);
int gfhip_spectrum_counts(gfhip_spectrum *spectrum, uint64_t *samples, uint64_t *outside, uint64_t *skipped);
int gfhip_spectrum_state(gfhip_spectrum *spectrum, int64_t *limbs);
int gfhip_spectrum_merge(gfhip_spectrum *spectrum, const int64_t *limbs, size_t ns, size_t nn, uint64_t samples, uint64_t outside,
                         uint64_t skipped);
int gfhip_spectrum_read(gfhip_spectrum *spectrum, double divisor, double *values);
int gfhip_spectrum_info(gfhip_spectrum *spectrum, struct gfhip_flux_info *info);
void gfhip_spectrum_destroy(gfhip_spectrum *spectrum);
int gfhip_spectrum_npar_host(const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                             const double *const columns[7], size_t count, double *label, double *npar);
gfhip_spectrum *gfhip_spectrum_create_batched(gfhip_context *ctx, const struct gfhip_flux_map *map,
                                              const struct gfhip_spectrum_field *field, const double *sedges, size_t ns,
                                              const double *nedges, size_t nn, size_t batches);
int gfhip_spectrum_add_rays(gfhip_spectrum *spectrum, const uint64_t keys[8], size_t count, uint64_t first_ray);
int gfhip_spectrum_merge_batches(gfhip_spectrum *spectrum, const int64_t *limbs, size_t batches, size_t ns, size_t nn,
                                 uint64_t samples, uint64_t outside, uint64_t skipped);

/* Distribution of particles over the flux label, the pitch cosine and gamma: the particles of a push (x, y, z, ux,
 * uy, uz, gamma) binned where they lie on the device, every cell the EXACT sum of its particles' weights (state shape
 * (ns, np, ng, 67), cell (is, ip, ig) at (is*np + ip)*ng + ig).
 *
 * The seven columns are fp32 or fp64; an fp32 value is widened to fp64 first, which is exact, and everything after
 * that is the fp64 arithmetic of csrc/flux_label.hpp, every line one IEEE fp64 operation in this order, nothing fused.
 * The label, gR, gZ and f are those of the spectrum above; with u in place of k,
 *     a = ux*x + uy*y;  b = uy*x - ux*y
 *     num = (a*gZ + b*f)/R - uz*gR;  den = sqrt((gZ*gZ + f*f) + gR*gR);  cosine = num/den
 *     uu = (ux*ux + uy*uy) + uz*uz;  p = sqrt(uu);  xi = cosine/p
 *     if (xi > 1) xi = 1;  if (xi < -1) xi = -1        (comparisons: a NaN stays a NaN)
 * The clamp is needed: for u parallel to B the quotient comes out up to 7e-16 above 1 in a third of the cases.  u = 0
 * gives 0/0, a NaN.  gamma is read from its column as it is.  A NaN label or xi is handed out as the quiet NaN without
 * payload.
 * A particle belongs to cell (is, ip, ig) iff sedges[is] <= label < sedges[is+1], pedges[ip] <= xi < pedges[ip+1] and
 * gedges[ig] <= gamma < gedges[ig+1].  The last edge of an axis is outside it: pitch edges that should hold xi = 1
 * end above 1 (the Python helper pitch_edges(n) ends at nextafter(1, 2)).  It deposits its weight, an eighth column
 * of the same type, or 1.0 without one.  `outside`: off the map, off any axis, or a NaN label, xi or gamma; `skipped`:
 * inside with a NaN or infinite weight.
 *
 * Batches of particles: a cell is a Monte-Carlo estimate over the pushed particles, and its standard error comes
 * from the same tally kept per batch of particles.  The rule is that of the batches of rays (gfhip_flux_create_batched,
 * csrc/ray_batches.hpp) with the particle's index p in the whole ensemble, over all ranks and shards, in place of the
 * ray's: batch (p >> 6) % G.  A batched distribution has the state (G, ns, np, ng, 67), slab g the state of a plain
 * distribution fed batch g's particles alone with the same weights; the counters are those of all particles.
 *
 * gfhip_phase_create: as gfhip_spectrum_create with three edge arrays; the field's c is ignored.  Refused: what
 *   gfhip_flux_create refuses for the map and gfhip_spectrum_create for the field (c apart); an axis outside 1-4096
 *   cells (fewer than two edges); ns*np*ng > 2^20; edges not finite or not strictly increasing.  Up to 256 cells
 *   (ns*np*ng) every workgroup sums its deposits in LDS, unless the map sets GFHIP_FLUX_NO_PRIVATE_SUMS; the state is
 *   the same bytes either way, and for fp32 and fp64 columns of equal values.
 * gfhip_phase_add: keys = x, y, z, ux, uy, uz, gamma, and weight_key when has_weight is non-zero: context buffers of
 *   at least `count` elements, all fp32 or all fp64 (the type comes from the buffers).  Asynchronous on the context's
 *   stream; launches of at most 2^30 particles, normalised by the rule of gfhip_flux_add.  Refused before any launch:
 *   an unknown key, a complex or mixed type, a buffer shorter than `count`.
 * gfhip_phase_coordinates: the label and xi of `count` particles into two fp64 buffers, both NaN outside the map.
 * gfhip_phase_counts / _state / _read / _info / _destroy: as the spectrum's; _merge takes the three cell counts of the
 *   incoming state and refuses another shape.
 * gfhip_phase_coordinates_host: no device, no context; the same lines on the CPU from the caller's tables, the seven
 *   columns float when is_f32 is non-zero and double otherwise.  Errors: gfhip_last_error(NULL).
 * gfhip_phase_create_batched: gfhip_phase_create with 1 <= batches <= 256 and batches*ns*np*ng <= 2^20.  A workgroup
 *   sums one batch at a time, so the LDS path is taken up to 256 cells PER BATCH; gfhip_phase_info describes that launch.
 * gfhip_phase_add_particles: gfhip_phase_add for a batched distribution: particle i of the buffers is particle
 *   first_particle + i.  Refused before any launch: what gfhip_phase_add refuses; a distribution without batches;
 *   first_particle + count overflowing 64 bits.  gfhip_phase_add refuses a batched distribution.
 * gfhip_phase_merge_batches: gfhip_phase_merge for a batched distribution; it takes the batches and the three cell
 *   counts of the incoming state and refuses another shape or a distribution without batches; gfhip_phase_merge
 *   refuses a batched one.  _counts, _state, _read, _info and _destroy serve both kinds, _state and _read batch-major.
 * gfhip_phase_add_particles_host: no device, no context; the batched deposit on the CPU (csrc/phase_host.hpp) into
 *   `limbs` (batches*ns*np*ng*67, canonical on return) and `counters` (3), columns[7] NULL without weights. */
typedef struct gfhip_phase gfhip_phase;

gfhip_phase *gfhip_phase_create(gfhip_context *ctx, const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                                const double *sedges, size_t ns, const double *pedges, size_t np, const double *gedges, size_t ng);
int gfhip_phase_add(gfhip_phase *phase, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count);
int gfhip_phase_coordinates(gfhip_phase *phase, const uint64_t keys[7], uint64_t label_key, uint64_t pitch_key, size_t count);
int gfhip_phase_counts(gfhip_phase *phase, uint64_t *samples, uint64_t *outside, uint64_t *skipped);
int gfhip_phase_state(gfhip_phase *phase, int64_t *limbs);
int gfhip_phase_merge(gfhip_phase *phase, const int64_t *limbs, size_t ns, size_t np, size_t ng, uint64_t samples,
                      uint64_t outside, uint64_t skipped);
int gfhip_phase_read(gfhip_phase *phase, double divisor, double *values);
int gfhip_phase_info(gfhip_phase *phase, struct gfhip_flux_info *info);
void gfhip_phase_destroy(gfhip_phase *phase);
int gfhip_phase_coordinates_host(const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                                 const void *const columns[7], int is_f32, size_t count, double *label, double *pitch);
gfhip_phase *gfhip_phase_create_batched(gfhip_context *ctx, const struct gfhip_flux_map *map,
                                        const struct gfhip_spectrum_field *field, const double *sedges, size_t ns,
                                        const double *pedges, size_t np, const double *gedges, size_t ng, size_t batches);
int gfhip_phase_add_particles(gfhip_phase *phase, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count,
                              uint64_t first_particle);
int gfhip_phase_merge_batches(gfhip_phase *phase, const int64_t *limbs, size_t batches, size_t ns, size_t np, size_t ng,
                              uint64_t samples, uint64_t outside, uint64_t skipped);
int gfhip_phase_add_particles_host(const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                                   const double *sedges, size_t ns, const double *pedges, size_t np, const double *gedges,
                                   size_t ng, size_t batches, const void *const columns[8], int is_f32, size_t count,
                                   uint64_t first_particle, int64_t *limbs, uint64_t counters[3]);

/* First-exit tracking of the particles of one push: which particles have left the plasma, at which step, where they
 * crossed and at what energy, kept on the device from one check to the next (csrc/confinement.hip).
 *
 * Per particle the tracker holds lost_step (uint32, GFHIP_CONFINED = 0xFFFFFFFF while confined) and `alive`, a context
 * buffer of the push's type under the caller's key, 1 while confined and 0 afterwards, which every other entry point
 * takes as a weight.  A check with step number `step` examines the particles that are still confined, in the fixed fp64
 * arithmetic above (fp32 columns widened first):
 *     label = the label of (x, y, z), a NaN as the quiet NaN, NaN off the map
 *     lost  iff  !(label < limit)       off the map, a NaN position and label == limit are all lost
 * A particle found lost is settled once and never examined again, even if a later step carries it back inside:
 * lost_step = step, alive = 0, exit_r = sqrt(x*x + y*y) and exit_z = z (fp64, a NaN as the quiet NaN; NaN while the
 * particle is confined) where exit buffers are given, and its weight, or 1.0 without a weight column, is added to the
 * EXACT cell (ir, iz, ig) of (R, z, gamma as stored): redges[ir] <= R < redges[ir+1] and so on, state shape
 * (nr, nz, ng, 67), cell at (ir*nz + iz)*ng + ig.  newly_lost[check] counts the particles the check found lost.  The
 * counters are those of the cells restricted to the lost: `samples` particles lost, `outside` lost but in no footprint
 * cell, `skipped` in a cell with a NaN or infinite weight.
 *
 * gfhip_confine_create: `count` particles, fp32 when is_f32 is non-zero; `alive_key` is allocated with
 *   gfhip_allocate_buffer's rule (an existing buffer must have the type and the length) and set to 1; `capacity` is the
 *   most checks.  Refused: what gfhip_phase_create refuses for the map and the edges; nr*nz*ng > 2^20; a NaN limit;
 *   count = 0; capacity = 0.
 * gfhip_confine_check: keys as gfhip_phase_add's (ux, uy, uz are checked and not read); exit_r_key and exit_z_key when
 *   has_exit is non-zero: fp64 buffers of at least `count` elements, filled with NaN when the tracker first sees them
 *   (particles settled before that keep NaN there).  Asynchronous on the context's stream.  Refused before any launch,
 *   with everything unchanged: an unknown key, mixed or complex columns or columns not of the tracker's type, a buffer
 *   shorter than the tracker's count, exit buffers that are not fp64, step = GFHIP_CONFINED, a step below the previous
 *   check's, more checks than `capacity`.
 * gfhip_confine_lost_steps: the `count` lost_step values, after the stream has drained.
 * gfhip_confine_history: the steps of the checks made and what each found lost, `*checks` of them (at most `capacity`;
 *   steps and newly_lost may be NULL to ask for the number alone).
 * gfhip_confine_counts / _state / _merge / _read / _info / _destroy: as the distribution's.
 * gfhip_confine_check_host: no device, no context; the same lines on the CPU on the caller's arrays in place: columns
 *   as above (columns[3..5] unread, columns[7] NULL without weights), `alive` of the columns' type, exit_r and exit_z both
 *   NULL or both given, *newly_lost goes up by the particles found lost.  With `limbs` (nr*nz*ng*67, canonical on
 *   return) and `counters` (3) the footprint is deposited too; with limbs = NULL the edges are not looked at.  Errors:
 *   gfhip_last_error(NULL). */
#define GFHIP_CONFINED 0xFFFFFFFFu
typedef struct gfhip_confine gfhip_confine;

gfhip_confine *gfhip_confine_create(gfhip_context *ctx, const struct gfhip_flux_map *map, double limit, const double *redges,
                                    size_t nr, const double *zedges, size_t nz, const double *gedges, size_t ng, size_t count,
                                    int is_f32, uint64_t alive_key, size_t capacity);
int gfhip_confine_check(gfhip_confine *confine, const uint64_t keys[7], uint64_t weight_key, int has_weight, uint64_t exit_r_key,
                        uint64_t exit_z_key, int has_exit, uint32_t step);
int gfhip_confine_lost_steps(gfhip_confine *confine, uint32_t *lost_step);
int gfhip_confine_history(gfhip_confine *confine, uint32_t *steps, uint64_t *newly_lost, size_t *checks);
int gfhip_confine_counts(gfhip_confine *confine, uint64_t *samples, uint64_t *outside, uint64_t *skipped);
int gfhip_confine_state(gfhip_confine *confine, int64_t *limbs);
int gfhip_confine_merge(gfhip_confine *confine, const int64_t *limbs, size_t nr, size_t nz, size_t ng, uint64_t samples,
                        uint64_t outside, uint64_t skipped);
int gfhip_confine_read(gfhip_confine *confine, double divisor, double *values);
int gfhip_confine_info(gfhip_confine *confine, struct gfhip_flux_info *info);
void gfhip_confine_destroy(gfhip_confine *confine);
int gfhip_confine_check_host(const struct gfhip_flux_map *map, double limit, const double *redges, size_t nr,
                             const double *zedges, size_t nz, const double *gedges, size_t ng, const void *const columns[8],
                             int is_f32, size_t count, uint32_t step, uint32_t *lost_step, void *alive, double *exit_r,
                             double *exit_z, uint64_t *newly_lost, int64_t *limbs, uint64_t counters[3]);

/* Moments of the particles of a push per flux surface: density, parallel current, kinetic energy and synchrotron-radiated
 * power, exact sums (csrc/moment_bins.hip).  In the push's normalised units: no physical constants are applied.
 *
 * The seven columns are a distribution's; the label, R, gR, gZ and f are those above, in the same fixed fp64 arithmetic of
 * csrc/flux_label.hpp (fp32 columns widened first), every line one IEEE fp64 operation, nothing fused:
 *     upar = cosine                            (u.B)/|B|, the value xi is cosine/p of
 *     vpar = upar/gamma;  kin = gamma - 1.0
 *     uu = (ux*ux + uy*uy) + uz*uz;  upup = upar*upar
 *     perp = uu - upup;  if (perp < 0) perp = 0          (a comparison: a NaN stays a NaN)
 *     bsum = (gZ*gZ + f*f) + gR*gR;  rr = R*R;  bsq = bsum/rr          (|B|^2)
 *     rad = perp*bsq
 *     m = {1.0, vpar, kin, rad}                GFHIP_MOMENT_DENSITY, _CURRENT, _ENERGY, _RADIATION
 *     v[0] = w;  v[k] = w*m[k], k = 1..3       w: the weight, an eighth column of the same type, or 1.0 without one
 * A particle belongs to surface `is` iff sedges[is] <= label < sedges[is+1] and deposits v[k] into the exact cell
 * (is, k), flat index is*4 + k; state shape (ns, 4, 67).  The counters count particles: `samples` one per particle,
 * `outside` the label in no cell (off the map, NaN, off the edges), `skipped` inside with any of the four v[k] NaN or
 * infinite; such a particle deposits none of the four, so the four moments are sums over the same particles.  u = 0 is
 * not skipped (upar = 0, rad = 0); gamma = 0 is (0/0).
 *
 * gfhip_moments_create: as gfhip_phase_create with the label edges alone.  Refused: what gfhip_phase_create refuses for
 *   the map, the field and the edges (1 to 4096 surfaces); ns*4 > 2^20.  Up to 256 cells (64 surfaces) every workgroup
 *   sums its deposits in LDS, unless the map sets GFHIP_FLUX_NO_PRIVATE_SUMS; the state is the same bytes either way, and
 *   for fp32 and fp64 columns of equal values.
 * gfhip_moments_add: keys and weight as gfhip_phase_add's.  Asynchronous on the context's stream; launches of at most
 *   2^30 particles, normalised by the rule of gfhip_flux_add (a cell takes one deposit per particle).  Refused before
 *   any launch, the state unchanged: an unknown key, a complex or mixed type, count = 0, a buffer shorter than `count`.
 * gfhip_moments_values: the label and the four m[k] (a NaN as the quiet NaN, all NaN off the map) of `count` particles
 *   into the fp64 buffers label_key (count) and values_key (4*count, [particle][k]).  Refused as _add, and a
 *   destination that is not fp64 or too short.
 * gfhip_moments_counts / _state / _read / _info / _destroy: as the distribution's; _merge takes the incoming state's
 *   (ns, nm) and refuses another shape, nm != 4 included.
 * gfhip_moments_values_host, gfhip_moments_add_host: no device, no context; the same lines on the CPU from the caller's
 *   tables and arrays (csrc/moments_host.hpp), the columns float when is_f32 is non-zero and double otherwise,
 *   columns[7] NULL without weights.  add_host adds to `limbs` (ns*4*67, canonical on return) and `counters` (3).
 *   Errors: gfhip_last_error(NULL).
 * gfhip_moments_create_batched, gfhip_moments_add_particles, gfhip_moments_merge_batches (which takes batches, ns, nm)
 *   and gfhip_moments_add_particles_host: the batches of particles of gfhip_phase_create_batched for a moment profile,
 *   state (G, ns, 4, 67), batches*ns*4 <= 2^20, the LDS path up to 64 surfaces PER BATCH.  A particle deposits all
 *   four of its values into its batch's slab or none; the counters count the particles of all batches.  The refusals are
 *   those of the distribution's calls, and count = 0 as gfhip_moments_add. */
#define GFHIP_MOMENTS 4
#define GFHIP_MOMENT_DENSITY 0
#define GFHIP_MOMENT_CURRENT 1
#define GFHIP_MOMENT_ENERGY 2
#define GFHIP_MOMENT_RADIATION 3
typedef struct gfhip_moments gfhip_moments;

gfhip_moments *gfhip_moments_create(gfhip_context *ctx, const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                                    const double *sedges, size_t ns);
int gfhip_moments_add(gfhip_moments *moments, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count);
int gfhip_moments_values(gfhip_moments *moments, const uint64_t keys[7], uint64_t label_key, uint64_t values_key, size_t count);
int gfhip_moments_counts(gfhip_moments *moments, uint64_t *samples, uint64_t *outside, uint64_t *skipped);
int gfhip_moments_state(gfhip_moments *moments, int64_t *limbs);
int gfhip_moments_merge(gfhip_moments *moments, const int64_t *limbs, size_t ns, size_t nm, uint64_t samples, uint64_t outside,
                        uint64_t skipped);
int gfhip_moments_read(gfhip_moments *moments, double divisor, double *values);
int gfhip_moments_info(gfhip_moments *moments, struct gfhip_flux_info *info);
void gfhip_moments_destroy(gfhip_moments *moments);
int gfhip_moments_values_host(const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                              const void *const columns[7], int is_f32, size_t count, double *label, double *values);
int gfhip_moments_add_host(const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field, const double *sedges,
                           size_t ns, const void *const columns[8], int is_f32, size_t count, int64_t *limbs,
                           uint64_t counters[3]);
gfhip_moments *gfhip_moments_create_batched(gfhip_context *ctx, const struct gfhip_flux_map *map,
                                            const struct gfhip_spectrum_field *field, const double *sedges, size_t ns,
                                            size_t batches);
int gfhip_moments_add_particles(gfhip_moments *moments, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count,
                                uint64_t first_particle);
int gfhip_moments_merge_batches(gfhip_moments *moments, const int64_t *limbs, size_t batches, size_t ns, size_t nm,
                                uint64_t samples, uint64_t outside, uint64_t skipped);
int gfhip_moments_add_particles_host(const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                                     const double *sedges, size_t ns, size_t batches, const void *const columns[8], int is_f32,
                                     size_t count, uint64_t first_particle, int64_t *limbs, uint64_t counters[3]);

/* A particle source: the seven columns of a push filled where they lie on the device, from a stated distribution
 * (csrc/particle_source.hip).  Particle p, its index in the WHOLE ensemble, is drawn from Philox4x32-10 with counter
 * (lo32(p), hi32(p), attempt, purpose) and key (lo32(seed), hi32(seed)), in the fixed fp64 arithmetic of
 * csrc/particle_draw.hpp, which states every line: p is the same particle, to the last bit, on any device, for any split
 * into shards, launch shape or route, and on the host.
 *     position   uniform in volume in the box rlo <= R < rhi, zlo <= z < zhi (R*R uniform, the toroidal angle uniform),
 *                rounded to the columns' type, kept iff slo <= label < shi for the label of the STORED position (a NaN or
 *                a point off the map is not), and with a profile iff also u < accept[is], `is` the cell of the label
 *                among sedges (in no cell: not kept); up to `attempts` candidates
 *     momentum   components of beta = v/c: |beta| uniform in [blo, bhi), the pitch cosine to the local field
 *                B = (psi_z, fpol, -psi_R)/R uniform in [xlo, xhi), the gyrophase uniform; gamma = 0.  The push's own
 *                initialize_gamma makes gamma and gamma*beta of them.
 * A particle that runs out of attempts, or sits where the field has no direction, is UNPLACED: the quiet NaN without
 * payload in all seven columns.  `placed`, a column of the same type, receives 1 or 0: a weight for every other entry
 * point.  The four counters: placed, unplaced, position_tries (the candidates examined, summed over the particles) and
 * gyro_tries.
 *
 * gfhip_source_create: box = {rlo, rhi, zlo, zhi}; sedges (ns + 1) and accept (ns) both NULL with ns = 0: no profile;
 *   fp32 columns when is_f32 is non-zero; flags: GFHIP_SOURCE_PLAIN (one lane, one particle) or GFHIP_SOURCE_REFILL (a
 *   lane that has settled its particle takes its wave's next one), neither: the library's choice, the same bytes either
 *   way; max_workgroups: 0 for the launch rule of the global deposits.  Refused: what gfhip_phase_create refuses for
 *   the map and the field; a box, label range, speed range or pitch range that is empty or has a NaN or an infinity;
 *   rlo < 0; blo < 0 or bhi >= 1; xlo < -1 or xhi > 1; attempts = 0 or > 4096; ns > 256, edges that are not finite and
 *   strictly increasing, accept outside [0, 1] or NaN, one of sedges and accept without the other; unknown flags or both
 *   routes.
 * gfhip_source_fill: particles first_particle .. first_particle + count into elements 0 .. count of the seven buffers
 *   (and of placed_key when has_placed is non-zero), which are allocated by gfhip_allocate_buffer's rule where absent.
 *   Asynchronous on the context's stream.  Refused before any launch, with nothing changed or allocated: count = 0,
 *   first_particle + count beyond 64 bits, an existing buffer of another type than the source's or shorter than
 *   `count`, the same key twice.
 * gfhip_source_counts: the four counters of all fills so far, after the stream has drained.
 * gfhip_source_info: private_sums 1 for the refill route, workgroup_size, max_workgroups and lds_bytes of a launch.
 * gfhip_source_fill_host: no device, no context; the same lines on the CPU (csrc/source_host.hpp) into the caller's
 *   arrays, columns[0..6] and columns[7] = placed or NULL, float when is_f32 is non-zero and double otherwise;
 *   counters[4] are added to.  flags are checked and otherwise without effect.  Errors: gfhip_last_error(NULL).
 * gfhip_source_block_host: one Philox4x32-10 block. */
#define GFHIP_SOURCE_PLAIN 1u
#define GFHIP_SOURCE_REFILL 2u
typedef struct gfhip_source gfhip_source;

gfhip_source *gfhip_source_create(gfhip_context *ctx, const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field,
                                  const double box[4], double slo, double shi, double blo, double bhi, double xlo, double xhi,
                                  const double *sedges, const double *accept, size_t ns, uint64_t seed, uint32_t attempts,
                                  int is_f32, uint32_t flags, size_t max_workgroups);
int gfhip_source_fill(gfhip_source *source, const uint64_t keys[7], uint64_t placed_key, int has_placed, uint64_t first_particle,
                      size_t count);
int gfhip_source_counts(gfhip_source *source, uint64_t counters[4]);
int gfhip_source_info(gfhip_source *source, struct gfhip_flux_info *info);
void gfhip_source_destroy(gfhip_source *source);
int gfhip_source_fill_host(const struct gfhip_flux_map *map, const struct gfhip_spectrum_field *field, const double box[4],
                           double slo, double shi, double blo, double bhi, double xlo, double xhi, const double *sedges,
                           const double *accept, size_t ns, uint64_t seed, uint32_t attempts, uint32_t flags,
                           void *const columns[8], int is_f32, uint64_t first_particle, size_t count, uint64_t counters[4]);
void gfhip_source_block_host(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);

/* Host side, no device: the correctly rounded sum of `count` finite doubles through the same
 * superaccumulator functions the kernels run; `limbs` (67 words, or NULL) receives the canonical state.
 * Non-zero for a NaN or an infinity among the values (gfhip_last_error(NULL)). */
int gfhip_exact_sum(const double *values, size_t count, double *sum, int64_t *limbs);

#ifdef __cplusplus
}
#endif

#endif /* GF_HIP_H */
