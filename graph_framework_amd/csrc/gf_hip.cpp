//------------------------------------------------------------------------------
///  @file gf_hip.cpp
///  @brief libgf_hip.so: the C ABI of include/gf_hip.h on the HIP runtime.
///
///  Host side of the MI355X backend: owns the device buffers (keyed like the
///  reference's kernel_arguments maps, cuda_context.hpp:78-80), lowers GFIR work
///  items with codegen.hpp, builds them (cached code objects or hipRTC), packs
///  and uploads the coefficient tables, launches on one HIP stream per context
///  and runs the converge loop of workflow.hpp:179-205 around the device max
///  reduction of reduce.hip.
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sys/stat.h>

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <memory>
#include <new>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gf_hip.h"
#include "plan.hpp"

#include "cell_launch.hpp"
#include "confinement_host.hpp"
#include "converge_state.hpp"
#include "flux_label.hpp"
#include "hand_over.hpp"
#include "moments_host.hpp"
#include "phase_host.hpp"
#include "ray_batches.hpp"
#include "source_host.hpp"
#include "superacc.hpp"

namespace gfhip {
void launch_max_reduce(const void *in, const size_t n, const bool f64,
                       unsigned long long *result, const unsigned int num_cus, hipStream_t stream);
void launch_converge_decide(const bool f64, unsigned long long *reduced, void *state, const unsigned int count, hipStream_t stream);
void launch_max_modulus(const void *in, const size_t n, const bool f64, void *result, hipStream_t stream);
}

namespace {

thread_local std::string creation_error;

//  Owning holders of HIP resources: destruction releases them.
template<typename H, hipError_t (*release)(H)>
struct releaser {
    void operator()(H handle) const { (void)release(handle); }
};
template<typename T = void> using device_ptr = std::unique_ptr<T, releaser<void *, hipFree>>;
template<typename T = void> using host_ptr = std::unique_ptr<T, releaser<void *, hipHostFree>>;       // pinned
using module_ptr = std::unique_ptr<std::remove_pointer_t<hipModule_t>, releaser<hipModule_t, hipModuleUnload>>;
using event_ptr = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, releaser<hipEvent_t, hipEventDestroy>>;
using stream_ptr = std::unique_ptr<std::remove_pointer_t<hipStream_t>, releaser<hipStream_t, hipStreamDestroy>>;

template<typename T>
hipError_t allocate(device_ptr<T> &p, const size_t bytes) {
    void *raw = nullptr;
    const hipError_t status = hipMalloc(&raw, bytes);
    if (status == hipSuccess) p.reset(static_cast<T *> (raw));
    return status;
}

template<typename T>
hipError_t allocate(host_ptr<T> &p, const size_t bytes) {
    void *raw = nullptr;
    const hipError_t status = hipHostMalloc(&raw, bytes, hipHostMallocDefault);
    if (status == hipSuccess) p.reset(static_cast<T *> (raw));
    return status;
}

struct event_pair {
    event_ptr start, stop;
};

struct buffer {
    device_ptr<> owned;         // null for a buffer adopted by gfhip_set_buffer, which is never freed here
    void *pointer = nullptr;
    size_t count = 0;
    uint32_t dtype = GFIR_F64;
    host_ptr<> mirror;          // host copy handed out by gfhip_get_host_buffer, refreshed by gfhip_wait
};

std::string library_directory() {
    Dl_info info;
    if (dladdr(reinterpret_cast<void *> (&gfhip_max_concurrency), &info) && info.dli_fname) {
        std::string path(info.dli_fname);
        const size_t slash = path.rfind('/');
        return slash == std::string::npos ? "." : path.substr(0, slash);
    }
    return ".";
}

bool read_file(const std::string &path, std::vector<char> &data) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    f.seekg(0, std::ios::end);
    const std::streamoff size = f.tellg();
    f.seekg(0, std::ios::beg);
    data.resize(static_cast<size_t> (size));
    f.read(data.data(), size);
    return static_cast<bool> (f);
}

size_t element_bytes(const uint32_t dtype) {
    return gfhip::item::element_size(dtype);
}

std::string hash_name(const uint64_t hash) {
    char buf[32];
    std::snprintf(buf, sizeof(buf), "%016llx", static_cast<unsigned long long> (hash));
    return buf;
}

}  // namespace

//  Members are released last to first: the kernels and buffers, then the owned stream.
struct gfhip_context {
    int device = 0;
    stream_ptr own_stream;                         // set when the context created `stream`
    hipStream_t stream = nullptr;
    unsigned int num_cus = 256;
    device_ptr<unsigned long long> device_scalar;  // 8 words: one per pass of a batch
    host_ptr<unsigned long long> host_scalar;      // 8 words
    device_ptr<unsigned int> device_flags;         // bit 0: a lane redid a pass with the compiler's division
    device_ptr<gfhip::converge_state> device_converge;
    host_ptr<gfhip::converge_state> host_converge;
    std::map<uint64_t, buffer> buffers;
    std::map<uint64_t, device_ptr<>> random_states;    // MT19937 states per random_state node (raw bytes)
    std::vector<std::unique_ptr<gfhip_kernel>> kernels;
    std::vector<std::unique_ptr<gfhip_bins>> bins;     // deposition grids (gfhip_bins_create), until gfhip_bins_destroy
    std::vector<std::unique_ptr<gfhip_flux>> fluxes;   // flux profiles (gfhip_flux_create), until gfhip_flux_destroy
    std::vector<std::unique_ptr<gfhip_spectrum>> spectra;      // spectra (gfhip_spectrum_create), until gfhip_spectrum_destroy
    std::vector<std::unique_ptr<gfhip_phase>> phases;          // distributions (gfhip_phase_create), until gfhip_phase_destroy
    std::vector<std::unique_ptr<gfhip_confine>> confines;      // trackers (gfhip_confine_create), until gfhip_confine_destroy
    std::vector<std::unique_ptr<gfhip_moments>> moments;       // moment profiles (gfhip_moments_create), until gfhip_moments_destroy
    std::vector<std::unique_ptr<gfhip_source>> sources;        // particle sources (gfhip_source_create), until gfhip_source_destroy
    std::string error;
    gfhip_kernel *running_ahead = nullptr;         // the kernel whose last batch ran passes the caller has not asked for yet
    gfhip_kernel *max_streak = nullptr;            // the kernel the last entry point was gfhip_run_max of
    unsigned int timing = 0;                       // 0 = off, N = events around every Nth launch of a kernel
    event_ptr hand_over_before, hand_over_after;   // order gfhip_hand_over into this context from another stream (made on first use)

    int fail(const std::string &message) {
        error = message;
        return 1;
    }
    int check(const hipError_t status, const char *what) {
        if (status != hipSuccess) {
            return fail(std::string(what) + ": " + hipGetErrorString(status));
        }
        return 0;
    }
};

//  One compiled kernel of a work item: the item itself, one segment of it (segments.hpp) or its redo launch,
//  as planned (`plan`: the piece as an item and what its symbols and outputs are; `low`: its text) and as loaded.
struct built_piece : gfhip::planned_piece {
    built_piece() = default;
    explicit built_piece(gfhip::planned_piece &&planned) : gfhip::planned_piece(std::move(planned)) {}
    module_ptr module;
    hipFunction_t function = nullptr;
    hipFunction_t max_function = nullptr;          // `<name>_max`
    hipFunction_t converge_function = nullptr;     // `<name>_converge`
    hipFunction_t batch_function = nullptr;        // `<name>_batch`: several passes per launch, one max per pass
    std::vector<device_ptr<>> packs;
    unsigned int grid = 1;
    int vgprs = 0, lds_static = 0, scratch = 0;
    bool from_cache = false;
};

struct gfhip_kernel {
    gfhip_context *ctx = nullptr;
    gfhip::item item;
    built_piece whole;                             // the item's kernel; of a segmented item, its name and hash and the pieces' totals
    std::vector<built_piece> pieces;               // non-empty: the item runs as this sequence of segment kernels
    std::vector<device_ptr<>> handover;            // one device array of `chunk` elements per hand-over slot
    size_t chunk = 0;                              // rays per walk of the segment sequence
    std::optional<built_piece> redo;               // lanes outside the division window are redone by this launch of its own:
                                                   // the whole item with the compiler's division, over the redo list
    device_ptr<unsigned char> flagged;             // per ray: a segment before the last found it outside the window
    device_ptr<unsigned int> redo_list, redo_count;
    size_t num_rays = 0;
    uint32_t level = 0;                            // lowering level the item was planned at (options.hpp)
    std::vector<device_ptr<>> undo;                // per setter: the target's values at the beginning of the last batch
//  gfhip_run_max called in a row (the reference's converge_item::run, workflow.hpp:179-205, through hip_context's
//  create_max_call): passes of the last `<name>_batch` launch that ran ahead of the caller, their maxes waiting here.
    std::vector<double> ahead;
    unsigned int ahead_taken = 0;
    bool built = false;
    std::vector<uint64_t> input_keys, output_keys;
    void *random_states = nullptr;                 // device copy of the item's random_state node (items with draws)
    bool bound = false;
    std::vector<event_pair> events;
    std::vector<event_pair> free_events;
    uint64_t launch_count = 0;
    std::vector<double> samples;                   // durations drained by the last gfhip_kernel_timing
};

//  A store of exact sums, what a deposition grid and a flux profile both are: per cell the 67 limbs of superacc.hpp,
//  [cell][limb], and what became of the samples.  The entry points check their own arguments and call these.
struct exact_cells {
    gfhip_context *ctx = nullptr;
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
};

//  A 3-D deposition grid.
struct gfhip_bins : exact_cells {
    int n[3] = {0, 0, 0};
    double scale[3] = {0.0, 0.0, 0.0};                 // n/(last edge - first edge): the kernel's first guess of a cell
    device_ptr<double> edges;                          // the three axes' edges one after the other
};

//  What a flux-surface profile and a spectrum share: the map, the psi tables as [table cell][16], the edges the
//  deposit kernel stages in LDS and the shape of its launches.
struct flux_cells : exact_cells {
    gfhip::flux::map map = {};
    device_ptr<double> packed, edges;
    bool is_private = false;
    size_t cap = 0, max_workgroups = 0, lds_bytes = 0;
    unsigned int block = 0;
//  Batches of rays (ray_batches.hpp): 0 for a plain object; otherwise the state is [batch][cell][limb], `cells` counts
//  all of them and `slab` those of one batch, which the launch shape is decided by.
    size_t batches = 0, slab = 0;

    int create(gfhip_context *context, const gfhip_flux_map *given, size_t count, const std::vector<double> &all_edges,
               hipError_t (*prepare)(), size_t batch_count = 0);
    void info_to(struct gfhip_flux_info *info) const;
    const char *rays_refused(uint64_t first_ray, size_t count) const;
    const char *particles_refused(uint64_t first_particle, size_t count) const;
};

//  A flux-surface profile.
struct gfhip_flux : flux_cells {
    double scale = 0.0;                                // cells/(last edge - first edge)
};

//  A spectrum over the flux label and N: cell is*nn + in; the edges of the label, then those of N; fpol as [interval][4].
struct gfhip_spectrum : flux_cells {
    gfhip::flux::field field = {};
    size_t ns = 0, nn = 0;
    double sscale = 0.0, nscale = 0.0;
    device_ptr<double> fpol;
};

//  A distribution of particles over the flux label, the pitch cosine and gamma: cell (is*np + ip)*ng + ig; the three
//  axes' edges one after the other; fpol as [interval][4].
struct gfhip_phase : flux_cells {
    gfhip::flux::field field = {};
    size_t n[3] = {0, 0, 0};
    double scale[3] = {0.0, 0.0, 0.0};
    device_ptr<double> fpol;
};

//  A first-exit tracker of the particles of one push (confinement.hip): per particle lost_step and the context buffer
//  `alive_key`; per check its step (here) and the number of particles it found lost (on the device); the footprint of
//  the losses, cell (ir*nz + iz)*ng + ig, the three axes' edges one after the other.
struct gfhip_confine : flux_cells {
    double limit = 0.0;
    size_t n[3] = {0, 0, 0};
    double scale[3] = {0.0, 0.0, 0.0};
    size_t count = 0, capacity = 0;
    bool is_f32 = false;
    uint64_t alive_key = 0;
    device_ptr<uint32_t> lost_step;
    device_ptr<unsigned long long> newly_lost;         // [capacity]
    std::vector<uint32_t> steps;                       // the checks made
    bool exit_ready = false;                           // the exit buffers of `exit_keys` hold NaN for every confined particle
    uint64_t exit_keys[2] = {0, 0};
};

//  The moments of particles per flux surface (moment_bins.hip): cell is*4 + k, k = density, current, energy, radiation;
//  the edges of the label; fpol as [interval][4].
struct gfhip_moments : flux_cells {
    gfhip::flux::field field = {};
    size_t ns = 0;
    double sscale = 0.0;
    device_ptr<double> fpol;
};

//  A particle source (particle_source.hip): the map and the field as a distribution holds them, the profile's edges and
//  then its probabilities, and the counters placed, unplaced, position_tries, gyro_tries.
struct gfhip_source {
    gfhip_context *ctx = nullptr;
    gfhip::flux::map map = {};
    gfhip::flux::field field = {};
    gfhip::draw::parameters par = {};
    device_ptr<double> packed, fpol, profile;
    double scale = 0.0;                                // ns/(last edge - first edge)
    bool is_f32 = false, refill = false;
    size_t max_workgroups = 0;
    device_ptr<unsigned long long> counters;
};

#define GFHIP_TRY(ctx, call, what) do { if ((ctx)->check((call), (what))) return 1; } while (0)

extern "C" int gfhip_max_concurrency(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) {
        return 0;
    }
    return count;
}

extern "C" const char *gfhip_device_type(void) {
    return "HIP GPU";
}

extern "C" int gfhip_shard_bounds(size_t total, size_t shards, size_t index, size_t *begin, size_t *end) {
    if (shards == 0 || index >= shards) return 1;
    const size_t batch = total/shards;
    const size_t extra = total%shards;
    const size_t first = index*batch + (index < extra ? index : extra);
    if (begin) *begin = first;
    if (end) *end = first + batch + (extra > index ? 1 : 0);
    return 0;
}

extern "C" const char *gfhip_last_error(const gfhip_context *ctx) {
    return ctx ? ctx->error.c_str() : creation_error.c_str();
}

extern "C" gfhip_context *gfhip_create_context(int index, void *stream) {
    int count = 0;
    hipError_t status = hipGetDeviceCount(&count);
    if (status != hipSuccess || count == 0) {
        creation_error = "no HIP device available";
        return nullptr;
    }
    if (index < 0 || index >= count) {
        creation_error = "device index out of range";
        return nullptr;
    }
    std::unique_ptr<gfhip_context> ctx(new gfhip_context);
    ctx->device = index;
    if ((status = hipSetDevice(index)) != hipSuccess) {
        creation_error = std::string("hipSetDevice: ") + hipGetErrorString(status);
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, index) == hipSuccess) {
        ctx->num_cus = static_cast<unsigned int> (prop.multiProcessorCount);
        const std::string arch(prop.gcnArchName);
        if (arch.rfind("gfx950", 0) != 0) {
            creation_error = "libgf_hip is built for gfx950 (MI355X); device is " + arch;
            return nullptr;
        }
    }
    if (stream) {
        ctx->stream = static_cast<hipStream_t> (stream);
    } else {
        if ((status = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
            creation_error = std::string("hipStreamCreate: ") + hipGetErrorString(status);
            return nullptr;
        }
        ctx->own_stream.reset(ctx->stream);
    }
    if (allocate(ctx->device_flags, sizeof(unsigned int)) != hipSuccess ||
        hipMemset(ctx->device_flags.get(), 0, sizeof(unsigned int)) != hipSuccess ||
        allocate(ctx->device_scalar, 8*sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(ctx->device_scalar.get(), 0, 8*sizeof(unsigned long long)) != hipSuccess ||
        allocate(ctx->host_scalar, 8*sizeof(unsigned long long)) != hipSuccess ||
        allocate(ctx->device_converge, sizeof(gfhip::converge_state)) != hipSuccess ||
        allocate(ctx->host_converge, sizeof(gfhip::converge_state)) != hipSuccess) {
        creation_error = "cannot allocate reduction scalars";
        return nullptr;
    }
    return ctx.release();
}

extern "C" void gfhip_destroy_context(gfhip_context *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete ctx;
}

//  Where code objects, and the emission orders the assembly search chose, are looked for: GFHIP_CACHE_DIR, then the package.
static std::vector<std::string> cache_directories() {
    std::vector<std::string> directories;
    if (const char *env = std::getenv("GFHIP_CACHE_DIR")) directories.push_back(env);
    directories.push_back(library_directory() + "/kernel_cache");
    return directories;
}

//  Parse an item and plan its lowering (plan.hpp) at the level the caller asks for, under the options of the environment
//  (GFHIP_LEVEL among them: it overrides the caller), read here once per entry point.
static bool parse_and_plan(const void *gfir, const size_t bytes, const uint32_t level, gfhip::item &it, gfhip::item_plan &plan,
                           std::string &error, uint32_t *planned_level = nullptr) {
    if (!it.parse(gfir, bytes, error)) return false;
    const gfhip::codegen_options options = gfhip::codegen_options::from_environment(level);
    if (planned_level) *planned_level = options.level;
    plan = gfhip::plan_item(it, options, cache_directories());
    return true;
}

extern "C" gfhip_kernel *gfhip_add_kernel(gfhip_context *ctx, const void *gfir, size_t bytes, size_t num_rays) {
    return gfhip_add_kernel_at(ctx, gfir, bytes, num_rays, 0);
}

extern "C" gfhip_kernel *gfhip_add_kernel_at(gfhip_context *ctx, const void *gfir, size_t bytes, size_t num_rays, uint32_t level) {
    if (!ctx) return nullptr;
    std::unique_ptr<gfhip_kernel> k(new gfhip_kernel);
    k->ctx = ctx;
    k->num_rays = num_rays;
    gfhip::item_plan plan;
    if (!parse_and_plan(gfir, bytes, level, k->item, plan, ctx->error, &k->level)) {
        return nullptr;
    }
    k->whole.low = std::move(plan.whole);
    for (auto &piece : plan.pieces) k->pieces.emplace_back(std::move(piece));
    if (plan.redo) k->redo.emplace(std::move(*plan.redo));
    if (!k->pieces.empty()) {
        k->chunk = plan.chunk(num_rays, k->item.element_size());
        k->handover.resize(plan.slots);
    }
    ctx->kernels.push_back(std::move(k));
    return ctx->kernels.back().get();
}

extern "C" int gfhip_export_piece(const void *gfir, size_t bytes, uint32_t index, void **piece, size_t *piece_bytes) {
    return gfhip_export_piece_at(gfir, bytes, index, piece, piece_bytes, 0);
}

extern "C" int gfhip_export_piece_at(const void *gfir, size_t bytes, uint32_t index, void **piece, size_t *piece_bytes, uint32_t level) {
    gfhip::item it;
    gfhip::item_plan planned;
    if (!piece || !piece_bytes) return 1;
    *piece = nullptr;
    *piece_bytes = 0;
    if (!parse_and_plan(gfir, bytes, level, it, planned, creation_error)) return 1;
    if (index >= planned.pieces.size()) return 0;
    const gfhip::segment &plan = planned.pieces[index].plan;
    std::vector<int32_t> head = {static_cast<int32_t> (plan.piece.symbols.size()), static_cast<int32_t> (plan.piece.outputs.size()),
                                 static_cast<int32_t> (planned.slots), static_cast<int32_t> (planned.pieces.size())};
    head.insert(head.end(), plan.symbol_state.begin(), plan.symbol_state.end());
    head.insert(head.end(), plan.symbol_slot.begin(), plan.symbol_slot.end());
    head.insert(head.end(), plan.output_slot.begin(), plan.output_slot.end());
    head.insert(head.end(), plan.output_original.begin(), plan.output_original.end());
    const std::vector<uint8_t> body = plan.piece.serialize();
    *piece_bytes = head.size()*4 + body.size();
    *piece = std::malloc(*piece_bytes);
    std::memcpy(*piece, head.data(), head.size()*4);
    std::memcpy(static_cast<char *> (*piece) + head.size()*4, body.data(), body.size());
    return 0;
}

extern "C" int gfhip_generate_piece_source(const void *gfir, size_t bytes, uint32_t index, char **source, uint64_t *source_hash) {
    return gfhip_generate_piece_source_at(gfir, bytes, index, source, source_hash, 0);
}

extern "C" int gfhip_generate_piece_source_at(const void *gfir, size_t bytes, uint32_t index, char **source, uint64_t *source_hash,
                                              uint32_t level) {
    gfhip::item it;
    gfhip::item_plan plan;
    if (!source) return 1;
    *source = nullptr;
    if (!parse_and_plan(gfir, bytes, level, it, plan, creation_error)) return 1;
    const gfhip::lowered *low = nullptr;
    if (plan.pieces.empty()) {
        if (index == 0) low = &plan.whole;
    } else if (index < plan.pieces.size()) {
        low = &plan.pieces[index].low;
    } else if (plan.redo && index == plan.pieces.size()) {
        low = &plan.redo->low;
    }
    if (!low) return 0;                                 // past the last piece: *source stays NULL
    if (source_hash) *source_hash = low->hash;
    *source = static_cast<char *> (std::malloc(low->source.size() + 1));
    std::memcpy(*source, low->source.c_str(), low->source.size() + 1);
    return 0;
}

extern "C" char *gfhip_generate_source(const void *gfir, size_t bytes, uint64_t *source_hash) {
    return gfhip_generate_source_at(gfir, bytes, source_hash, 0);
}

extern "C" char *gfhip_generate_source_at(const void *gfir, size_t bytes, uint64_t *source_hash, uint32_t level) {
    gfhip::item it;
    gfhip::item_plan plan;
    if (!parse_and_plan(gfir, bytes, level, it, plan, creation_error)) return nullptr;
//  An item in pieces: the texts of its pieces one after the other (each is a translation unit of its
//  own: gfhip_generate_piece_source hands them out one by one).
    std::string text = plan.whole.source;
    for (auto &piece : plan.pieces) text += piece.low.source;
    if (source_hash) *source_hash = plan.whole.hash;
    char *copy = static_cast<char *> (std::malloc(text.size() + 1));
    std::memcpy(copy, text.c_str(), text.size() + 1);
    return copy;
}

extern "C" void gfhip_free_string(char *text) {
    std::free(text);
}

//  The code object of one lowered kernel text: from the kernel cache (by source hash) or hipRTC.
static int load_code_object(gfhip_context *ctx, const std::string &name, const gfhip::lowered &low,
                            std::vector<char> &code, bool &from_cache) {
    const std::string file = hash_name(low.hash) + ".hsaco";
    from_cache = false;
    for (auto &d : cache_directories()) {
        if (read_file(d + "/" + file, code)) {
            from_cache = true;
            return 0;
        }
    }
    if (std::getenv("GFHIP_REQUIRE_CACHE")) {
        return ctx->fail("kernel " + name + " (" + file + ") not in the kernel cache and GFHIP_REQUIRE_CACHE is set");
    }
    hiprtcProgram program;
    if (hiprtcCreateProgram(&program, low.source.c_str(), (name + ".hip").c_str(), 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        return ctx->fail("hiprtcCreateProgram failed");
    }
    const char *options[] = {"-O3", "-ffp-contract=off", "-fno-slp-vectorize", "--offload-arch=gfx950"};
    const hiprtcResult result = hiprtcCompileProgram(program, 4, options);
    if (result != HIPRTC_SUCCESS) {
        size_t log_size = 0;
        hiprtcGetProgramLogSize(program, &log_size);
        std::string log(log_size, '\0');
        if (log_size) hiprtcGetProgramLog(program, &log[0]);
        hiprtcDestroyProgram(&program);
        return ctx->fail("hipRTC failed for " + name + ": " + log);
    }
    size_t size = 0;
    hiprtcGetCodeSize(program, &size);
    code.resize(size);
    hiprtcGetCode(program, code.data());
    hiprtcDestroyProgram(&program);
    if (const char *env = std::getenv("GFHIP_CACHE_DIR")) {
        ::mkdir(env, 0755);
        std::ofstream f(std::string(env) + "/" + file, std::ios::binary);
        f.write(code.data(), static_cast<std::streamsize> (code.size()));
    }
    return 0;
}

//  Build one kernel of `rays` lanes of work per launch from `piece.low`.  Module, functions and packs are
//  committed to `piece` only when every step has succeeded, so a failed build leaves it as it was (a later
//  gfhip_compile retries).
static int build_module(gfhip_context *ctx, const gfhip::item &item, built_piece &piece, const size_t rays) {
    const gfhip::lowered &low = piece.low;
    built_piece out;
    std::vector<char> code;
    if (load_code_object(ctx, item.name, low, code, out.from_cache)) return 1;

    hipModule_t module = nullptr;
    GFHIP_TRY(ctx, hipModuleLoadData(&module, code.data()), "hipModuleLoadData");
    out.module.reset(module);
    GFHIP_TRY(ctx, hipModuleGetFunction(&out.function, module, low.kernel_name.c_str()), "hipModuleGetFunction");
    if (low.has_max) {
        GFHIP_TRY(ctx, hipModuleGetFunction(&out.max_function, module, (low.kernel_name + "_max").c_str()), "hipModuleGetFunction(max)");
    }
    if (low.has_converge) {
        GFHIP_TRY(ctx, hipModuleGetFunction(&out.converge_function, module, (low.kernel_name + "_converge").c_str()),
                  "hipModuleGetFunction(converge)");
    }
    if (low.batch > 1) {
        GFHIP_TRY(ctx, hipModuleGetFunction(&out.batch_function, module, (low.kernel_name + "_batch").c_str()),
                  "hipModuleGetFunction(batch)");
    }
    (void)hipFuncGetAttribute(&out.vgprs, HIP_FUNC_ATTRIBUTE_NUM_REGS, out.function);
    (void)hipFuncGetAttribute(&out.lds_static, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, out.function);
    (void)hipFuncGetAttribute(&out.scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, out.function);
    if (low.lds_bytes > 48*1024) {
        for (hipFunction_t f : {out.function, out.max_function, out.converge_function, out.batch_function}) {
            if (f) (void)hipFuncSetAttribute(reinterpret_cast<const void *> (f), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int> (low.lds_bytes));
        }
    }

//  Pack and upload the tables: [cell][column], padded to the pack stride.
    const size_t esize = item.element_size();
    const size_t parts = item.is_complex() ? 2 : 1;
    const bool wide = item.base_is_f64();
    for (const gfhip::pack &pk : low.packs) {
        const size_t cells = pk.cells();
        std::vector<unsigned char> host(pk.elements()*esize, 0);
        for (size_t column = 0; column < pk.tables.size(); column++) {
            const gfhip::table &t = item.tables[pk.tables[column]];
            for (size_t cell = 0; cell < cells; cell++) {
                for (size_t part = 0; part < parts; part++) {
                    const size_t at = (cell*pk.stride + column)*parts + part;
                    if (wide) {
                        reinterpret_cast<double *> (host.data())[at] = t.data[cell*parts + part];
                    } else {
                        reinterpret_cast<float *> (host.data())[at] = static_cast<float> (t.data[cell*parts + part]);
                    }
                }
            }
        }
        out.packs.emplace_back();
        GFHIP_TRY(ctx, allocate(out.packs.back(), host.size() ? host.size() : 8), "hipMalloc(pack)");
        GFHIP_TRY(ctx, hipMemcpy(out.packs.back().get(), host.data(), host.size(), hipMemcpyHostToDevice), "hipMemcpy(pack)");
    }

//  Launch geometry: one lane per ray; the kernel grid-strides, so cap the grid
//  at a few waves of workgroups per CU.
    const size_t block = low.block_size;
    size_t want = (rays + block - 1)/block;
    if (want < 1) want = 1;
//  Persistent-style grid: a few workgroups per resident slot, the kernel grid-strides.
//  Measured (1e7-particle fp64 push): exact grid 0.276 ms, 64 per CU 0.245, 16 per CU 0.235.
//  Register-bound items that fit one workgroup per CU (the RK4 kernel: 507 registers, one wave
//  per SIMD) run best with exactly one workgroup per CU: 0.279 vs 0.298 ms per step at 1e6
//  rays (the coefficient packs are staged into LDS once per workgroup instead of 15 times).
    int resident = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&resident, out.function, static_cast<int> (block),
                                                           low.lds_bytes) != hipSuccess || resident < 1) {
        resident = 1;
    }
    size_t cap = static_cast<size_t> (ctx->num_cus)*static_cast<size_t> (resident)*(resident == 1 ? 1 : 4);
//  The assembly body (two workgroups resident per CU, VALU busy 98 % of the time its waves are resident): the finer the
//  grid the better the CUs finish together — 2 per CU 1.90 ms per RK4 step at 1e7 rays, 8: 1.79, 16..48: 1.76, 64: 1.75,
//  one workgroup per tile (153): 1.78 (profiles/r03_asm_grid.jsonl).
    if (low.assembly) cap = static_cast<size_t> (ctx->num_cus)*64u;
    if (const char *env = std::getenv("GFHIP_GRID_PER_CU")) {
        cap = static_cast<size_t> (ctx->num_cus)*static_cast<size_t> (std::atoi(env) > 0 ? std::atoi(env) : 1);
    }
    out.grid = static_cast<unsigned int> (want < cap ? want : cap);
//  A kernel that draws random numbers: lane t owns MT19937 state t of 1024 and serves elements
//  t, t + 1024, ... in order (cuda_context.hpp:509-522 launches one 1024-thread block per 1024
//  elements, one after the other).
    if (item.has_random() && out.grid*block > 1024) out.grid = static_cast<unsigned int> (1024/block);

//  The piece keeps its plan and lowering (`item` may be the plan's: not used past this point).
    out.plan = std::move(piece.plan);
    out.low = std::move(piece.low);
    piece = std::move(out);
    return 0;
}

static int build_kernel(gfhip_context *ctx, gfhip_kernel *k) {
    if (k->pieces.empty()) {
        if (build_module(ctx, k->item, k->whole, k->num_rays)) return 1;
        k->built = true;
        return 0;
    }
//  A segmented item: every piece is a kernel of its own over one chunk of rays; one device array
//  per hand-over slot.  The kernel counts as built only when every piece has been.
    for (auto &piece : k->pieces) {
        if (build_module(ctx, piece.plan.piece, piece, k->chunk)) return 1;
    }
    const size_t bytes = k->chunk*k->item.element_size();
    for (auto &slot : k->handover) {
        GFHIP_TRY(ctx, allocate(slot, bytes ? bytes : 8), "hipMalloc(hand-over)");
    }
    if (k->redo) {
        if (build_module(ctx, k->redo->plan.piece, *k->redo, 64*256)) return 1;
        const size_t rays = k->num_rays ? k->num_rays : 1;
        GFHIP_TRY(ctx, allocate(k->flagged, rays), "hipMalloc(flagged)");
        GFHIP_TRY(ctx, hipMemset(k->flagged.get(), 0, rays), "hipMemset(flagged)");
        GFHIP_TRY(ctx, allocate(k->redo_list, rays*sizeof(unsigned int)), "hipMalloc(redo list)");
        GFHIP_TRY(ctx, allocate(k->redo_count, 2*sizeof(unsigned int)), "hipMalloc(redo count)");
        GFHIP_TRY(ctx, hipMemset(k->redo_count.get(), 0, 2*sizeof(unsigned int)), "hipMemset(redo count)");
    }
    built_piece &whole = k->whole;
    whole.from_cache = true;
    for (auto &piece : k->pieces) {
        whole.vgprs = std::max(whole.vgprs, piece.vgprs);
        whole.scratch = std::max(whole.scratch, piece.scratch);
        whole.lds_static = std::max(whole.lds_static, piece.lds_static);
        whole.from_cache = whole.from_cache && piece.from_cache;
    }
    whole.grid = k->pieces[0].grid;
    k->built = true;
    return 0;
}

//  Passes that ran ahead of a caller iterating on gfhip_run_max are taken back before anything else looks at the state
//  (defined with the batch launches below).
static int settle(gfhip_context *ctx);

//  Entry points that touch the device begin here: the context's device, then the state settled.  gfhip_run_max
//  settles only when it does not continue a streak (run_max_ahead); gfhip_compile, gfhip_allocate_buffer and
//  gfhip_kernel_timing look at no state and set the device alone.
static int enter(gfhip_context *ctx) {
    GFHIP_TRY(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    return settle(ctx);
}

//  Whether `k` may be launched: misuse is reported before anything is enqueued.
static int ready(gfhip_kernel *k) {
    if (!k->built) return k->ctx->fail("kernel has not been compiled (gfhip_compile)");
    if (!k->bound) return k->ctx->fail("kernel arguments are not bound (gfhip_create_kernel_call)");
    return 0;
}

extern "C" int gfhip_compile(gfhip_context *ctx) {
    if (!ctx) return 1;
    GFHIP_TRY(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    for (auto &k : ctx->kernels) {
        if (!k->built) {
            if (build_kernel(ctx, k.get())) return 1;
        }
    }
    return 0;
}

static int ensure_buffer(gfhip_context *ctx, const uint64_t key, const size_t count, const uint32_t dtype,
                         const void *init, size_t init_count = ~static_cast<size_t> (0)) {
    auto found = ctx->buffers.find(key);
    if (found == ctx->buffers.end()) {
        buffer b;
        b.count = count;
        b.dtype = dtype;
        const size_t esize = element_bytes(dtype);
        const size_t bytes = count*esize;
        if (init_count > count) init_count = count;
        GFHIP_TRY(ctx, allocate(b.owned, bytes ? bytes : 8), "hipMalloc(buffer)");
        b.pointer = b.owned.get();
        if (!init || init_count < count) {
//  On the context's stream and finished before anything else: hipMemset returns before the fill of device memory has
//  run, on the null stream, which the context's non-blocking stream is not ordered with; an upload queued right behind
//  the allocation (gfhip_copy_to_device) could land first and be zeroed.
            GFHIP_TRY(ctx, hipMemsetAsync(b.pointer, 0, bytes, ctx->stream), "hipMemset(buffer)");
            GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        }
        if (init && init_count) {
            GFHIP_TRY(ctx, hipMemcpy(b.pointer, init, init_count*esize, hipMemcpyHostToDevice), "hipMemcpy(init)");
        }
        ctx->buffers[key] = std::move(b);
        return 0;
    }
    if (found->second.count < count) {
        return ctx->fail("buffer is smaller than the kernel's ensemble size");
    }
    if (found->second.dtype != dtype) {
        return ctx->fail("buffer element type does not match the kernel");
    }
    return 0;
}

extern "C" int gfhip_create_kernel_call(gfhip_kernel *k, const uint64_t *input_keys,
                                        const void *const *input_init, const size_t *input_counts,
                                        const uint64_t *output_keys) {
    if (!k) return 1;
    gfhip_context *ctx = k->ctx;
    if (enter(ctx)) return 1;
    const size_t ni = k->item.symbols.size(), no = k->item.outputs.size();
    for (size_t i = 0; i < ni; i++) {
//  An input that index nodes read (index_1D/2D_node) is a buffer of its own length.
        const size_t indexed = k->item.indexed_length(static_cast<uint32_t> (i));
        const size_t given = input_counts ? input_counts[i] : k->num_rays;
        size_t count = k->num_rays;
        if (indexed > count) count = indexed;
        if (input_init && input_init[i] && given > count) count = given;
        if (input_init && input_init[i] && given < indexed) {
            return ctx->fail("initial values of an input that index nodes read are shorter than the indexed length");
        }
        if (ensure_buffer(ctx, input_keys[i], count, k->item.dtype, input_init ? input_init[i] : nullptr, given)) return 1;
    }
    for (size_t o = 0; o < no; o++) {
        if (ensure_buffer(ctx, output_keys[o], k->num_rays, k->item.dtype, nullptr)) return 1;
    }
//  The kernel's pointers are __restrict__: written buffers must be distinct.
    for (size_t o = 0; o < no; o++) {
        for (size_t i = 0; i < ni; i++) {
            if (output_keys[o] == input_keys[i]) return ctx->fail("an output buffer aliases an input buffer");
        }
        for (size_t p = o + 1; p < no; p++) {
            if (output_keys[o] == output_keys[p]) return ctx->fail("two outputs share one buffer");
        }
    }
    for (size_t i = 0; i < ni; i++) {
        for (size_t j = i + 1; j < ni; j++) {
            if (input_keys[i] == input_keys[j]) return ctx->fail("two inputs share one buffer");
        }
    }
    k->input_keys.assign(input_keys, input_keys + ni);
    k->output_keys.assign(output_keys, output_keys + no);
    k->bound = true;
    return 0;
}

//  Kernel arguments by value, in order, one 8-byte slot each (a 4-byte argument in its low half):
//  hipModuleLaunchKernel is handed the slots' addresses and copies as many bytes from each as its argument takes.
struct arguments {
    std::vector<uint64_t> slots;
    template<typename T> arguments &add(const T value) {
        static_assert(sizeof(T) <= sizeof(uint64_t) && std::is_trivially_copyable<T>::value, "one slot per argument");
        uint64_t slot = 0;
        std::memcpy(&slot, &value, sizeof(T));
        slots.push_back(slot);
        return *this;
    }
};

//  What every kernel of an item takes first: its inputs, its outputs, its packs, the random states (items
//  that draw), device_flags and the number of lanes `n`.  A segment (segments.hpp) reads and writes the rays
//  from `first` on, or the hand-over slots its plan names.
static arguments state_arguments(gfhip_kernel *k, const built_piece &code, const unsigned long long n,
                                 const bool segment = false, const size_t first = 0) {
    gfhip_context *ctx = k->ctx;
    auto state = [&] (const uint64_t key) -> void * {
        return static_cast<char *> (ctx->buffers[key].pointer) + first*k->item.element_size();
    };
    arguments args;
    if (segment) {
        const gfhip::segment &plan = code.plan;
        for (size_t i = 0; i < plan.piece.symbols.size(); i++) {
            args.add(plan.symbol_state[i] >= 0 ? state(k->input_keys[plan.symbol_state[i]]) : k->handover[plan.symbol_slot[i]].get());
        }
        for (size_t o = 0; o < plan.piece.outputs.size(); o++) {
            args.add(plan.output_slot[o] >= 0 ? k->handover[plan.output_slot[o]].get() : state(k->output_keys[plan.output_original[o]]));
        }
    } else {
        for (auto key : k->input_keys) args.add(state(key));
        for (auto key : k->output_keys) args.add(state(key));
    }
    for (auto &p : code.packs) args.add(p.get());
    if (k->item.has_random()) args.add(k->random_states);
    args.add(ctx->device_flags.get());
    args.add(n);
    return args;
}

//  One hipModuleLaunchKernel: `function` of `code` over `grid` workgroups of its block size, with its LDS bytes.
static int enqueue(gfhip_context *ctx, const built_piece &code, hipFunction_t function, const unsigned int grid,
                   arguments &args, const char *what) {
    std::vector<void *> params;
    for (auto &slot : args.slots) params.push_back(&slot);
    return ctx->check(hipModuleLaunchKernel(function, grid, 1, 1, code.low.block_size, 1, 1, static_cast<unsigned int> (code.low.lds_bytes),
                                            ctx->stream, params.data(), nullptr), what);
}

//  A segmented item (segments.hpp): `steps` passes, each a walk over the ensemble in chunks, each chunk
//  through the sequence of segment kernels.  A piece's symbols are state arrays (offset to the chunk) or
//  hand-over slots; its outputs are slots or, in the last piece, the item's outputs.  Only the last
//  piece stores state, so a chunk's pieces all read the state of the beginning of the pass.
static int walk_pieces(gfhip_kernel *k, const uint32_t steps) {
    gfhip_context *ctx = k->ctx;
    for (uint32_t step = 0; step < steps; step++) {
        for (size_t first = 0; first < k->num_rays; first += k->chunk) {
            const unsigned long long n = std::min(k->chunk, k->num_rays - first);
            for (auto &piece : k->pieces) {
                arguments args = state_arguments(k, piece, n, true, first);
                if (k->redo) {
                    args.add(k->flagged.get() + first);
                    if (&piece == &k->pieces.back()) {
                        args.add(k->redo_list.get()).add(k->redo_count.get()).add(static_cast<unsigned int> (first));
                    }
                }
                args.add(1u);
                const size_t want = (n + piece.low.block_size - 1)/piece.low.block_size;
                const unsigned int grid = static_cast<unsigned int> (want < piece.grid ? want : piece.grid);
                if (enqueue(ctx, piece, piece.function, grid, args, "hipModuleLaunchKernel(segment)")) return 1;
            }
        }
        if (k->redo) {
//  The lanes the segments left alone: the whole item with the compiler's division, from the untouched state.
//  One workgroup per CU: an empty list costs the launch either way (5 us), a long one (the O-mode step on the CLI beam
//  sends a third of its lanes here) is walked by the whole chip.
            arguments args = state_arguments(k, *k->redo, k->num_rays);
            args.add(k->flagged.get()).add(k->redo_list.get()).add(k->redo_count.get()).add(1u);
            if (enqueue(ctx, *k->redo, k->redo->function, ctx->num_cus, args, "hipModuleLaunchKernel(redo)")) return 1;
//  (the redo kernel leaves the count — and its arrival counter, the second word — at zero)
        }
    }
    return 0;
}

//  Every launch of an item goes through here: `<name>` (`steps` passes; a segmented item walks its segment
//  kernels and its redo launch instead), `<name>_max` (`tail`: reduce, stop — a non-null `stop` word that reads
//  non-zero makes the launch return at once), `<name>_batch` (`tail`: reduce, stop, the undo arrays) or
//  `<name>_converge` (`tail`: tolerance, max_iterations, counter; no `steps` argument).  A launch of no work
//  enqueues nothing.  With `timed`, every ctx->timing-th launch of the item is bracketed by an event pair.
static int launch(gfhip_kernel *k, const gfhip::entry which, const uint32_t steps, const arguments &tail = arguments(),
                  const bool timed = true) {
    gfhip_context *ctx = k->ctx;
    if (ready(k)) return 1;
    if (k->num_rays == 0 || steps == 0) return 0;
    if (k->item.has_random() && !k->random_states) {
        return ctx->fail("the item draws random numbers but no random state is bound (gfhip_set_random_state)");
    }
    event_pair ev;
    const bool time_this = timed && ctx->timing && (k->launch_count++ % ctx->timing) == 0;
    if (time_this) {
        if (!k->free_events.empty()) {
            ev = std::move(k->free_events.back());
            k->free_events.pop_back();
        } else {
            hipEvent_t start = nullptr, stop = nullptr;
            GFHIP_TRY(ctx, hipEventCreate(&start), "hipEventCreate");
            ev.start.reset(start);
            GFHIP_TRY(ctx, hipEventCreate(&stop), "hipEventCreate");
            ev.stop.reset(stop);
        }
        GFHIP_TRY(ctx, hipEventRecord(ev.start.get(), ctx->stream), "hipEventRecord");
    }
    if (!k->pieces.empty()) {
        if (walk_pieces(k, steps)) return 1;
    } else {
        const built_piece &whole = k->whole;
        hipFunction_t function = whole.function;
        const char *what = "hipModuleLaunchKernel";
        if (which == gfhip::entry::max) function = whole.max_function;
        if (which == gfhip::entry::converge) function = whole.converge_function, what = "hipModuleLaunchKernel(converge)";
        if (which == gfhip::entry::batch) function = whole.batch_function, what = "hipModuleLaunchKernel(batch)";
        arguments args = state_arguments(k, whole, k->num_rays);
        if (which != gfhip::entry::converge) args.add(steps);
        args.slots.insert(args.slots.end(), tail.slots.begin(), tail.slots.end());
        if (enqueue(ctx, whole, function, whole.grid, args, what)) return 1;
    }
    if (time_this) {
        GFHIP_TRY(ctx, hipEventRecord(ev.stop.get(), ctx->stream), "hipEventRecord");
        k->events.push_back(std::move(ev));
    }
    return 0;
}

extern "C" int gfhip_run(gfhip_kernel *k, uint32_t steps) {
    if (!k) return 1;
    if (enter(k->ctx)) return 1;
    return launch(k, gfhip::entry::plain, steps);
}

static double decode_max(const unsigned long long key, const bool f64) {
    return f64 ? gfhip::from_ordered_key<double> (key) : static_cast<double> (gfhip::from_ordered_key<float> (key));
}

//  One pass + the max of its last output left in ctx->device_scalar (ordered image), no sync:
//  inside the launch for items that have `<name>_max`, else the separate reduction kernel.
static int enqueue_pass_with_max(gfhip_kernel *k, const unsigned int *stop) {
    gfhip_context *ctx = k->ctx;
    if (k->whole.max_function) {
        return launch(k, gfhip::entry::max, 1, arguments().add(ctx->device_scalar.get()).add(stop));
    }
    if (launch(k, gfhip::entry::plain, 1)) return 1;
    const buffer &b = ctx->buffers[k->output_keys.back()];
    gfhip::launch_max_reduce(b.pointer, k->num_rays, k->item.dtype == GFIR_F64, ctx->device_scalar.get(),
                             ctx->num_cus, ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "max_reduce launch");
    return 0;
}

//  The max left in ctx->device_scalar, on the host.
static int read_max(gfhip_context *ctx, const bool f64, double *value) {
    GFHIP_TRY(ctx, hipMemcpyAsync(ctx->host_scalar.get(), ctx->device_scalar.get(), sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    *value = decode_max(*ctx->host_scalar, f64);
    return 0;
}

//  The largest of `count` real values (reduce.hip), on the host.
static int max_of(gfhip_context *ctx, const void *values, const size_t count, const bool f64, double *value) {
    GFHIP_TRY(ctx, hipMemsetAsync(ctx->device_scalar.get(), 0, sizeof(unsigned long long), ctx->stream), "hipMemsetAsync");
    gfhip::launch_max_reduce(values, count, f64, ctx->device_scalar.get(), ctx->num_cus, ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "max_reduce launch");
    return read_max(ctx, f64, value);
}

//  The element of largest modulus of `count` complex values, as cpu_context.hpp:314-318 selects it
//  (std::max_element on std::abs, the first of equals), on the host: value[0] + i value[1].
static int max_modulus(gfhip_context *ctx, const void *values, const size_t count, const bool wide, double *value) {
    gfhip::launch_max_modulus(values, count, wide, ctx->device_converge.get(), ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "max_modulus launch");
    GFHIP_TRY(ctx, hipMemcpyAsync(ctx->host_converge.get(), ctx->device_converge.get(), 16, hipMemcpyDeviceToHost, ctx->stream),
              "hipMemcpyAsync");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (wide) {
        std::memcpy(value, ctx->host_converge.get(), 16);
    } else {
        float narrow[2];
        std::memcpy(narrow, ctx->host_converge.get(), 8);
        value[0] = narrow[0];
        value[1] = narrow[1];
    }
    return 0;
}

//  Complex items: run, then the element of largest modulus of the last output.
extern "C" int gfhip_run_max_complex(gfhip_kernel *k, double *value) {
    if (!k || !value) return 1;
    gfhip_context *ctx = k->ctx;
    if (ready(k)) return 1;
    if (k->output_keys.empty()) return ctx->fail("converge item has no output to reduce");
    if (!k->item.is_complex()) {
        value[1] = 0.0;
        return gfhip_run_max(k, value);
    }
    if (enter(ctx) || launch(k, gfhip::entry::plain, 1)) return 1;
    value[0] = value[1] = 0.0;
    if (k->num_rays == 0) return 0;
    return max_modulus(ctx, ctx->buffers[k->output_keys.back()].pointer, k->num_rays, k->item.base_is_f64(), value);
}

extern "C" int gfhip_reduce_max(gfhip_context *ctx, uint64_t key, double *value) {
    if (!ctx || !value) return 1;
    if (enter(ctx)) return 1;
    auto found = ctx->buffers.find(key);
    if (found == ctx->buffers.end()) return ctx->fail("unknown buffer key");
    const buffer &b = found->second;
    const bool wide = b.dtype == GFIR_F64 || b.dtype == GFIR_C64;
    value[0] = value[1] = 0.0;
    if (b.dtype == GFIR_C32 || b.dtype == GFIR_C64) {
        return b.count ? max_modulus(ctx, b.pointer, b.count, wide, value) : 0;
    }
    if (b.count == 0) {
        value[0] = -std::numeric_limits<double>::infinity();
        return 0;
    }
    return max_of(ctx, b.pointer, b.count, wide, value);
}

static int run_max_ahead(gfhip_kernel *k, double *max_value, bool &answered);

extern "C" int gfhip_run_max(gfhip_kernel *k, double *max_value) {
    if (!k) return 1;
    gfhip_context *ctx = k->ctx;
    GFHIP_TRY(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    if (ready(k)) return 1;
    if (k->output_keys.empty()) return ctx->fail("converge item has no output to reduce");
    if (k->item.is_complex()) return ctx->fail("complex item: use gfhip_run_max_complex");
    bool answered = false;
    if (run_max_ahead(k, max_value, answered)) return 1;
    if (!answered) {
        GFHIP_TRY(ctx, hipMemsetAsync(ctx->device_scalar.get(), 0, sizeof(unsigned long long), ctx->stream), "hipMemsetAsync");
        if (enqueue_pass_with_max(k, nullptr) || read_max(ctx, k->item.dtype == GFIR_F64, max_value)) return 1;
        if (k->num_rays == 0) *max_value = -std::numeric_limits<double>::infinity();
    }
    ctx->max_streak = k;
    return 0;
}

//  One pass and its max in the item's own type V: through the C ABI's entries, so that a streak of them runs ahead.
//  The second value is what gfhip_converge reports of it: the value itself, the modulus of a complex one.
template<typename T>
static int pass_with_max(gfhip_kernel *k, T &max, double &reported) {
    if (gfhip_run_max(k, &reported)) return 1;
    max = static_cast<T> (reported);
    reported = static_cast<double> (max);
    return 0;
}
template<typename B>
static int pass_with_max(gfhip_kernel *k, std::complex<B> &max, double &reported) {
    double value[2];
    if (gfhip_run_max_complex(k, value)) return 1;
    max = std::complex<B> (static_cast<B> (value[0]), static_cast<B> (value[1]));
    reported = static_cast<double> (gfhip::mag(max));
    return 0;
}

//  workflow::converge_item::run, workflow.hpp:179-205, in the item's own type (converge_state.hpp has the loop's
//  test), one host synchronisation per pass: the form for complex items (max = the element of largest modulus; the
//  loop compares moduli), for items without `<name>_max` and for empty ensembles.
template<typename V>
static int converge_loop(gfhip_kernel *k, const double tolerance, const size_t max_iterations,
                         size_t *iterations_out, double *last_max) {
    gfhip::converge_step<V> step(tolerance, max_iterations);
    V max_residual;
    double reported;
    do {
        if (pass_with_max(k, max_residual, reported)) return 1;
    } while (step.advance(max_residual));
    if (iterations_out) *iterations_out = static_cast<size_t> (step.iterations);
    if (last_max) *last_max = reported;
    return 0;
}

//  One launch of `<name>_batch`: `passes` passes on state kept in registers, the max of each pass folded
//  into reduce[pass]; the setter targets as they were before the launch are saved in the undo arrays.
static int launch_batch(gfhip_kernel *k, const unsigned int passes, const unsigned int *stop) {
    arguments tail;
    tail.add(k->ctx->device_scalar.get()).add(stop);
    for (auto &u : k->undo) tail.add(u.get());
    return launch(k, gfhip::entry::batch, passes, tail);
}

static int ensure_undo(gfhip_kernel *k) {
    if (!k->undo.empty()) return 0;
    std::vector<device_ptr<>> undo(k->item.setters.size());
    for (auto &u : undo) {
        GFHIP_TRY(k->ctx, allocate(u, k->num_rays*k->item.element_size()), "hipMalloc(undo)");
    }
    k->undo = std::move(undo);
    return 0;
}

//  Back to the state of the beginning of the last batch, then only its first `keep` passes: the ones that count.
static int take_back(gfhip_kernel *k, const unsigned int keep) {
    gfhip_context *ctx = k->ctx;
    for (size_t s = 0; s < k->item.setters.size(); s++) {
        void *target = ctx->buffers[k->input_keys[k->item.setters[s].input]].pointer;
        GFHIP_TRY(ctx, hipMemcpyAsync(target, k->undo[s].get(), k->num_rays*k->item.element_size(), hipMemcpyDeviceToDevice,
                                      ctx->stream), "hipMemcpyAsync(undo)");
    }
    return launch_batch(k, keep, nullptr);
}

//  gfhip_run_max called again and again with nothing in between is the reference's converge loop seen from below
//  (workflow.hpp:179-205: the host tests every max; hip_context's create_max_call forwards each call here).  From the
//  second call of such a streak on, a `<name>_batch` launch runs the pass that is asked for AND the next ones, each with
//  its own max; the following calls are answered from those maxes without a launch or a synchronisation.  Whatever
//  entry point comes next (settle) takes back the passes nobody asked for: the state of the beginning of the batch is
//  in the undo arrays, the passes that were asked for run again.  25 passes of the benchmark's Newton solve: 10 launches
//  and host synchronisations instead of 25.  GFHIP_RUN_AHEAD=0 turns it off.
static int settle(gfhip_context *ctx) {
    ctx->max_streak = nullptr;
    gfhip_kernel *k = ctx->running_ahead;
    if (!k) return 0;
    ctx->running_ahead = nullptr;
    const unsigned int asked = k->ahead_taken, ran = static_cast<unsigned int> (k->ahead.size());
    k->ahead.clear();
    k->ahead_taken = 0;
    return asked == ran ? 0 : take_back(k, asked);
}

static int run_max_ahead(gfhip_kernel *k, double *max_value, bool &answered) {
    gfhip_context *ctx = k->ctx;
    answered = false;
    static const bool enabled = !(std::getenv("GFHIP_RUN_AHEAD") && std::string(std::getenv("GFHIP_RUN_AHEAD")) == "0");
    if (ctx->running_ahead == k && k->ahead_taken < k->ahead.size()) {
        *max_value = k->ahead[k->ahead_taken++];
        answered = true;
        return 0;
    }
    const bool streak = ctx->max_streak == k;
    if (settle(ctx)) return 1;                     // nothing to take back if every pass of k's last batch was asked for
    if (!enabled || !streak || !k->whole.batch_function || k->num_rays == 0 || k->whole.low.batch < 2) return 0;
    if (ensure_undo(k)) return 1;
    const unsigned int batch = std::min(k->whole.low.batch, 8u);
    GFHIP_TRY(ctx, hipMemsetAsync(ctx->device_scalar.get(), 0, 8*sizeof(unsigned long long), ctx->stream), "hipMemsetAsync");
    if (launch_batch(k, batch, nullptr)) return 1;
    GFHIP_TRY(ctx, hipMemcpyAsync(ctx->host_scalar.get(), ctx->device_scalar.get(), batch*sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    k->ahead.clear();
    for (unsigned int b = 0; b < batch; b++) k->ahead.push_back(decode_max(ctx->host_scalar.get()[b], k->item.dtype == GFIR_F64));
    k->ahead_taken = 1;
    ctx->running_ahead = k;
    *max_value = k->ahead[0];
    answered = true;
    return 0;
}

//  One launch of `passes` passes, the max of each left in ctx->device_scalar[pass] (ordered image), no sync.
static int enqueue_passes_with_max(gfhip_kernel *k, const unsigned int passes, const unsigned int *stop) {
    return passes > 1 ? launch_batch(k, passes, stop) : enqueue_pass_with_max(k, stop);
}

//  Launches per host synchronisation in converge_on_device, the first time and at most: of one pass, of several.
static const size_t queue_depth[2][2] = {{16, 64}, {6, 24}};

//  The same loop with its test on the device (converge_state.hpp: decide): passes are
//  enqueued ahead of the host in growing batches, each followed by the one-thread test; once
//  the test has come out false the passes still queued return at once (`stop`), so exactly the
//  passes of the host loop run, with the same iteration count — and the host synchronises once
//  per batch (twice for the benchmark's 25 passes) instead of once per pass.
//
//  Items with `<name>_batch` (codegen.hpp) run several passes per launch.  A pass of this loop
//  only feeds the next pass of the same ray and the max the loop's test looks at, so a launch may run a
//  few passes on state kept in registers — each pass leaving its own max — and the test (on the device,
//  the same decide) is applied to those maxima in order afterwards.  If the loop
//  turns out to have ended before the last pass of a batch, the state of the beginning of that batch is
//  restored from the undo arrays and the batch is redone with exactly the passes the loop ran: the same
//  passes, iteration count, state and output as one launch per pass, at a third of the sweeps over the
//  state.
static int converge_on_device(gfhip_kernel *k, const double tolerance, const size_t max_iterations,
                              size_t *iterations_out, double *last_max) {
    gfhip_context *ctx = k->ctx;
    const bool f64 = k->item.dtype == GFIR_F64;
    const unsigned int batch = k->whole.batch_function ? k->whole.low.batch : 1;        // passes per launch
    if (batch > 1 && ensure_undo(k)) return 1;
    gfhip::converge_state &host = *ctx->host_converge;
    host = f64 ? gfhip::converge_begin<double> (tolerance, max_iterations) : gfhip::converge_begin<float> (tolerance, max_iterations);
    GFHIP_TRY(ctx, hipMemcpyAsync(ctx->device_converge.get(), &host, sizeof(host), hipMemcpyHostToDevice, ctx->stream),
              "hipMemcpyAsync(converge state)");
    GFHIP_TRY(ctx, hipMemsetAsync(ctx->device_scalar.get(), 0, 8*sizeof(unsigned long long), ctx->stream), "hipMemsetAsync");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");     // `host` is written again below
    const unsigned int *stop = &ctx->device_converge->done;
    const uint64_t first_launch = k->launch_count;
    const size_t events_before = k->events.size();
    size_t queued = queue_depth[batch > 1][0];             // growing
    const size_t most = queue_depth[batch > 1][1];
    for (;;) {
        for (size_t q = 0; q < queued; q++) {
            if (enqueue_passes_with_max(k, batch, stop)) return 1;
            gfhip::launch_converge_decide(f64, ctx->device_scalar.get(), ctx->device_converge.get(), batch, ctx->stream);
            GFHIP_TRY(ctx, hipGetLastError(), "converge_decide launch");
        }
        GFHIP_TRY(ctx, hipMemcpyAsync(&host, ctx->device_converge.get(), sizeof(host), hipMemcpyDeviceToHost, ctx->stream),
                  "hipMemcpyAsync(converge state)");
        GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
        if (host.done) break;
        if (queued < most) queued *= 2;
    }
//  Launch timing: keep the event pairs of the launches that ran; the queued launches that returned at once
//  are not launches of the item's work.
    if (ctx->timing) {
        const uint64_t ran = (static_cast<uint64_t> (host.passes) + host.extra + batch - 1)/batch;
        size_t kept = 0;
        for (uint64_t l = first_launch; l < first_launch + ran; l++) {
            if (l % ctx->timing == 0) kept++;
        }
        while (k->events.size() > events_before + kept) {
            k->free_events.push_back(std::move(k->events.back()));
            k->events.pop_back();
        }
    }
    if (host.extra) {
//  The loop ended inside the last batch: back to the state of its beginning, then only the loop's passes.
        if (take_back(k, host.batch_passes)) return 1;
        GFHIP_TRY(ctx, hipMemsetAsync(ctx->device_scalar.get(), 0, 8*sizeof(unsigned long long), ctx->stream), "hipMemsetAsync");
        GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    }
    if (iterations_out) *iterations_out = static_cast<size_t> (host.iterations);
    if (last_max) *last_max = host.max_residual;
    return 0;
}

extern "C" int gfhip_converge(gfhip_kernel *k, double tolerance, size_t max_iterations,
                              size_t *iterations, double *last_max) {
    if (!k) return 1;
    gfhip_context *ctx = k->ctx;
    if (enter(ctx) || ready(k)) return 1;
    if (k->output_keys.empty()) return ctx->fail("converge item has no output to reduce");
    size_t used = 0;
    double residual = 0.0;
    int status;
    if (k->item.is_complex()) {
        status = k->item.base_is_f64() ? converge_loop<std::complex<double>> (k, tolerance, max_iterations, &used, &residual)
                                       : converge_loop<std::complex<float>> (k, tolerance, max_iterations, &used, &residual);
    } else if (k->whole.max_function && k->num_rays > 0) {             // (every item with `<name>_batch` has `<name>_max`)
        status = converge_on_device(k, tolerance, max_iterations, &used, &residual);
    } else if (k->item.dtype == GFIR_F64) {
        status = converge_loop<double> (k, tolerance, max_iterations, &used, &residual);
    } else {
        status = converge_loop<float> (k, tolerance, max_iterations, &used, &residual);
    }
    if (status) return status;
    if (iterations) *iterations = used;
    if (last_max) *last_max = residual;
    if (used > max_iterations) {
//  Same report as workflow.hpp:197-204.
        std::fprintf(stderr, "Workitem failed to converge with in given iterations.\nMinimum residual reached: %g\n", residual);
    }
    return 0;
}

//  Per-ray converge loop inside one launch (`<name>_converge`, see codegen.hpp).
extern "C" int gfhip_converge_per_ray(gfhip_kernel *k, double tolerance, size_t max_iterations,
                                      size_t *iterations, double *last_max) {
    if (!k) return 1;
    gfhip_context *ctx = k->ctx;
    if (enter(ctx)) return 1;
    if (k->built && !k->whole.converge_function) return ctx->fail("item has no setter/output to converge on");
    if (ready(k)) return 1;
    if (k->num_rays == 0) {
        if (iterations) *iterations = 0;
        if (last_max) *last_max = -std::numeric_limits<double>::infinity();
        return 0;
    }
    const bool f64 = k->item.dtype == GFIR_F64;
    arguments tail;
    if (f64) {
        tail.add(tolerance);
    } else {
        tail.add(static_cast<float> (tolerance));
    }
    tail.add(static_cast<unsigned int> (max_iterations > 0xFFFFFFFEull ? 0xFFFFFFFEull : max_iterations));
//  The iteration counter shares the 8-byte reduction scalar (low word).
    tail.add(reinterpret_cast<unsigned int *> (ctx->device_scalar.get()));
    GFHIP_TRY(ctx, hipMemsetAsync(ctx->device_scalar.get(), 0, sizeof(unsigned long long), ctx->stream), "hipMemsetAsync");
    if (launch(k, gfhip::entry::converge, 1, tail, false)) return 1;
    GFHIP_TRY(ctx, hipMemcpyAsync(ctx->host_scalar.get(), ctx->device_scalar.get(), sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    if (iterations) *iterations = static_cast<unsigned int> (*ctx->host_scalar & 0xFFFFFFFFull);
    if (last_max) return max_of(ctx, ctx->buffers[k->output_keys.back()].pointer, k->num_rays, f64, last_max);
    return 0;
}

extern "C" int gfhip_wait(gfhip_context *ctx) {
    if (!ctx) return 1;
    if (enter(ctx)) return 1;
//  Host mirrors handed out by gfhip_get_host_buffer hold the device contents as of this drain:
//  all copies are queued behind the kernels, then ONE synchronisation.
    for (auto &kv : ctx->buffers) {
        buffer &b = kv.second;
        if (b.mirror && b.count) {
            GFHIP_TRY(ctx, hipMemcpyAsync(b.mirror.get(), b.pointer, b.count*element_bytes(b.dtype),
                                          hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(mirror)");
        }
    }
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return 0;
}

extern "C" int gfhip_get_flags(gfhip_context *ctx, unsigned int *flags) {
    if (!ctx || !flags) return 1;
    if (enter(ctx)) return 1;
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    GFHIP_TRY(ctx, hipMemcpy(flags, ctx->device_flags.get(), sizeof(unsigned int), hipMemcpyDeviceToHost), "hipMemcpy(flags)");
    return 0;
}

static buffer *find_buffer(gfhip_context *ctx, const uint64_t key) {
    auto found = ctx->buffers.find(key);
    if (found == ctx->buffers.end()) {
        ctx->error = "unknown buffer key";
        return nullptr;
    }
    return &found->second;
}

extern "C" int gfhip_copy_to_device(gfhip_context *ctx, uint64_t key, const void *host) {
    if (!ctx) return 1;
    buffer *b = find_buffer(ctx, key);
    if (!b) return 1;
    if (enter(ctx)) return 1;
    GFHIP_TRY(ctx, hipMemcpyAsync(b->pointer, host, b->count*element_bytes(b->dtype),
                                  hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync(H2D)");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return 0;
}

extern "C" int gfhip_copy_to_host(gfhip_context *ctx, uint64_t key, void *host) {
    if (!ctx) return 1;
    buffer *b = find_buffer(ctx, key);
    if (!b) return 1;
    if (enter(ctx)) return 1;
    GFHIP_TRY(ctx, hipMemcpyAsync(host, b->pointer, b->count*element_bytes(b->dtype),
                                  hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(D2H)");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return 0;
}

extern "C" int gfhip_read_element(gfhip_context *ctx, uint64_t key, size_t index, void *element) {
    if (!ctx || !element) return 1;
    buffer *b = find_buffer(ctx, key);
    if (!b) return 1;
    if (index >= b->count) return ctx->fail("index out of range");
    if (enter(ctx)) return 1;
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    const size_t esize = element_bytes(b->dtype);
    GFHIP_TRY(ctx, hipMemcpy(element, static_cast<char *> (b->pointer) + index*esize, esize, hipMemcpyDeviceToHost), "hipMemcpy");
    return 0;
}

extern "C" int gfhip_check_value(gfhip_context *ctx, uint64_t key, size_t index, double *value) {
    if (!ctx || !value) return 1;
    double parts[2] = {0.0, 0.0};
    float narrow[2] = {0.0f, 0.0f};
    buffer *b = find_buffer(ctx, key);
    if (!b) return 1;
    const bool wide = b->dtype == GFIR_F64 || b->dtype == GFIR_C64;
    if (gfhip_read_element(ctx, key, index, wide ? static_cast<void *> (parts) : static_cast<void *> (narrow))) return 1;
    *value = wide ? parts[0] : static_cast<double> (narrow[0]);        // the real part of a complex element
    return 0;
}

extern "C" int gfhip_set_random_state(gfhip_kernel *k, uint64_t key, const void *states, size_t bytes) {
    if (!k) return 1;
    gfhip_context *ctx = k->ctx;
    if (!k->item.has_random()) return 0;
//  The kernel indexes 1024 states of 2500 bytes (random.hpp:44-52 without the CUDA padding).
    const size_t needed = 1024*2500;
    if (!states || bytes < needed) return ctx->fail("a random state of 1024 MT19937 states (2500 bytes each) is required");
    if (enter(ctx)) return 1;
    auto found = ctx->random_states.find(key);
    if (found == ctx->random_states.end()) {
        device_ptr<> device;
        GFHIP_TRY(ctx, allocate(device, bytes), "hipMalloc(random state)");
        GFHIP_TRY(ctx, hipMemcpy(device.get(), states, bytes, hipMemcpyHostToDevice), "hipMemcpy(random state)");
        found = ctx->random_states.emplace(key, std::move(device)).first;
    }
    k->random_states = found->second.get();
    return 0;
}

extern "C" void *gfhip_get_buffer(gfhip_context *ctx, uint64_t key, size_t *count) {
    if (!ctx) return nullptr;
    buffer *b = find_buffer(ctx, key);
    if (!b) return nullptr;
    if (enter(ctx)) return nullptr;            // the caller is about to look at the device buffer
    if (count) *count = b->count;
    return b->pointer;
}

extern "C" int gfhip_allocate_buffer(gfhip_context *ctx, uint64_t key, size_t count, uint32_t dtype) {
    if (!ctx) return 1;
    if (dtype > GFIR_C64) return ctx->fail("bad dtype");
    GFHIP_TRY(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    return ensure_buffer(ctx, key, count, dtype, nullptr);
}

extern "C" int gfhip_get_buffer_info(gfhip_context *ctx, uint64_t key, size_t *count, uint32_t *dtype) {
    if (!ctx) return 1;
    buffer *b = find_buffer(ctx, key);
    if (!b) return 1;
    if (count) *count = b->count;
    if (dtype) *dtype = b->dtype;
    return 0;
}

extern "C" void *gfhip_get_host_buffer(gfhip_context *ctx, uint64_t key, size_t *count) {
    if (!ctx) return nullptr;
    buffer *b = find_buffer(ctx, key);
    if (!b) return nullptr;
    if (enter(ctx)) return nullptr;
    const size_t bytes = b->count*element_bytes(b->dtype);
    if (!b->mirror) {
        if (ctx->check(allocate(b->mirror, bytes ? bytes : 8), "hipHostMalloc(mirror)") ||
            ctx->check(hipMemcpyAsync(b->mirror.get(), b->pointer, bytes, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync(mirror)") ||
            ctx->check(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
            return nullptr;
        }
    }
    if (count) *count = b->count;
    return b->mirror.get();
}

extern "C" int gfhip_set_buffer(gfhip_context *ctx, uint64_t key, void *device_pointer, size_t count, uint32_t dtype) {
    if (!ctx) return 1;
    if (enter(ctx)) return 1;
    if (!device_pointer && count) return ctx->fail("null device pointer");
    if (dtype > GFIR_C64) return ctx->fail("bad dtype");
    buffer &b = ctx->buffers[key];
    b = buffer();                                  // frees what an earlier buffer of this key owned
    b.pointer = device_pointer;
    b.count = count;
    b.dtype = dtype;
    return 0;
}

//  gfhip_hand_over: arrays from `from`'s buffers to `to`'s in one launch (hand_over.hip).  Everything is checked
//  before anything is queued; the failure is left in both contexts.
static int hand_over_fail(gfhip_context *to, gfhip_context *from, const std::string &message) {
    from->fail(message);
    return to->fail(message);
}

extern "C" int gfhip_hand_over(gfhip_context *to, gfhip_context *from, const struct gfhip_hand_over_entry *entries, size_t count) {
    if (!to || !from || (!entries && count)) {
        const char *message = "gfhip_hand_over: null argument";
        creation_error = message;
        if (to) to->fail(message);
        if (from) from->fail(message);
        return 1;
    }
    if (to->device != from->device) return hand_over_fail(to, from, "gfhip_hand_over: the contexts are on different devices");
    std::vector<gfhip::hand_over_slot> slots;
    slots.reserve(count);
    for (size_t e = 0; e < count; e++) {
        const gfhip_hand_over_entry &entry = entries[e];
        const std::string where = "gfhip_hand_over: entry " + std::to_string(e) + ": ";
        if (entry.reserved) return hand_over_fail(to, from, where + "reserved is not 0");
        const auto target = to->buffers.find(entry.to_key);
        const auto source = from->buffers.find(entry.from_key);
        if (target == to->buffers.end()) return hand_over_fail(to, from, where + "unknown destination key");
        if (source == from->buffers.end()) return hand_over_fail(to, from, where + "unknown source key");
        const buffer &t = target->second, &f = source->second;
        if (t.count != f.count) return hand_over_fail(to, from, where + "the buffers differ in element count");
        const bool t_wide = t.dtype == GFIR_F64 || t.dtype == GFIR_C64, f_wide = f.dtype == GFIR_F64 || f.dtype == GFIR_C64;
        const bool t_complex = t.dtype == GFIR_C32 || t.dtype == GFIR_C64, f_complex = f.dtype == GFIR_C32 || f.dtype == GFIR_C64;
        if (t_wide != f_wide) return hand_over_fail(to, from, where + "the buffers differ in precision");
        if (entry.part > 1) return hand_over_fail(to, from, where + "part is 0 (real) or 1 (imaginary)");
        if (entry.part && !(f_complex && !t_complex)) {
            return hand_over_fail(to, from, where + "part = 1 needs a complex source and a real destination");
        }
        gfhip::hand_over_slot slot = {t.pointer, f.pointer, f.count, 0, 0};
        slot.mode = (f_complex == t_complex ? gfhip::hand_over_copy : (t_complex ? gfhip::hand_over_widen : gfhip::hand_over_part))
                  | (f_wide ? gfhip::hand_over_wide : 0u) | (f_complex && t_complex ? gfhip::hand_over_complex : 0u)
                  | (entry.part ? gfhip::hand_over_imaginary : 0u);
        if (gfhip::hand_over_vector_ok(slot.mode, slot.to, slot.from)) slot.mode |= gfhip::hand_over_vector;
        if (slot.count) slots.push_back(slot);
    }
//  Both contexts settled: passes that ran ahead of their caller are not handed over, nor overwritten later.
    if (enter(to)) return hand_over_fail(to, from, std::string(to->error));
    if (enter(from)) return hand_over_fail(to, from, std::string(from->error));
    if (slots.empty()) return 0;
//  On the source's stream: behind the kernels that wrote the sources and before those that overwrite them.  Another
//  stream on the destination's side: what it has queued may still read the destinations, and what it queues next waits.
    const bool two_streams = to->stream != from->stream;
    if (two_streams) {
        for (event_ptr *event : {&to->hand_over_before, &to->hand_over_after}) {
            if (*event) continue;
            hipEvent_t made = nullptr;
            GFHIP_TRY(to, hipEventCreateWithFlags(&made, hipEventDisableTiming), "hipEventCreate");
            event->reset(made);
        }
        GFHIP_TRY(to, hipEventRecord(to->hand_over_before.get(), to->stream), "hipEventRecord");
        GFHIP_TRY(to, hipStreamWaitEvent(from->stream, to->hand_over_before.get(), 0), "hipStreamWaitEvent");
    }
    for (size_t first = 0; first < slots.size(); first += gfhip::hand_over_table_size) {
        gfhip::hand_over_table table = {};
        const unsigned int used = static_cast<unsigned int> (std::min<size_t> (slots.size() - first, gfhip::hand_over_table_size));
        std::copy(slots.begin() + first, slots.begin() + first + used, table.slot);
        gfhip::launch_hand_over(table, used, from->num_cus, from->stream);
        if (from->check(hipGetLastError(), "hand-over launch")) return hand_over_fail(to, from, std::string(from->error));
    }
    if (two_streams) {
        GFHIP_TRY(to, hipEventRecord(to->hand_over_after.get(), from->stream), "hipEventRecord");
        GFHIP_TRY(to, hipStreamWaitEvent(to->stream, to->hand_over_after.get(), 0), "hipStreamWaitEvent");
    }
    return 0;
}

extern "C" int gfhip_kernel_get_info(const gfhip_kernel *k, struct gfhip_kernel_info *info) {
    if (!k || !info) return 1;
    std::memset(info, 0, sizeof(*info));
    info->dtype = k->item.dtype;
    info->num_inputs = static_cast<uint32_t> (k->item.symbols.size());
    info->num_outputs = static_cast<uint32_t> (k->item.outputs.size());
    info->num_setters = static_cast<uint32_t> (k->item.setters.size());
    info->num_tables = static_cast<uint32_t> (k->item.tables.size());
    info->num_instructions = static_cast<uint32_t> (k->item.code.size());
    const built_piece &whole = k->whole;
    info->vgprs = static_cast<uint32_t> (whole.vgprs);
    size_t lds = whole.low.lds_bytes;
    for (auto &piece : k->pieces) lds = std::max(lds, piece.low.lds_bytes);
    info->lds_bytes = static_cast<uint32_t> (whole.lds_static + lds);
    info->segments = static_cast<uint32_t> (k->pieces.size());          // segments the item runs as (0: one kernel)
    info->converge_batch = whole.batch_function ? whole.low.batch : 0;
    info->level = k->level;
    info->scratch_bytes = static_cast<uint32_t> (whole.scratch);
    info->block_size = whole.low.block_size;
    info->grid_size = whole.grid;
    info->from_cache = whole.from_cache ? 1 : 0;
    info->source_hash = whole.low.hash;
    std::strncpy(info->name, whole.low.kernel_name.c_str(), sizeof(info->name) - 1);
    return 0;
}

extern "C" int gfhip_enable_timing(gfhip_context *ctx, int enable) {
    if (!ctx) return 1;
    ctx->timing = enable > 0 ? static_cast<unsigned int> (enable) : 0;
    return 0;
}

extern "C" int gfhip_kernel_timing(gfhip_kernel *k, double *average_ms, uint64_t *launches) {
    if (!k) return 1;
    gfhip_context *ctx = k->ctx;
    GFHIP_TRY(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    double total = 0.0;
    k->samples.clear();
    for (auto &e : k->events) {
        float ms = 0.0f;
        GFHIP_TRY(ctx, hipEventElapsedTime(&ms, e.start.get(), e.stop.get()), "hipEventElapsedTime");
        total += ms;
        k->samples.push_back(ms);
    }
    if (launches) *launches = k->events.size();
    if (average_ms) *average_ms = k->events.empty() ? 0.0 : total/static_cast<double> (k->events.size());
    for (auto &e : k->events) k->free_events.push_back(std::move(e));
    k->events.clear();
    return 0;
}

extern "C" int gfhip_kernel_timing_samples(gfhip_kernel *k, double *ms, size_t capacity, size_t *count) {
    if (!k) return 1;
    if (!k->events.empty() && gfhip_kernel_timing(k, nullptr, nullptr)) return 1;
    const size_t n = k->samples.size() < capacity ? k->samples.size() : capacity;
    if (ms && n) std::memcpy(ms, k->samples.data(), n*sizeof(double));
    if (count) *count = k->samples.size();
    return 0;
}

//  Stores of exact sums (cell_launch.hpp, superacc.hpp): what deposition grids and flux profiles share.
int exact_cells::create(gfhip_context *context, const size_t count) {
    ctx = context;
    cells = count;
    const size_t bytes = cells*gfhip::superacc::limbs*sizeof(int64_t);
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

//  `count` deposits, `launch(first, piece)` enqueueing those of the samples first .. first + piece: at most 2^30
//  between two normalisations (superacc.hpp); a workgroup-private limb sees fewer than its launch.
template<typename LAUNCH>
int exact_cells::add(const size_t count, LAUNCH launch) {
    if (enter(ctx)) return 1;
    for (size_t first = 0; first < count;) {
        const size_t piece = std::min<size_t> (count - first, gfhip::superacc::deposits_per_normalise);
        if (pending + piece > gfhip::superacc::deposits_per_normalise && normalise()) return 1;
        launch(first, piece);
        GFHIP_TRY(ctx, hipGetLastError(), "deposit launch");
        pending += piece;
        first += piece;
    }
    return 0;
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
    GFHIP_TRY(ctx, hipMemcpyAsync(limbs, state.get(), cells*gfhip::superacc::limbs*sizeof(int64_t), hipMemcpyDeviceToHost,
                                  ctx->stream), "hipMemcpyAsync(cells)");
    GFHIP_TRY(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return 0;
}

int exact_cells::merge(const int64_t *limbs, const uint64_t samples, const uint64_t outside, const uint64_t skipped) {
    if (enter(ctx)) return 1;
    const size_t words = cells*gfhip::superacc::limbs;
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

//  Whether the n + 1 edges of an axis are finite and strictly increasing.
static bool edges_increase(const double *edges, const size_t n) {
    for (size_t i = 0; i <= n; i++) {
        if (!std::isfinite(edges[i]) || (i && !(edges[i - 1] < edges[i]))) return false;
    }
    return true;
}

//  N fp64 buffers of at least `count` elements, or the message about `noun`; nothing is enqueued.
template<size_t N>
static int fp64_columns(gfhip_context *ctx, const char *noun, const uint64_t (&keys)[N], const size_t count, double **columns) {
    for (size_t c = 0; c < N; c++) {
        const buffer *found = find_buffer(ctx, keys[c]);
        if (!found) return 1;
        if (found->dtype != GFIR_F64) return ctx->fail(std::string(noun) + " takes fp64 buffers");
        if (found->count < count) return ctx->fail(std::string(noun) + " buffer is shorter than the sample count");
        columns[c] = static_cast<double *> (found->pointer);
    }
    return 0;
}

//  gfhip_*_destroy: behind everything the context has queued, out of the context's list.
template<typename T>
static void destroy_in(std::vector<std::unique_ptr<T>> gfhip_context::*list, T *object) {
    if (!object) return;
    gfhip_context *ctx = object->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    auto &owned = ctx->*list;
    for (auto it = owned.begin(); it != owned.end(); ++it) {
        if (it->get() == object) {
            owned.erase(it);
            return;
        }
    }
}

//  Deposition grids (deposition.hip).  The limits of a grid: at most 2047 cells per axis, so that the
//  three axes' edges (3 x 2048 doubles, 48 KiB) fit the LDS a workgroup gets without asking; at most 2^25 cells
//  (536 B each: 16.8 GiB of state), so that cell*64 + limb fits the 32-bit key the deposit kernel compares.
static const size_t bins_axis_limit = 2047, bins_cell_limit = static_cast<size_t> (1) << 25;

extern "C" gfhip_bins *gfhip_bins_create(gfhip_context *ctx, const double *xedges, size_t nx,
                                         const double *yedges, size_t ny, const double *zedges, size_t nz) {
    if (!ctx) return nullptr;
    const double *axes[3] = {xedges, yedges, zedges};
    const size_t n[3] = {nx, ny, nz};
    std::vector<double> edges;
    size_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (!axes[a] || n[a] < 1 || n[a] > bins_axis_limit) {
            ctx->fail("a deposition grid has 1 to 2047 cells per axis");
            return nullptr;
        }
        if (!edges_increase(axes[a], n[a])) {
            ctx->fail("the edges of a deposition grid must be finite and strictly increasing");
            return nullptr;
        }
        edges.insert(edges.end(), axes[a], axes[a] + n[a] + 1);
        cells *= n[a];
    }
    if (cells > bins_cell_limit) {
        ctx->fail("a deposition grid has at most 2^25 cells (536 B each)");
        return nullptr;
    }
    if (ctx->check(hipSetDevice(ctx->device), "hipSetDevice")) return nullptr;
    std::unique_ptr<gfhip_bins> b(new gfhip_bins);
    for (int a = 0; a < 3; a++) {
        b->n[a] = static_cast<int> (n[a]);
        b->scale[a] = static_cast<double> (n[a])/(axes[a][n[a]] - axes[a][0]);
    }
    if (ctx->check(allocate(b->edges, edges.size()*sizeof(double)), "hipMalloc(edges)") ||
        ctx->check(hipMemcpy(b->edges.get(), edges.data(), edges.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(edges)") ||
        b->create(ctx, cells)) {
        return nullptr;
    }
    ctx->bins.push_back(std::move(b));
    return ctx->bins.back().get();
}

extern "C" void gfhip_bins_destroy(gfhip_bins *b) {
    destroy_in(&gfhip_context::bins, b);
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
    return b ? b->counts(samples, outside, skipped) : 1;
}

extern "C" int gfhip_bins_state(gfhip_bins *b, int64_t *limbs) {
    if (!b) return 1;
    if (!limbs) return b->ctx->fail("gfhip_bins_state needs a destination");
    return b->state_to(limbs);
}

extern "C" int gfhip_bins_merge(gfhip_bins *b, const int64_t *limbs, uint64_t samples, uint64_t outside, uint64_t skipped) {
    if (!b) return 1;
    if (!limbs) return b->ctx->fail("gfhip_bins_merge needs a state");
    return b->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_bins_read(gfhip_bins *b, double divisor, double *bins) {
    if (!b) return 1;
    if (!bins) return b->ctx->fail("gfhip_bins_read needs a destination");
    return b->read(divisor, bins);
}

//  Flux profiles (flux_profile.hip, flux_label.hpp).  At most 4096 cells: the edges are staged in LDS on both paths.
static const size_t flux_cell_limit = 4096;

//  The scalars of a caller's map, or why it is refused.
static const char *flux_map_of(const gfhip_flux_map *given, gfhip::flux::map &m) {
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
    if (given->flags & ~gfhip::flux::known_flags) return "unknown flag bits in a flux map";
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

//  The 16 psi tables as [table cell][16]: a lane's coefficients are one 128-byte line.  False: no memory.
static bool psi_lines(const gfhip_flux_map *given, std::vector<double> &lines) {
    const size_t table = static_cast<size_t> (given->numr*given->numz);
    try {
        lines.resize(table*16);
    } catch (const std::bad_alloc &) {
        return false;
    }
    for (size_t k = 0; k < 16; k++) {
        const double *from = given->coefficients + k*table;
        for (size_t at = 0; at < table; at++) lines[at*16 + k] = from[at];
    }
    return true;
}

//  The map checked and copied, its tables repacked to [table cell][16] (a lane's coefficients are one 128-byte line) and
//  uploaded with the edges, the launch shape decided and the `count` cells allocated.  prepare: the deposit kernels'
//  request for large dynamic LDS, made when the private path is taken.
//  batch_count: 0, or the batches of rays a batched object keeps `count` cells each for.
int flux_cells::create(gfhip_context *context, const gfhip_flux_map *given, const size_t count,
                       const std::vector<double> &all_edges, hipError_t (*prepare)(), const size_t batch_count) {
    if (const char *refused = flux_map_of(given, map)) return context->fail(refused);
    if (context->check(hipSetDevice(context->device), "hipSetDevice")) return 1;
    batches = batch_count;
    slab = count;
    gfhip::flux_launch_shape(count, all_edges.size(), !(given->flags & gfhip::flux::flag_no_private_sums), context->num_cus,
                             &is_private, &cap, &block, &max_workgroups, &lds_bytes);
    std::vector<double> lines;
    if (!psi_lines(given, lines)) return context->fail("a flux map's tables do not fit the host's memory");
    return context->check(allocate(packed, lines.size()*sizeof(double)), "hipMalloc(flux tables)") ||
           context->check(hipMemcpy(packed.get(), lines.data(), lines.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(flux tables)") ||
           context->check(allocate(edges, all_edges.size()*sizeof(double)), "hipMalloc(edges)") ||
           context->check(hipMemcpy(edges.get(), all_edges.data(), all_edges.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(edges)") ||
           exact_cells::create(context, batch_count ? batch_count*count : count) ||
           (is_private && context->check(prepare(), "hipFuncSetAttribute(flux deposit)"));
}

//  The batches of a batched object, or why they are refused: 1 to 256, and at most 2^20 cells in all.
static const char *batches_refused(const size_t batch_count, const size_t count) {
    if (batch_count < 1 || batch_count > gfhip::batches::max_batches) return "a batched object has 1 to 256 batches";
    if (batch_count*count > (static_cast<size_t> (1) << 20)) return "batches x cells is at most 2^20 (536 B each)";
    return nullptr;
}

//  Why an add with a ray index is refused: only a batched object takes one, and first_ray + count fits 64 bits.
const char *flux_cells::rays_refused(const uint64_t first_ray, const size_t count) const {
    if (!batches) return "only a batched object (gfhip_flux_create_batched, gfhip_spectrum_create_batched) takes samples with a ray index";
    if (first_ray + static_cast<uint64_t> (count) < first_ray) return "first_ray + count overflows 64 bits";
    return nullptr;
}

//  The same for an add with a particle index (distributions and moment profiles).
const char *flux_cells::particles_refused(const uint64_t first_particle, const size_t count) const {
    if (!batches) return "only a batched object (gfhip_phase_create_batched, gfhip_moments_create_batched) takes particles with their index";
    if (first_particle + static_cast<uint64_t> (count) < first_particle) return "first_particle + count overflows 64 bits";
    return nullptr;
}

void flux_cells::info_to(struct gfhip_flux_info *info) const {
    info->private_sums = is_private ? 1u : 0u;
    info->workgroup_size = block;
    info->cap_cells = cap;
    info->max_workgroups = max_workgroups;
    info->lds_bytes = lds_bytes;
}

//  batch_count: 0 for gfhip_flux_create.
static gfhip_flux *flux_create(gfhip_context *ctx, const gfhip_flux_map *map, const double *edges, const size_t cells,
                               const size_t batch_count) {
    if (!map || !edges) {
        ctx->fail("a flux profile needs a map and edges");
        return nullptr;
    }
    if (cells < 1 || cells > flux_cell_limit) {
        ctx->fail("a flux profile has 1 to 4096 cells");
        return nullptr;
    }
    if (!edges_increase(edges, cells)) {
        ctx->fail("the edges of a flux profile must be finite and strictly increasing");
        return nullptr;
    }
    std::unique_ptr<gfhip_flux> f(new gfhip_flux);
    f->scale = static_cast<double> (cells)/(edges[cells] - edges[0]);
    if (f->create(ctx, map, cells, std::vector<double> (edges, edges + cells + 1), gfhip::flux_prepare, batch_count)) return nullptr;
    ctx->fluxes.push_back(std::move(f));
    return ctx->fluxes.back().get();
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
    destroy_in(&gfhip_context::fluxes, f);
}

extern "C" int gfhip_flux_add(gfhip_flux *f, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t value_key, size_t count) {
    if (!f) return 1;
    if (f->batches) return f->ctx->fail("a batched flux profile takes its samples with their ray index: gfhip_flux_add_rays");
    double *columns[4];
    if (fp64_columns(f->ctx, "a flux profile", {x_key, y_key, z_key, value_key}, count, columns)) return 1;
    return f->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_flux_deposit(columns[0] + first, columns[1] + first, columns[2] + first, columns[3] + first, piece,
                                   f->map, f->packed.get(), f->edges.get(), f->cells, f->scale, f->is_private, f->block,
                                   f->max_workgroups, f->lds_bytes, f->state.get(), f->counters.get(), f->ctx->stream);
    });
}

extern "C" int gfhip_flux_add_rays(gfhip_flux *f, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t value_key, size_t count,
                                   uint64_t first_ray) {
    if (!f) return 1;
    if (const char *refused = f->rays_refused(first_ray, count)) return f->ctx->fail(refused);
    double *columns[4];
    if (fp64_columns(f->ctx, "a flux profile", {x_key, y_key, z_key, value_key}, count, columns)) return 1;
    return f->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_flux_deposit_rays(columns[0] + first, columns[1] + first, columns[2] + first, columns[3] + first, piece,
                                        first_ray + first, f->batches, f->map, f->packed.get(), f->edges.get(), f->slab,
                                        f->scale, f->is_private, f->block, f->max_workgroups, f->lds_bytes, f->state.get(),
                                        f->counters.get(), f->ctx->stream);
    });
}

extern "C" int gfhip_flux_label(gfhip_flux *f, uint64_t x_key, uint64_t y_key, uint64_t z_key, uint64_t label_key, size_t count) {
    if (!f) return 1;
    gfhip_context *ctx = f->ctx;
    double *columns[4];
    if (fp64_columns(ctx, "a flux profile", {x_key, y_key, z_key, label_key}, count, columns)) return 1;
    if (enter(ctx)) return 1;
    gfhip::launch_flux_label(columns[0], columns[1], columns[2], count, f->map, f->packed.get(), columns[3], ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "flux label launch");
    return 0;
}

extern "C" int gfhip_flux_counts(gfhip_flux *f, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return f ? f->counts(samples, outside, skipped) : 1;
}

extern "C" int gfhip_flux_state(gfhip_flux *f, int64_t *limbs) {
    if (!f) return 1;
    if (!limbs) return f->ctx->fail("gfhip_flux_state needs a destination");
    return f->state_to(limbs);
}

extern "C" int gfhip_flux_merge(gfhip_flux *f, const int64_t *limbs, size_t cells, uint64_t samples, uint64_t outside, uint64_t skipped) {
    if (!f) return 1;
    if (!limbs) return f->ctx->fail("gfhip_flux_merge needs a state");
    if (f->batches || cells != f->cells) return f->ctx->fail("merge: a flux profile of another shape");
    return f->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_flux_merge_batches(gfhip_flux *f, const int64_t *limbs, size_t batches, size_t cells, uint64_t samples,
                                        uint64_t outside, uint64_t skipped) {
    if (!f) return 1;
    if (!limbs) return f->ctx->fail("gfhip_flux_merge_batches needs a state");
    if (!f->batches || batches != f->batches || cells != f->slab) return f->ctx->fail("merge: a flux profile of another shape");
    return f->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_flux_read(gfhip_flux *f, double divisor, double *values) {
    if (!f) return 1;
    if (!values) return f->ctx->fail("gfhip_flux_read needs a destination");
    return f->read(divisor, values);
}

//  Not through enter(): it reads what gfhip_flux_create decided on the host and touches neither the device nor the stream.
extern "C" int gfhip_flux_info(gfhip_flux *f, struct gfhip_flux_info *info) {
    if (!f) return 1;
    if (!info) return f->ctx->fail("gfhip_flux_info needs a destination");
    f->info_to(info);
    return 0;
}

//  Host side, no device: flux_label.hpp on the caller's 16 tables.
extern "C" int gfhip_flux_label_host(const gfhip_flux_map *map, const double *x, const double *y, const double *z,
                                     size_t count, double *label) {
    if (!map || ((!x || !y || !z || !label) && count)) {
        creation_error = "gfhip_flux_label_host needs a map, three coordinate arrays and a destination";
        return 1;
    }
    gfhip::flux::map m;
    if (const char *refused = flux_map_of(map, m)) {
        creation_error = refused;
        return 1;
    }
    const size_t table = static_cast<size_t> (map->numr*map->numz);
    for (size_t s = 0; s < count; s++) {
        double tr, tz, c[16];
        const long long at = gfhip::flux::locate(m, x[s], y[s], z[s], tr, tz);
        if (at < 0) {
            label[s] = std::numeric_limits<double>::quiet_NaN();
            continue;
        }
        for (size_t k = 0; k < 16; k++) c[k] = map->coefficients[k*table + static_cast<size_t> (at)];
        label[s] = gfhip::flux::label_of(m, gfhip::flux::psi_of(c, tr, tz));
    }
    return 0;
}

//  Spectra over the flux label and N (flux_spectrum.hip, flux_label.hpp).  At most 4096 cells per axis and 2^16 in all
//  (536 B each: 35 MB of state); the two axes' edges are staged in LDS on both paths.
static const size_t spectrum_cell_limit = static_cast<size_t> (1) << 16;

//  The scalars of a caller's field, or why it is refused.
static const char *spectrum_field_of(const gfhip_spectrum_field *given, gfhip::flux::field &f) {
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

//  The four fpol tables as [interval][4]: a lane's coefficients are one 32-byte line.  False: no memory.
static bool fpol_lines(const gfhip_spectrum_field *field, std::vector<double> &lines) {
    try {
        lines.resize(static_cast<size_t> (field->numpsi)*4);
    } catch (const std::bad_alloc &) {
        return false;
    }
    for (size_t k = 0; k < 4; k++) {
        for (size_t q = 0; q < field->numpsi; q++) lines[q*4 + k] = field->fpol[k][q];
    }
    return true;
}

//  batch_count: 0 for gfhip_spectrum_create.
static gfhip_spectrum *spectrum_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                       const double *sedges, const size_t ns, const double *nedges, const size_t nn,
                                       const size_t batch_count) {
    if (!map || !field || !sedges || !nedges) {
        ctx->fail("a spectrum needs a map, a field and two edge arrays");
        return nullptr;
    }
    if (ns < 1 || ns > flux_cell_limit || nn < 1 || nn > flux_cell_limit) {
        ctx->fail("a spectrum has 1 to 4096 cells per axis");
        return nullptr;
    }
    if (ns*nn > spectrum_cell_limit) {
        ctx->fail("a spectrum has at most 65536 cells (536 B each)");
        return nullptr;
    }
    if (!edges_increase(sedges, ns) || !edges_increase(nedges, nn)) {
        ctx->fail("the edges of a spectrum must be finite and strictly increasing");
        return nullptr;
    }
    std::unique_ptr<gfhip_spectrum> s(new gfhip_spectrum);
    if (const char *refused = spectrum_field_of(field, s->field)) {
        ctx->fail(refused);
        return nullptr;
    }
    s->ns = ns;
    s->nn = nn;
    s->sscale = static_cast<double> (ns)/(sedges[ns] - sedges[0]);
    s->nscale = static_cast<double> (nn)/(nedges[nn] - nedges[0]);
    std::vector<double> edges(sedges, sedges + ns + 1);
    edges.insert(edges.end(), nedges, nedges + nn + 1);
    std::vector<double> lines;
    if (!fpol_lines(field, lines)) {
        ctx->fail("a spectrum's fpol tables do not fit the host's memory");
        return nullptr;
    }
    if (s->create(ctx, map, ns*nn, edges, gfhip::spectrum_prepare, batch_count) ||
        ctx->check(allocate(s->fpol, lines.size()*sizeof(double)), "hipMalloc(fpol tables)") ||
        ctx->check(hipMemcpy(s->fpol.get(), lines.data(), lines.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(fpol tables)")) {
        return nullptr;
    }
    ctx->spectra.push_back(std::move(s));
    return ctx->spectra.back().get();
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
    destroy_in(&gfhip_context::spectra, s);
}

extern "C" int gfhip_spectrum_add(gfhip_spectrum *s, const uint64_t keys[8], size_t count) {
    if (!s) return 1;
    if (!keys) return s->ctx->fail("gfhip_spectrum_add needs its 8 keys");
    if (s->batches) return s->ctx->fail("a batched spectrum takes its samples with their ray index: gfhip_spectrum_add_rays");
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], keys[7]};
    double *columns[8];
    if (fp64_columns(s->ctx, "a spectrum", all, count, columns)) return 1;
    return s->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_spectrum_deposit(columns, first, piece, s->map, s->field, s->packed.get(), s->fpol.get(), s->edges.get(),
                                       s->ns, s->nn, s->sscale, s->nscale, s->is_private, s->block, s->max_workgroups,
                                       s->lds_bytes, s->state.get(), s->counters.get(), s->ctx->stream);
    });
}

extern "C" int gfhip_spectrum_add_rays(gfhip_spectrum *s, const uint64_t keys[8], size_t count, uint64_t first_ray) {
    if (!s) return 1;
    if (!keys) return s->ctx->fail("gfhip_spectrum_add_rays needs its 8 keys");
    if (const char *refused = s->rays_refused(first_ray, count)) return s->ctx->fail(refused);
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], keys[7]};
    double *columns[8];
    if (fp64_columns(s->ctx, "a spectrum", all, count, columns)) return 1;
    return s->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_spectrum_deposit_rays(columns, first, piece, first_ray + first, s->batches, s->map, s->field,
                                            s->packed.get(), s->fpol.get(), s->edges.get(), s->ns, s->nn, s->sscale, s->nscale,
                                            s->is_private, s->block, s->max_workgroups, s->lds_bytes, s->state.get(),
                                            s->counters.get(), s->ctx->stream);
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
    gfhip::launch_spectrum_npar(columns, count, s->map, s->field, s->packed.get(), s->fpol.get(), columns[7], columns[8], ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "spectrum npar launch");
    return 0;
}

extern "C" int gfhip_spectrum_counts(gfhip_spectrum *s, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return s ? s->counts(samples, outside, skipped) : 1;
}

extern "C" int gfhip_spectrum_state(gfhip_spectrum *s, int64_t *limbs) {
    if (!s) return 1;
    if (!limbs) return s->ctx->fail("gfhip_spectrum_state needs a destination");
    return s->state_to(limbs);
}

extern "C" int gfhip_spectrum_merge(gfhip_spectrum *s, const int64_t *limbs, size_t ns, size_t nn, uint64_t samples, uint64_t outside,
                                    uint64_t skipped) {
    if (!s) return 1;
    if (!limbs) return s->ctx->fail("gfhip_spectrum_merge needs a state");
    if (s->batches || ns != s->ns || nn != s->nn) return s->ctx->fail("merge: a spectrum of another shape");
    return s->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_spectrum_merge_batches(gfhip_spectrum *s, const int64_t *limbs, size_t batches, size_t ns, size_t nn,
                                            uint64_t samples, uint64_t outside, uint64_t skipped) {
    if (!s) return 1;
    if (!limbs) return s->ctx->fail("gfhip_spectrum_merge_batches needs a state");
    if (!s->batches || batches != s->batches || ns != s->ns || nn != s->nn) return s->ctx->fail("merge: a spectrum of another shape");
    return s->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_spectrum_read(gfhip_spectrum *s, double divisor, double *values) {
    if (!s) return 1;
    if (!values) return s->ctx->fail("gfhip_spectrum_read needs a destination");
    return s->read(divisor, values);
}

//  Not through enter(): as gfhip_flux_info.
extern "C" int gfhip_spectrum_info(gfhip_spectrum *s, struct gfhip_flux_info *info) {
    if (!s) return 1;
    if (!info) return s->ctx->fail("gfhip_spectrum_info needs a destination");
    s->info_to(info);
    return 0;
}

//  Host side, no device: flux_label.hpp on the caller's 16 + 4 tables.
extern "C" int gfhip_spectrum_npar_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *const columns[7],
                                        size_t count, double *label, double *npar) {
    if (!map || !field || !columns || ((!label || !npar) && count)) {
        creation_error = "gfhip_spectrum_npar_host needs a map, a field, seven columns and two destinations";
        return 1;
    }
    for (int k = 0; k < 7; k++) {
        if (!columns[k] && count) {
            creation_error = "gfhip_spectrum_npar_host needs a map, a field, seven columns and two destinations";
            return 1;
        }
    }
    gfhip::flux::map m;
    gfhip::flux::field f;
    const char *refused = flux_map_of(map, m);
    if (!refused) refused = spectrum_field_of(field, f);
    if (refused) {
        creation_error = refused;
        return 1;
    }
    const size_t table = static_cast<size_t> (map->numr*map->numz);
    for (size_t s = 0; s < count; s++) {
        const double x = columns[0][s], y = columns[1][s];
        double tr, tz, tp, gr, gz, c[16], cubic[4];
        const long long at = gfhip::flux::locate(m, x, y, columns[2][s], tr, tz);
        if (at < 0) {
            label[s] = npar[s] = std::numeric_limits<double>::quiet_NaN();
            continue;
        }
        for (size_t k = 0; k < 16; k++) c[k] = map->coefficients[k*table + static_cast<size_t> (at)];
        const double psi = gfhip::flux::psi_gradient(m, c, tr, tz, gr, gz);
        label[s] = gfhip::flux::canonical(gfhip::flux::label_of(m, psi));
        const int q = gfhip::flux::fpol_interval(f, psi, tp);
        for (size_t k = 0; k < 4; k++) cubic[k] = field->fpol[k][q];
        npar[s] = gfhip::flux::npar_of(f, x, y, gfhip::flux::radius_of(x, y), columns[3][s], columns[4][s], columns[5][s],
                                       columns[6][s], gr, gz, gfhip::flux::fpol_of(cubic, tp));
    }
    return 0;
}

//  Distributions of particles over the flux label, the pitch cosine and gamma (phase_bins.hip, flux_label.hpp).  At most
//  4096 cells per axis and 2^20 in all (536 B each: 563 MB of state); the three axes' edges are staged in LDS on both
//  paths.
static const size_t phase_cell_limit = static_cast<size_t> (1) << 20;

//  The scalars of a distribution's field: a spectrum's, whose c takes no part here.
static const char *phase_field_of(const gfhip_spectrum_field *given, gfhip::flux::field &f) {
    gfhip_spectrum_field without_c = *given;
    without_c.c = 1.0;
    return spectrum_field_of(&without_c, f);
}

//  The label and the pitch cosine of one particle from the caller's 16 + 4 tables, both NaN outside the map.
static void phase_point(const gfhip::flux::map &m, const gfhip::flux::field &f, const gfhip_flux_map *map,
                        const gfhip_spectrum_field *field, const double x, const double y, const double z, const double ux,
                        const double uy, const double uz, double &label, double &pitch) {
    const size_t table = static_cast<size_t> (map->numr*map->numz);
    double tr, tz, tp, gr, gz, c[16], cubic[4];
    const long long at = gfhip::flux::locate(m, x, y, z, tr, tz);
    if (at < 0) {
        label = pitch = std::numeric_limits<double>::quiet_NaN();
        return;
    }
    for (size_t k = 0; k < 16; k++) c[k] = map->coefficients[k*table + static_cast<size_t> (at)];
    const double psi = gfhip::flux::psi_gradient(m, c, tr, tz, gr, gz);
    label = gfhip::flux::canonical(gfhip::flux::label_of(m, psi));
    const int q = gfhip::flux::fpol_interval(f, psi, tp);
    for (size_t k = 0; k < 4; k++) cubic[k] = field->fpol[k][q];
    pitch = gfhip::flux::pitch_of(x, y, gfhip::flux::radius_of(x, y), ux, uy, uz, gr, gz, gfhip::flux::fpol_of(cubic, tp));
}

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
    std::vector<double> edges;
    size_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (n[a] < 1 || n[a] > flux_cell_limit) {
            ctx->fail("a distribution has 1 to 4096 cells per axis (at least two edges)");
            return nullptr;
        }
        if (!edges_increase(axes[a], n[a])) {
            ctx->fail("the edges of a distribution must be finite and strictly increasing");
            return nullptr;
        }
        edges.insert(edges.end(), axes[a], axes[a] + n[a] + 1);
        cells *= n[a];                                 // at most 2^36
    }
    if (cells > phase_cell_limit) {
        ctx->fail("a distribution has at most 2^20 cells (536 B each)");
        return nullptr;
    }
    if (const char *refused = batched ? batches_refused(batch_count, cells) : nullptr) {
        ctx->fail(refused);
        return nullptr;
    }
    std::unique_ptr<gfhip_phase> p(new gfhip_phase);
    if (const char *refused = phase_field_of(field, p->field)) {
        ctx->fail(refused);
        return nullptr;
    }
    for (int a = 0; a < 3; a++) {
        p->n[a] = n[a];
        p->scale[a] = static_cast<double> (n[a])/(axes[a][n[a]] - axes[a][0]);
    }
    std::vector<double> lines;
    if (!fpol_lines(field, lines)) {
        ctx->fail("a distribution's fpol tables do not fit the host's memory");
        return nullptr;
    }
    if (p->create(ctx, map, cells, edges, gfhip::phase_prepare, batch_count) ||
        ctx->check(allocate(p->fpol, lines.size()*sizeof(double)), "hipMalloc(fpol tables)") ||
        ctx->check(hipMemcpy(p->fpol.get(), lines.data(), lines.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(fpol tables)")) {
        return nullptr;
    }
    ctx->phases.push_back(std::move(p));
    return ctx->phases.back().get();
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
    destroy_in(&gfhip_context::phases, p);
}

//  `used` real buffers of ONE type, fp32 or fp64, of at least `count` elements, or the message; nothing is enqueued.
static int particle_columns(gfhip_context *ctx, const uint64_t *keys, const size_t used, const size_t count,
                            const void **columns, bool &is_f32, const char *noun = "a distribution") {
    uint32_t dtype = 0;
    for (size_t c = 0; c < used; c++) {
        const buffer *found = find_buffer(ctx, keys[c]);
        if (!found) return 1;
        if (found->dtype != GFIR_F64 && found->dtype != GFIR_F32) return ctx->fail(std::string(noun) + " takes fp32 or fp64 buffers");
        if (c && found->dtype != dtype) return ctx->fail(std::string(noun) + " takes buffers of one type, all fp32 or all fp64");
        if (found->count < count) return ctx->fail(std::string(noun) + " buffer is shorter than the particle count");
        dtype = found->dtype;
        columns[c] = found->pointer;
    }
    is_f32 = dtype == GFIR_F32;
    return 0;
}

extern "C" int gfhip_phase_add(gfhip_phase *p, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count) {
    if (!p) return 1;
    if (!keys) return p->ctx->fail("gfhip_phase_add needs its 7 keys");
    if (p->batches) return p->ctx->fail("a batched distribution takes its particles with their index: gfhip_phase_add_particles");
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], weight_key};
    const void *columns[8] = {};
    bool is_f32 = false;
    if (particle_columns(p->ctx, all, has_weight ? 8 : 7, count, columns, is_f32)) return 1;
    return p->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_phase_deposit(columns, is_f32, first, piece, p->map, p->field, p->packed.get(), p->fpol.get(),
                                    p->edges.get(), p->n, p->scale, p->is_private, p->block, p->max_workgroups, p->lds_bytes,
                                    p->state.get(), p->counters.get(), p->ctx->stream);
    });
}

extern "C" int gfhip_phase_add_particles(gfhip_phase *p, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count,
                                         uint64_t first_particle) {
    if (!p) return 1;
    if (!keys) return p->ctx->fail("gfhip_phase_add_particles needs its 7 keys");
    if (const char *refused = p->particles_refused(first_particle, count)) return p->ctx->fail(refused);
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], weight_key};
    const void *columns[8] = {};
    bool is_f32 = false;
    if (particle_columns(p->ctx, all, has_weight ? 8 : 7, count, columns, is_f32)) return 1;
    return p->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_phase_deposit_particles(columns, is_f32, first, piece, first_particle + first, p->batches, p->map, p->field,
                                              p->packed.get(), p->fpol.get(), p->edges.get(), p->n, p->scale, p->is_private,
                                              p->block, p->max_workgroups, p->lds_bytes, p->state.get(), p->counters.get(),
                                              p->ctx->stream);
    });
}

extern "C" int gfhip_phase_coordinates(gfhip_phase *p, const uint64_t keys[7], uint64_t label_key, uint64_t pitch_key, size_t count) {
    if (!p) return 1;
    gfhip_context *ctx = p->ctx;
    if (!keys) return ctx->fail("gfhip_phase_coordinates needs its 7 keys");
    const void *columns[8] = {};
    bool is_f32 = false;
    if (particle_columns(ctx, keys, 7, count, columns, is_f32)) return 1;
    double *out[2];
    if (fp64_columns(ctx, "a distribution's label and pitch", {label_key, pitch_key}, count, out)) return 1;
    if (enter(ctx)) return 1;
    gfhip::launch_phase_coordinates(columns, is_f32, count, p->map, p->field, p->packed.get(), p->fpol.get(), out[0], out[1],
                                    ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "phase coordinates launch");
    return 0;
}

extern "C" int gfhip_phase_counts(gfhip_phase *p, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return p ? p->counts(samples, outside, skipped) : 1;
}

extern "C" int gfhip_phase_state(gfhip_phase *p, int64_t *limbs) {
    if (!p) return 1;
    if (!limbs) return p->ctx->fail("gfhip_phase_state needs a destination");
    return p->state_to(limbs);
}

extern "C" int gfhip_phase_merge(gfhip_phase *p, const int64_t *limbs, size_t ns, size_t np, size_t ng, uint64_t samples,
                                 uint64_t outside, uint64_t skipped) {
    if (!p) return 1;
    if (!limbs) return p->ctx->fail("gfhip_phase_merge needs a state");
    if (p->batches || ns != p->n[0] || np != p->n[1] || ng != p->n[2]) return p->ctx->fail("merge: a distribution of another shape");
    return p->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_phase_merge_batches(gfhip_phase *p, const int64_t *limbs, size_t batches, size_t ns, size_t np, size_t ng,
                                         uint64_t samples, uint64_t outside, uint64_t skipped) {
    if (!p) return 1;
    if (!limbs) return p->ctx->fail("gfhip_phase_merge_batches needs a state");
    if (!p->batches || batches != p->batches || ns != p->n[0] || np != p->n[1] || ng != p->n[2]) {
        return p->ctx->fail("merge: a distribution of another shape");
    }
    return p->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_phase_read(gfhip_phase *p, double divisor, double *values) {
    if (!p) return 1;
    if (!values) return p->ctx->fail("gfhip_phase_read needs a destination");
    return p->read(divisor, values);
}

//  Not through enter(): as gfhip_flux_info.
extern "C" int gfhip_phase_info(gfhip_phase *p, struct gfhip_flux_info *info) {
    if (!p) return 1;
    if (!info) return p->ctx->fail("gfhip_phase_info needs a destination");
    p->info_to(info);
    return 0;
}

//  Host side, no device: flux_label.hpp on the caller's 16 + 4 tables.
extern "C" int gfhip_phase_coordinates_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                            const void *const columns[7], int is_f32, size_t count, double *label, double *pitch) {
    bool complete = map && field && columns && ((label && pitch) || !count);
    for (int k = 0; complete && k < 7; k++) complete = columns[k] || !count;
    if (!complete) {
        creation_error = "gfhip_phase_coordinates_host needs a map, a field, seven columns and two destinations";
        return 1;
    }
    gfhip::flux::map m;
    gfhip::flux::field f;
    const char *refused = flux_map_of(map, m);
    if (!refused) refused = phase_field_of(field, f);
    if (refused) {
        creation_error = refused;
        return 1;
    }
    for (size_t s = 0; s < count; s++) {
        double v[6];
        for (int k = 0; k < 6; k++) {
            v[k] = is_f32 ? static_cast<double> (static_cast<const float *> (columns[k])[s]) : static_cast<const double *> (columns[k])[s];
        }
        phase_point(m, f, map, field, v[0], v[1], v[2], v[3], v[4], v[5], label[s], pitch[s]);
    }
    return 0;
}

//  Moment profiles (moment_bins.hip, flux_label.hpp): four cells per flux surface.  The surfaces are an axis of a
//  distribution, 1 to 4096 (their edges are staged in LDS on both paths), so the 2^20 cells are never reached by an
//  accepted axis; the check stands first for callers that ask for more.
static const size_t moment_count = gfhip::moments::count;

//  The label axis checked, or why it is refused.
static const char *moments_axis_of(const double *sedges, const size_t ns) {
    if (ns > phase_cell_limit/moment_count) return "a moment profile has at most 2^20 cells (four per surface, 536 B each)";
    if (ns < 1 || ns > flux_cell_limit) return "a moment profile has 1 to 4096 surfaces (at least two edges)";
    if (!edges_increase(sedges, ns)) return "the edges of a moment profile must be finite and strictly increasing";
    return nullptr;
}

//  batch_count: 0 for gfhip_moments_create.
static gfhip_moments *moments_create(gfhip_context *ctx, const gfhip_flux_map *map, const gfhip_spectrum_field *field,
                                     const double *sedges, size_t ns, const size_t batch_count, const bool batched) {
    if (!map || !field || !sedges) {
        ctx->fail("a moment profile needs a map, a field and the label edges");
        return nullptr;
    }
    if (const char *refused = moments_axis_of(sedges, ns)) {
        ctx->fail(refused);
        return nullptr;
    }
    if (const char *refused = batched ? batches_refused(batch_count, ns*moment_count) : nullptr) {
        ctx->fail(refused);
        return nullptr;
    }
    std::unique_ptr<gfhip_moments> p(new gfhip_moments);
    if (const char *refused = phase_field_of(field, p->field)) {
        ctx->fail(refused);
        return nullptr;
    }
    p->ns = ns;
    p->sscale = static_cast<double> (ns)/(sedges[ns] - sedges[0]);
    std::vector<double> lines;
    if (!fpol_lines(field, lines)) {
        ctx->fail("a moment profile's fpol tables do not fit the host's memory");
        return nullptr;
    }
    if (p->create(ctx, map, ns*moment_count, std::vector<double> (sedges, sedges + ns + 1), gfhip::moments_prepare, batch_count) ||
        ctx->check(allocate(p->fpol, lines.size()*sizeof(double)), "hipMalloc(fpol tables)") ||
        ctx->check(hipMemcpy(p->fpol.get(), lines.data(), lines.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(fpol tables)")) {
        return nullptr;
    }
    ctx->moments.push_back(std::move(p));
    return ctx->moments.back().get();
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
    destroy_in(&gfhip_context::moments, p);
}

extern "C" int gfhip_moments_add(gfhip_moments *p, const uint64_t keys[7], uint64_t weight_key, int has_weight, size_t count) {
    if (!p) return 1;
    if (!keys) return p->ctx->fail("gfhip_moments_add needs its 7 keys");
    if (p->batches) return p->ctx->fail("a batched moment profile takes its particles with their index: gfhip_moments_add_particles");
    if (count == 0) return p->ctx->fail("a moment profile takes at least one particle");
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], weight_key};
    const void *columns[8] = {};
    bool is_f32 = false;
    if (particle_columns(p->ctx, all, has_weight ? 8 : 7, count, columns, is_f32, "a moment profile")) return 1;
    return p->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_moment_deposit(columns, is_f32, first, piece, p->map, p->field, p->packed.get(), p->fpol.get(),
                                     p->edges.get(), p->ns, p->sscale, p->is_private, p->block, p->max_workgroups, p->lds_bytes,
                                     p->state.get(), p->counters.get(), p->ctx->stream);
    });
}

extern "C" int gfhip_moments_add_particles(gfhip_moments *p, const uint64_t keys[7], uint64_t weight_key, int has_weight,
                                           size_t count, uint64_t first_particle) {
    if (!p) return 1;
    if (!keys) return p->ctx->fail("gfhip_moments_add_particles needs its 7 keys");
    if (const char *refused = p->particles_refused(first_particle, count)) return p->ctx->fail(refused);
    if (count == 0) return p->ctx->fail("a moment profile takes at least one particle");
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], weight_key};
    const void *columns[8] = {};
    bool is_f32 = false;
    if (particle_columns(p->ctx, all, has_weight ? 8 : 7, count, columns, is_f32, "a moment profile")) return 1;
    return p->add(count, [&](const size_t first, const size_t piece) {
        gfhip::launch_moment_deposit_particles(columns, is_f32, first, piece, first_particle + first, p->batches, p->map, p->field,
                                               p->packed.get(), p->fpol.get(), p->edges.get(), p->ns, p->sscale, p->is_private,
                                               p->block, p->max_workgroups, p->lds_bytes, p->state.get(), p->counters.get(),
                                               p->ctx->stream);
    });
}

extern "C" int gfhip_moments_values(gfhip_moments *p, const uint64_t keys[7], uint64_t label_key, uint64_t values_key, size_t count) {
    if (!p) return 1;
    gfhip_context *ctx = p->ctx;
    if (!keys) return ctx->fail("gfhip_moments_values needs its 7 keys");
    if (count == 0) return ctx->fail("a moment profile takes at least one particle");
    if (count > std::numeric_limits<size_t>::max()/moment_count) return ctx->fail("a moment profile's values buffer is shorter than 4 x the particle count");
    const void *columns[8] = {};
    bool is_f32 = false;
    if (particle_columns(ctx, keys, 7, count, columns, is_f32, "a moment profile")) return 1;
    double *label = nullptr, *values = nullptr;
    if (fp64_columns(ctx, "a moment profile's label", {label_key}, count, &label) ||
        fp64_columns(ctx, "a moment profile's values (4 per particle)", {values_key}, count*moment_count, &values)) {
        return 1;
    }
    if (enter(ctx)) return 1;
    gfhip::launch_moment_values(columns, is_f32, count, p->map, p->field, p->packed.get(), p->fpol.get(), label, values, ctx->stream);
    GFHIP_TRY(ctx, hipGetLastError(), "moment values launch");
    return 0;
}

extern "C" int gfhip_moments_counts(gfhip_moments *p, uint64_t *samples, uint64_t *outside, uint64_t *skipped) {
    return p ? p->counts(samples, outside, skipped) : 1;
}

extern "C" int gfhip_moments_state(gfhip_moments *p, int64_t *limbs) {
    if (!p) return 1;
    if (!limbs) return p->ctx->fail("gfhip_moments_state needs a destination");
    return p->state_to(limbs);
}

extern "C" int gfhip_moments_merge(gfhip_moments *p, const int64_t *limbs, size_t ns, size_t nm, uint64_t samples,
                                   uint64_t outside, uint64_t skipped) {
    if (!p) return 1;
    if (!limbs) return p->ctx->fail("gfhip_moments_merge needs a state");
    if (p->batches || ns != p->ns || nm != moment_count) return p->ctx->fail("merge: a moment profile of another shape");
    return p->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_moments_merge_batches(gfhip_moments *p, const int64_t *limbs, size_t batches, size_t ns, size_t nm,
                                           uint64_t samples, uint64_t outside, uint64_t skipped) {
    if (!p) return 1;
    if (!limbs) return p->ctx->fail("gfhip_moments_merge_batches needs a state");
    if (!p->batches || batches != p->batches || ns != p->ns || nm != moment_count) {
        return p->ctx->fail("merge: a moment profile of another shape");
    }
    return p->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_moments_read(gfhip_moments *p, double divisor, double *values) {
    if (!p) return 1;
    if (!values) return p->ctx->fail("gfhip_moments_read needs a destination");
    return p->read(divisor, values);
}

//  Not through enter(): as gfhip_flux_info.
extern "C" int gfhip_moments_info(gfhip_moments *p, struct gfhip_flux_info *info) {
    if (!p) return 1;
    if (!info) return p->ctx->fail("gfhip_moments_info needs a destination");
    p->info_to(info);
    return 0;
}

//  The map, the field and the tables of a host call, or why they are refused.
static const char *moments_host_of(const gfhip_flux_map *map, const gfhip_spectrum_field *field, gfhip::flux::map &m,
                                   gfhip::flux::field &f, gfhip::moments::host_tables &t) {
    if (const char *refused = flux_map_of(map, m)) return refused;
    if (const char *refused = phase_field_of(field, f)) return refused;
    t.coefficients = map->coefficients;
    t.table = static_cast<size_t> (map->numr*map->numz);
    for (size_t k = 0; k < 4; k++) t.fpol[k] = field->fpol[k];
    return nullptr;
}

//  Host side, no device: flux_label.hpp on the caller's 16 + 4 tables (moments_host.hpp).
extern "C" int gfhip_moments_values_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const void *const columns[7],
                                         int is_f32, size_t count, double *label, double *values) {
    bool complete = map && field && columns && ((label && values) || !count);
    for (int k = 0; complete && k < 7; k++) complete = columns[k] || !count;
    if (!complete) {
        creation_error = "gfhip_moments_values_host needs a map, a field, seven columns and two destinations";
        return 1;
    }
    gfhip::flux::map m;
    gfhip::flux::field f;
    gfhip::moments::host_tables t;
    if (const char *refused = moments_host_of(map, field, m, f, t)) {
        creation_error = refused;
        return 1;
    }
    if (is_f32) {
        gfhip::moments::values_host<float> (m, f, t, columns, count, label, values);
    } else {
        gfhip::moments::values_host<double> (m, f, t, columns, count, label, values);
    }
    return 0;
}

extern "C" int gfhip_moments_add_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *sedges, size_t ns,
                                      const void *const columns[8], int is_f32, size_t count, int64_t *limbs, uint64_t counters[3]) {
    bool complete = map && field && sedges && columns && limbs && counters;
    for (int k = 0; complete && k < 7; k++) complete = columns[k] || !count;
    if (!complete) {
        creation_error = "gfhip_moments_add_host needs a map, a field, the label edges, seven columns, limbs and counters";
        return 1;
    }
    gfhip::flux::map m;
    gfhip::flux::field f;
    gfhip::moments::host_tables t;
    const char *refused = moments_axis_of(sedges, ns);
    if (!refused) refused = moments_host_of(map, field, m, f, t);
    if (refused) {
        creation_error = refused;
        return 1;
    }
    if (is_f32) {
        gfhip::moments::add_host<float> (m, f, t, sedges, ns, columns, count, limbs, counters);
    } else {
        gfhip::moments::add_host<double> (m, f, t, sedges, ns, columns, count, limbs, counters);
    }
    return 0;
}

//  The batches and the particle range of a host call, or why they are refused.
static const char *host_batches_refused(const size_t batches, const uint64_t first_particle, const size_t count) {
    if (batches < 1 || batches > gfhip::batches::max_batches) return "a batched object has 1 to 256 batches";
    if (first_particle + static_cast<uint64_t> (count) < first_particle) return "first_particle + count overflows 64 bits";
    return nullptr;
}

//  limbs: [batches][ns][4][67] (moments_host.hpp's add_particles_host).
extern "C" int gfhip_moments_add_particles_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *sedges,
                                                size_t ns, size_t batches, const void *const columns[8], int is_f32, size_t count,
                                                uint64_t first_particle, int64_t *limbs, uint64_t counters[3]) {
    bool complete = map && field && sedges && columns && limbs && counters;
    for (int k = 0; complete && k < 7; k++) complete = columns[k] || !count;
    if (!complete) {
        creation_error = "gfhip_moments_add_particles_host needs a map, a field, the label edges, seven columns, limbs and counters";
        return 1;
    }
    gfhip::flux::map m;
    gfhip::flux::field f;
    gfhip::moments::host_tables t;
    const char *refused = moments_axis_of(sedges, ns);
    if (!refused) refused = host_batches_refused(batches, first_particle, count);
    if (!refused) refused = moments_host_of(map, field, m, f, t);
    if (refused) {
        creation_error = refused;
        return 1;
    }
    if (is_f32) {
        gfhip::moments::add_particles_host<float> (m, f, t, sedges, ns, static_cast<unsigned int> (batches), first_particle, columns,
                                                   count, limbs, counters);
    } else {
        gfhip::moments::add_particles_host<double> (m, f, t, sedges, ns, static_cast<unsigned int> (batches), first_particle,
                                                    columns, count, limbs, counters);
    }
    return 0;
}

//  limbs: [batches][ns][np][ng][67] (phase_host.hpp's add_particles_host).
extern "C" int gfhip_phase_add_particles_host(const gfhip_flux_map *map, const gfhip_spectrum_field *field, const double *sedges,
                                              size_t ns, const double *pedges, size_t np, const double *gedges, size_t ng,
                                              size_t batches, const void *const columns[8], int is_f32, size_t count,
                                              uint64_t first_particle, int64_t *limbs, uint64_t counters[3]) {
    bool complete = map && field && sedges && pedges && gedges && columns && limbs && counters;
    for (int k = 0; complete && k < 7; k++) complete = columns[k] || !count;
    if (!complete) {
        creation_error = "gfhip_phase_add_particles_host needs a map, a field, three edge arrays, seven columns, limbs and counters";
        return 1;
    }
    const double *axes[3] = {sedges, pedges, gedges};
    const size_t n[3] = {ns, np, ng};
    gfhip::flux::map m;
    gfhip::flux::field f;
    gfhip::moments::host_tables t;
    const char *refused = nullptr;
    size_t cells = 1;
    for (int a = 0; !refused && a < 3; a++) {
        if (n[a] < 1 || n[a] > flux_cell_limit) {
            refused = "a distribution has 1 to 4096 cells per axis (at least two edges)";
        } else if (!edges_increase(axes[a], n[a])) {
            refused = "the edges of a distribution must be finite and strictly increasing";
        }
        cells *= n[a];
    }
    if (!refused && cells > phase_cell_limit) refused = "a distribution has at most 2^20 cells (536 B each)";
    if (!refused) refused = host_batches_refused(batches, first_particle, count);
    if (!refused) refused = moments_host_of(map, field, m, f, t);
    if (refused) {
        creation_error = refused;
        return 1;
    }
    if (is_f32) {
        gfhip::phase::add_particles_host<float> (m, f, t, axes, n, static_cast<unsigned int> (batches), first_particle, columns,
                                                 count, limbs, counters);
    } else {
        gfhip::phase::add_particles_host<double> (m, f, t, axes, n, static_cast<unsigned int> (batches), first_particle, columns,
                                                  count, limbs, counters);
    }
    return 0;
}

//  First-exit trackers (confinement.hip, flux_label.hpp).  The axes and the cells are a distribution's; deposits always
//  go to the global state, so the launch shape is the global path's whatever the map's flags say.

//  The three axes of a footprint checked and laid one after the other, or why they are refused.
static const char *confine_axes_of(const double *const *axes, const size_t *n, std::vector<double> &edges, size_t &cells) {
    cells = 1;
    for (int a = 0; a < 3; a++) {
        if (n[a] < 1 || n[a] > flux_cell_limit) return "a loss footprint has 1 to 4096 cells per axis (at least two edges)";
        if (!edges_increase(axes[a], n[a])) return "the edges of a loss footprint must be finite and strictly increasing";
        edges.insert(edges.end(), axes[a], axes[a] + n[a] + 1);
        cells *= n[a];                                 // at most 2^36
    }
    if (cells > phase_cell_limit) return "a loss footprint has at most 2^20 cells (536 B each)";
    return nullptr;
}

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
    std::vector<double> edges;
    size_t cells = 0;
    if (const char *refused = confine_axes_of(axes, n, edges, cells)) {
        ctx->fail(refused);
        return nullptr;
    }
    if (limit != limit) {
        ctx->fail("the limit of a confinement tracker must not be NaN");
        return nullptr;
    }
    if (count == 0 || capacity == 0) {
        ctx->fail("a confinement tracker needs at least one particle and room for at least one check");
        return nullptr;
    }
    gfhip_flux_map global = *map;
    global.flags |= gfhip::flux::flag_no_private_sums;
    std::unique_ptr<gfhip_confine> c(new gfhip_confine);
    c->limit = limit;
    c->count = count;
    c->capacity = capacity;
    c->is_f32 = is_f32 != 0;
    c->alive_key = alive_key;
    for (int a = 0; a < 3; a++) {
        c->n[a] = n[a];
        c->scale[a] = static_cast<double> (n[a])/(axes[a][n[a]] - axes[a][0]);
    }
    if (c->create(ctx, &global, cells, edges, nullptr) || enter(ctx) ||
        ensure_buffer(ctx, alive_key, count, c->is_f32 ? GFIR_F32 : GFIR_F64, nullptr) ||
        ctx->check(allocate(c->lost_step, count*sizeof(uint32_t)), "hipMalloc(lost steps)") ||
        ctx->check(allocate(c->newly_lost, capacity*sizeof(unsigned long long)), "hipMalloc(newly lost)") ||
        ctx->check(hipMemsetAsync(c->newly_lost.get(), 0, capacity*sizeof(unsigned long long), ctx->stream), "hipMemset(newly lost)")) {
        return nullptr;
    }
    gfhip::launch_confinement_reset(count, c->lost_step.get(), find_buffer(ctx, alive_key)->pointer, c->is_f32, nullptr, nullptr,
                                    ctx->stream);
    if (ctx->check(hipGetLastError(), "confinement reset launch")) return nullptr;
    ctx->confines.push_back(std::move(c));
    return ctx->confines.back().get();
}

extern "C" void gfhip_confine_destroy(gfhip_confine *c) {
    destroy_in(&gfhip_context::confines, c);
}

extern "C" int gfhip_confine_check(gfhip_confine *c, const uint64_t keys[7], uint64_t weight_key, int has_weight,
                                   uint64_t exit_r_key, uint64_t exit_z_key, int has_exit, uint32_t step) {
    if (!c) return 1;
    gfhip_context *ctx = c->ctx;
    if (!keys) return ctx->fail("gfhip_confine_check needs its 7 keys");
    const uint64_t all[8] = {keys[0], keys[1], keys[2], keys[3], keys[4], keys[5], keys[6], weight_key};
    const void *columns[8] = {};
    bool is_f32 = false;
    if (particle_columns(ctx, all, has_weight ? 8 : 7, c->count, columns, is_f32, "a confinement tracker")) return 1;
    if (is_f32 != c->is_f32) return ctx->fail("the columns are not of the confinement tracker's type");
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
            gfhip::launch_confinement_check(columns, alive->pointer, c->is_f32, first, piece, c->map, c->packed.get(), c->limit,
                                            c->edges.get(), c->n, c->scale, step, c->lost_step.get(), exits[0], exits[1], entry,
                                            c->block, c->max_workgroups, c->lds_bytes, c->state.get(), c->counters.get(),
                                            ctx->stream);
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
    return c ? c->counts(samples, outside, skipped) : 1;
}

extern "C" int gfhip_confine_state(gfhip_confine *c, int64_t *limbs) {
    if (!c) return 1;
    if (!limbs) return c->ctx->fail("gfhip_confine_state needs a destination");
    return c->state_to(limbs);
}

extern "C" int gfhip_confine_merge(gfhip_confine *c, const int64_t *limbs, size_t nr, size_t nz, size_t ng, uint64_t samples,
                                   uint64_t outside, uint64_t skipped) {
    if (!c) return 1;
    if (!limbs) return c->ctx->fail("gfhip_confine_merge needs a state");
    if (nr != c->n[0] || nz != c->n[1] || ng != c->n[2]) return c->ctx->fail("merge: a loss footprint of another shape");
    return c->merge(limbs, samples, outside, skipped);
}

extern "C" int gfhip_confine_read(gfhip_confine *c, double divisor, double *values) {
    if (!c) return 1;
    if (!values) return c->ctx->fail("gfhip_confine_read needs a destination");
    return c->read(divisor, values);
}

//  Not through enter(): as gfhip_flux_info.
extern "C" int gfhip_confine_info(gfhip_confine *c, struct gfhip_flux_info *info) {
    if (!c) return 1;
    if (!info) return c->ctx->fail("gfhip_confine_info needs a destination");
    c->info_to(info);
    return 0;
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
        creation_error = "gfhip_confine_check_host needs a map, the columns x, y, z and gamma, lost_step, alive and newly_lost, "
                         "both exit arrays or neither, and with limbs the three edge arrays and the counters";
        return 1;
    }
    gfhip::flux::map m;
    const double *axes[3] = {redges, zedges, gedges};
    const size_t n[3] = {nr, nz, ng};
    std::vector<double> edges;
    size_t cells = 0;
    const char *refused = flux_map_of(map, m);
    if (!refused && limbs) refused = confine_axes_of(axes, n, edges, cells);
    if (!refused && limit != limit) refused = "the limit of a confinement tracker must not be NaN";
    if (!refused && step == GFHIP_CONFINED) refused = "step 0xFFFFFFFF means confined: a check cannot have it";
    if (refused) {
        creation_error = refused;
        return 1;
    }
    const size_t table = static_cast<size_t> (map->numr*map->numz);
    if (is_f32) {
        gfhip::confine::check_host<float> (m, map->coefficients, table, limit, axes, n, columns, count, step, lost_step, static_cast<float *> (alive), exit_r,
                                   exit_z, newly_lost, limbs, counters);
    } else {
        gfhip::confine::check_host<double> (m, map->coefficients, table, limit, axes, n, columns, count, step, lost_step, static_cast<double *> (alive), exit_r,
                                    exit_z, newly_lost, limbs, counters);
    }
    return 0;
}

//  Particle sources (particle_source.hip, particle_draw.hpp).

//  The route of a source made with neither route flag.
static const bool source_refill_by_default = true;

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
    if (ns && !edges_increase(sedges, ns)) return "the edges of a particle source's profile must be finite and strictly increasing";
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
    std::vector<double> lines, cubics, profile(1, 0.0);
    if (!psi_lines(map, lines) || !fpol_lines(field, cubics)) {
        ctx->fail("a particle source's tables do not fit the host's memory");
        return nullptr;
    }
    if (ns) {
        profile.assign(sedges, sedges + ns + 1);
        profile.insert(profile.end(), accept, accept + ns);
        s->scale = static_cast<double> (ns)/(sedges[ns] - sedges[0]);
    }
    if (enter(ctx) ||
        ctx->check(allocate(s->packed, lines.size()*sizeof(double)), "hipMalloc(flux tables)") ||
        ctx->check(hipMemcpy(s->packed.get(), lines.data(), lines.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(flux tables)") ||
        ctx->check(allocate(s->fpol, cubics.size()*sizeof(double)), "hipMalloc(fpol tables)") ||
        ctx->check(hipMemcpy(s->fpol.get(), cubics.data(), cubics.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(fpol tables)") ||
        ctx->check(allocate(s->profile, profile.size()*sizeof(double)), "hipMalloc(profile)") ||
        ctx->check(hipMemcpy(s->profile.get(), profile.data(), profile.size()*sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(profile)") ||
        ctx->check(allocate(s->counters, 4*sizeof(unsigned long long)), "hipMalloc(counters)") ||
        ctx->check(hipMemsetAsync(s->counters.get(), 0, 4*sizeof(unsigned long long), ctx->stream), "hipMemset(counters)") ||
        ctx->check(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
        return nullptr;
    }
    ctx->sources.push_back(std::move(s));
    return ctx->sources.back().get();
}

extern "C" void gfhip_source_destroy(gfhip_source *s) {
    destroy_in(&gfhip_context::sources, s);
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
    bool complete = map && field && columns && counters;
    for (int k = 0; complete && k < 7; k++) complete = columns[k] || !count;
    if (!complete) {
        creation_error = "gfhip_source_fill_host needs a map, a field, the seven columns and the counters";
        return 1;
    }
    gfhip::flux::map m;
    gfhip::flux::field f;
    gfhip::draw::parameters par;
    const char *refused = flux_map_of(map, m);
    if (!refused) refused = phase_field_of(field, f);
    if (!refused) refused = source_parameters_of(box, slo, shi, blo, bhi, xlo, xhi, sedges, accept, ns, seed, attempts, flags, par);
    if (!refused && first_particle + static_cast<uint64_t> (count) < first_particle) refused = "first_particle + count overflows 64 bits";
    if (refused) {
        creation_error = refused;
        return 1;
    }
    const gfhip::draw::host_tables tables = {map->coefficients, static_cast<size_t> (map->numr*map->numz),
                                             {field->fpol[0], field->fpol[1], field->fpol[2], field->fpol[3]}, sedges, accept, ns};
    if (is_f32) {
        gfhip::draw::fill_host<float> (m, f, par, tables, columns, columns[7], first_particle, count, counters);
    } else {
        gfhip::draw::fill_host<double> (m, f, par, tables, columns, columns[7], first_particle, count, counters);
    }
    return 0;
}

extern "C" void gfhip_source_block_host(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
    gfhip::draw::philox(counter, key, out);
}

//  What a run of quadrature points needs beside the map (flux_label.hpp), or why it is refused.
struct volume_points {
    unsigned long long row = 0;                        // numz*sub: the sub-cells along z
    double twice_sub = 0.0, area = 0.0;
    gfhip::flux::window window = {};
};

static const char *volume_points_of(const gfhip::flux::map &m, const uint32_t sub, const gfhip_flux_window *window,
                                    const uint64_t first, const uint64_t count, volume_points &p) {
    if (sub < 1 || sub > 256) return "flux volumes: sub must be 1 to 256";
    if (!(m.dr > 0.0) || !(m.dz > 0.0) || !(m.rmin >= 0.0)) return "flux volumes need a map with dr > 0, dz > 0 and rmin >= 0";
//  numr*numz <= 2^31 and sub*sub <= 2^16: the total fits 64 bits with room to spare.
    p.row = m.columns*sub;
    const uint64_t total = static_cast<uint64_t> (m.numr)*sub*p.row;
    if (first + count < first || first + count > total) return "flux volumes: first + count exceeds the numr*sub*numz*sub points of the map";
    const double inf = std::numeric_limits<double>::infinity();
    p.window = window ? gfhip::flux::window{window->rlo, window->rhi, window->zlo, window->zhi} : gfhip::flux::window{-inf, inf, -inf, inf};
    if (!(p.window.rlo < p.window.rhi) || !(p.window.zlo < p.window.zhi)) return "flux volumes: a window needs rlo < rhi and zlo < zhi, no NaN";
    p.twice_sub = static_cast<double> (2u*sub);
    p.area = gfhip::flux::sub_area(m, sub);
    return nullptr;
}

extern "C" int gfhip_flux_add_volumes(gfhip_flux *f, uint32_t sub, const gfhip_flux_window *window, uint64_t first, uint64_t count) {
    if (!f) return 1;
    if (f->batches) return f->ctx->fail("flux volumes have no rays: a batched flux profile does not take them");
    volume_points p;
    if (const char *refused = volume_points_of(f->map, sub, window, first, count, p)) return f->ctx->fail(refused);
    return f->add(count, [&](const size_t done, const size_t piece) {
        gfhip::launch_flux_volumes(first + done, piece, p.row, p.twice_sub, p.area, p.window, f->map, f->packed.get(),
                                   f->edges.get(), f->cells, f->scale, f->is_private, f->block, f->max_workgroups,
                                   f->lds_bytes, f->state.get(), f->counters.get(), f->ctx->stream);
    });
}

//  Host side, no device: the quadrature and the label of flux_label.hpp and superacc.hpp's deposit on the CPU.
extern "C" int gfhip_flux_volumes_host(const gfhip_flux_map *map, const double *edges, size_t cells, uint32_t sub,
                                       const gfhip_flux_window *window, uint64_t first, uint64_t count,
                                       int64_t *limbs, uint64_t counters[3]) {
    if (!map || !edges || !limbs || !counters) {
        creation_error = "gfhip_flux_volumes_host needs a map, edges, limbs and counters";
        return 1;
    }
    if (cells < 1 || cells > flux_cell_limit) {
        creation_error = "a flux profile has 1 to 4096 cells";
        return 1;
    }
    if (!edges_increase(edges, cells)) {
        creation_error = "the edges of a flux profile must be finite and strictly increasing";
        return 1;
    }
    gfhip::flux::map m;
    volume_points p;
    const char *refused = flux_map_of(map, m);
    if (!refused) refused = volume_points_of(m, sub, window, first, count, p);
    if (refused) {
        creation_error = refused;
        return 1;
    }
    const size_t table = static_cast<size_t> (map->numr*map->numz);
    const auto normalise_all = [&]() {
        for (size_t cell = 0; cell < cells; cell++) gfhip::superacc::normalise(limbs + cell*gfhip::superacc::limbs);
    };
    uint64_t pending = 0, outside = 0, skipped = 0;
    unsigned long long gr = first/p.row, gz = first%p.row;
    for (uint64_t t = 0; t < count; t++) {
        const double r = gfhip::flux::sub_centre(m.rmin, m.dr, gr, p.twice_sub);
        const double z = gfhip::flux::sub_centre(m.zmin, m.dz, gz, p.twice_sub);
        if (++gz == p.row) {
            gz = 0;
            gr++;
        }
        double tr, tz, c[16];
        const long long at = gfhip::flux::in_window(p.window, r, z) ? gfhip::flux::locate(m, r, 0.0, z, tr, tz) : -1;
        if (at < 0) {
            outside++;
            continue;
        }
        for (size_t k = 0; k < 16; k++) c[k] = map->coefficients[k*table + static_cast<size_t> (at)];
        const double label = gfhip::flux::label_of(m, gfhip::flux::psi_of(c, tr, tz));
        if (!(label >= edges[0] && label < edges[cells])) {
            outside++;
            continue;
        }
        const size_t cell = static_cast<size_t> (std::upper_bound(edges, edges + cells + 1, label) - edges) - 1;
        const double w = gfhip::flux::sub_weight(r, p.area);
        if (!gfhip::superacc::is_finite(w)) {
            skipped++;
            continue;
        }
        if (++pending > gfhip::superacc::deposits_per_normalise) {
            normalise_all();
            pending = 1;
        }
        gfhip::superacc::deposit(limbs + cell*gfhip::superacc::limbs, w);
    }
    normalise_all();
    counters[0] += count;
    counters[1] += outside;
    counters[2] += skipped;
    return 0;
}

//  Host side, no device: the functions of superacc.hpp that the kernels run, on one accumulator.
extern "C" int gfhip_exact_sum(const double *values, size_t count, double *sum, int64_t *limbs) {
    if ((!values && count) || !sum) return 1;
    int64_t acc[gfhip::superacc::limbs] = {0};
    uint64_t pending = 0;
    for (size_t i = 0; i < count; i++) {
        if (!gfhip::superacc::is_finite(values[i])) {
            creation_error = "gfhip_exact_sum takes finite values";
            return 1;
        }
        if (++pending > gfhip::superacc::deposits_per_normalise) {
            gfhip::superacc::normalise(acc);
            pending = 1;
        }
        gfhip::superacc::deposit(acc, values[i]);
    }
    gfhip::superacc::normalise(acc);
    *sum = gfhip::superacc::round(acc);
    if (limbs) std::memcpy(limbs, acc, sizeof(acc));
    return 0;
}
