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

#include "converge_state.hpp"
#include "hand_over.hpp"
#include "runtime.hpp"

using namespace gfhip::runtime;

thread_local std::string gfhip::runtime::creation_error;

namespace gfhip {
void launch_max_reduce(const void *in, const size_t n, const bool f64,
                       unsigned long long *result, const unsigned int num_cus, hipStream_t stream);
void launch_converge_decide(const bool f64, unsigned long long *reduced, void *state, const unsigned int count, hipStream_t stream);
void launch_max_modulus(const void *in, const size_t n, const bool f64, void *result, hipStream_t stream);
}

namespace {

struct event_pair {
    event_ptr start, stop;
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

//  Here, where gfhip_kernel is complete (runtime.hpp).
gfhip_context::gfhip_context() = default;
gfhip_context::~gfhip_context() = default;

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
int gfhip::runtime::enter(gfhip_context *ctx) {
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

int gfhip::runtime::ensure_buffer(gfhip_context *ctx, const uint64_t key, const size_t count, const uint32_t dtype,
                                  const void *init, size_t init_count) {
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

buffer *gfhip::runtime::find_buffer(gfhip_context *ctx, const uint64_t key) {
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
