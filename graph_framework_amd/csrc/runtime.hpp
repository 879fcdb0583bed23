//------------------------------------------------------------------------------
///  @file runtime.hpp
///  @brief What the translation units of libgf_hip.so share (not installed): the owning holders of HIP resources, a
///  context's buffers, the context itself and the few functions of gf_hip.cpp that the exact-sum objects of
///  cells_rays.cpp and cells_particles.cpp call.
//------------------------------------------------------------------------------
#ifndef GFHIP_RUNTIME_HPP
#define GFHIP_RUNTIME_HPP

#include <hip/hip_runtime.h>

#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gf_hip.h"
#include "../../include/gfir.h"
#include "converge_state.hpp"

namespace gfhip {
namespace runtime {

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

struct buffer {
    device_ptr<> owned;         // null for a buffer adopted by gfhip_set_buffer, which is never freed here
    void *pointer = nullptr;
    size_t count = 0;
    uint32_t dtype = GFIR_F64;
    host_ptr<> mirror;          // host copy handed out by gfhip_get_host_buffer, refreshed by gfhip_wait
};

//  What a context owns beside its kernels and buffers (deposition grids, profiles, spectra, distributions, trackers,
//  moment profiles, particle sources), from gfhip_*_create until gfhip_*_destroy or the context's end.
struct context_object {
    gfhip_context *ctx = nullptr;
    virtual ~context_object() = default;
};

//  Where the entry points that have no context leave their message (gfhip_last_error(NULL)).
extern thread_local std::string creation_error;

}  // namespace runtime
}  // namespace gfhip

//  Members are released last to first: the objects, the kernels and the buffers, then the owned stream.
struct gfhip_context {
    int device = 0;
    gfhip::runtime::stream_ptr own_stream;         // set when the context created `stream`
    hipStream_t stream = nullptr;
    unsigned int num_cus = 256;
    gfhip::runtime::device_ptr<unsigned long long> device_scalar;  // 8 words: one per pass of a batch
    gfhip::runtime::host_ptr<unsigned long long> host_scalar;      // 8 words
    gfhip::runtime::device_ptr<unsigned int> device_flags;         // bit 0: a lane redid a pass with the compiler's division
    gfhip::runtime::device_ptr<gfhip::converge_state> device_converge;
    gfhip::runtime::host_ptr<gfhip::converge_state> host_converge;
    std::map<uint64_t, gfhip::runtime::buffer> buffers;
    std::map<uint64_t, gfhip::runtime::device_ptr<>> random_states;    // MT19937 states per random_state node (raw bytes)
    std::vector<std::unique_ptr<gfhip_kernel>> kernels;
    std::vector<std::unique_ptr<gfhip::runtime::context_object>> objects;
    std::string error;
    gfhip_kernel *running_ahead = nullptr;         // the kernel whose last batch ran passes the caller has not asked for yet
    gfhip_kernel *max_streak = nullptr;            // the kernel the last entry point was gfhip_run_max of
    unsigned int timing = 0;                       // 0 = off, N = events around every Nth launch of a kernel
    gfhip::runtime::event_ptr hand_over_before, hand_over_after;   // order gfhip_hand_over into this context from another stream (made on first use)

    gfhip_context();
    ~gfhip_context();                              // in gf_hip.cpp, where gfhip_kernel is complete

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

#define GFHIP_TRY(ctx, call, what) do { if ((ctx)->check((call), (what))) return 1; } while (0)

namespace gfhip {
namespace runtime {

//  gf_hip.cpp.  Entry points that touch the device begin with enter(): the context's device, then the state settled.
int enter(gfhip_context *ctx);
//  The buffer of `key`, or null with the context's message.
buffer *find_buffer(gfhip_context *ctx, uint64_t key);
//  The buffer of `key` made if there is none (zeroed, or the first init_count elements from `init`), else checked.
int ensure_buffer(gfhip_context *ctx, uint64_t key, size_t count, uint32_t dtype, const void *init,
                  size_t init_count = ~static_cast<size_t> (0));

}  // namespace runtime
}  // namespace gfhip

#endif
