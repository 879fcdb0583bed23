//------------------------------------------------------------------------------
///  @file converge_state.hpp
///  @brief The converge loop of workflow.hpp:179-205, written once: its test as one step, the step applied on the
///  device to the maxima a launch has reduced, and the order-preserving integer image those maxima travel in.
///
///      while (|max| > |tol| && |last - max| > |tol| && |off_last - max| > |tol| && iterations++ < limit) {
///          last = max;  if (!(iterations%2)) off_last = max;  max = run_max(); }
///
///  Shared by the host runtime (gf_hip.cpp), the reduction and decide kernels (reduce.hip) and a host-only test
///  (tests/converge_step_check.cpp): no HIP header, plain C++17.
//------------------------------------------------------------------------------
#ifndef gfhip_converge_state_hpp
#define gfhip_converge_state_hpp

#include <cmath>
#include <complex>
#include <limits>

#ifndef GFHIP_HD                    // (superacc.hpp has the same)
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GFHIP_HD __host__ __device__ inline
#else
#define GFHIP_HD inline
#endif
#endif

namespace gfhip {

//  Monotone map real -> unsigned so that integer max == floating max (+0 images above -0), and back.  The all-ones
//  key of the value's width, which no number has, comes back as a NaN: max_reduce_kernel plants it for a NaN at
//  element 0.
GFHIP_HD unsigned long long ordered_key(const double x) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
GFHIP_HD unsigned long long ordered_key(const float x) {
    const unsigned int b = __builtin_bit_cast(unsigned int, x);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
template<typename T>
GFHIP_HD T from_ordered_key(const unsigned long long key) {
    if constexpr (sizeof(T) == 8) {
        return __builtin_bit_cast(T, (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key);
    } else {
        const unsigned int k32 = static_cast<unsigned int> (key);
        return __builtin_bit_cast(T, (k32 >> 31) ? (k32 & 0x7FFFFFFFu) : ~k32);
    }
}

//  What the loop compares: |x|.
GFHIP_HD float mag(const float x) { return x < 0.0f ? -x : x; }
GFHIP_HD double mag(const double x) { return x < 0.0 ? -x : x; }
//  std::abs of a complex value as the reference's build has it: the C library's cabs, that is hypot.  In a HIP
//  translation unit std::abs(std::complex) is the textbook scaled formula instead (the compiler's complex wrapper
//  turns the C99 functions off): NaN for an infinite part, and not always hypot's last bit.  Host only.
template<typename B>
inline B mag(const std::complex<B> &z) {
    return std::hypot(z.real(), z.imag());
}

//  One turn of the loop's test, everything in the item's own type V: the tolerance is narrowed to V before its
//  magnitude is taken, and last and off_last start at numeric_limits<V>::max() — the largest finite value for a
//  real V, V() for std::complex, whose numeric_limits is the unspecialised one.
template<typename V>
struct converge_step {
    V last = std::numeric_limits<V>::max(), off_last = std::numeric_limits<V>::max();
    decltype(mag(V())) mag_tol;
    unsigned long long iterations = 0, limit;

    GFHIP_HD converge_step(const double tolerance, const unsigned long long limit_) :
    mag_tol(mag(static_cast<V> (tolerance))), limit(limit_) {}

//  `max` is the maximum of the pass that has just run: does the loop run another?  (`iterations++ < limit`: the
//  test that fails on the limit is counted too.)
    GFHIP_HD bool advance(const V max) {
        bool go = mag(max) > mag_tol && mag(last - max) > mag_tol && mag(off_last - max) > mag_tol;
        if (go) {
            go = iterations < limit;
            iterations++;
        }
        if (go) {
            last = max;
            if (!(iterations%2)) off_last = max;
        }
        return go;
    }
};

//  Device-resident state of one loop whose test runs on the device.
struct converge_state {
    double max_residual;            ///< max of the last pass that ran
    double last, off_last;          ///< the step's last / off_last (exact images of the item's type)
    double tolerance;
    unsigned long long iterations;  ///< the step's `iterations`
    unsigned long long limit;       ///< max_iterations
    unsigned int done;              ///< the loop's condition came out false: later passes return at once
    unsigned int passes;            ///< passes that really ran
    unsigned int extra;             ///< passes of the last launch that ran BEYOND the loop's last one — the state is
                                    ///< then restored from the undo arrays and the launch redone without them
    unsigned int batch_passes;      ///< passes of the last launch that belong to the loop
};

template<typename T>
GFHIP_HD converge_state converge_begin(const double tolerance, const unsigned long long limit) {
    const converge_step<T> step(tolerance, limit);
    converge_state state = converge_state();
    state.last = static_cast<double> (step.last);
    state.off_last = static_cast<double> (step.off_last);
    state.tolerance = tolerance;
    state.limit = limit;
    return state;
}

//  Device side of the loop: a launch of `count` passes (`<name>_max`: one; `<name>_batch`, codegen.hpp: several, on
//  state kept in registers) has left the ordered key of each pass's max in reduced[pass]; one thread applies the step
//  to them in order, in the item's own precision T.  The loop may end on any of them: `done`, and later launches
//  return at once.  If it ends before the last pass of the launch, `extra` passes ran that the host loop would not
//  have run; the host restores the state of the beginning of the launch and redoes `batch_passes`.  Every slot is left
//  zero, ready for the next launch's atomicMax.
template<typename T>
GFHIP_HD void decide(converge_state &state, unsigned long long *reduced, const unsigned int count) {
    if (state.done) return;
    converge_step<T> step(state.tolerance, state.limit);
    step.last = static_cast<T> (state.last);
    step.off_last = static_cast<T> (state.off_last);
    step.iterations = state.iterations;
    for (unsigned int pass = 0; pass < count; pass++) {
        const unsigned long long key = reduced[pass];
        reduced[pass] = 0ull;
        if (state.done) continue;                    // still clear the slots of the passes beyond the end
        const T value = from_ordered_key<T> (key);
        state.max_residual = static_cast<double> (value);
        state.passes++;
        if (!step.advance(value)) {
            state.done = 1u;
            state.batch_passes = pass + 1u;
            state.extra = count - (pass + 1u);
        }
    }
    state.last = static_cast<double> (step.last);
    state.off_last = static_cast<double> (step.off_last);
    state.iterations = step.iterations;
}

}  // namespace gfhip

#endif /* gfhip_converge_state_hpp */
