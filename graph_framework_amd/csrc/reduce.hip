//------------------------------------------------------------------------------
///  @file reduce.hip
///  @brief Device-wide max reduction for converge items (hand-written, gfx950): max_reduce_kernel for real outputs,
///  max_modulus_kernel for complex ones, and converge_decide_kernel, the launch around the loop's test on the
///  device (converge_state.hpp, which also has the integer image `ordered_key` the maxima travel in).
///
///  Replaces the reference's generated `max_reduction` kernel
///  (cuda_context.hpp:954-995: one block of 1024 threads, 32-wide shuffles, result
///  read through managed memory) and cpu_context's std::max_element
///  (cpu_context.hpp:306-322).  Here: a grid-stride pass with 16 B/lane loads,
///  a 64-lane wavefront reduction with __shfl_down (no LDS traffic), one LDS
///  word per wave, and ONE device-scope atomicMax per workgroup on an
///  order-preserving integer image of the value.  max is exact and order
///  independent, so the result is the maximum a serial scan finds, as a number:
///  the same bits unless it is a zero (-0 and +0 are equal; a scan keeps the first
///  of them, the integer image prefers +0, and which one a lane or a wave hands on
///  depends on the grid), and a canonical NaN, not the element's payload, when
///  element 0 is a NaN (the only place where std::max_element selects one).
///  HBM-bound: 8 (4) bytes per element, one pass.
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "converge_state.hpp"

namespace gfhip {

template<typename T> struct alignas(2*sizeof(T)) vec2 { T a, b; };

template<typename T>
__global__ void __launch_bounds__(256)
max_reduce_kernel(const T *__restrict__ base, const unsigned long long total, const unsigned int head,
                  unsigned long long *__restrict__ result) {
    const T lowest = -__builtin_huge_val();
    T m = lowest;

//  `head` leading elements bring the pointer to 16 B alignment (caller-owned
//  buffers may be shards that start at an odd element).
    const T *in = base + head;
    const unsigned long long n = total - head;
    if (blockIdx.x == 0 && threadIdx.x < head) {
//  The same compare as everywhere below: a NaN among the head elements is not selected
//  (element 0 is handled by first_is_nan).
        const T v = base[threadIdx.x];
        m = v > m ? v : m;
    }
//  std::max_element (cpu_context.hpp:306-322) returns element 0 if that is a NaN: every later
//  `max < x` is false.  Elsewhere a NaN is never selected (`v > m` is false).
    const bool first_is_nan = total > 0 && base[0] != base[0];

//  Pairs of elements per lane per load (16 B for double).
    const unsigned long long pairs = n/2;
    const vec2<T> *in2 = reinterpret_cast<const vec2<T> *> (in);
    for (unsigned long long i = blockIdx.x*static_cast<unsigned long long> (blockDim.x) + threadIdx.x;
         i < pairs; i += gridDim.x*static_cast<unsigned long long> (blockDim.x)) {
        const vec2<T> v = in2[i];
        m = v.a > m ? v.a : m;
        m = v.b > m ? v.b : m;
    }
    if ((n & 1ull) && blockIdx.x == 0 && threadIdx.x == 0) {
        const T v = in[n - 1];
        m = v > m ? v : m;
    }

//  64-lane wavefront reduction.
    for (int offset = 32; offset > 0; offset >>= 1) {
        const T other = __shfl_down(m, offset, 64);
        m = other > m ? other : m;
    }

    __shared__ T wave_max[4];
    const unsigned int lane = threadIdx.x & 63u;
    const unsigned int wave = threadIdx.x >> 6;
    if (lane == 0) {
        wave_max[wave] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        T block = wave_max[0];
        for (unsigned int w = 1; w < (blockDim.x >> 6); w++) {
            block = wave_max[w] > block ? wave_max[w] : block;
        }
        atomicMax(result, ordered_key(block));
        if (blockIdx.x == 0 && first_is_nan) atomicMax(result, ~0ull >> (sizeof(T) == 8 ? 0 : 32));
    }
}

//  Device side of the converge loop (converge_state.hpp: decide): one thread applies the loop's test to the maxima
//  the `count` passes of the launch before it have reduced.
template<typename T>
__global__ void converge_decide_kernel(unsigned long long *__restrict__ reduced, converge_state *__restrict__ state,
                                       const unsigned int count) {
    decide<T> (*state, reduced, count);
}

void launch_converge_decide(const bool f64, unsigned long long *reduced, void *state, const unsigned int count, hipStream_t stream) {
    if (f64) {
        hipLaunchKernelGGL(converge_decide_kernel<double>, dim3(1), dim3(1), 0, stream, reduced, static_cast<converge_state *> (state), count);
    } else {
        hipLaunchKernelGGL(converge_decide_kernel<float>, dim3(1), dim3(1), 0, stream, reduced, static_cast<converge_state *> (state), count);
    }
}

//  Complex outputs: the element of largest modulus, the first of equals — std::max_element with
//  std::abs as cpu_context.hpp:314-318 calls it (one workgroup, as cuda_context.hpp:954-995).
template<typename T> struct complex_pair { T re, im; };

template<typename T>
__global__ void __launch_bounds__(1024)
max_modulus_kernel(const complex_pair<T> *__restrict__ in, const unsigned long long n, complex_pair<T> *__restrict__ result) {
    T best = -1;
    unsigned long long where = n;
    for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x) {
        const T modulus = sizeof(T) == 8 ? static_cast<T> (hypot(static_cast<double> (in[i].re), static_cast<double> (in[i].im)))
                                         : static_cast<T> (hypotf(static_cast<float> (in[i].re), static_cast<float> (in[i].im)));
        if (modulus > best) {                          // strictly greater: the first of equals stays
            best = modulus;
            where = i;
        }
    }
    __shared__ T moduli[1024];
    __shared__ unsigned long long places[1024];
    moduli[threadIdx.x] = best;
    places[threadIdx.x] = where;
    __syncthreads();
    for (unsigned int half = 512; half > 0; half >>= 1) {
        if (threadIdx.x < half) {
            const T other = moduli[threadIdx.x + half];
            const unsigned long long place = places[threadIdx.x + half];
            if (other > moduli[threadIdx.x] || (other == moduli[threadIdx.x] && place < places[threadIdx.x])) {
                moduli[threadIdx.x] = other;
                places[threadIdx.x] = place;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
//  std::max_element keeps element 0 when every comparison is false: all moduli NaN, or the modulus of
//  element 0 a NaN whatever follows (`abs(in[0]) < abs(x)` is never true) — as first_is_nan above.
        const T first = sizeof(T) == 8 ? static_cast<T> (hypot(static_cast<double> (in[0].re), static_cast<double> (in[0].im)))
                                       : static_cast<T> (hypotf(static_cast<float> (in[0].re), static_cast<float> (in[0].im)));
        *result = in[places[0] < n && first == first ? places[0] : 0];
    }
}

void launch_max_modulus(const void *in, const size_t n, const bool f64, void *result, hipStream_t stream) {
    if (f64) {
        hipLaunchKernelGGL(max_modulus_kernel<double>, dim3(1), dim3(1024), 0, stream,
                           static_cast<const complex_pair<double> *> (in), static_cast<unsigned long long> (n),
                           static_cast<complex_pair<double> *> (result));
    } else {
        hipLaunchKernelGGL(max_modulus_kernel<float>, dim3(1), dim3(1024), 0, stream,
                           static_cast<const complex_pair<float> *> (in), static_cast<unsigned long long> (n),
                           static_cast<complex_pair<float> *> (result));
    }
}

void launch_max_reduce(const void *in, const size_t n, const bool f64,
                       unsigned long long *result, const unsigned int num_cus, hipStream_t stream) {
    const unsigned int block = 256;
    const uintptr_t address = reinterpret_cast<uintptr_t> (in);
    const size_t element = f64 ? 8 : 4;
    size_t head = ((16 - address%16)%16)/element;
    if (head > n) head = n;
    unsigned long long want = (n/2 + block - 1)/block;
    if (want < 1) want = 1;
//  One atomicMax per workgroup lands on one address (~11 ns each, serialised): keep the grid
//  at one workgroup per CU and let the lanes stride (24 us -> 4 us for 1e6 doubles).
    const unsigned long long cap = static_cast<unsigned long long> (num_cus);
    const unsigned int grid = static_cast<unsigned int> (want < cap ? want : cap);
    if (f64) {
        hipLaunchKernelGGL(max_reduce_kernel<double>, dim3(grid), dim3(block), 0, stream,
                           static_cast<const double *> (in), static_cast<unsigned long long> (n),
                           static_cast<unsigned int> (head), result);
    } else {
        hipLaunchKernelGGL(max_reduce_kernel<float>, dim3(grid), dim3(block), 0, stream,
                           static_cast<const float *> (in), static_cast<unsigned long long> (n),
                           static_cast<unsigned int> (head), result);
    }
}

}  // namespace gfhip
