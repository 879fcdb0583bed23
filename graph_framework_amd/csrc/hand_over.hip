//------------------------------------------------------------------------------
///  @file hand_over.hip
///  @brief Arrays handed from one context's buffers to another's in one launch (hand-written, gfx950).
///
///  gfhip_hand_over (include/gf_hip.h): element i of every source goes to element i of its destination,
///  as it is, as the real part of a complex element whose imaginary part is +0.0, or as one part of a
///  complex source.  Values move as words of 4 or 8 bytes, never through a floating-point instruction:
///  NaN payloads, signed zeros and subnormals arrive bit for bit.
///
///  A streaming kernel: blockIdx.y selects the array (the pointer table is the kernel's by-value
///  argument, read with scalar loads), the lanes stride over it in x.  Where the pointers allow it
///  (hand_over_vector_ok, decided per array on the host) every lane stores 16 bytes: a copy moves 16 B per
///  lane, a widening lane reads 8 B and writes 16 B, a lane that takes parts reads 32 B and writes 16 B;
///  the few elements that do not fill 16 bytes go word by word through the first lanes.  Otherwise
///  every access is one word, which only needs the alignment of an element.
//------------------------------------------------------------------------------
#include <hip/hip_runtime.h>

#include "hand_over.hpp"

namespace gfhip {

namespace {

constexpr unsigned int hand_over_block = 256;

typedef unsigned int u32;
typedef unsigned long long u64;
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

//  Word by word: W is the base type's width.
template<typename W>
__device__ __forceinline__ void by_word(const hand_over_slot &s, const u64 first, const u64 stride) {
    W *to = static_cast<W *> (s.to);
    const W *from = static_cast<const W *> (s.from);
    const unsigned int kind = s.mode & hand_over_kind;
    if (kind == hand_over_copy) {
        const u64 words = s.mode & hand_over_complex ? 2*s.count : s.count;
        for (u64 i = first; i < words; i += stride) to[i] = from[i];
    } else if (kind == hand_over_widen) {
        for (u64 i = first; i < s.count; i += stride) {
            to[2*i] = from[i];
            to[2*i + 1] = 0;
        }
    } else {
        const u64 part = s.mode & hand_over_imaginary ? 1 : 0;
        for (u64 i = first; i < s.count; i += stride) to[i] = from[2*i + part];
    }
}

//  16 bytes stored per lane; the words past the last full 16 bytes through the first lanes.
__device__ __forceinline__ void by_vector(const hand_over_slot &s, const u64 first, const u64 stride) {
    const unsigned int kind = s.mode & hand_over_kind;
    const bool wide = s.mode & hand_over_wide;
    const u64 n = s.count;
    if (kind == hand_over_copy) {
        const u64 words = n*(wide ? 2u : 1u)*(s.mode & hand_over_complex ? 2u : 1u);       // of 4 bytes
        const u64 full = words/4;
        u32x4 *to = static_cast<u32x4 *> (s.to);
        const u32x4 *from = static_cast<const u32x4 *> (s.from);
        for (u64 i = first; i < full; i += stride) to[i] = from[i];
        if (first < words - 4*full) {
            static_cast<u32 *> (s.to)[4*full + first] = static_cast<const u32 *> (s.from)[4*full + first];
        }
    } else if (kind == hand_over_widen && wide) {
        u64x2 *to = static_cast<u64x2 *> (s.to);
        const u64 *from = static_cast<const u64 *> (s.from);
        for (u64 i = first; i < n; i += stride) {
            u64x2 v;
            v.x = from[i];
            v.y = 0;
            to[i] = v;
        }
    } else if (kind == hand_over_widen) {
        const u64 full = n/2;
        u32x4 *to = static_cast<u32x4 *> (s.to);
        const u32x2 *from = static_cast<const u32x2 *> (s.from);
        for (u64 i = first; i < full; i += stride) {
            const u32x2 a = from[i];
            u32x4 v;
            v.x = a.x;
            v.y = 0;
            v.z = a.y;
            v.w = 0;
            to[i] = v;
        }
        if (first == 0 && (n & 1)) {
            u32x2 v;
            v.x = static_cast<const u32 *> (s.from)[n - 1];
            v.y = 0;
            static_cast<u32x2 *> (s.to)[n - 1] = v;          // a complex element is 8-byte aligned
        }
    } else if (wide) {
        const bool imaginary = s.mode & hand_over_imaginary;
        const u64 full = n/2;
        u64x2 *to = static_cast<u64x2 *> (s.to);
        const u64x2 *from = static_cast<const u64x2 *> (s.from);
        for (u64 i = first; i < full; i += stride) {
            const u64x2 a = from[2*i], b = from[2*i + 1];
            u64x2 v;
            v.x = imaginary ? a.y : a.x;
            v.y = imaginary ? b.y : b.x;
            to[i] = v;
        }
        if (first == 0 && (n & 1)) {
            static_cast<u64 *> (s.to)[n - 1] = static_cast<const u64 *> (s.from)[2*(n - 1) + (imaginary ? 1 : 0)];
        }
    } else {
        const bool imaginary = s.mode & hand_over_imaginary;
        const u64 full = n/4;
        u32x4 *to = static_cast<u32x4 *> (s.to);
        const u32x4 *from = static_cast<const u32x4 *> (s.from);
        for (u64 i = first; i < full; i += stride) {
            const u32x4 a = from[2*i], b = from[2*i + 1];
            u32x4 v;
            v.x = imaginary ? a.y : a.x;
            v.y = imaginary ? a.w : a.z;
            v.z = imaginary ? b.y : b.x;
            v.w = imaginary ? b.w : b.z;
            to[i] = v;
        }
        if (first < n - 4*full) {
            const u64 e = 4*full + first;
            static_cast<u32 *> (s.to)[e] = static_cast<const u32 *> (s.from)[2*e + (imaginary ? 1 : 0)];
        }
    }
}

__global__ void __launch_bounds__(hand_over_block)
hand_over_kernel(const hand_over_table table) {
    const hand_over_slot &s = table.slot[blockIdx.y];
    const u64 first = static_cast<u64> (blockIdx.x)*hand_over_block + threadIdx.x;
    const u64 stride = static_cast<u64> (gridDim.x)*hand_over_block;
    if (s.mode & hand_over_vector) {
        by_vector(s, first, stride);
    } else if (s.mode & hand_over_wide) {
        by_word<u64> (s, first, stride);
    } else {
        by_word<u32> (s, first, stride);
    }
}

}  // namespace

void launch_hand_over(const hand_over_table &table, const unsigned int used, const unsigned int num_cus, void *stream) {
    unsigned long long lanes = 0;
    for (unsigned int e = 0; e < used; e++) {
        const unsigned long long wanted = hand_over_lanes(table.slot[e]);
        if (wanted > lanes) lanes = wanted;
    }
    if (used == 0 || lanes == 0) return;
//  A few workgroups per CU over all arrays, the lanes stride over the rest.
    const unsigned long long want = (lanes + hand_over_block - 1)/hand_over_block;
    const unsigned long long cap = (static_cast<unsigned long long> (num_cus)*8u + used - 1)/used;
    const unsigned int grid = static_cast<unsigned int> (want < cap ? want : cap);
    hipLaunchKernelGGL(hand_over_kernel, dim3(grid, used), dim3(hand_over_block), 0, static_cast<hipStream_t> (stream), table);
}

}  // namespace gfhip
