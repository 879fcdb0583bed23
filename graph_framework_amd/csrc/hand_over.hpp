//------------------------------------------------------------------------------
///  @file hand_over.hpp
///  @brief What gfhip_hand_over (gf_hip.cpp) passes to the hand-over kernel (hand_over.hip).
//------------------------------------------------------------------------------
#ifndef GFHIP_HAND_OVER_HPP
#define GFHIP_HAND_OVER_HPP

#include <stddef.h>
#include <stdint.h>

namespace gfhip {

//  One array to move.  `count` elements of the SOURCE's type; words are the 4 or 8 bytes of the base type.
struct hand_over_slot {
    void *to;
    const void *from;
    unsigned long long count;
    unsigned int mode;              // hand_over_mode bits
    unsigned int reserved;
};

enum hand_over_mode : unsigned int {
    hand_over_copy = 0,             // same type on both sides
    hand_over_widen = 1,            // real -> complex: (value, +0.0)
    hand_over_part = 2,             // complex -> real: the real or the imaginary parts
    hand_over_kind = 3,             // mask of the three above
    hand_over_wide = 4,             // words of 8 bytes (f64, c64), else of 4 (f32, c32)
    hand_over_complex = 8,          // copy only: an element is two words
    hand_over_imaginary = 16,       // part only: the second word of each element
    hand_over_vector = 32           // the pointers allow the 16-byte path (hand_over_vector_ok)
};

constexpr unsigned int hand_over_table_size = 16;

//  The kernel's by-value argument: 512 bytes of the kernel-argument segment.
struct hand_over_table {
    hand_over_slot slot[hand_over_table_size];
};

//  Whether the 16-byte path may be taken for these pointers.  Buffers the context allocates are 256-byte aligned;
//  adopted ones (gfhip_set_buffer) are only element aligned.  The path reads the source in pieces of 16 bytes (8 when
//  widening) and writes the destination in pieces of 16.
inline bool hand_over_vector_ok(const unsigned int mode, const void *to, const void *from) {
    const uintptr_t t = reinterpret_cast<uintptr_t> (to), f = reinterpret_cast<uintptr_t> (from);
    const uintptr_t source = (mode & hand_over_kind) == hand_over_widen ? 8 : 16;
    return t%16 == 0 && f%source == 0;
}

//  Lanes that have work in the slot, tail included: what the grid is sized by.
inline unsigned long long hand_over_lanes(const hand_over_slot &s) {
    const unsigned int kind = s.mode & hand_over_kind;
    const bool wide = s.mode & hand_over_wide;
    if (!(s.mode & hand_over_vector)) {
        return kind == hand_over_copy && (s.mode & hand_over_complex) ? 2*s.count : s.count;
    }
    if (kind == hand_over_copy) {
        const unsigned long long bytes = s.count*(wide ? 8u : 4u)*(s.mode & hand_over_complex ? 2u : 1u);
        return bytes/16 > 3 ? bytes/16 : 3;
    }
    if (kind == hand_over_widen) return wide ? s.count : s.count/2 + 1;
    return wide ? s.count/2 + 1 : s.count/4 + 3;
}

//  hand_over.hip: one launch for `used` slots, on `stream`.
void launch_hand_over(const hand_over_table &table, const unsigned int used, const unsigned int num_cus, void *stream);

}  // namespace gfhip

#endif
