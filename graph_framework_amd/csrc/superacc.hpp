//------------------------------------------------------------------------------
///  @file superacc.hpp
///  @brief Exact sums of doubles on an integer superaccumulator, host and device.
///
///  A sum is 67 signed 64-bit limbs (536 B); limb k has weight 2^(32k - 1074), so limb 0 counts
///  units of the smallest subnormal and limbs 0-65 span every finite double.  A deposit splits the
///  shifted significand into three 32-bit chunks and adds them to three adjacent limbs without
///  carrying (carry-save): integer addition is associative, so the limbs do not depend on the
///  order of arrival, and a limb takes 2^31 deposits before it could overflow.  normalise() makes
///  the state canonical (base-2^32 two's-complement digits), round() gives the correctly rounded
///  double of the exact sum (nearest, ties to even).  Plain C++: the same functions run in
///  deposition.hip's kernels and in gfhip_exact_sum on the host.
//------------------------------------------------------------------------------
#ifndef GFHIP_SUPERACC_HPP
#define GFHIP_SUPERACC_HPP

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GFHIP_HD __host__ __device__ inline
#else
#define GFHIP_HD inline
#endif

namespace gfhip {
namespace superacc {

constexpr int limbs = 67;
//  Deposits a limb takes between two normalise() calls with room to spare: 2^30 chunks below 2^32 on top of a
//  canonical digit stay below 2^63.
constexpr uint64_t deposits_per_normalise = 1ull << 30;

//  What a finite double adds: `chunk[j]` to limb `first + j` (first <= 63), negated when `negative`.
struct pieces {
    uint32_t chunk[3];
    int first;
    bool negative;
};

GFHIP_HD uint64_t bits_of(const double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return b;
}

GFHIP_HD bool is_finite(const double v) {
    return ((bits_of(v) >> 52) & 0x7ffull) != 0x7ffull;
}

//  v = +-m 2^(s - 1074) with m the 53-bit significand (52 bits and no hidden one for a subnormal) and
//  s = max(biased exponent, 1) - 1; the 85-bit m << (s%32) in three 32-bit chunks from limb s/32 on.
GFHIP_HD pieces split(const double v) {
    const uint64_t b = bits_of(v);
    const unsigned int e = static_cast<unsigned int> ((b >> 52) & 0x7ffull);
    uint64_t m = b & 0xfffffffffffffull;
    if (e) m |= 1ull << 52;
    const unsigned int s = (e ? e : 1u) - 1u;
    const unsigned int r = s%32u;
    const uint64_t low = m << r;
    const uint64_t high = r ? m >> (64u - r) : 0ull;
    pieces p;
    p.chunk[0] = static_cast<uint32_t> (low);
    p.chunk[1] = static_cast<uint32_t> (low >> 32);
    p.chunk[2] = static_cast<uint32_t> (high);
    p.first = static_cast<int> (s/32u);
    p.negative = (b >> 63) != 0;
    return p;
}

//  Add one finite double (the caller has checked is_finite).
GFHIP_HD void deposit(int64_t *acc, const double v) {
    const pieces p = split(v);
    for (int j = 0; j < 3; j++) {
        const int64_t c = static_cast<int64_t> (p.chunk[j]);
        acc[p.first + j] += p.negative ? -c : c;
    }
}

//  Carries from low to high: limbs 0-65 become digits in [0, 2^32), limb 66 takes what is left, signed: 0 or -1
//  (the sign) for every sum below 2^1038 in magnitude.  The digits of a number are unique, so two canonical
//  states of the same multiset of samples are byte-identical.
GFHIP_HD void normalise(int64_t *acc) {
    int64_t carry = 0;
    for (int k = 0; k < limbs - 1; k++) {
        const int64_t t = acc[k] + carry;
        acc[k] = t & 0xffffffffll;
        carry = t >> 32;                               // arithmetic shift
    }
    acc[limbs - 1] += carry;
}

//  The correctly rounded double of a CANONICAL state: exact with 53 significant bits or fewer (every subnormal
//  result), else nearest with ties to even; +-inf past DBL_MAX; an exact zero is +0.0.
GFHIP_HD double round(const int64_t *acc) {
    constexpr int digits = limbs + 1;                  // 68 of 32 bits: limbs 0-65 and the two halves of limb 66
    uint32_t mag[digits];
    const bool negative = acc[limbs - 1] < 0;
    uint64_t carry = negative ? 1u : 0u;
    for (int k = 0; k < limbs - 1; k++) {
        const uint32_t d = static_cast<uint32_t> (acc[k]);
        const uint64_t t = static_cast<uint64_t> (negative ? ~d : d) + carry;
        mag[k] = static_cast<uint32_t> (t);
        carry = t >> 32;
    }
    const uint64_t top = (negative ? ~static_cast<uint64_t> (acc[limbs - 1]) : static_cast<uint64_t> (acc[limbs - 1])) + carry;
    mag[digits - 2] = static_cast<uint32_t> (top);
    mag[digits - 1] = static_cast<uint32_t> (top >> 32);

    int lead = digits - 1;
    while (lead >= 0 && mag[lead] == 0) lead--;
    if (lead < 0) return 0.0;
    int width = 0;                                     // significant bits of the leading digit
    for (uint32_t d = mag[lead]; d; d >>= 1) width++;
    const int length = 32*lead + width;                // bits of the magnitude, in units of 2^-1074
    const uint64_t sign = negative ? 1ull << 63 : 0ull;
    uint64_t result;
    if (length <= 53) {
//  m 2^-1074 with m < 2^53: the bit pattern of that double is m itself (subnormal, or biased exponent 1).
        result = static_cast<uint64_t> (mag[0]) | (static_cast<uint64_t> (mag[1]) << 32);
    } else {
        const int shift = length - 53;                 // bits below the 53 kept
        const int word = shift/32, offset = shift%32;
        uint64_t q = (static_cast<uint64_t> (mag[word]) | (static_cast<uint64_t> (word + 1 < digits ? mag[word + 1] : 0u) << 32)) >> offset;
        if (offset && word + 2 < digits) q |= static_cast<uint64_t> (mag[word + 2]) << (64 - offset);
        q &= (1ull << 53) - 1ull;
        const int guard_at = shift - 1;
        const bool guard = (mag[guard_at/32] >> (guard_at%32)) & 1u;
        bool sticky = (mag[guard_at/32] & ((1u << (guard_at%32)) - 1u)) != 0;
        for (int k = 0; k < guard_at/32; k++) sticky = sticky || mag[k] != 0;
        int exponent = shift + 1;                      // q 2^(shift - 1074) = q 2^(exponent - 1075)
        if (guard && (sticky || (q & 1ull))) {
            q++;
            if (q == 1ull << 53) {
                q >>= 1;
                exponent++;
            }
        }
        result = exponent >= 2047 ? 0x7ffull << 52 : (static_cast<uint64_t> (exponent) << 52) | (q & 0xfffffffffffffull);
    }
    result |= sign;
    double value;
    memcpy(&value, &result, 8);
    return value;
}

}  // namespace superacc
}  // namespace gfhip

#endif
