//  The converge loop of csrc/converge_state.hpp on scripted maxima, on the host alone (tests/test_converge_step.py
//  builds this with -fsanitize=address,undefined and holds what it prints to tests/max_model.py).
//
//  One case per line of standard input, every number as the hexadecimal bits of its type:
//      <type> <tolerance: double> <limit: decimal> loop      <maximum> ...      type f32 f64 c32 c64 (complex: re im re im ...)
//      <type> <tolerance: double> <limit: decimal> decide <N> <maximum> ...     type f32 f64; N maxima per launch
//      <type> keys <value> ...                                                   type f32 f64
//  and one line of output per case:
//      loop:    iterations, bits of the last maximum (re im), maxima consumed
//      decide:  iterations, bits of the last maximum, maxima consumed, passes, batch_passes, extra,
//               1 if every slot was left zero after every launch, 1 if a further decide changed neither state nor slots
//      keys:    <key>:<bits of from_ordered_key(key)> per value
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../graph_framework_amd/csrc/converge_state.hpp"

template<typename T> struct bits_of;
template<> struct bits_of<float> { typedef uint32_t type; };
template<> struct bits_of<double> { typedef uint64_t type; };

template<typename T>
static T value_of(const uint64_t bits) {
    return __builtin_bit_cast(T, static_cast<typename bits_of<T>::type> (bits));
}
template<typename T>
static uint64_t bits(const T value) {
    return __builtin_bit_cast(typename bits_of<T>::type, value);
}

template<typename B>
static void take(const std::vector<uint64_t> &script, size_t &at, B &max) {
    max = value_of<B> (script.at(at++));
}
template<typename B>
static void take(const std::vector<uint64_t> &script, size_t &at, std::complex<B> &max) {
    const B re = value_of<B> (script.at(at++));
    max = std::complex<B> (re, value_of<B> (script.at(at++)));
}
template<typename B>
static void print(const B max) {
    std::printf(" %" PRIx64, bits(max));
}
template<typename B>
static void print(const std::complex<B> max) {
    std::printf(" %" PRIx64 " %" PRIx64, bits(max.real()), bits(max.imag()));
}

//  The host loop of gf_hip.cpp: one maximum per pass until the step says stop.
template<typename V>
static void loop(const double tolerance, const unsigned long long limit, const std::vector<uint64_t> &script) {
    gfhip::converge_step<V> step(tolerance, limit);
    size_t at = 0, passes = 0;
    V max;
    do {
        take(script, at, max);
        passes++;
    } while (step.advance(max));
    std::printf("%llu", step.iterations);
    print(max);
    std::printf(" %zu\n", passes);
}

//  converge_on_device without the device: launches of `count` passes, the key of each maximum where the reduction
//  leaves it — for a NaN the all-ones key it plants — and the decide of the launch that follows.
template<typename T>
static void decide(const double tolerance, const unsigned long long limit, const unsigned int count,
                   const std::vector<uint64_t> &script) {
    const unsigned long long nan_key = ~0ull >> (sizeof(T) == 8 ? 0 : 32);
    gfhip::converge_state state = gfhip::converge_begin<T> (tolerance, limit);
    std::vector<unsigned long long> reduced(count, 0ull);
    size_t at = 0;
    bool cleared = true;
    while (!state.done) {
        for (unsigned int pass = 0; pass < count; pass++) {
            const T max = value_of<T> (script.at(at++));
            reduced[pass] = max != max ? nan_key : gfhip::ordered_key(max);
        }
        gfhip::decide<T> (state, reduced.data(), count);
        for (const unsigned long long slot : reduced) cleared = cleared && slot == 0ull;
    }
    const gfhip::converge_state before = state;
    const std::vector<unsigned long long> planted(count, gfhip::ordered_key(static_cast<T> (3)));
    reduced = planted;
    gfhip::decide<T> (state, reduced.data(), count);
    const bool idle = !std::memcmp(&before, &state, sizeof(state)) && reduced == planted;
    std::printf("%llu", state.iterations);
    print(static_cast<T> (state.max_residual));
    std::printf(" %zu %u %u %u %d %d\n", at, state.passes, state.batch_passes, state.extra, cleared ? 1 : 0, idle ? 1 : 0);
}

template<typename T>
static void keys(const std::vector<uint64_t> &values) {
    for (const uint64_t v : values) {
        const unsigned long long key = gfhip::ordered_key(value_of<T> (v));
        std::printf("%llx:%" PRIx64 " ", key, bits(gfhip::from_ordered_key<T> (key)));
    }
    std::printf("\n");
}

static std::vector<uint64_t> rest(std::istringstream &in) {
    std::vector<uint64_t> out;
    std::string word;
    while (in >> word) out.push_back(std::stoull(word, nullptr, 16));
    return out;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string type, word, mode;
        in >> type >> word;
        if (word == "keys") {
            if (type == "f32") keys<float> (rest(in)); else if (type == "f64") keys<double> (rest(in)); else return 2;
            continue;
        }
        const double tolerance = value_of<double> (std::stoull(word, nullptr, 16));
        unsigned long long limit;
        in >> limit >> mode;
        if (mode == "loop") {
            const std::vector<uint64_t> script = rest(in);
            if (type == "f32") loop<float> (tolerance, limit, script);
            else if (type == "f64") loop<double> (tolerance, limit, script);
            else if (type == "c32") loop<std::complex<float>> (tolerance, limit, script);
            else if (type == "c64") loop<std::complex<double>> (tolerance, limit, script);
            else return 2;
        } else if (mode == "decide") {
            unsigned int count;
            in >> count;
            const std::vector<uint64_t> script = rest(in);
            if (count < 1) return 2;
            if (type == "f32") decide<float> (tolerance, limit, count, script);
            else if (type == "f64") decide<double> (tolerance, limit, count, script);
            else return 2;
        } else {
            return 2;
        }
    }
    return 0;
}
