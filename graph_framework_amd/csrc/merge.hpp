//------------------------------------------------------------------------------
///  @file merge.hpp
///  @brief Merge records of a work item that provably hold the same bits.
///
///  GFIR arrives as leaf_node::compile() recursed: a sub-expression that the graph builds twice is two
///  records, and pow(x, 3) recomputes the x*x that pow(x, 2) of the same x already holds.  The RK4 step is
///  bound by the NUMBER of vector instructions, so every such record is time.
///
///  One linear pass gives every record a value number: two records share one when they have the same
///  operation, the same `aux` and immediates where the operation reads them, and operands with the same
///  value numbers.  powi(x, p) is numbered as the product the lowering computes, mul(powi(x, p - 1), x) with
///  powi(x, 2) = mul(x, x), so that a power shares with its prefix and with plain mul records.  Nothing here
///  is "equal except at ...": operand order is kept (x + y and y + x differ in the payload of a NaN), no
///  factor is moved, no reciprocal derived.
///
///  What the pass does with equal records:
///    * add, sub, mul, fma, div, powi: a later record is MERGED into the earliest one (its representative).
///      Every use — operands, setters, outputs — is redirected to the representative; the merged record stays
///      in place as a dead copy of it, marked in item::merged_into.  The record count is unchanged, the
///      serialized item is an ordinary item, and the writers emit a merged record as a name for its
///      representative (`const real rJ = rI;`, `; alias rJ = rI`) instead of instructions;
///    * powi(x, p), p >= 3, whose prefix powi(x, p - 1) is an earlier record becomes mul(prefix, x);
///    * constants, inputs and gathers only share their value number (they cost nothing: gathers of one cell are
///      one load through the writers' own cell aliases), and so do sqrt and pow: their sequences join the window
///      check, one per record, and the lowering's tests count them (tests/test_cabi.py) — merging the RK4 step's
///      3 duplicate square roots is left to a change that may touch those counts.
///  Complex, SAFE_MATH, random and index items are left alone.
///
///  LEVEL 1 (options.hpp, `level`; only the assembly statement of asm_body.hpp is written from it) also merges what is equal
///  for every operand that is not a NaN, because every lane that stores a NaN is computed again by the redo launch
///  (DESIGN.md section 3):
///    * add, mul and the product of fma are numbered with their operands sorted (x + y and y + x);
///    * mul(-1.0, x) is numbered as neg(x): twins merge whatever side the constant is on, and neg(neg(x)) is x;
///    * sqrt and pow records are merged like the others.
///  At level 0 the pass is exactly what it was.
//------------------------------------------------------------------------------
#ifndef gfhip_merge_hpp
#define gfhip_merge_hpp

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "gfir_item.hpp"

namespace gfhip {

struct merge_report {
    size_t add = 0, sub = 0, mul = 0, fma = 0, div = 0, powi = 0;      ///< merged records per operation
    size_t sqrt = 0, pow = 0;                                           ///< level 1: merged square roots and pow records
    size_t commuted = 0, negations = 0;                                 ///< level 1: merges found only by sorting operands / numbering neg
    size_t prefixes = 0;                                                ///< powi records that became mul(prefix, x)
    size_t instructions = 0;                                            ///< vector instructions of the assembly body they no longer cost
    std::vector<std::pair<uint32_t, uint32_t>> merged;                  ///< (record, its representative)
    std::vector<std::pair<uint32_t, uint32_t>> prefixed;                ///< (powi record, the record of its prefix)

    size_t records() const { return add + sub + mul + fma + div + powi + sqrt + pow; }
    void print(FILE *out, const std::string &name) const {
        std::fprintf(out, "merge of %s: %zu records merged (add %zu, sub %zu, mul %zu, fma %zu, div %zu, powi %zu), %zu powi prefixes, "
                          "%zu vector instructions\n", name.c_str(), records(), add, sub, mul, fma, div, powi, prefixes, instructions);
        if (sqrt + pow + commuted + negations) {
            std::fprintf(out, "  level 1: %zu sqrt and %zu pow records merged, %zu merges by sorted operands, %zu by neg numbering\n",
                         sqrt, pow, commuted, negations);
        }
        for (auto &m : merged) std::fprintf(out, "  merged r%u into r%u\n", m.first, m.second);
        for (auto &p : prefixed) std::fprintf(out, "  powi r%u from its prefix r%u\n", p.first, p.second);
    }
};

inline bool can_merge(const item &it) {
    if (it.is_complex() || it.safe_math() || it.has_random()) return false;
    for (auto &c : it.code) {
        if (c.op == GFIR_INDEX1 || c.op == GFIR_INDEX2) return false;
    }
    return true;
}

///  @param[in] level 0: bit-equal records only; 1: also records equal for every operand that is not a NaN (see above).
///  An item that went through level 0 may go through level 1 afterwards: its dead copies are found again.
inline item merge_records(const item &in, merge_report *report = nullptr, const uint32_t level = 0) {
    if (!can_merge(in)) return in;
    const size_t n = in.code.size();

    struct key {
        uint32_t op, a, b, c, aux;
        uint64_t imm[4];
        bool operator==(const key &o) const {
            return op == o.op && a == o.a && b == o.b && c == o.c && aux == o.aux && std::memcmp(imm, o.imm, sizeof(imm)) == 0;
        }
    };
    struct key_hash {
        size_t operator()(const key &k) const {
            uint64_t h = 1469598103934665603ull;
            auto mix = [&h] (const uint64_t v) { h = (h ^ v)*1099511628211ull; h ^= h >> 29; };
            mix(k.op); mix(k.a); mix(k.b); mix(k.c); mix(k.aux);
            for (const uint64_t v : k.imm) mix(v);
            return static_cast<size_t> (h);
        }
    };
    std::unordered_map<key, uint32_t, key_hash> numbers;
    numbers.reserve(2*n);
    std::vector<uint32_t> holder;                       // value number -> earliest record that computes it (GFIR_NONE: a prefix no record holds)
    auto number_of = [&] (const key &k) -> uint32_t {
        auto found = numbers.find(k);
        if (found != numbers.end()) return found->second;
        holder.push_back(GFIR_NONE);
        numbers.insert({k, static_cast<uint32_t> (holder.size() - 1)});
        return static_cast<uint32_t> (holder.size() - 1);
    };
    auto plain = [] (const uint32_t op, const uint32_t a, const uint32_t b = GFIR_NONE, const uint32_t c = GFIR_NONE, const uint32_t aux = 0) {
        key k;
        k.op = op; k.a = a; k.b = b; k.c = c; k.aux = aux;
        std::memset(k.imm, 0, sizeof(k.imm));
        return k;
    };

    item out = in;
    constexpr uint32_t neg_op = 0xffff0001u;            // level 1: the key of neg(x); no record has this operation
    std::vector<uint32_t> negates;                      // value number -> the value number it is the negative of
    std::vector<std::pair<uint32_t, uint32_t>> written;  // value number -> the operands of its holder in the order the item has them
    auto minus_one = [&out] (const uint32_t record) {
        const gfir_instruction &k = out.code[record];
        return k.op == GFIR_CONST && k.imm[0] == -1.0 && k.imm[1] == 0.0;
    };

    std::vector<uint32_t> value(n, GFIR_NONE);          // record -> value number
    std::vector<uint32_t> stands(n);                    // record -> the record its users read
    std::vector<uint32_t> merged_into(n, GFIR_NONE);
    merge_report counts;
    for (size_t i = 0; i < n; i++) {
        gfir_instruction &c = out.code[i];
        stands[i] = static_cast<uint32_t> (i);
        const int operands = operand_count(c.op);
        uint32_t va = GFIR_NONE, vb = GFIR_NONE, vc = GFIR_NONE;
        if (operands > 0) { va = value[c.a]; c.a = stands[c.a]; }
        if (operands > 1) { vb = value[c.b]; c.b = stands[c.b]; }
        if (operands > 2) { vc = value[c.c]; c.c = stands[c.c]; }
        bool mergeable = false;
        int found_by = 0;                               // level 1: what finds a twin that level 0 does not: 1 = the sorted operands, 2 = neg(x)
        uint32_t id, prefix = GFIR_NONE;
        switch (c.op) {
            case GFIR_CONST: {
                key k = plain(c.op, GFIR_NONE);
                std::memcpy(k.imm, c.imm, 2*sizeof(uint64_t));
                id = number_of(k);
                break;
            }
            case GFIR_INPUT:
                id = number_of(plain(c.op, c.a));
                break;
            case GFIR_GATHER1: case GFIR_GATHER2: {
                key k = plain(c.op, va, vb, GFIR_NONE, c.aux);
                std::memcpy(k.imm, c.imm, sizeof(k.imm));
                id = number_of(k);
                break;
            }
            case GFIR_POWI:
                if (c.aux < 2) {
                    id = number_of(plain(c.op, va, GFIR_NONE, GFIR_NONE, c.aux));
                    break;
                }
                id = number_of(plain(GFIR_MUL, va, va));
                for (uint32_t p = 3; p <= c.aux; p++) {
                    prefix = id;
                    id = number_of(plain(GFIR_MUL, prefix, va));
                }
                mergeable = true;
                break;
            case GFIR_ADD: case GFIR_SUB: case GFIR_MUL: case GFIR_DIV: case GFIR_FMA: {
                mergeable = true;
                if (level == 0) {
                    id = number_of(plain(c.op, va, vb, vc));
                    break;
                }
                if (c.op == GFIR_MUL && (minus_one(c.a) != minus_one(c.b))) {
                    const uint32_t x = minus_one(c.a) ? vb : va;
                    if (x < negates.size() && negates[x] != GFIR_NONE) {
                        id = negates[x];
                    } else {
                        id = number_of(plain(neg_op, x));
                        negates.resize(holder.size(), GFIR_NONE);
                        negates[id] = x;
                    }
                    found_by = 2;
                    break;
                }
                const bool sorted = c.op != GFIR_SUB && c.op != GFIR_DIV && vb < va;
                id = number_of(sorted ? plain(c.op, vb, va, vc) : plain(c.op, va, vb, vc));
                found_by = 1;
                break;
            }
            case GFIR_SQRT: case GFIR_POW:
                mergeable = level >= 1;
                id = number_of(plain(c.op, va, vb, vc));
                break;
            default:
                id = number_of(plain(c.op, va, vb, vc));
        }
        value[i] = id;
        if (found_by) {
            written.resize(holder.size(), {GFIR_NONE, GFIR_NONE});
            if (holder[id] != GFIR_NONE && written[id] == std::make_pair(va, vb)) found_by = 0;
            if (holder[id] == GFIR_NONE) written[id] = {va, vb};
        }
        if (holder[id] == GFIR_NONE) {
            holder[id] = static_cast<uint32_t> (i);
            if (c.op == GFIR_POWI && prefix != GFIR_NONE && holder[prefix] != GFIR_NONE) {
//  (the holder of a product's value number is a mul or a powi record: never a merged one, never a constant)
                counts.prefixes++;
                counts.instructions += c.aux - 2;
                counts.prefixed.push_back({static_cast<uint32_t> (i), holder[prefix]});
                c.op = GFIR_MUL;
                c.b = c.a;
                c.a = holder[prefix];
                c.aux = 0;
            }
            continue;
        }
        if (!mergeable) continue;
        const uint32_t first = holder[id];
        if (level >= 1 && in.is_merged(i)) {
//  (a dead copy of the level-0 pass found again: counted there)
        } else switch (c.op) {
            case GFIR_ADD: counts.add++; counts.instructions += 1; break;
            case GFIR_SUB: counts.sub++; counts.instructions += 1; break;
            case GFIR_MUL: counts.mul++; counts.instructions += 1; break;
            case GFIR_FMA: counts.fma++; counts.instructions += 1; break;
            case GFIR_DIV: counts.div++; counts.instructions += 3; break;
            case GFIR_SQRT: counts.sqrt++; counts.instructions += 11; break;
            case GFIR_POW: counts.pow++; counts.instructions += 20; break;
            default: counts.powi++; counts.instructions += c.aux - 1;
        }
        if (level >= 1 && !in.is_merged(i)) {
            counts.commuted += found_by == 1;
            counts.negations += found_by == 2;
        }
        counts.merged.push_back({static_cast<uint32_t> (i), first});
        c = out.code[first];
        stands[i] = first;
        merged_into[i] = first;
    }
    for (auto &s : out.setters) s.value = stands[s.value];
    for (auto &o : out.outputs) o = stands[o];
    if (level == 0 ? counts.records() != 0 : !counts.merged.empty()) out.merged_into = merged_into;
    if (report) *report = counts;
    return out;
}

}  // namespace gfhip

#endif /* gfhip_merge_hpp */
