//------------------------------------------------------------------------------
///  @file schedule.hpp
///  @brief Re-order the records of a work item to lower register pressure.
///
///  Any topological order of the DAG computes the same IEEE values.  GFIR arrives
///  in the order leaf_node::compile() recurses (depth first, setters before
///  outputs), which keeps ~174 fp64 values alive at the peak of the RK4 item.
///  A greedy list schedule — always emit the ready node that frees the most
///  operands (an operand is freed when its last consumer is emitted), ties to
///  the node that became ready last (continue the chain just unblocked) —
///  reaches ~150, and the compiler's own scheduler does the rest: the RK4 step
///  drops from 0.242 to 0.223 ms (1e6 rays; AGPR copies 700 -> 540 of 7300
///  VALU instructions).  Tie-breaks tried on the GPU (FIFO, height, eight random
///  seeds, one unit of slack): all within 0.222..0.229 ms, so the deterministic
///  LIFO rule is kept.  The re-ordered item is a plain renumbering; the lowering
///  does not know about it.
//------------------------------------------------------------------------------
#ifndef gfhip_schedule_hpp
#define gfhip_schedule_hpp

#include <set>
#include <vector>

#include "gfir_item.hpp"

namespace gfhip {

///  Renumber the records of `in` so that record p of the result is record order[p].
inline item reorder(const item &in, const std::vector<uint32_t> &order) {
    const size_t n = in.code.size();
    std::vector<uint32_t> new_index(n, GFIR_NONE);
    for (size_t p = 0; p < order.size(); p++) new_index[order[p]] = static_cast<uint32_t> (p);
    item out = in;
    for (size_t p = 0; p < order.size(); p++) {
        gfir_instruction c = in.code[order[p]];
        const int count = operand_count(c.op);
        if (count > 0) c.a = new_index[c.a];
        if (count > 1) c.b = new_index[c.b];
        if (count > 2) c.c = new_index[c.c];
        out.code[p] = c;
    }
    for (auto &s : out.setters) s.value = new_index[s.value];
    for (auto &o : out.outputs) o = new_index[o];
    for (size_t p = 0; p < order.size() && !in.merged_into.empty(); p++) {
        out.merged_into[p] = in.is_merged(order[p]) ? new_index[in.merged_into[order[p]]] : GFIR_NONE;
    }
    return out;
}

///  How the list schedule breaks a tie (equal score, equal age).
struct tie_break {
    bool seeded = false;                ///< false: the lowest record; true: a pick of the generator below
    uint64_t state = 0;
    static tie_break lowest_record() { return tie_break(); }
    static tie_break from_seed(const uint32_t seed) { return {true, 0x9E3779B97F4A7C15ull*(seed + 1u)}; }
    size_t pick(const size_t candidates) {
        if (!seeded) return 0;
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);      // splitmix64: the same sequence on every platform
        z = (z ^ (z >> 30))*0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27))*0x94D049BB133111EBull;
        return static_cast<size_t> ((z ^ (z >> 31))%candidates);
    }
};

///  The greedy list schedule: the order of the records of `in`.  The peak number of live values varies by a factor of
///  TWO between tie-breaks on the RK4 item (the LDS slots its assembly body needs: 19 to 113 over a hundred seeds), which
///  is what asm_body.hpp's schedule_for_assembly searches.
inline std::vector<uint32_t> list_schedule(const item &in, tie_break ties) {
    const size_t n = in.code.size();
    std::vector<std::vector<uint32_t>> users(n);
    std::vector<uint32_t> pending(n, 0), consumers_left(n, 0);
    std::vector<bool> is_root(n, false);
    for (auto &s : in.setters) is_root[s.value] = true;
    for (auto o : in.outputs) is_root[o] = true;
//  The distinct operands of every record, once (the loop below looks at every ready record at every step).
    std::vector<uint32_t> distinct_operands(3*n, GFIR_NONE);
    std::vector<uint8_t> distinct_count(n, 0);
//  A merged record (merge.hpp) is a name for its representative: it reads nothing and follows it at once.
    std::vector<std::vector<uint32_t>> names(in.merged_into.empty() ? 0 : n);
    for (size_t i = 0; i < n; i++) {
        if (in.is_merged(i)) {
            names[in.merged_into[i]].push_back(static_cast<uint32_t> (i));
            pending[i] = 1;
            continue;
        }
        for (const uint32_t o : in.operands(i)) {
            bool seen = false;
            for (int j = 0; j < distinct_count[i]; j++) seen = seen || distinct_operands[3*i + j] == o;
            if (!seen) distinct_operands[3*i + distinct_count[i]++] = o;
        }
        pending[i] = distinct_count[i];
        for (int k = 0; k < distinct_count[i]; k++) {
            users[distinct_operands[3*i + k]].push_back(static_cast<uint32_t> (i));
            consumers_left[distinct_operands[3*i + k]]++;
        }
    }
    std::set<uint32_t> ready;
    std::vector<uint32_t> stamp(n, 0), order, best;     // stamp: emission count when the node became ready
    for (size_t i = 0; i < n; i++) {
        if (pending[i] == 0) ready.insert(static_cast<uint32_t> (i));
    }
    order.reserve(n);
    while (!ready.empty()) {
        best.clear();
        int best_score = 1 << 30;
        uint32_t best_stamp = 0;
        for (const uint32_t v : ready) {
            int freed = 0;
            for (int k = 0; k < distinct_count[v]; k++) {
                const uint32_t o = distinct_operands[3*static_cast<size_t> (v) + k];
                if (in.code[o].op != GFIR_CONST && consumers_left[o] == 1 && !is_root[o]) freed++;
            }
//  Constants cost nothing; inputs become live only when first read.
            const int score = (in.code[v].op == GFIR_CONST ? 0 : 1) - freed;
            if (score < best_score || (score == best_score && stamp[v] > best_stamp)) {
                best_score = score;
                best_stamp = stamp[v];
                best.clear();
            }
            if (score == best_score && stamp[v] == best_stamp) best.push_back(v);
        }
        const uint32_t pick = best[ties.pick(best.size())];
        ready.erase(pick);
        order.push_back(pick);
        if (!names.empty()) order.insert(order.end(), names[pick].begin(), names[pick].end());
        for (int k = 0; k < distinct_count[pick]; k++) consumers_left[distinct_operands[3*static_cast<size_t> (pick) + k]]--;
        for (auto u : users[pick]) {
            if (--pending[u] == 0) {
                ready.insert(u);
                stamp[u] = static_cast<uint32_t> (order.size());
            }
        }
    }
    return order;
}

//  The list schedule is O(nodes x ready set); items far larger than anything on the path (the RK4 item has 3.9 k
//  nodes) keep their own order rather than stall the lowering.
inline bool too_large_to_schedule(const item &in) { return in.code.size() > 20000; }

///  The order for the compiler: ties to the lowest record.
inline item schedule_for_pressure(const item &in) {
    return too_large_to_schedule(in) ? in : reorder(in, list_schedule(in, tie_break::lowest_record()));
}

///  The same with its ties broken by a seeded generator.
inline std::vector<uint32_t> list_schedule(const item &in, const uint32_t seed) {
    return list_schedule(in, tie_break::from_seed(seed));
}

}  // namespace gfhip

#endif /* gfhip_schedule_hpp */
