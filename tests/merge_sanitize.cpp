// Host-only driver for the merge pass (csrc/merge.hpp; no HIP runtime): built with -fsanitize=address,undefined by
// tests/test_merge.py and run over every exported workload and over mutated items.  Every item that parses is merged in the
// order it arrives in and in the pressure-aware order; what the pass returns is held to its contract (a merged record is a
// copy of an earlier, unmerged record; nothing reads a merged record), ordered again, cut into 2..4 segments, and written by
// both kernel writers.  Every item that parses also goes through plan_item() itself (csrc/plan.hpp, what libgf_hip.so
// calls) under three sets of options.
// Usage: merge_sanitize <file.gfir>... [--mutate seed trials file.gfir]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <vector>

#include "../include/gfir.h"
#include "../graph_framework_amd/csrc/plan.hpp"

static std::vector<char> read_file(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char> ((std::istreambuf_iterator<char> (f)), std::istreambuf_iterator<char> ());
}

static void fail(const char *what, const size_t record) {
    std::fprintf(stderr, "merge contract broken: %s (record %zu)\n", what, record);
    std::exit(1);
}

static void check(const gfhip::item &before, const gfhip::item &after, const gfhip::merge_report &report) {
    const size_t n = before.code.size();
    if (after.code.size() != n || after.outputs.size() != before.outputs.size() || after.setters.size() != before.setters.size()) fail("counts changed", 0);
    if (!after.merged_into.empty() && after.merged_into.size() != n) fail("merged_into has another length", 0);
    size_t merged = 0;
    for (size_t i = 0; i < n; i++) {
        const gfir_instruction &c = after.code[i];
        for (const uint32_t o : after.operands(i)) {
            if (o >= i) fail("an operand is not an earlier record", i);
            if (after.is_merged(o)) fail("a merged record is read", i);
        }
        if (!after.is_merged(i)) continue;
        merged++;
        const uint32_t first = after.merged_into[i];
        if (first >= i || after.is_merged(first)) fail("the representative is not an earlier, unmerged record", i);
        if (std::memcmp(&c, &after.code[first], sizeof(c)) != 0) fail("a merged record is not a copy of its representative", i);
    }
    for (auto &s : after.setters) if (after.is_merged(s.value)) fail("a setter stores a merged record", s.value);
    for (auto o : after.outputs) if (after.is_merged(o)) fail("an output is a merged record", o);
    if (merged != report.records() || merged != report.merged.size()) fail("the report counts other merges", merged);
}

//  The shipped planning code: the defaults, three segments, and the assembly body whatever the size.
static uint64_t plan_hash(const gfhip::item &it) {
    gfhip::codegen_options three, assembly;
    three.segments = 3;
    three.segments_min_nodes = 40;
    assembly.asm_min_nodes = 0;
    assembly.asm_schedule_tries = 3;
    uint64_t hash = 0;
    for (const gfhip::codegen_options &opt : {gfhip::codegen_options(), three, assembly}) {
        const gfhip::item_plan plan = gfhip::plan_item(it, opt, {});
        for (auto &piece : plan.pieces) {
            const gfhip::item &part = piece.plan.piece;
            for (size_t i = 0; i < part.code.size(); i++) {
                if (part.is_merged(i) && (part.merged_into[i] >= i || part.is_merged(part.merged_into[i]))) fail("a planned piece names a later record", i);
            }
            hash ^= piece.low.hash;
        }
        hash ^= plan.whole.hash ^ (plan.redo ? plan.redo->low.hash : 0);
    }
    return hash;
}

//  What plan_item() hands the writer for a `last` piece: the statement, if the piece is a candidate for one.
static gfhip::asm_body_text statement_of(const gfhip::item &piece, const gfhip::codegen_options &opt, const gfhip::piece_info &role) {
    const bool offered = role.role == gfhip::piece_role::last && gfhip::assembly_candidate(piece, opt);
    return offered ? gfhip::assembly_statement(piece, opt) : gfhip::asm_body_text();
}

static bool merge_bytes(const std::vector<char> &bytes, size_t &merged) {
    gfhip::item it;
    std::string error;
    if (!it.parse(bytes.data(), bytes.size(), error)) return false;
    gfhip::merge_report report;
    const gfhip::item in_source_order = gfhip::merge_records(it, &report);
    check(it, in_source_order, report);
    merged += report.records();
    uint64_t hash = plan_hash(it);
    if (it.code.size() >= 20000) return hash != 1;      // (the 54 k-record VMEC step: the pass, its contract and its plan only)
    const gfhip::item ordered = gfhip::schedule_for_pressure(it);
    const gfhip::item merged_item = gfhip::merge_records(ordered, &report);
    check(ordered, merged_item, report);
//  merging what is merged finds the same pairs again
    gfhip::merge_report again;
    check(merged_item, gfhip::merge_records(merged_item, &again), again);
    if (again.records() != report.records()) fail("the pass is not idempotent", 0);
//  ordering a merged item keeps every merged record behind its representative
    const gfhip::item reordered = gfhip::schedule_for_pressure(in_source_order);
    for (size_t i = 0; i < reordered.code.size(); i++) {
        if (reordered.is_merged(i) && reordered.merged_into[i] >= i) fail("a merged record is ordered before its representative", i);
    }
    const gfhip::codegen_options defaults;
    hash ^= gfhip::write_item(gfhip::in_emission_order(it, defaults), defaults).hash;
    if (gfhip::can_split(it) && it.code.size() >= 40) {
        for (size_t count = 2; count <= 4; count++) {
            gfhip::segmentation plan = gfhip::split_item(merged_item, gfhip::choose_cuts(merged_item, count));
            for (size_t p = 0; p < plan.segments.size(); p++) {
                const gfhip::item &piece = plan.segments[p].piece;
                for (size_t i = 0; i < piece.code.size(); i++) {
                    if (piece.is_merged(i) && (piece.merged_into[i] >= i || piece.is_merged(piece.merged_into[i]))) fail("a segment names a later record", i);
                }
                gfhip::piece_info role;
                role.role = p + 1 == plan.segments.size() ? gfhip::piece_role::last : gfhip::piece_role::middle;
                for (auto slot : plan.segments[p].output_slot) role.output_handed_over.push_back(slot >= 0);
                hash ^= gfhip::write_item(piece, defaults, role, statement_of(piece, defaults, role)).hash;
            }
        }
//  the whole item as one piece whose pass is the assembly body, with a small register pool
        if (it.code.size() < 6000) {
            gfhip::codegen_options assembly;
            assembly.asm_min_nodes = 0;
            assembly.asm_schedule_tries = 2;
            assembly.asm_pool_lo = 200;
            assembly.asm_waves = 1;
            const gfhip::item chosen = gfhip::merge_records(gfhip::schedule_for_assembly(it, assembly));
            gfhip::piece_info whole;
            whole.role = gfhip::piece_role::last;
            hash ^= gfhip::write_item(chosen, assembly, whole, statement_of(chosen, assembly, whole)).hash;
        }
    }
    return hash != 1;
}

int main(int argc, char **argv) {
    size_t items = 0, rejected = 0, merged = 0;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--mutate") && i + 3 < argc) {
            std::mt19937_64 rng(std::strtoull(argv[i + 1], nullptr, 10));
            const size_t trials = std::strtoull(argv[i + 2], nullptr, 10);
            const std::vector<char> base = read_file(argv[i + 3]);
            for (size_t t = 0; t < trials; t++) {
                std::vector<char> b = base;
                const unsigned kind = rng()%10;
                if (kind < 2) {
                    b.resize(rng()%b.size());
                } else if (kind < 6) {
                    for (unsigned k = 0, n = 1 + rng()%5; k < n; k++) b[rng()%b.size()] = static_cast<char> (rng());
                } else {
//  an operand field of a record redirected to another record: duplicates appear and disappear
                    const uint32_t values[4] = {0u, 1u, 7u, static_cast<uint32_t> (rng()%64)};
                    const uint32_t v = values[rng()%4];
                    std::memcpy(b.data() + b.size()/2 + (rng()%(b.size()/8))*4, &v, 4);
                }
                (merge_bytes(b, merged) ? items : rejected)++;
            }
            i += 3;
            continue;
        }
        if (!merge_bytes(read_file(argv[i]), merged)) {
            std::fprintf(stderr, "%s: rejected\n", argv[i]);
            return 1;
        }
        items++;
    }
    std::printf("merged %zu records in %zu items, rejected %zu\n", merged, items, rejected);
    return 0;
}
