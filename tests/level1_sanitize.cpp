// Host-only driver for lowering level 1 (graph_framework_amd/csrc/options.hpp `level`; no HIP runtime): built with
// -fsanitize=address,undefined by tests/test_level1.py and run over every exported workload and over mutated items.
// Every item that parses goes through plan_item() (csrc/plan.hpp, what libgf_hip.so calls) at level 1 under the default
// options (four tie-breaks of the order search), with the assembly body whatever the size through a 28-pair register pool, cut
// into three segments and without the level-0 merge; and through the level-1 merge on its own, once on the item as it arrives and once on what
// the level-0 merge returns.  What must hold for every plan is checked here as well: level 1 keeps the number of pieces, the
// redo kernel and every text that has no assembly statement; a merged record names an earlier one.
// Usage: level1_sanitize <file.gfir>... [--mutate seed trials file.gfir]
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

static void require(const bool holds, const char *what, const gfhip::item &it) {
    if (holds) return;
    std::fprintf(stderr, "%s: %s\n", it.name.c_str(), what);
    std::exit(1);
}

static void check_merge(const gfhip::item &it, const gfhip::item &merged) {
    require(merged.code.size() == it.code.size(), "the level-1 merge changed the number of records", it);
    for (size_t i = 0; i < merged.code.size(); i++) {
        if (merged.is_merged(i)) require(merged.merged_into[i] < i && !merged.is_merged(merged.merged_into[i]), "a merged record does not name an earlier live one", it);
    }
}

static uint64_t plan_both_levels(const gfhip::item &it, gfhip::codegen_options opt) {
    opt.level = 0;
    const gfhip::item_plan level0 = gfhip::plan_item(it, opt, {});
    opt.level = 1;
    const gfhip::item_plan level1 = gfhip::plan_item(it, opt, {});
    require(level0.pieces.size() == level1.pieces.size() && level0.redo.has_value() == level1.redo.has_value(), "level 1 changed the shape of the plan", it);
    if (level0.redo) require(level0.redo->low.hash == level1.redo->low.hash, "level 1 changed the redo kernel", it);
    if (level0.pieces.empty()) require(level0.whole.hash == level1.whole.hash, "level 1 changed a kernel without pieces", it);
    uint64_t hash = level1.whole.hash;
    for (size_t p = 0; p < level0.pieces.size(); p++) {
        const gfhip::lowered &a = level0.pieces[p].low, &b = level1.pieces[p].low;
        if (!a.assembly) require(a.hash == b.hash, "level 1 changed a text without an assembly statement", it);
        require(a.assembly == b.assembly && a.block_size == b.block_size, "level 1 changed how a piece is launched", it);
        hash ^= b.hash;
    }
    return hash;
}

static bool lower_bytes(const std::vector<char> &bytes, uint64_t &hash) {
    gfhip::item it;
    std::string error;
    if (!it.parse(bytes.data(), bytes.size(), error)) return false;
    const gfhip::item twice = gfhip::merge_records(gfhip::merge_records(it), nullptr, 1);
    check_merge(it, gfhip::merge_records(it, nullptr, 1));
    check_merge(it, twice);
    gfhip::codegen_options defaults, small, three, unmerged;
    defaults.asm_schedule_tries = 4;                    // (the order search does not depend on the level: a few tie-breaks do)
    small = defaults;
    small.asm_min_nodes = 0;
    small.asm_schedule_tries = 2;
    small.asm_pool_lo = 200;
    small.asm_waves = 1;
    three = defaults;
    three.segments = 3;
    three.segments_min_nodes = 40;
    three.asm_min_nodes = 0;
    unmerged = small;
    unmerged.asm_pool_lo = 40;
    unmerged.merge = false;
    hash = 0;
    if (it.code.size() >= 20000) {                      // (the 54 k-record items, cut by size: one plan, at level 1)
        defaults.level = 1;
        hash = gfhip::plan_item(it, defaults, {}).whole.hash;
        return true;
    }
    for (const gfhip::codegen_options &opt : {defaults, small, three, unmerged}) hash ^= plan_both_levels(it, opt);
    return true;
}

int main(int argc, char **argv) {
    size_t planned = 0, rejected = 0;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--mutate") && i + 3 < argc) {
            std::mt19937_64 rng(std::strtoull(argv[i + 1], nullptr, 10));
            const size_t trials = std::strtoull(argv[i + 2], nullptr, 10);
            const std::vector<char> base = read_file(argv[i + 3]);
            for (size_t t = 0; t < trials; t++) {
                std::vector<char> b = base;
                const unsigned kind = rng()%10;
                if (kind < 3) {
                    b.resize(rng()%b.size());
                } else if (kind < 8) {
                    for (unsigned k = 0, n = 1 + rng()%5; k < n; k++) b[rng()%b.size()] = static_cast<char> (rng());
                } else {
                    const uint32_t values[5] = {0xFFFFFFFFu, 0x7FFFFFFFu, 0x80000000u, 100000u, static_cast<uint32_t> (rng())};
                    const uint32_t v = values[rng()%5];
                    std::memcpy(b.data() + (rng()%(b.size()/4))*4, &v, 4);
                }
                uint64_t hash;
                (lower_bytes(b, hash) ? planned : rejected)++;
            }
            i += 3;
            continue;
        }
        uint64_t hash = 0;
        if (!lower_bytes(read_file(argv[i]), hash)) {
            std::fprintf(stderr, "%s: rejected\n", argv[i]);
            return 1;
        }
        planned++;
    }
    std::printf("planned %zu rejected %zu\n", planned, rejected);
    return 0;
}
