//------------------------------------------------------------------------------
///  @file plan.hpp
///  @brief From a parsed item and the options to what is compiled: the one place that decides.
///
///  plan_item() puts the item into emission order and merges it (codegen.hpp, in_emission_order), decides whether its
///  pass is the assembly statement (asm_body.hpp, assembly_candidate — by writing it), cuts it into segments where the
///  options ask for that (segments.hpp), and has every piece written once (codegen.hpp, write_item).  Nothing here needs
///  the device: gf_hip.cpp adds modules and launches, the sanitizer drivers under tests/ call the same function.
///
///  The forms an item takes:
///    * one kernel with the IEEE pass compiled into it as a function (`pieces` empty, `whole` is its lowering);
///    * one piece with the assembly body and a redo launch for the lanes outside the division window (the RK4 step);
///    * GFHIP_SEGMENTS=n: n pieces (`middle`..., `last`) and the redo launch;
///    * more than segment_nodes records: pieces of about that size with the compiler's division, no redo launch.
//------------------------------------------------------------------------------
#ifndef gfhip_plan_hpp
#define gfhip_plan_hpp

#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "asm_body.hpp"
#include "codegen.hpp"
#include "segments.hpp"

namespace gfhip {

///  One kernel of an item: a segment of it (or the whole of it) as an item of its own, and its text.
struct planned_piece {
    segment plan;
    lowered low;
};

struct item_plan {
    lowered whole;                          ///< the item's kernel; of an item in pieces, its name, block size, written inputs and the
                                            ///< FNV fold of the pieces' hashes (without the redo piece)
    std::vector<planned_piece> pieces;      ///< not empty: the item runs as this sequence of kernels
    std::optional<planned_piece> redo;      ///< the WHOLE item with the compiler's division, over the rays of the redo list
    uint32_t slots = 0;                     ///< hand-over slots between the pieces
    size_t handover_bytes = 0;

///  Rays per walk of the piece sequence: the hand-over buffers of one chunk stay in the Infinity Cache.  One piece hands
///  nothing over: one walk over all rays.
    size_t chunk(const size_t num_rays, const size_t element_size) const {
        if (slots == 0) return num_rays;
        const size_t rays = std::max<size_t> (handover_bytes/(slots*element_size)/1024*1024, 16384);
        return std::min(num_rays, rays);
    }
};

//------------------------------------------------------------------------------
///  @param[in] order_directories Where the assembly search remembers the order it chose (asm_body.hpp).
//------------------------------------------------------------------------------
inline item_plan plan_item(const item &it, const codegen_options &opt, const std::vector<std::string> &order_directories) {
    item_plan result;
    result.handover_bytes = opt.handover_bytes;
    size_t count = 1;
    bool by_size = false;
    if (can_split(it)) {
        if (opt.segments >= 1 && it.code.size() >= opt.segments_min_nodes && it.code.size() >= 2*opt.segments) {
            count = opt.segments;
        } else if (opt.segment_nodes && it.code.size() > opt.segment_nodes) {
            count = (it.code.size() + opt.segment_nodes - 1)/opt.segment_nodes;
            by_size = true;
        }
    }
//  Very large items are off the hot path: the compiler's division, no checks, no second body.  Every other item in pieces
//  keeps the shared reciprocals and has NO IEEE function compiled into its pieces (so that they fit two waves per SIMD):
//  lanes outside the window are redone by one more launch.
    codegen_options piece_options = opt;
    if (by_size) piece_options.division = division_mode::ieee;
    const bool with_redo = piece_options.division != division_mode::ieee;
    auto cut = [&] (const item &ordered) {
        segmentation parts = split_item(ordered, choose_cuts(ordered, count));
//  A one-kernel item keeps its name (profiles show gfhip_<name> and gfhip_<name>_redo).
        if (parts.segments.size() == 1) parts.segments[0].piece.name = it.name;
        return parts;
    };

//  The assembly body for an item that stays whole: if the statement of its only piece can be written in the order
//  the search finds, the item is that one `last` piece; else it stays one kernel.
    item ordered;
    segmentation parts;
    asm_body_text statement;
    if (count < 2 && opt.segments == 0 && opt.schedule_for_pressure && assembly_candidate(it, opt)) {
        const item chosen = schedule_for_assembly(it, opt, order_directories);
        ordered = in_emission_order(it, opt, &chosen);
        parts = cut(ordered);
        statement = assembly_statement(parts.segments[0].piece, piece_options);
    }
    if (!statement.ok) {
        ordered = in_emission_order(it, opt);
        if (count < 2 && opt.segments != 1) {
            result.whole = write_item(ordered, opt);
            return result;
        }
        parts = cut(ordered);
    }

//  Which values of the item depend on a quotient: a handed-over one keeps that mark in the pieces that read it.
    const std::vector<bool> quotient = after_division(ordered);
    for (size_t p = 0; p < parts.segments.size(); p++) {
        planned_piece piece;
        piece.plan = std::move(parts.segments[p]);
        piece_info info;
        if (with_redo) {
            info.role = p + 1 == parts.segments.size() ? piece_role::last : piece_role::middle;
            for (auto slot : piece.plan.output_slot) info.output_handed_over.push_back(slot >= 0);
            for (auto record : piece.plan.symbol_record) info.symbol_after_division.push_back(record >= 0 && quotient[record]);
        }
        if (info.role == piece_role::last && !statement.ok && assembly_candidate(piece.plan.piece, piece_options)) {
            statement = assembly_statement(piece.plan.piece, piece_options);
        }
//  Known oddities, kept because they are part of the text: with GFHIP_ASM=0 a piece is ordered
//  again on its own, and a piece without a role in which no record is merged goes through the merge once more.
        codegen_options again = piece_options;
        again.schedule_for_pressure = opt.schedule_for_pressure && !opt.asm_body;
        again.merge = opt.merge && info.role == piece_role::none && piece.plan.piece.merged_into.empty();
        const bool rewritten = again.schedule_for_pressure || again.merge;
        piece.low = write_item(rewritten ? in_emission_order(piece.plan.piece, again) : piece.plan.piece, piece_options, info,
                               info.role == piece_role::last ? statement : asm_body_text());
        result.pieces.push_back(std::move(piece));
    }
    if (with_redo) {
        codegen_options plain = opt;
        plain.division = division_mode::ieee;
        plain.waves_per_simd = 0;
        piece_info info;
        info.role = piece_role::redo;
//  (in the order for the compiler, whatever order the assembly search chose for the pass)
        planned_piece &redo = result.redo.emplace();
        redo.plan.piece = it;
        redo.plan.piece.name = it.name + "_redo";
        redo.plan.piece = in_emission_order(redo.plan.piece, plain);
        redo.low = write_item(redo.plan.piece, plain, info);
    }
    result.whole.kernel_name = "gfhip_" + it.name;
    result.whole.block_size = result.pieces[0].low.block_size;
    result.whole.input_written.assign(it.symbols.size(), false);
    for (auto &s : it.setters) result.whole.input_written[s.input] = true;
    for (auto &piece : result.pieces) result.whole.hash = result.whole.hash*1099511628211ull ^ piece.low.hash;
    result.slots = parts.slots;
    return result;
}

}  // namespace gfhip

#endif /* gfhip_plan_hpp */
