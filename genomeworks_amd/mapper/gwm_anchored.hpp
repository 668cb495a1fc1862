// gwm_anchored.hpp -- what the chunk loop (gwm_align.hip) takes from gwm_anchored.hip when a call brings the anchors
// of its records (gwm_align_overlaps_anchored in include/gwhip_mapper.h; the rules are gwm_anchor_plan.hpp): the plan
// of the whole call, and per chunk the gather of the pieces, the record-level slice starts and the stitching of the
// pieces' states into the records' slots.
#ifndef GWM_ANCHORED_HPP
#define GWM_ANCHORED_HPP

#include "gwhip_mapper.h"

#include "gwm_host_utils.hpp"

#include <vector>

namespace gwm
{

// The pieces of a call of n records: piece p is slice [u, u + query length) x [v, v + target length) of its record;
// record i owns pieces [piece_first[i], piece_first[i + 1]), in order. The device arrays are owned.
struct AnchorPlan
{
    int64_t n = 0, pieces = 0;
    int64_t longest_query_piece = 0;
    int64_t* piece_lengths = nullptr; // device [2 pieces + 1]: query, target bases of piece p; the last entry 0
    uint32_t* piece_u      = nullptr; // device [pieces]
    uint32_t* piece_v      = nullptr;
    uint32_t* piece_record = nullptr; // device [pieces]: the record of the call
    int64_t* piece_first   = nullptr; // device [n + 1]
    std::vector<int64_t> host_starts; // [2 pieces + 1]: the exclusive sums of piece_lengths
    std::vector<int64_t> host_piece_first;
    AnchorPlan()                  = default;
    AnchorPlan(const AnchorPlan&) = delete;
    AnchorPlan& operator=(const AnchorPlan&) = delete;
    ~AnchorPlan()
    {
        (void)hipFree(piece_lengths);
        (void)hipFree(piece_u);
        (void)hipFree(piece_v);
        (void)hipFree(piece_record);
        (void)hipFree(piece_first);
    }
};

// k, S and the number of anchors of `lists` out of range: std::invalid_argument opened by `who`
void check_anchor_parameters(const std::string& who, const gwm_anchor_lists& lists);

// the same and the offsets of `lists` (copied to the host), refused before anything is launched
void check_anchor_lists(const std::string& who, const gwm_anchor_lists& lists, int64_t n, hipStream_t s);

// G1-G5 for validated device overlaps[0..n); throws std::invalid_argument that names the first record whose valid
// anchors are not strictly increasing (G3). Waits for s.
void build_anchor_plan(const std::string& who, const gwm_overlap* overlaps, int64_t n, const gwm_anchor_lists& lists,
                       hipStream_t s, AnchorPlan& plan);

// Slices 2 j, 2 j + 1 of the chunk's pieces [first_piece, first_piece + count) -- query and target side of piece
// first_piece + j, the target side reverse-complemented on '-' -- to sequences[starts[2 j] ..): one wave64 a slice.
void gather_pieces(const AnchorPlan& plan, const gwm_overlap* overlaps, int64_t first_piece, int64_t count, const ReadSet& q,
                   const ReadSet& t, const int64_t* starts, uint8_t* sequences, hipStream_t s);

// starts[0 .. 2 m]: the slice starts of records [first, first + m) within the chunk, from its pieces' starts
void record_starts(const AnchorPlan& plan, const gwm_overlap* overlaps, int64_t first, int64_t m, const int64_t* piece_starts,
                   int64_t* starts, hipStream_t s);

// G6: the states of records [first, first + m), back to front at results[starts[2 i]], from the states of their
// pieces, back to front at piece_results[piece_starts[2 j]]; result_lengths[i] their number, 0 where a piece has none
void stitch_pieces(const AnchorPlan& plan, int64_t first, int64_t m, const uint8_t* piece_results, const int64_t* piece_starts,
                   const int32_t* piece_result_lengths, uint8_t* results, const int64_t* starts, int32_t* result_lengths,
                   hipStream_t s);

} // namespace gwm

#endif
