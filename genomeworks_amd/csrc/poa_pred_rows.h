// poa_pred_rows.h -- where the predecessor ROWS of a row of the packed row table come from without a trip to HBM: predecessors
// 0..2 from the row's table word (RowInfo<true>, poa_device.h), predecessors 3..5 of a row with 4..6 of them from the side
// table build_rowinfo leaves in LDS (one 64-bit entry per row & 255; the last writer of a slot wins, so a reader checks the
// entry against its row). One decode for classify_kinds, mark_score_rows, the general row and the walk's recomputed step.
// Plain integer code for host and device, so that the CPU can check it against a restatement (tests/cpp/pred_rows_check.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GWHIP_PRED_ROWS_FN __host__ __device__ inline
#else
#define GWHIP_PRED_ROWS_FN inline
#endif

namespace gwhip
{

constexpr int kTablePreds    = 3; // predecessor rows in the table word: [24:36) [36:48) [48:60)
constexpr int kSideTablePreds = 6; // a row with up to this many predecessors has the rest in its side-table entry
constexpr int kSideTableSlots = 256;

// table word of a row without band start, kind and scores-to-HBM bit (RowInfo<true>::set): base [0:8), predecessor count
// [8:14), sink [14], predecessor rows 0..2 [24:36) [36:48) [48:60)
GWHIP_PRED_ROWS_FN uint64_t table_word(int32_t base, int32_t cnt, bool sink, int32_t p0, int32_t p1, int32_t p2)
{
    return (uint64_t)(base & 0xff) | ((uint64_t)(cnt & 0x3f) << 8) | ((uint64_t)(sink ? 1 : 0) << 14) |
           ((uint64_t)(p0 & 0xfff) << 24) | ((uint64_t)(p1 & 0xfff) << 36) | ((uint64_t)(p2 & 0xfff) << 48);
}
// table word: predecessor count [8:14), predecessor row k = 0..2
GWHIP_PRED_ROWS_FN int32_t table_pred_count(uint64_t w) { return (int32_t)((w >> 8) & 0x3fu); }
GWHIP_PRED_ROWS_FN int32_t table_pred_row(uint64_t w, int32_t k) { return (int32_t)((w >> (24 + 12 * k)) & 0xfffu); }

// side-table entry: {row [0:12), valid [12], count [13:19), pred 3 [20:32), pred 4 [32:44), pred 5 [44:56)}
GWHIP_PRED_ROWS_FN uint64_t xpred_entry(int32_t row, int32_t cnt, int32_t p3, int32_t p4, int32_t p5)
{
    return (uint64_t)((uint32_t)row | (1u << 12) | ((uint32_t)(cnt & 63) << 13) | ((uint32_t)(p3 & 0xfff) << 20)) |
           ((uint64_t)(p4 & 0xfff) << 32) | ((uint64_t)(p5 & 0xfff) << 44);
}
GWHIP_PRED_ROWS_FN bool xpred_hit(uint64_t e, int32_t row, int32_t cnt)
{
    return (int32_t)(e & 0xfffu) == row && ((e >> 12) & 1u) != 0 && (int32_t)((e >> 13) & 63u) == cnt;
}
GWHIP_PRED_ROWS_FN int32_t xpred_row(uint64_t e, int32_t k) { return (int32_t)((e >> (20 + 12 * (k - 3))) & 0xfffu); } // k = 3..5

// the row needs its side-table entry at all (4..6 predecessors): only then is the slot worth a load
GWHIP_PRED_ROWS_FN bool pred_rows_want_entry(int32_t cnt) { return cnt > kTablePreds && cnt <= kSideTablePreds; }
// every predecessor row of `row` (cnt of them) is in LDS: in the table word alone, or with the entry `e` of its slot
GWHIP_PRED_ROWS_FN bool pred_rows_in_lds(int32_t row, int32_t cnt, uint64_t e)
{
    return cnt <= kTablePreds || (cnt <= kSideTablePreds && xpred_hit(e, row, cnt));
}
// predecessor row k < cnt of a row for which pred_rows_in_lds holds
GWHIP_PRED_ROWS_FN int32_t lds_pred_row(uint64_t w, uint64_t e, int32_t k) { return k < kTablePreds ? table_pred_row(w, k) : xpred_row(e, k); }

} // namespace gwhip
