// poa_forward_row_operands.h -- the per-row operands of the packed forward pass's row loop (poa_forward_moves.h), packed
// once per block of rows by all lanes (one row per lane) and fetched by the row loop with v_readlane: what a row body would
// otherwise derive from the row-table word with scalar instructions, on the critical path of a lone wavefront that pays
// ~8 cycles per issued instruction of any kind. Plain integer code for host and device, so that the CPU can check the
// packing against the straightforward decode (tests/cpp/forward_row_operands_sanitized.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define GWHIP_ROW_OPERANDS_FN __host__ __device__ inline
#else
#define GWHIP_ROW_OPERANDS_FN inline
#endif

namespace gwhip
{

// DESCRIPTOR kinds: the table kinds of classify_kinds (0, 1, 2, 4 keep their meaning), with table kind 3 (two to six
// predecessors from the ring) split by predecessor count so that each has a body without a count test, and 7 = end of block
constexpr uint32_t kDkPrev = 0, kDkPrevMoved = 1, kDkRingOne = 2, kDkRingTwo = 3, kDkGeneral = 4, kDkRingThree = 5, kDkRingMany = 6,
                   kDkEnd = 7;
constexpr uint32_t kRowOpSlots = 8, kRowOpSlotBytes = 1024; // the LDS ring's geometry (kPkSlots, kPkSlotBytes)
constexpr uint32_t kRowOpScoresToHbm = 1u << 3;             // d0: the row's score row goes to HBM (bit 63 of the table word)
// d0: one bit each for the most frequent kinds after 0, so that the row loop's dispatch is a chain of single-bit tests in the
// order of frequency (a chain of compares of the kind field becomes a switch, which is lowered to a binary search)
constexpr uint32_t kRowOpIsRingTwo = 1u << 4, kRowOpIsRingOne = 1u << 5, kRowOpIsPrevMoved = 1u << 6, kRowOpIsEnd = 1u << 7;
constexpr int kRowOpReadShift      = 8; // d0 >> this: LDS byte address of the read character of column band start + 1

struct RowOperands
{
    uint32_t d0;                  // descriptor kind [0:3), scores-to-HBM [3], kind bits [4:8), read_base + band start [8:32)
    uint32_t base4;               // the row's base replicated into four bytes
    uint32_t slot0, slot1, slot2; // LDS byte addresses of the ring slots of predecessors 0..2 (ring base and slot size folded in)
    uint32_t bs2;                 // the band start in bytes of a score row (2 x band start)
    // packed 16-bit move constants, both halves alike. One ring predecessor d rows up: mv0 = 2 d + 1 (diagonal move),
    // mv1 = 1 - 2 d. Several (distances d0, d1, d2): mv0 = 2 d0 + 1, mv1 = 2 d0, mv2 = E1 = 2 (d1 - d0), mv3 = E2 = 2 (d2 - d1)
    uint32_t mv0, mv1, mv2, mv3;
};

GWHIP_ROW_OPERANDS_FN uint32_t row_operand_dup16(int32_t v) { return ((uint32_t)v & 0xffffu) | ((uint32_t)v << 16); }

// the descriptor kind of a row of table kind `kind` with `cnt` predecessors
GWHIP_ROW_OPERANDS_FN uint32_t row_descriptor_kind(uint32_t kind, uint32_t cnt)
{
    if (kind == 3u) return cnt == 2u ? kDkRingTwo : (cnt == 3u ? kDkRingThree : kDkRingMany);
    return kind > 4u ? kDkGeneral : kind;
}

// w: the row's table word with its kind (classify_kinds) and its scores-to-HBM bit (mark_score_rows); row: its index;
// in_block: false for the lanes past the block's or the phase's last row, which read as "end of block"
GWHIP_ROW_OPERANDS_FN RowOperands pack_row_operands(uint64_t w, uint32_t row, bool in_block, uint32_t ring_base, uint32_t read_base)
{
    const uint32_t kind = (uint32_t)(w >> 60) & 7u;
    const uint32_t cnt  = (uint32_t)(w >> 8) & 0x3fu;
    const uint32_t bs   = ((uint32_t)(w >> 15) & 0x1ffu) << 2;
    const uint32_t p0 = (uint32_t)(w >> 24) & 0xfffu, p1 = (uint32_t)(w >> 36) & 0xfffu, p2 = (uint32_t)(w >> 48) & 0xfffu;
    const int32_t dd0 = (int32_t)((row - p0) & 7u), dd1 = (int32_t)((row - p1) & 7u), dd2 = (int32_t)((row - p2) & 7u);
    const uint32_t dk = in_block ? row_descriptor_kind(kind, cnt) : kDkEnd;
    RowOperands o;
    const uint32_t kind_bits = dk == kDkRingTwo ? kRowOpIsRingTwo : (dk == kDkRingOne ? kRowOpIsRingOne : (dk == kDkPrevMoved ? kRowOpIsPrevMoved : (dk == kDkEnd ? kRowOpIsEnd : 0u)));
    o.d0    = dk | ((uint32_t)(w >> 63) << 3) | kind_bits | ((read_base + bs) << kRowOpReadShift);
    o.base4 = ((uint32_t)w & 0xffu) * 0x01010101u;
    o.slot0 = ring_base + (p0 & (kRowOpSlots - 1)) * kRowOpSlotBytes;
    o.slot1 = ring_base + (p1 & (kRowOpSlots - 1)) * kRowOpSlotBytes;
    o.slot2 = ring_base + (p2 & (kRowOpSlots - 1)) * kRowOpSlotBytes;
    o.bs2   = 2u * bs;
    const bool one = kind == kDkRingOne;
    o.mv0 = row_operand_dup16(2 * dd0 + 1);
    o.mv1 = row_operand_dup16(one ? 1 - 2 * dd0 : 2 * dd0);
    o.mv2 = row_operand_dup16(2 * (dd1 - dd0));
    o.mv3 = row_operand_dup16(2 * (dd2 - dd1));
    return o;
}

} // namespace gwhip
