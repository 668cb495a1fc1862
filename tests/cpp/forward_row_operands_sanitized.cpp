// forward_row_operands_sanitized.cpp -- a stand-alone check of the row operands the packed forward pass packs once per
// block of rows (genomeworks_amd/csrc/poa_forward_row_operands.h), built by tests/test_forward_row_operands.py under
// -fsanitize=address,undefined. Every combination of table kind, predecessor count 1..6, predecessor distances 1..7,
// row index modulo 8 (low rows and rows past 256 and 2048), a spread of band starts including 0 and the largest, the
// scores-to-HBM bit and in / past the block is compared with the plain expressions the row loop used to evaluate per
// row from the row-table word (the straightforward decode below). Prints "ok <cases>", or the first mismatch.
#include "../../genomeworks_amd/csrc/poa_forward_row_operands.h"

#include <cstdio>

namespace
{

constexpr uint32_t kSlotBytes = 1024, kSlots = 8;

uint32_t pk_dup(int32_t v) { return ((uint32_t)v & 0xffffu) | ((uint32_t)v << 16); }

// the row-table word (RowInfo<true>, poa_device.h): [0:8) base [8:14) count [14] sink [15:24) band start / 4
// [24:36) [36:48) [48:60) predecessor rows [60:63) kind [63] scores to HBM
uint64_t table_word(uint32_t base, uint32_t cnt, uint32_t bs, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t kind, bool scores)
{
    return (uint64_t)(base & 0xff) | ((uint64_t)(cnt & 0x3f) << 8) | ((uint64_t)((bs >> 2) & 0x1ff) << 15) | ((uint64_t)(p0 & 0xfff) << 24) |
           ((uint64_t)(p1 & 0xfff) << 36) | ((uint64_t)(p2 & 0xfff) << 48) | ((uint64_t)kind << 60) | ((uint64_t)(scores ? 1 : 0) << 63);
}

struct Plain // what a row body derived for itself
{
    uint32_t kind, cnt3, bs, b0, b1, b2, dd0, dd1, dd2, base4;
    bool scores;
};

Plain plain_decode(uint64_t w, uint32_t rr, uint32_t ring_base)
{
    Plain d;
    d.kind              = (uint32_t)(w >> 60) & 7u;
    const uint32_t cnt  = (uint32_t)(w >> 8) & 0x3fu;
    d.cnt3              = cnt <= 3 ? cnt : 0u; // 2, 3, or 0 = more than three
    d.bs                = ((uint32_t)(w >> 15) & 0x1ffu) << 2;
    const uint32_t p0 = (uint32_t)(w >> 24) & 0xfffu, p1 = (uint32_t)(w >> 36) & 0xfffu, p2 = (uint32_t)(w >> 48) & 0xfffu;
    d.b0     = ring_base + ((p0 & (kSlots - 1)) * kSlotBytes);
    d.b1     = ring_base + ((p1 & (kSlots - 1)) * kSlotBytes);
    d.b2     = ring_base + ((p2 & (kSlots - 1)) * kSlotBytes);
    d.dd0    = (rr - p0) & 7u;
    d.dd1    = (rr - p1) & 7u;
    d.dd2    = (rr - p2) & 7u;
    d.base4  = ((uint32_t)w & 0xffu) * 0x01010101u;
    d.scores = (w & (1ull << 63)) != 0;
    return d;
}

int fail(const char* what, uint64_t w, uint32_t row, uint32_t got, uint32_t want)
{
    std::printf("mismatch in %s: word %016llx row %u: %08x, expected %08x\n", what, (unsigned long long)w, row, got, want);
    return 1;
}

} // namespace

int main()
{
    using namespace gwhip;
    const uint32_t band_starts[] = {0, 4, 8, 60, 252, 1000, 2040, 2044}; // 2044 = the largest the table word holds
    const uint32_t row_bases[]   = {8, 264, 2048, 3064};                 // + 0..7: every row index modulo 8
    const uint32_t ring_bases[]  = {0, 4096};
    const uint32_t read_base     = 33040;
    long cases = 0;
    for (uint32_t kind = 0; kind <= 4; kind++)
        for (uint32_t cnt = 1; cnt <= 6; cnt++)
            for (uint32_t d0 = 1; d0 <= 7; d0++)
                for (uint32_t d1 = 1; d1 <= 7; d1++)
                    for (uint32_t d2 = 1; d2 <= 7; d2++)
                        for (uint32_t rb : row_bases)
                            for (uint32_t m = 0; m < 8; m++)
                                for (uint32_t bs : band_starts)
                                    for (int flags = 0; flags < 4; flags++)
                                    {
                                        const uint32_t row = rb + m, ring_base = ring_bases[(row >> 3) & 1];
                                        const bool scores = (flags & 1) != 0, in_block = (flags & 2) != 0;
                                        const uint64_t w = table_word("ACGT"[(row + d0) & 3], cnt, bs, row - d0, row - d1, row - d2, kind, scores);
                                        const Plain d    = plain_decode(w, row, ring_base);
                                        const RowOperands o = pack_row_operands(w, row, in_block, ring_base, read_base);
                                        cases++;
                                        // the kind the row loop dispatches on: the table kind, table kind 3 by predecessor count
                                        uint32_t dk = d.kind;
                                        if (d.kind == 3) dk = d.cnt3 == 2 ? 3u : (d.cnt3 == 3 ? 5u : 6u);
                                        if (!in_block) dk = 7;
                                        if ((o.d0 & 7u) != dk) return fail("descriptor kind", w, row, o.d0 & 7u, dk);
                                        const uint32_t bits = (dk == 3 ? kRowOpIsRingTwo : 0u) | (dk == 2 ? kRowOpIsRingOne : 0u) |
                                                              (dk == 1 ? kRowOpIsPrevMoved : 0u) | (dk == 7 ? kRowOpIsEnd : 0u);
                                        if ((o.d0 & 0xf0u) != bits) return fail("kind bits", w, row, o.d0 & 0xf0u, bits);
                                        if (((o.d0 & kRowOpScoresToHbm) != 0) != d.scores) return fail("scores-to-HBM bit", w, row, o.d0, d.scores);
                                        if ((o.d0 >> kRowOpReadShift) != read_base + d.bs) return fail("read address", w, row, o.d0 >> kRowOpReadShift, read_base + d.bs);
                                        if (o.base4 != d.base4) return fail("base", w, row, o.base4, d.base4);
                                        if (o.bs2 != 2u * d.bs) return fail("band start in bytes", w, row, o.bs2, 2u * d.bs);
                                        if (o.slot0 != d.b0) return fail("slot 0", w, row, o.slot0, d.b0);
                                        if (o.slot1 != d.b1) return fail("slot 1", w, row, o.slot1, d.b1);
                                        if (o.slot2 != d.b2) return fail("slot 2", w, row, o.slot2, d.b2);
                                        if (d.dd0 != d0 || d.dd1 != d1 || d.dd2 != d2) return fail("distance", w, row, d.dd0, d0);
                                        if (d.kind == 2)
                                        {
                                            const uint32_t cD = pk_dup((int32_t)(2u * d.dd0 + 1u)), cV = pk_dup(1 - (int32_t)(2u * d.dd0));
                                            if (o.mv0 != cD) return fail("cD", w, row, o.mv0, cD);
                                            if (o.mv1 != cV) return fail("cV", w, row, o.mv1, cV);
                                        }
                                        if (d.kind == 3)
                                        {
                                            const uint32_t mD0 = pk_dup((int32_t)(2u * d.dd0 + 1u)), mV0 = pk_dup((int32_t)(2u * d.dd0));
                                            const uint32_t E1  = pk_dup(2 * ((int32_t)d.dd1 - (int32_t)d.dd0));
                                            const uint32_t E2  = pk_dup(2 * ((int32_t)d.dd2 - (int32_t)d.dd1));
                                            if (o.mv0 != mD0) return fail("mD0", w, row, o.mv0, mD0);
                                            if (o.mv1 != mV0) return fail("mV0", w, row, o.mv1, mV0);
                                            if (o.mv2 != E1) return fail("E1", w, row, o.mv2, E1);
                                            if (d.cnt3 != 2 && o.mv3 != E2) return fail("E2", w, row, o.mv3, E2);
                                        }
                                    }
    std::printf("ok %ld\n", cases);
    return 0;
}
