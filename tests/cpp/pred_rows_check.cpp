// pred_rows_check.cpp -- a stand-alone check of the decode of a row's predecessor rows from the packed row table and the side
// table of predecessors 3..5 (genomeworks_amd/csrc/poa_pred_rows.h), built by tests/test_pred_rows.py once plain and once under
// -fsanitize=address,undefined. Random graphs' rows (predecessor lists of 0..3, 4..6 and 7+ rows, up to 4095 rows, so that
// rows 256 apart fight for a slot) are put into table words and into a side table the way build_rowinfo does it -- ascending
// rows, the last writer of a slot wins -- and every row's answer is compared with the plain statement: its predecessors are all
// in LDS when it has at most three, or four to six and still owns its slot; they are then its list. Entries that must not hit
// are made by hand as well: another row's entry, the row's own with a wrong count, a cleared valid bit, the empty slot.
// Prints "ok <rows checked> <hits> <lost slots> <rows with 7+>", or the first mismatch.
#include "../../genomeworks_amd/csrc/poa_pred_rows.h"

#include <cstdio>
#include <random>
#include <vector>

namespace
{

// the row-table word as the kernels build it: gwhip::table_word (what RowInfo<true>::set stores), then the fields the forward
// pass adds -- band start / 4 [15:24) (set_bs), row kind [60:63) (classify_kinds), scores to HBM [63] (mark_score_rows)
uint64_t full_table_word(uint32_t base, uint32_t cnt, bool sink, uint32_t bs, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t kind, bool scores)
{
    return gwhip::table_word((int32_t)base, (int32_t)cnt, sink, (int32_t)p0, (int32_t)p1, (int32_t)p2) | ((uint64_t)((bs >> 2) & 0x1ff) << 15) |
           ((uint64_t)kind << 60) | ((uint64_t)(scores ? 1 : 0) << 63);
}

int fail(const char* what, int32_t row, long got, long want)
{
    std::printf("mismatch in %s: row %d: %ld, expected %ld\n", what, row, got, want);
    return 1;
}

} // namespace

int main()
{
    using namespace gwhip;
    std::mt19937 rng(20240611u);
    long checked = 0, hits = 0, lost = 0, wide = 0;
    const int32_t sizes[] = {1, 3, 200, 256, 257, 700, 2048, 4095};
    for (int round = 0; round < 40; round++)
        for (int32_t n : sizes)
        {
            // rows 1..n with their predecessor lists (row 0 = the virtual source); the share of rows with many predecessors
            // grows with the round, so that early rounds have few collisions and late ones many
            std::vector<std::vector<int32_t>> preds(n + 1);
            std::vector<uint64_t> word(n + 1, 0);
            std::vector<uint64_t> side(kSideTableSlots, 0);
            std::vector<int32_t> owner(kSideTableSlots, -1); // plain statement: the last row with more than three that wrote the slot
            for (int32_t r = 1; r <= n; r++)
            {
                const uint32_t dice = rng() % 100u;
                int32_t cnt = dice < (uint32_t)(90 - 2 * round) ? (int32_t)(rng() % 4u) : (dice < 97u ? 4 + (int32_t)(rng() % 3u) : 7 + (int32_t)(rng() % 44u));
                for (int32_t k = 0; k < cnt; k++) preds[r].push_back((int32_t)(rng() % (uint32_t)r)); // any earlier row, near or far
                const int32_t p0 = cnt > 0 ? preds[r][0] : 0, p1 = cnt > 1 ? preds[r][1] : 0, p2 = cnt > 2 ? preds[r][2] : 0;
                word[r] = full_table_word("ACGT"[rng() & 3u], (uint32_t)cnt, (rng() & 1u) != 0, (rng() % 512u) * 4u, p0, p1, p2, rng() % 5u, (rng() & 1u) != 0);
                if (cnt > kTablePreds)
                {
                    // (build_rowinfo: slots past the in-degree hold whatever the edge list held; any 12-bit value here)
                    const int32_t p3 = preds[r][3], p4 = cnt > 4 ? preds[r][4] : (int32_t)(rng() & 0xfffu), p5 = cnt > 5 ? preds[r][5] : (int32_t)(rng() & 0xfffu);
                    side[r & (kSideTableSlots - 1)]  = xpred_entry(r, cnt, p3, p4, p5);
                    owner[r & (kSideTableSlots - 1)] = r;
                }
            }
            for (int32_t r = 1; r <= n; r++)
            {
                const int32_t cnt = (int32_t)preds[r].size();
                if (table_pred_count(word[r]) != cnt) return fail("count", r, table_pred_count(word[r]), cnt);
                for (int32_t k = 0; k < cnt && k < kTablePreds; k++)
                    if (table_pred_row(word[r], k) != preds[r][k]) return fail("table predecessor", r, table_pred_row(word[r], k), preds[r][k]);
                const bool want_entry = cnt >= 4 && cnt <= 6;
                if (pred_rows_want_entry(cnt) != want_entry) return fail("wants its entry", r, pred_rows_want_entry(cnt), want_entry);
                // what a reader does: load the slot only when the row can use it
                const uint64_t e   = want_entry ? side[r & (kSideTableSlots - 1)] : 0ull;
                const bool in_lds  = cnt <= 3 || (cnt <= 6 && owner[r & (kSideTableSlots - 1)] == r);
                if (pred_rows_in_lds(r, cnt, e) != in_lds) return fail("predecessors in LDS", r, pred_rows_in_lds(r, cnt, e), in_lds);
                // ... and the answer does not depend on that economy: the slot's entry, whatever it is, says the same
                if (pred_rows_in_lds(r, cnt, side[r & (kSideTableSlots - 1)]) != in_lds) return fail("predecessors in LDS (entry always loaded)", r, 0, in_lds);
                if (in_lds)
                    for (int32_t k = 0; k < cnt; k++)
                        if (lds_pred_row(word[r], e, k) != preds[r][k]) return fail("predecessor row", r, lds_pred_row(word[r], e, k), preds[r][k]);
                checked++;
                hits += want_entry && in_lds;
                lost += want_entry && !in_lds;
                wide += cnt > 6;
                if (want_entry && in_lds)
                {
                    // entries that must not hit: the row's own with a wrong count or without its valid bit, a neighbour's, none
                    for (int32_t other = 0; other < 64; other++)
                        if (other != cnt && xpred_hit(xpred_entry(r, other, preds[r][3], 0, 0), r, cnt)) return fail("hit with a wrong count", r, other, cnt);
                    if (xpred_hit(e & ~(1ull << 12), r, cnt)) return fail("hit without the valid bit", r, 1, 0);
                    if (xpred_hit(e, r ^ 256, cnt) || xpred_hit(e, (r + 1) & 0xfff, cnt)) return fail("hit for another row", r, 1, 0);
                    if (xpred_hit(0ull, r, cnt)) return fail("hit in an empty slot", r, 1, 0);
                }
            }
        }
    // the empty slot never hits, not even for row 0 with no predecessors
    if (xpred_hit(0ull, 0, 0)) return fail("hit in an empty slot for row 0", 0, 1, 0);
    std::printf("ok %ld %ld %ld %ld\n", checked, hits, lost, wide);
    return 0;
}
