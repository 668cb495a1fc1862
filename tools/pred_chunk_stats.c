/* pred_chunk_stats.c -- analysis aid (CPU, oracle side): observes the rows of the oracle's banded forward passes the way
 * mark_score_rows of the packed pass walks them, 64 rows at a time, and counts per pass what that walk used to wait for: the
 * chunks that hold a row with more than three predecessors, the dependent HBM round trips of such a chunk when predecessors 3
 * and up come from the edge list (row -> node, then in-edge -> its row for every further predecessor of the chunk's widest
 * row), and the rows the side table of predecessors 3..5 cannot serve (more than six predecessors; a slot taken by a later row
 * of the same pass). Built by tools/pred_chunk_stats.py into tools/bin/ as a library of its own: the script puts pcs_hook into
 * the stock oracle library's poa_oracle_row_hook. TEST/ANALYSIS INFRASTRUCTURE ONLY. */
#include <stdint.h>
#include <string.h>

enum { kMaxRows = 4096 };
static int32_t cnt_of[kMaxRows];
static int32_t rows_in_pass;
/* passes, rows, chunks, chunks with a wide row, round trips, rows with 4..6, rows with more than 6, rows that lost their slot */
static int64_t totals[8];

static void close_pass(void)
{
    int32_t owner[256];
    if (rows_in_pass == 0) return;
    memset(owner, 0, sizeof(owner));
    totals[0]++;
    totals[1] += rows_in_pass;
    for (int32_t r = 1; r <= rows_in_pass; r++)
        if (cnt_of[r] > 3) owner[r & 255] = r;
    for (int32_t r0 = 1; r0 <= rows_in_pass; r0 += 64)
    {
        int32_t widest = 0;
        for (int32_t r = r0; r < r0 + 64 && r <= rows_in_pass; r++)
        {
            widest = cnt_of[r] > widest ? cnt_of[r] : widest;
            if (cnt_of[r] > 3 && cnt_of[r] <= 6) totals[5]++;
            if (cnt_of[r] > 6) totals[6]++;
            if (cnt_of[r] > 3 && cnt_of[r] <= 6 && owner[r & 255] != r) totals[7]++;
        }
        totals[2]++;
        if (widest > 3)
        {
            totals[3]++;
            totals[4] += 1 + 2 * (widest - 3);
        }
    }
    rows_in_pass = 0;
}

void pcs_hook(int32_t row, int32_t pred_count, int32_t far, int32_t band_start)
{
    (void)far; (void)band_start;
    if (row == 1) close_pass();
    if (row < kMaxRows)
    {
        cnt_of[row]  = pred_count;
        rows_in_pass = row;
    }
}
void pcs_get(int64_t* out)
{
    close_pass();
    memcpy(out, totals, sizeof(totals));
}
