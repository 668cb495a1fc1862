/* oracle_extender.c -- sequential CPU statement of cudaextender's ungapped X-drop extension (the contract the HIP
 * library in genomeworks_amd/extender/ must reproduce bit for bit). One seed at a time, one position at a time; no
 * tiles, so the result cannot depend on a tile width. Built by tests/oracle_extender.py with -ffp-contract=off.
 *
 * Sequences are encoded A=0 C=1 G=2 T=3 L=4 N=5 X=6 E=7; the score of a column is M[8*t + q]. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* One output row, in the memory order of ScoredSegmentPair {query, target, length, score}. */
typedef struct
{
    uint32_t query;
    uint32_t target;
    int32_t length;
    int32_t score;
} gwx_segment;

/* X-drop walk from (t, q) in direction dir (+1: offsets 0, 1, ...; -1: offsets 1, 2, ...). Returns the best prefix
 * score (0 if none is positive) and stores the offset of its first occurrence (or `none_pos`) in *pos. */
static int32_t walk(const int8_t* T, int64_t tlen, const int8_t* Q, int64_t qlen, const int32_t* M, int32_t X,
                    int64_t t, int64_t q, int dir, int32_t none_pos, int32_t* pos)
{
    int32_t s = 0, m = 0;
    *pos = none_pos;
    for (int64_t k = (dir > 0 ? 0 : 1);; k++)
    {
        const int64_t tt = dir > 0 ? t + k : t - k, qq = dir > 0 ? q + k : q - k;
        if (tt < 0 || qq < 0 || tt >= tlen || qq >= qlen) break;
        s += M[8 * T[tt] + Q[qq]];
        if (s > m)
        {
            m    = s;
            *pos = (int32_t)k;
        }
        if (m - s > X) break;
    }
    return m;
}

/* Extends one seed. Returns 1 and fills *out when the seed yields a segment. */
int gwx_oracle_extend_one(const int8_t* T, int64_t tlen, const int8_t* Q, int64_t qlen, const int32_t* M, int32_t X,
                          int32_t thr, int32_t no_entropy, uint32_t t, uint32_t q, gwx_segment* out)
{
    if ((int64_t)t >= tlen || (int64_t)q >= qlen) return 0;
    int32_t rpos, lpos;
    const int32_t R      = walk(T, tlen, Q, qlen, M, X, t, q, +1, -1, &rpos);
    const int32_t L      = walk(T, tlen, Q, qlen, M, X, t, q, -1, 0, &lpos);
    const int32_t total  = R + L;
    const int32_t extent = rpos + lpos;
    double e             = 1.0;
    if (!no_entropy && total >= thr && total <= 3 * thr)
    {
        int32_t c[4] = {0, 0, 0, 0};
        for (int32_t j = -lpos; j <= rpos; j++)
        {
            const int8_t a = T[(int64_t)t + j], b = Q[(int64_t)q + j];
            if (a == b && a >= 0 && a < 4) c[a]++;
        }
        if (c[0] + c[1] + c[2] + c[3] >= 20)
        {
            double acc = 0.0;
            for (int b = 0; b < 4; b++)
            {
                if (c[b] > 0)
                {
                    const double p = (double)c[b] / (double)(extent + 1);
                    acc += p * log(p);
                }
            }
            e = -acc / (double)logf(4.0f);
        }
    }
    const int32_t score = (int32_t)((double)total * e);
    if (score < thr) return 0;
    out->target = t - (uint32_t)lpos;
    out->query  = q - (uint32_t)lpos;
    out->length = extent;
    out->score  = score;
    return 1;
}

static int seg_less(const gwx_segment* x, const gwx_segment* y)
{
    const uint32_t dx = x->target - x->query, dy = y->target - y->query;
    if (dx != dy) return dx < dy;
    if (x->target != y->target) return x->target < y->target;
    if (x->length != y->length) return x->length > y->length;
    return x->score > y->score;
}

/* same unsigned diagonal and one [target, target + length] interval (uint32 arithmetic) inside the other */
int gwx_oracle_overlap(const gwx_segment* x, const gwx_segment* y)
{
    if (x->target - x->query != y->target - y->query) return 0;
    const uint32_t xe = x->target + (uint32_t)x->length, ye = y->target + (uint32_t)y->length;
    return (x->target >= y->target && xe <= ye) || (y->target >= x->target && ye <= xe);
}

/* Stable sort of seg[0..n) (insertion into a merge sort, both stable), then the adjacent de-duplication of
 * thrust::unique_copy: element i is dropped when it overlaps input element i-1, kept or not. Returns the new count. */
int64_t gwx_oracle_sort_unique(gwx_segment* seg, int64_t n)
{
    if (n <= 0) return 0;
    gwx_segment* tmp = (gwx_segment*)malloc((size_t)n * sizeof(gwx_segment));
    for (int64_t w = 1; w < n; w *= 2)
    {
        for (int64_t lo = 0; lo < n; lo += 2 * w)
        {
            int64_t mid = lo + w < n ? lo + w : n, hi = lo + 2 * w < n ? lo + 2 * w : n, a = lo, b = mid, o = lo;
            while (a < mid && b < hi) tmp[o++] = seg_less(&seg[b], &seg[a]) ? seg[b++] : seg[a++];
            while (a < mid) tmp[o++] = seg[a++];
            while (b < hi) tmp[o++] = seg[b++];
        }
        memcpy(seg, tmp, (size_t)n * sizeof(gwx_segment));
    }
    int64_t kept = 1;
    for (int64_t i = 1; i < n; i++)
        if (!gwx_oracle_overlap(&tmp[i - 1], &tmp[i])) seg[kept++] = tmp[i];
    free(tmp);
    return kept;
}

/* The whole extend call: seeds (target[i], query[i]) in chunks of `chunk` seeds (<= 0: one chunk); each chunk is
 * extended, compacted in seed order, sorted and de-duplicated on its own and appended to out. Returns the count. */
int64_t gwx_oracle_extend(const int8_t* T, int64_t tlen, const int8_t* Q, int64_t qlen, const int32_t* M, int32_t X,
                          int32_t thr, int32_t no_entropy, const uint32_t* seed_t, const uint32_t* seed_q, int64_t n,
                          int64_t chunk, gwx_segment* out)
{
    if (chunk <= 0) chunk = n > 0 ? n : 1;
    int64_t total = 0;
    for (int64_t c0 = 0; c0 < n; c0 += chunk)
    {
        const int64_t c1 = c0 + chunk < n ? c0 + chunk : n;
        int64_t k        = 0;
        for (int64_t i = c0; i < c1; i++)
            k += gwx_oracle_extend_one(T, tlen, Q, qlen, M, X, thr, no_entropy, seed_t[i], seed_q[i], &out[total + k]);
        total += gwx_oracle_sort_unique(out + total, k);
    }
    return total;
}
