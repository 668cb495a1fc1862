/* oracle_mapper.c -- plain-C, single-thread restatement of cudamapper: (k,w)-minimizer sketch -> index (stable sort,
 * unique representations, frequency filter) -> anchors -> triggered overlapper (chain, fuse, filter). The rules are
 * those of GenomeWorks' cudamapper (DESIGN.md "cudamapper"); the GPU path (genomeworks_amd/mapper/) must match it
 * array for array. Built by tests/oracle_mapper.py with the system C compiler. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct
{
    uint32_t qr, tr, qp, tp;
} om_anchor;

typedef struct
{
    uint32_t qr, tr, qs, ts, qe, te;
    uint8_t strand;
    uint32_t residues;
    uint8_t complete;
} om_overlap;

static uint64_t wang_hash64(uint64_t key)
{
    const uint64_t mask = (UINT64_C(1) << 32) - 1;
    key                 = (~key + (key << 21)) & mask;
    key                 = key ^ key >> 24;
    key                 = ((key + (key << 3)) + (key << 8)) & mask;
    key                 = key ^ key >> 14;
    key                 = ((key + (key << 2)) + (key << 4)) & mask;
    key                 = key ^ key >> 28;
    key                 = (key + (key << 31)) & mask;
    return key;
}

/* the reference shifts an int: shifts >= 32 give 0 and a set bit 31 sign-extends into the 64-bit representation */
static uint64_t place(uint32_t code, uint32_t shift)
{
    if (shift >= 32)
        return 0;
    return (uint64_t)(int64_t)(int32_t)(code << shift);
}

static const uint8_t kComplement[8] = {0, 4, 0, 7, 1, 0, 0, 3};

/* Sketch: capacity of the outputs is sum over kept reads of (len - k + w). Returns the number of elements, in read
 * and position order. A read shorter than k + w - 1 is skipped and the reads after it take its id. Needs k + w <= 513.
 * direction_mode 0: dir_out is the strand of the minimizer (0 forward, 1 reverse) -- what the GPU path gives;
 * 1: the byte the reference gives, which for some elements of reads of more than one central step is a byte of a window
 * position (see below); 2: 1 for exactly those elements, else 0. */
int64_t om_sketch(const char* bases, const int64_t* offsets, int32_t n_reads, uint32_t first_read_id, int32_t k,
                  int32_t w, int32_t hash, int32_t direction_mode, uint64_t* rep_out, uint32_t* rid_out,
                  uint32_t* pos_out, uint8_t* dir_out)
{
    int64_t n       = 0;
    uint32_t rank   = 0;
    int64_t longest = 0;
    for (int32_t r = 0; r < n_reads; ++r)
        if (offsets[r + 1] - offsets[r] > longest)
            longest = offsets[r + 1] - offsets[r];
    uint64_t* rep = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(longest + 1));
    uint8_t* dir  = (uint8_t*)malloc((size_t)(longest + 1));
    int64_t* at_of = (int64_t*)malloc(sizeof(int64_t) * (size_t)(longest + w + 1));
    for (int32_t r = 0; r < n_reads; ++r)
    {
        const unsigned char* s = (const unsigned char*)bases + offsets[r];
        const int64_t len      = offsets[r + 1] - offsets[r];
        if (len < (int64_t)k + w - 1)
            continue;
        const int64_t nk = len - k + 1;
        for (int64_t p = 0; p < nk; ++p)
        {
            uint64_t f = 0, rv = 0;
            for (int32_t i = 0; i < k; ++i)
            {
                const uint32_t b  = s[p + i];
                const uint32_t ct = kComplement[b & 7];
                f |= place(3u & ((b >> 2) ^ (b >> 1)), 2u * (uint32_t)(k - i - 1));
                rv |= place(3u & ((ct >> 2) ^ (ct >> 1)), 2u * (uint32_t)i);
            }
            if (hash)
            {
                f  = wang_hash64(f);
                rv = wang_hash64(rv);
            }
            rep[p] = f <= rv ? f : rv;
            dir[p] = f <= rv ? 0 : 1;
        }
        /* window j covers k-mers [max(0, j-w+1), min(nk-1, j)]; the last smallest wins */
        const int64_t nw = nk + w - 1, wir = nk - w + 1; /* all windows; the central ones are j in [w-1, w-1+wir) */
        for (int64_t j = 0; j < nw; ++j)
        {
            const int64_t lo = j - w + 1 > 0 ? j - w + 1 : 0;
            const int64_t hi = j < nk - 1 ? j : nk - 1;
            int64_t at       = lo;
            for (int64_t i = lo + 1; i <= hi; ++i)
                if (rep[i] <= rep[at])
                    at = i;
            at_of[j] = at;
        }
        /* A window emits its minimizer when it sits elsewhere than its left neighbour's. The reference walks the central
         * windows in steps of s = 514 - k - w (64 threads x 8 bases) and hands the last window's position from step to step
         * through a carry that the thread `s % 64 - 1` stores: when s is a multiple of 64 (k + w = 2 mod 64) no thread does, the
         * carry keeps its first value -- the position of the last front-end element, 0 when w == 1 -- and the first window of
         * every later step is compared with that. The first back-end window is compared with the last element written. */
        const int64_t step = (int64_t)(uint16_t)((uint16_t)(512 - (k - 1)) - (w - 1));
        int64_t carry = 0, written = -1;
        for (int64_t j = 0; j < nw; ++j)
        {
            const int64_t c  = j - (w - 1); /* central window number */
            const int64_t at = at_of[j];
            int central      = c >= 0 && c < wir;
            int64_t left;
            if (j == 0)
                left = -1;
            else if (central && c % step == 0)
                left = c == 0 ? written : carry;
            else if (c == wir)
                left = written;
            else
                left = at_of[j - 1];
            if (c == 0)
                carry = written < 0 ? 0 : written;
            if (at != left)
            {
                uint8_t d = dir[at];
                /* the directions of a central step live in an array of `step` bytes, rounded up to 8, that the reference indexes
                 * by k-mer, up to step + w - 2: the bytes behind it are those of the step's window positions (uint32, little
                 * endian), written after the directions and before they are read */
                const int64_t room = (step + 7) / 8 * 8;
                const int aliased  = central && at - c / step * step >= room;
                if (aliased && direction_mode == 1)
                {
                    const int64_t b = at - c / step * step - room;
                    d               = (uint8_t)((uint32_t)at_of[w - 1 + c / step * step + b / 4] >> (8 * (b % 4)));
                }
                if (direction_mode == 2)
                    d = (uint8_t)aliased;
                rep_out[n] = rep[at];
                rid_out[n] = first_read_id + rank;
                pos_out[n] = (uint32_t)at;
                dir_out[n] = d;
                ++n;
                written = at;
            }
            if (central && c % step == step - 1 && c + 1 < wir && step % 64 != 0)
                carry = at;
        }
        ++rank;
    }
    free(rep);
    free(dir);
    free(at_of);
    return n;
}

/* stable merge sort of the permutation `idx` by key[idx] */
static void merge_sort(uint32_t* idx, uint32_t* tmp, int64_t n, const uint64_t* key)
{
    for (int64_t width = 1; width < n; width *= 2)
    {
        for (int64_t lo = 0; lo < n; lo += 2 * width)
        {
            int64_t mid = lo + width < n ? lo + width : n, hi = lo + 2 * width < n ? lo + 2 * width : n;
            int64_t a = lo, b = mid, o = lo;
            while (a < mid && b < hi)
                tmp[o++] = key[idx[b]] < key[idx[a]] ? idx[b++] : idx[a++];
            while (a < mid)
                tmp[o++] = idx[a++];
            while (b < hi)
                tmp[o++] = idx[b++];
        }
        memcpy(idx, tmp, sizeof(uint32_t) * (size_t)n);
    }
}

/* Index from the sketch arrays (in place, n elements): stable sort by representation, unique representations with
 * first occurrences (+ trailing total), then the frequency filter when filtering_parameter < 1. Writes n_out and
 * n_unique_out; unique_out has capacity n, first_out capacity n + 1. */
void om_index(int64_t n, uint64_t* rep, uint32_t* rid, uint32_t* pos, uint8_t* dir, double filtering_parameter,
              uint64_t* unique_out, uint32_t* first_out, int64_t* n_out, int64_t* n_unique_out)
{
    *n_out = *n_unique_out = 0;
    if (n == 0)
        return;
    uint32_t* idx = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)n);
    uint32_t* tmp = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)n);
    for (int64_t i = 0; i < n; ++i)
        idx[i] = (uint32_t)i;
    merge_sort(idx, tmp, n, rep);
    uint64_t* r2 = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)n);
    uint32_t* i2 = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)n);
    uint32_t* p2 = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)n);
    uint8_t* d2  = (uint8_t*)malloc((size_t)n);
    for (int64_t i = 0; i < n; ++i)
    {
        r2[i] = rep[idx[i]];
        i2[i] = rid[idx[i]];
        p2[i] = pos[idx[i]];
        d2[i] = dir[idx[i]];
    }
    int64_t nu = 0;
    for (int64_t i = 0; i < n; ++i)
        if (i == 0 || r2[i] != r2[i - 1])
        {
            unique_out[nu] = r2[i];
            first_out[nu]  = (uint32_t)i;
            ++nu;
        }
    first_out[nu] = (uint32_t)n;
    int64_t m = 0, mu = 0;
    if (filtering_parameter < 1.0)
    {
        const uint64_t threshold = (uint64_t)((double)n * filtering_parameter + 0.001);
        for (int64_t u = 0; u < nu; ++u)
        {
            const uint32_t b = first_out[u], e = first_out[u + 1];
            if ((uint64_t)(e - b) >= threshold)
                continue;
            unique_out[mu] = unique_out[u];
            first_out[mu]  = (uint32_t)m;
            ++mu;
            for (uint32_t i = b; i < e; ++i, ++m)
            {
                rep[m] = r2[i];
                rid[m] = i2[i];
                pos[m] = p2[i];
                dir[m] = d2[i];
            }
        }
        first_out[mu] = (uint32_t)m;
    }
    else
    {
        memcpy(rep, r2, sizeof(uint64_t) * (size_t)n);
        memcpy(rid, i2, sizeof(uint32_t) * (size_t)n);
        memcpy(pos, p2, sizeof(uint32_t) * (size_t)n);
        memcpy(dir, d2, (size_t)n);
        m  = n;
        mu = nu;
    }
    *n_out        = m;
    *n_unique_out = mu;
    free(idx);
    free(tmp);
    free(r2);
    free(i2);
    free(p2);
    free(d2);
}

/* number of anchors between two indices (unique representations ascending) */
int64_t om_count_anchors(const uint64_t* qu, const uint32_t* qf, int64_t nqu, const uint64_t* tu, const uint32_t* tf,
                         int64_t ntu)
{
    int64_t total = 0, j = 0;
    for (int64_t u = 0; u < nqu; ++u)
    {
        while (j < ntu && tu[j] < qu[u])
            ++j;
        if (j < ntu && tu[j] == qu[u])
            total += (int64_t)(qf[u + 1] - qf[u]) * (int64_t)(tf[j + 1] - tf[j]);
    }
    return total;
}

static int cmp_anchor(const void* pa, const void* pb)
{
    const om_anchor* a = (const om_anchor*)pa;
    const om_anchor* b = (const om_anchor*)pb;
    if (a->qr != b->qr)
        return a->qr < b->qr ? -1 : 1;
    if (a->tr != b->tr)
        return a->tr < b->tr ? -1 : 1;
    if (a->qp != b->qp)
        return a->qp < b->qp ? -1 : 1;
    if (a->tp != b->tp)
        return a->tp < b->tp ? -1 : 1;
    return 0;
}

/* all anchors, sorted by (query read, target read, query position, target position) */
int64_t om_anchors(const uint64_t* qu, const uint32_t* qf, int64_t nqu, const uint32_t* qrid, const uint32_t* qpos,
                   const uint64_t* tu, const uint32_t* tf, int64_t ntu, const uint32_t* trid, const uint32_t* tpos,
                   om_anchor* out)
{
    int64_t n = 0, j = 0;
    for (int64_t u = 0; u < nqu; ++u)
    {
        while (j < ntu && tu[j] < qu[u])
            ++j;
        if (!(j < ntu && tu[j] == qu[u]))
            continue;
        for (uint32_t a = qf[u]; a < qf[u + 1]; ++a)
            for (uint32_t b = tf[j]; b < tf[j + 1]; ++b)
            {
                out[n].qr = qrid[a];
                out[n].tr = trid[b];
                out[n].qp = qpos[a];
                out[n].tp = tpos[b];
                ++n;
            }
    }
    qsort(out, (size_t)n, sizeof(om_anchor), cmp_anchor);
    return n;
}

static int same_chain(const om_anchor* prev, const om_anchor* cur)
{
    const int dt = (int)cur->tp - (int)prev->tp;
    return prev->qr == cur->qr && prev->tr == cur->tr && (uint32_t)(cur->qp - prev->qp) < 150u && abs(dt) < 150;
}

static int same_overlap(const om_anchor* a, const om_anchor* b)
{
    const int dq = abs((int)a->qp - (int)b->qp), dt = abs((int)a->tp - (int)b->tp);
    return a->qr == b->qr && a->tr == b->tr && abs(dq - dt) < 300;
}

/* Triggered overlapper; out has capacity n. Returns the number of overlaps kept. */
int64_t om_overlaps(const om_anchor* a, int64_t n, int32_t all_to_all, int64_t min_residues, int64_t min_overlap_len,
                    int64_t min_bases_per_residue, float min_overlap_fraction, om_overlap* out)
{
    int64_t n_out = 0;
    int64_t fused_start = -1, fused_end = 0, fused_first = 0; /* current fused run: anchors, first chain's start */
    uint32_t fused_res = 0;
    int64_t c = 0;
    while (c <= n)
    {
        /* next chain [c, e), or the flush at c == n */
        int64_t e = c + 1;
        while (c < n && e < n && same_chain(&a[e - 1], &a[e]))
            ++e;
        const int kept = c < n && e - c >= 3;
        if (kept && fused_start >= 0 && same_overlap(&a[fused_first], &a[c]))
        {
            fused_end = e;
            fused_res += (uint32_t)(e - c);
            fused_first = c;
        }
        else if (kept || c == n)
        {
            if (fused_start >= 0)
            {
                const om_anchor* s = &a[fused_start];
                const om_anchor* l = &a[fused_end - 1];
                om_overlap o;
                memset(&o, 0, sizeof(o));
                o.qr       = l->qr;
                o.tr       = l->tr;
                o.residues = fused_res;
                o.qs       = s->qp;
                o.qe       = l->qp;
                o.complete = 1;
                if (s->tp > l->tp)
                {
                    o.strand = '-';
                    o.ts     = l->tp;
                    o.te     = s->tp;
                }
                else
                {
                    o.strand = '+';
                    o.ts     = s->tp;
                    o.te     = l->tp;
                }
                const uint32_t tl = o.te - o.ts, ql = o.qe - o.qs, len = tl > ql ? tl : ql;
                const int self    = o.qr == o.tr && all_to_all;
                if (o.residues >= (uint64_t)min_residues && (uint64_t)(len / o.residues) < (uint64_t)min_bases_per_residue &&
                    ql >= (uint64_t)min_overlap_len && tl >= (uint64_t)min_overlap_len && !self &&
                    ((float)tl * 1.f / (float)len) > min_overlap_fraction &&
                    ((float)ql * 1.f / (float)len) > min_overlap_fraction)
                    out[n_out++] = o;
            }
            fused_start = -1;
            if (kept)
            {
                fused_start = c;
                fused_first = c;
                fused_end   = e;
                fused_res   = (uint32_t)(e - c);
            }
        }
        if (c == n)
            break;
        c = e;
    }
    return n_out;
}
