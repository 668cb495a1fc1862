// gwaffine2_rules.h -- the rules of the two-piece affine-gap global aligner as plain C++,
// next to gwaffine_rules.h, whose band geometry, bit-matrix layout, match predicate and kInf it shares: the per-cell
// update over five matrices, the traceback step, the optimality bound and the serial forms of both passes. No HIP in
// it: the kernels of gwaffine.hip include it, and a host program can run the very same code serially
// (tests/cpp/affine2_cells_sanitized.cpp does, under the sanitizers).
//
// Costs are minimised, a match costs 0, a gap run of L columns costs g(L) = min(o1 + L e1, o2 + L e2). A cell keeps one
// byte: bits 0-2 src of H (0 diagonal, 1 E1, 2 F1, 3 E2, 4 F2), bit 3 E1ext, bit 4 F1ext, bit 5 E2ext, bit 6 F2ext,
// bit 7 "the diagonal step into this cell is a mismatch". This layout is the two-piece aligner's alone.
#ifndef GWAFFINE2_RULES_H
#define GWAFFINE2_RULES_H

#include "gwaffine_rules.h"

namespace gwaffine
{

constexpr int64_t kMaxDiagonals2 = 1024; // GWHIP_AFFINE2_MAX_DIAGONALS: 16 diagonals a lane

constexpr uint32_t kSrcMask2 = 7u, kSrcE1 = 1u, kSrcF1 = 2u, kSrcE2 = 3u, kSrcF2 = 4u;
constexpr uint32_t kE1ext = 8u, kF1ext = 16u, kE2ext = 32u, kF2ext = 64u, kMismatch2 = 128u;

struct Costs2
{
    int32_t mismatch, gap_open, gap_extend, gap_open2, gap_extend2;
};

GWAFFINE_HD bool costs2_in_range(int64_t x, int64_t o1, int64_t e1, int64_t o2, int64_t e2, int64_t band)
{
    return costs_in_range(x, o1, e1, band) && o2 >= 0 && o2 <= 255 && e2 >= 1 && e2 <= 255;
}

// the band of gwaffine_rules.h; a pair of more than kMaxDiagonals2 diagonals gets no result
GWAFFINE_HD Band band_of2(int64_t n, int64_t m, int64_t B)
{
    Band b    = band_of(n, m, B);
    b.aligned = b.aligned && b.W <= kMaxDiagonals2;
    return b;
}

// g(L), L >= 1
GWAFFINE_HD int64_t gap_cost2(int64_t L, const Costs2& c)
{
    const int64_t a = int64_t(c.gap_open) + L * int64_t(c.gap_extend), b = int64_t(c.gap_open2) + L * int64_t(c.gap_extend2);
    return a < b ? a : b;
}

// A path that leaves the band through either edge holds at least B + 1 gap columns of one kind and B + 1 + |m - n| of
// the other; g is non-decreasing and sub-additive, so one whole run of each is the cheapest way to hold them.
GWAFFINE_HD bool cost_is_optimal2(int64_t cost, int64_t n, int64_t m, int64_t B, const Costs2& c)
{
    const int64_t diff = m > n ? m - n : n - m;
    return cost <= gap_cost2(B + 1, c) + gap_cost2(B + 1 + diff, c);
}

struct Cell2
{
    int32_t h, e1, f1, e2, f2;
    uint32_t bits;
};

// one gap matrix's value at a cell from its own value and H at the cell the gap comes from: extension before opening
GWAFFINE_HD int32_t gap_update2(int32_t g_from, int32_t h_from, int32_t open, int32_t extend, uint32_t ext_bit, uint32_t& bits)
{
    const int32_t ext = g_from + extend, opn = h_from + open + extend;
    if (g_from < kInf && ext <= opn)
    {
        bits |= ext_bit;
        return ext;
    }
    return h_from < kInf ? opn : kInf;
}

// Cell (i, j), not (0, 0), from H[i-1][j-1] (h_diag), H, E1 and E2 of (i, j-1) and H, F1 and F2 of (i-1, j); kInf
// stands for a cell that is absent or outside the matrix. H takes the diagonal, E1, F1, E2, F2 in this order, a later
// one only when strictly smaller.
GWAFFINE_HD Cell2 cell_update2(int32_t h_diag, int32_t h_left, int32_t e1_left, int32_t e2_left, int32_t h_up, int32_t f1_up,
                               int32_t f2_up, bool match, const Costs2& c)
{
    Cell2 r;
    r.bits    = match ? 0u : kMismatch2;
    r.e1      = gap_update2(e1_left, h_left, c.gap_open, c.gap_extend, kE1ext, r.bits);
    r.f1      = gap_update2(f1_up, h_up, c.gap_open, c.gap_extend, kF1ext, r.bits);
    r.e2      = gap_update2(e2_left, h_left, c.gap_open2, c.gap_extend2, kE2ext, r.bits);
    r.f2      = gap_update2(f2_up, h_up, c.gap_open2, c.gap_extend2, kF2ext, r.bits);
    int32_t h = h_diag < kInf ? h_diag + (match ? 0 : c.mismatch) : kInf;
    uint32_t src = 0;
    if (r.e1 < h)
    {
        h   = r.e1;
        src = kSrcE1;
    }
    if (r.f1 < h)
    {
        h   = r.f1;
        src = kSrcF1;
    }
    if (r.e2 < h)
    {
        h   = r.e2;
        src = kSrcE2;
    }
    if (r.f2 < h)
    {
        h   = r.f2;
        src = kSrcF2;
    }
    r.bits |= src;
    r.h = h;
    return r;
}

struct Walk2
{
    int64_t i, j;
    int32_t matrix; // 0 H, 1 E1, 2 F1, 3 E2, 4 F2
};

// One step of the traceback at (w.i, w.j) in w.matrix, whose cell has `bits`: returns the state it emits (0..3) or
// -1 for a switch of matrix (5, 6 and 7 are no src: H stays, the caller's guards end such a walk). A gap matrix
// returns to H when its ext bit is clear: E2 and F2 open from H, never from E1 or F1. The walk ends at (0, 0) in H.
GWAFFINE_HD int32_t walk_step2(Walk2& w, uint32_t bits)
{
    if (w.matrix == 0)
    {
        const uint32_t src = bits & kSrcMask2;
        if (src != 0 && src <= kSrcF2)
        {
            w.matrix = static_cast<int32_t>(src);
            return -1;
        }
        --w.i;
        --w.j;
        return (bits & kMismatch2) ? 1 : 0;
    }
    const bool target_only = w.matrix == 1 || w.matrix == 3;
    const uint32_t ext_bit = w.matrix == 1 ? kE1ext : w.matrix == 2 ? kF1ext : w.matrix == 3 ? kE2ext : kF2ext;
    if (target_only)
        --w.j;
    else
        --w.i;
    if (!(bits & ext_bit))
        w.matrix = 0;
    return target_only ? 2 : 3;
}

// The whole traceback of an aligned pair, serially, as walk_back of gwaffine_rules.h: states back to front at
// out[0 .. n + m), returns their number, or -1 when the bits lead out of the band or past the slot.
GWAFFINE_HD int32_t walk_back2(const Band& b, const uint8_t* bits, int8_t* out)
{
    Walk2 w{b.n, b.m, 0};
    int64_t len = 0;
    while (w.i != 0 || w.j != 0 || w.matrix != 0)
    {
        if (w.i < 0 || w.j < 0 || w.j - w.i < b.lo || w.j - w.i > b.hi)
            return -1;
        const int32_t s = walk_step2(w, bits[bits_index(b, w.i, w.j)]);
        if (s >= 0)
        {
            if (len >= b.n + b.m)
                return -1;
            out[len++] = static_cast<int8_t>(s);
        }
    }
    return static_cast<int32_t>(len);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The forward pass run serially in the wavefront's own order and storage: five values per diagonal, updated in place
// anti-diagonal by anti-diagonal. v: [5 W] as H, E1, F1, E2, F2 of W each; bits: bits_bytes(b). Returns H[n][m].
inline int32_t forward_serial2(const Band& b, const char* q, const char* t, const Costs2& c, int32_t* v, uint8_t* bits)
{
    int32_t *h = v, *e1 = v + b.W, *f1 = v + 2 * b.W, *e2 = v + 3 * b.W, *f2 = v + 4 * b.W;
    for (int64_t k = 0; k < 5 * b.W; ++k)
        v[k] = kInf;
    for (int64_t a = 0; a <= b.n + b.m; ++a)
        for (int64_t k = (a + b.lo) & 1; k < b.W; k += 2)
        {
            const int64_t d = k + b.lo, i = (a - d) >> 1, j = (a + d) >> 1;
            if (i < 0 || j < 0 || i > b.n || j > b.m)
            {
                h[k] = e1[k] = f1[k] = e2[k] = f2[k] = kInf;
                continue;
            }
            if (a == 0)
            {
                h[k]                      = 0;
                bits[bits_index(b, 0, 0)] = 0;
                continue;
            }
            const bool inner = i > 0 && j > 0, left = k > 0 && j > 0, up = k + 1 < b.W && i > 0;
            const Cell2 r = cell_update2(inner ? h[k] : kInf, left ? h[k - 1] : kInf, left ? e1[k - 1] : kInf,
                                         left ? e2[k - 1] : kInf, up ? h[k + 1] : kInf, up ? f1[k + 1] : kInf,
                                         up ? f2[k + 1] : kInf, inner && bases_match(q[i - 1], t[j - 1]), c);
            h[k]  = r.h;
            e1[k] = r.e1;
            f1[k] = r.f1;
            e2[k] = r.e2;
            f2[k] = r.f2;
            bits[bits_index(b, i, j)] = static_cast<uint8_t>(r.bits);
        }
    return h[b.m - b.n - b.lo];
}
#endif

} // namespace gwaffine

#endif
