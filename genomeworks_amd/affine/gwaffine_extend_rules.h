// gwaffine_extend_rules.h -- the rules of the affine X-drop extension as plain C++, on top
// of gwaffine_rules.h: the derived costs and their ranges, the extension band and its bit matrix, the stop test, the
// order of end cells, the serial forward pass with the stop rule (extend_serial) and the traceback from a given cell
// (walk_back_from). No HIP in it: the kernels of gwaffine_extend.h include it, and a host program runs the same code
// serially (tests/cpp/extend_cells_sanitized.cpp does, under the sanitizers).
//
// Scores are maximised: match +a, mismatch -x, a gap run of L columns -(o + L e). With x' = 2 (a + x), o' = 2 o,
// e' = a + 2 e and H' the cost matrix of section 3o under (x', o', e') from H'[0][0] = 0, the best score of Q[:i] with
// T[:j] is (a (i + j) - H'[i][j]) / 2. Everything here works in the doubled score D = a (i + j) - H', and the cell
// update, its ties, the cell's byte and the traceback step are those of gwaffine_rules.h, not copies of them.
//
// Diagonals d = j - i in [-B, B] whatever n and m are; k = d + B, W = 2 B + 1; rows 0 .. a_max of the bit matrix.
#ifndef GWAFFINE_EXTEND_RULES_H
#define GWAFFINE_EXTEND_RULES_H

#include "gwaffine_rules.h"

namespace gwaffine
{

constexpr int64_t kMaxExtendBand = 511;              // W <= 1023: at most 16 diagonals a lane
constexpr int64_t kMaxXdrop      = int64_t(1) << 20; // or -1: never stop
constexpr int32_t kNoTop         = -(1 << 30);       // the top of an anti-diagonal without a finite cell

struct ExtendScores
{
    int32_t match, mismatch, gap_open, gap_extend;
};

GWAFFINE_HD bool extend_in_range(int64_t a, int64_t x, int64_t o, int64_t e, int64_t band, int64_t xdrop)
{
    return a >= 1 && x >= 0 && o >= 0 && e >= 1 && a + x <= 127 && o <= 127 && a + 2 * e <= 255 && band >= 0 &&
           band <= kMaxExtendBand && xdrop >= -1 && xdrop <= kMaxXdrop;
}

// the costs under which section 3o's DP is the extension's
GWAFFINE_HD Costs derived_costs(const ExtendScores& s)
{
    return Costs{2 * (s.match + s.mismatch), 2 * s.gap_open, s.match + 2 * s.gap_extend};
}

// the extension's band as a Band: lo = -B, hi = B; aligned is false for n + m >= kMaxColumns (no result)
GWAFFINE_HD Band extend_band_of(int64_t n, int64_t m, int64_t B)
{
    Band b;
    b.n       = n;
    b.m       = m;
    b.lo      = -B;
    b.hi      = B;
    b.W       = 2 * B + 1;
    b.stride  = (((b.W + 2) >> 1) + 3) & ~int64_t(3);
    b.aligned = B <= kMaxExtendBand && n + m < kMaxColumns;
    return b;
}

// the last anti-diagonal that holds a cell
GWAFFINE_HD int64_t extend_a_max(const Band& b)
{
    const int64_t all = b.n + b.m, banded = 2 * (b.n < b.m ? b.n : b.m) + b.hi;
    return all < banded ? all : banded;
}

// bytes of the pair's bit matrix: a_max + 1 rows (0 for a pair without a result), rounded up to 256
GWAFFINE_HD int64_t extend_bits_bytes(const Band& b)
{
    return b.aligned ? (((extend_a_max(b) + 1) * b.stride + 255) & ~int64_t(255)) : 0;
}

// the doubled score of a cell of anti-diagonal a whose cost is h (kNoTop for an absent cell)
GWAFFINE_HD int32_t doubled_score(int32_t match, int32_t a, int32_t h)
{
    return h < kInf ? match * a - h : kNoTop;
}

// after anti-diagonal a >= 1 with tops top and top_before (of a - 1), `best` including a: does the extension stop?
GWAFFINE_HD bool extend_stops(int32_t top, int32_t top_before, int32_t best, int32_t xdrop)
{
    return xdrop >= 0 && (top > top_before ? top : top_before) < best - 2 * xdrop;
}

// the end cell so far: the largest D, then the smallest anti-diagonal, then the smallest diagonal index
struct EndCell
{
    int32_t D, a, k;
};

GWAFFINE_HD bool end_cell_before(const EndCell& x, const EndCell& y)
{
    return x.D != y.D ? x.D > y.D : x.a != y.a ? x.a < y.a : x.k < y.k;
}

struct Extended
{
    int32_t query_end, target_end, score; // -1 each: no result
    int32_t dropped;
    int32_t a_stop; // the last anti-diagonal that counts
};

// The traceback of an extension from cell (i, j) in H, serially: states back to front at out[0 .. i + j), returns
// their number; -1 as walk_back.
GWAFFINE_HD int32_t walk_back_from(const Band& b, const uint8_t* bits, int64_t i, int64_t j, int8_t* out)
{
    Walk w{i, j, 0};
    const int64_t cap = i + j;
    int64_t len       = 0;
    while (w.i != 0 || w.j != 0 || w.matrix != 0)
    {
        if (w.i < 0 || w.j < 0 || w.j - w.i < b.lo || w.j - w.i > b.hi)
            return -1;
        const int32_t s = walk_step(w, bits[bits_index(b, w.i, w.j)]);
        if (s >= 0)
        {
            if (len >= cap)
                return -1;
            out[len++] = static_cast<int8_t>(s);
        }
    }
    return static_cast<int32_t>(len);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// Forward pass, stop rule and end cell, serially in the wavefront's own order and storage. h, e, f: [W] each; bits:
// extend_bits_bytes(b), or nullptr for the score alone.
inline Extended extend_serial(const Band& b, const char* q, const char* t, const ExtendScores& s, int32_t xdrop,
                              int32_t* h, int32_t* e, int32_t* f, uint8_t* bits)
{
    const Costs c = derived_costs(s);
    for (int64_t k = 0; k < b.W; ++k)
        h[k] = e[k] = f[k] = kInf;
    h[-b.lo] = 0;
    if (bits)
        bits[bits_index(b, 0, 0)] = 0;
    EndCell end{0, 0, static_cast<int32_t>(-b.lo)};
    int32_t top_before = 0;
    Extended r{0, 0, 0, 0, 0};
    const int64_t a_max = extend_a_max(b);
    for (int64_t a = 1; a <= a_max; ++a)
    {
        int32_t top = kNoTop;
        for (int64_t k = (a + b.lo) & 1; k < b.W; k += 2)
        {
            const int64_t d = k + b.lo, i = (a - d) >> 1, j = (a + d) >> 1;
            if (i < 0 || j < 0 || i > b.n || j > b.m)
            {
                h[k] = e[k] = f[k] = kInf;
                continue;
            }
            const bool inner = i > 0 && j > 0;
            const Cell u     = cell_update(inner ? h[k] : kInf, k > 0 && j > 0 ? h[k - 1] : kInf,
                                           k > 0 && j > 0 ? e[k - 1] : kInf, k + 1 < b.W && i > 0 ? h[k + 1] : kInf,
                                           k + 1 < b.W && i > 0 ? f[k + 1] : kInf,
                                           inner && bases_match(q[i - 1], t[j - 1]), c);
            h[k] = u.h;
            e[k] = u.e;
            f[k] = u.f;
            if (bits)
                bits[bits_index(b, i, j)] = static_cast<uint8_t>(u.bits);
            const EndCell here{doubled_score(s.match, static_cast<int32_t>(a), u.h), static_cast<int32_t>(a),
                               static_cast<int32_t>(k)};
            if (here.D > top)
                top = here.D;
            if (end_cell_before(here, end))
                end = here;
        }
        r.a_stop = static_cast<int32_t>(a);
        if (extend_stops(top, top_before, end.D, xdrop))
        {
            r.dropped = 1;
            break;
        }
        top_before = top;
    }
    const int64_t d = end.k + b.lo;
    r.query_end     = static_cast<int32_t>((end.a - d) >> 1);
    r.target_end    = static_cast<int32_t>((end.a + d) >> 1);
    r.score         = end.D / 2;
    return r;
}
#endif

} // namespace gwaffine

#endif
