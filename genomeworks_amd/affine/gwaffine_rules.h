// gwaffine_rules.h -- the rules of the affine-gap global aligner as plain C++: the band
// geometry, the layout of the bit matrix in the workspace, the per-cell update, the traceback step and the optimality
// bound. No HIP in it: the kernels of gwaffine.hip include it, and a host program can run the very same code
// serially (forward_serial and walk_back below; tests/cpp/affine_cells_sanitized.cpp does, under the sanitizers).
//
// Costs are minimised, a match costs 0, a gap run of L columns costs o + L e. Diagonal d = j - i, band
// [lo, hi] = [min(0, m - n) - B, max(0, m - n) + B], k = d - lo the diagonal's index, W = hi - lo + 1. Anti-diagonal
// a = i + j holds the cells whose k has the parity of a + lo; cell (i, j) keeps one byte at
// bits[a * stride + (k >> 1)]: bits 0-1 src of H (0 diagonal, 1 E, 2 F), bit 2 Eext, bit 3 Fext, bit 4 "the diagonal
// step into this cell is a mismatch" (so that the traceback reads no sequence).
#ifndef GWAFFINE_RULES_H
#define GWAFFINE_RULES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GWAFFINE_HD __host__ __device__ __forceinline__
#else
#define GWAFFINE_HD inline
#endif

namespace gwaffine
{

constexpr int32_t kInf          = 1 << 29; // an absent cell; every cost of a pair with n + m < 2^21 stays below it
constexpr int64_t kMaxDiagonals = 2048;    // GWHIP_AFFINE_MAX_DIAGONALS
constexpr int64_t kMaxColumns   = int64_t(1) << 21; // n + m below this

constexpr uint32_t kSrcMask = 3u, kSrcE = 1u, kSrcF = 2u, kEext = 4u, kFext = 8u, kMismatch = 16u;

struct Costs
{
    int32_t mismatch, gap_open, gap_extend;
};

GWAFFINE_HD bool costs_in_range(int64_t x, int64_t o, int64_t e, int64_t band)
{
    return x >= 1 && x <= 255 && o >= 0 && o <= 255 && e >= 1 && e <= 255 && band >= 0;
}

struct Band
{
    int64_t n, m;
    int64_t lo, hi, W; // diagonals lo .. hi
    int64_t stride;    // bytes of one anti-diagonal's row of the bit matrix (a multiple of 4)
    bool aligned;      // false: the pair gets no result (W > kMaxDiagonals, or n + m >= kMaxColumns)
};

GWAFFINE_HD Band band_of(int64_t n, int64_t m, int64_t B)
{
    Band b;
    b.n       = n;
    b.m       = m;
    b.lo      = (m < n ? m - n : 0) - B;
    b.hi      = (m > n ? m - n : 0) + B;
    b.W       = b.hi - b.lo + 1;
    b.stride  = (((b.W + 2) >> 1) + 3) & ~int64_t(3);
    b.aligned = b.W <= kMaxDiagonals && n + m < kMaxColumns;
    return b;
}

// bytes of the pair's bit matrix: n + m + 1 rows (0 for a pair that is not aligned), rounded up to 256
GWAFFINE_HD int64_t bits_bytes(const Band& b)
{
    return b.aligned ? (((b.n + b.m + 1) * b.stride + 255) & ~int64_t(255)) : 0;
}

GWAFFINE_HD int64_t bits_index(const Band& b, int64_t i, int64_t j)
{
    return (i + j) * b.stride + ((j - i - b.lo) >> 1);
}

// cost <= the cheapest conceivable path that leaves the band: the cost is the full-matrix optimum
GWAFFINE_HD bool cost_is_optimal(int64_t cost, int64_t n, int64_t m, int64_t B, const Costs& c)
{
    const int64_t diff = m > n ? m - n : n - m;
    return cost <= 2 * int64_t(c.gap_open) + int64_t(c.gap_extend) * (diff + 2 * B + 2);
}

struct Cell
{
    int32_t h, e, f;
    uint32_t bits;
};

// Cell (i, j), not (0, 0), from H[i-1][j-1] (h_diag), H and E of (i, j-1) (h_left, e_left) and H and F of (i-1, j)
// (h_up, f_up); kInf stands for a cell that is absent or outside the matrix.
GWAFFINE_HD Cell cell_update(int32_t h_diag, int32_t h_left, int32_t e_left, int32_t h_up, int32_t f_up, bool match,
                             const Costs& c)
{
    Cell r;
    r.bits           = 0;
    const int32_t oe = c.gap_open + c.gap_extend;
    {
        const int32_t ext = e_left + c.gap_extend, opn = h_left + oe;
        if (e_left < kInf && ext <= opn)
        {
            r.e = ext;
            r.bits |= kEext;
        }
        else
            r.e = h_left < kInf ? opn : kInf;
    }
    {
        const int32_t ext = f_up + c.gap_extend, opn = h_up + oe;
        if (f_up < kInf && ext <= opn)
        {
            r.f = ext;
            r.bits |= kFext;
        }
        else
            r.f = h_up < kInf ? opn : kInf;
    }
    int32_t h = h_diag < kInf ? h_diag + (match ? 0 : c.mismatch) : kInf;
    if (!match)
        r.bits |= kMismatch;
    if (r.e < h)
    {
        h      = r.e;
        r.bits = (r.bits & ~kSrcMask) | kSrcE;
    }
    if (r.f < h)
    {
        h      = r.f;
        r.bits = (r.bits & ~kSrcMask) | kSrcF;
    }
    r.h = h;
    return r;
}

// the default aligner's predicate
GWAFFINE_HD bool bases_match(char q, char t)
{
    return q == "ACTG"[(static_cast<unsigned char>(t) >> 1) & 3];
}

struct Walk
{
    int64_t i, j;
    int32_t matrix; // 0 H, 1 E, 2 F
};

// One step of the traceback at (w.i, w.j) in w.matrix, whose cell has `bits`: returns the state it emits (0..3) or
// -1 for a switch of matrix. The walk ends at (0, 0) in H.
GWAFFINE_HD int32_t walk_step(Walk& w, uint32_t bits)
{
    if (w.matrix == 0)
    {
        const uint32_t src = bits & kSrcMask;
        if (src != 0)
        {
            w.matrix = static_cast<int32_t>(src);
            return -1;
        }
        --w.i;
        --w.j;
        return (bits & kMismatch) ? 1 : 0;
    }
    if (w.matrix == 1)
    {
        --w.j;
        if (!(bits & kEext))
            w.matrix = 0;
        return 2;
    }
    --w.i;
    if (!(bits & kFext))
        w.matrix = 0;
    return 3;
}

// The whole traceback of an aligned pair, serially: states back to front at out[0 .. n + m), returns their number.
// `bits` is the pair's bit matrix. -1: the bits lead out of the band or past the slot (a defect, never an input's
// property); nothing outside the matrix or the slot is touched then. (The device takes the same steps with the same
// guards, but reads the bytes from tiles of the matrix that a wave has brought into LDS.)
GWAFFINE_HD int32_t walk_back(const Band& b, const uint8_t* bits, int8_t* out)
{
    Walk w{b.n, b.m, 0};
    int64_t len = 0;
    while (w.i != 0 || w.j != 0 || w.matrix != 0)
    {
        if (w.i < 0 || w.j < 0 || w.j - w.i < b.lo || w.j - w.i > b.hi)
            return -1;
        const int32_t s = walk_step(w, bits[bits_index(b, w.i, w.j)]);
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
// The forward pass run serially in the wavefront's own order and storage: three values per diagonal, updated in place
// anti-diagonal by anti-diagonal. h, e, f: [W] each; bits: bits_bytes(b). Returns H[n][m].
inline int32_t forward_serial(const Band& b, const char* q, const char* t, const Costs& c, int32_t* h, int32_t* e,
                              int32_t* f, uint8_t* bits)
{
    for (int64_t k = 0; k < b.W; ++k)
        h[k] = e[k] = f[k] = kInf;
    for (int64_t a = 0; a <= b.n + b.m; ++a)
        for (int64_t k = (a + b.lo) & 1; k < b.W; k += 2)
        {
            const int64_t d = k + b.lo, i = (a - d) >> 1, j = (a + d) >> 1;
            if (i < 0 || j < 0 || i > b.n || j > b.m)
            {
                h[k] = e[k] = f[k] = kInf;
                continue;
            }
            if (a == 0)
            {
                h[k]                      = 0;
                bits[bits_index(b, 0, 0)] = 0;
                continue;
            }
            const bool inner = i > 0 && j > 0;
            const Cell r     = cell_update(inner ? h[k] : kInf, k > 0 && j > 0 ? h[k - 1] : kInf,
                                           k > 0 && j > 0 ? e[k - 1] : kInf, k + 1 < b.W && i > 0 ? h[k + 1] : kInf,
                                           k + 1 < b.W && i > 0 ? f[k + 1] : kInf,
                                           inner && bases_match(q[i - 1], t[j - 1]), c);
            h[k] = r.h;
            e[k] = r.e;
            f[k] = r.f;
            bits[bits_index(b, i, j)] = static_cast<uint8_t>(r.bits);
        }
    return h[b.m - b.n - b.lo];
}
#endif

} // namespace gwaffine

#endif
