// gwm_anchor_plan.hpp -- the rules of anchored overlap alignment (G1-G6 next to gwm_align_overlaps_anchored in
// include/gwhip_mapper.h) as plain C++: the slice coordinates of an anchor, which anchors
// count, where a record is cut and what its pieces are. No HIP in it: the kernels of gwm_anchored.hip include it and
// apply the element rules one anchor to a thread, and a host program can run the very same rules serially
// (plan_record_serial below; tests/cpp/anchor_plan_sanitized.cpp does, under the sanitizers).
//
// A record aligns its query slice of n bases against its target slice T' of m bases, T' the reverse complement of
// the slice on '-'. An anchor (q, t) -- minimizer starts in forward read coordinates, k-mers of k bases -- lies at
// (u, v) of the slices. All arithmetic is signed 64-bit and never wraps: positions are uint32.
#ifndef GWM_ANCHOR_PLAN_HPP
#define GWM_ANCHOR_PLAN_HPP

#include <stdint.h>

#if defined(__HIPCC__)
#define GWM_PLAN_HD __host__ __device__ __forceinline__
#else
#define GWM_PLAN_HD inline
#endif

namespace gwm_plan
{

constexpr int32_t kDefaultSpacing = 256; // a convention, not tuned

// what the rules read of an overlap record
struct Record
{
    int64_t query_start, query_end, target_start, target_end;
    bool minus;
};

GWM_PLAN_HD int64_t query_length(const Record& r) { return r.query_end - r.query_start; }
GWM_PLAN_HD int64_t target_length(const Record& r) { return r.target_end - r.target_start; }

GWM_PLAN_HD bool parameters_in_range(int64_t kmer_size, int64_t spacing)
{
    return kmer_size >= 1 && kmer_size <= 32 && spacing >= 1;
}

// Entry i of offsets[0 .. n] that breaks "starts at 0, never decreases, ends at n_anchors", or -1. Serial: the
// host checks the offsets of a call before anything is launched.
inline int64_t first_bad_offset(const int64_t* offsets, int64_t n, int64_t n_anchors)
{
    if (offsets[0] != 0)
        return 0;
    for (int64_t i = 1; i <= n; ++i)
        if (offsets[i] < offsets[i - 1])
            return i;
    return offsets[n] == n_anchors ? -1 : n;
}

// G1: on '-' the start of the k-mer in the reverse-complemented target slice
GWM_PLAN_HD void slice_coordinates(const Record& r, int64_t k, int64_t q, int64_t t, int64_t& u, int64_t& v)
{
    u = q - r.query_start;
    v = r.minus ? r.target_end - t - k : t - r.target_start;
}

// G2
GWM_PLAN_HD bool valid(int64_t u, int64_t v, int64_t n, int64_t m) { return 0 < u && u < n && 0 < v && v < m; }

// G3, of a valid anchor and the valid anchor before it in its record
GWM_PLAN_HD bool increasing(int64_t u_before, int64_t v_before, int64_t u, int64_t v)
{
    return u > u_before && v > v_before;
}

// G4, of a valid anchor; first: no valid anchor before it in its record
GWM_PLAN_HD bool is_cut(bool first, int64_t u_before, int64_t u, int64_t spacing)
{
    return first || u / spacing != u_before / spacing;
}

// G5: a piece starts at a cut, or at (0, 0), and reaches to the next piece's start, or to (n, m)
struct Piece
{
    int64_t u, v, query_length, target_length;
};

GWM_PLAN_HD Piece piece_between(int64_t u, int64_t v, int64_t u_next, int64_t v_next) { return {u, v, u_next - u, v_next - v}; }

// The pieces of one record from its anchors[0 .. count) as (q, t) pairs, serially, by the element rules above.
// Returns their number (>= 1), written to pieces[] where it is not null (room for count + 1), or -1 when two valid
// anchors are not strictly increasing (G3).
inline int64_t plan_record_serial(const Record& r, const uint32_t* anchors, int64_t count, int64_t k, int64_t spacing,
                                  Piece* pieces)
{
    const int64_t n = query_length(r), m = target_length(r);
    int64_t made = 0, at_u = 0, at_v = 0; // the open piece starts at (at_u, at_v)
    int64_t u_before = 0, v_before = 0;
    bool first = true;
    for (int64_t a = 0; a < count; ++a)
    {
        int64_t u, v;
        slice_coordinates(r, k, anchors[2 * a], anchors[2 * a + 1], u, v);
        if (!valid(u, v, n, m))
            continue;
        if (!first && !increasing(u_before, v_before, u, v))
            return -1;
        if (is_cut(first, u_before, u, spacing))
        {
            if (pieces)
                pieces[made] = piece_between(at_u, at_v, u, v);
            ++made;
            at_u = u;
            at_v = v;
        }
        first    = false;
        u_before = u;
        v_before = v;
    }
    if (pieces)
        pieces[made] = piece_between(at_u, at_v, n, m);
    return made + 1;
}

} // namespace gwm_plan

#endif
