// gwm_mapper.hip -- cudamapper on gfx950: (k,w)-minimizer sketch, index, anchor matcher, triggered overlapper
// (include/gwhip_mapper.h). Semantics are those of GenomeWorks' cudamapper (minimizer.cu, index_gpu.cuh,
// matcher_gpu.cu, overlapper_triggered.cu), restated from scratch; DESIGN.md "cudamapper" lists the parity rules.
//
// Layout: element-parallel kernels (one lane per base, window, representation or anchor; wave64) joined by rocPRIM
// scans, selects and stable radix sorts. The hand-written kernels keep their state in registers: no LDS, no scratch
// (rocPRIM's own kernels use LDS, and some of them scratch).
#include "gwhip_mapper.h"

#include "gwm_device_utils.hpp"
#include "gwm_overlap_filter.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace
{

thread_local std::string g_error;

// ------------------------------------------------------------------------------------------------------------------
// sketch
// ------------------------------------------------------------------------------------------------------------------

// Last i in [0, n) with v[i] <= x (v ascending, v[0] == 0 <= x).
__device__ inline uint32_t segment_of(const int64_t* v, uint32_t n, int64_t x)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1)
    {
        const uint32_t mid = (lo + hi) / 2;
        if (v[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ inline uint64_t wang_hash64(uint64_t key)
{
    const uint64_t mask = (uint64_t(1) << 32) - 1;
    key                 = (~key + (key << 21)) & mask;
    key                 = key ^ key >> 24;
    key                 = ((key + (key << 3)) + (key << 8)) & mask;
    key                 = key ^ key >> 14;
    key                 = ((key + (key << 2)) + (key << 4)) & mask;
    key                 = key ^ key >> 28;
    key                 = (key + (key << 31)) & mask;
    return key;
}

// One 2-bit code placed as the reference places it: the code is an int shifted in 32 bits (shifts of 32 or more give
// 0, a set bit 31 sign-extends) before it is OR-ed into the 64-bit representation. Identical to a plain 64-bit shift
// for k <= 15.
__device__ inline uint64_t place(uint32_t code, uint32_t shift)
{
    if (shift >= 32)
        return 0;
    return static_cast<uint64_t>(static_cast<int64_t>(static_cast<int32_t>(code << shift)));
}

// Canonical representation of the k-mer starting at every base that starts one (other slots are left untouched).
// Base code: 3 & (b >> 2 ^ b >> 1) (A0 C1 G2 T3, any other byte by the same formula); its complement goes through
// the table {0, 4, 0, 7, 1, 0, 0, 3}[b & 7]. The forward representation wins ties (palindromes read forward).
__global__ void __launch_bounds__(kThreads) kmer_kernel(const uint8_t* __restrict__ bases,
                                                        const int64_t* __restrict__ base_offsets, uint32_t n_reads,
                                                        int64_t total_bases, uint32_t k, int32_t hash,
                                                        uint64_t* __restrict__ rep, uint8_t* __restrict__ dir)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= total_bases)
        return;
    const uint32_t r    = segment_of(base_offsets, n_reads, p);
    const int64_t local = p - base_offsets[r];
    const int64_t len   = base_offsets[r + 1] - base_offsets[r];
    if (local + k > len)
        return;
    uint64_t f = 0, rv = 0;
    for (uint32_t i = 0; i < k; ++i)
    {
        const uint32_t b  = bases[p + i];
        // complement table {0, 4, 0, 7 | 1, 0, 0, 3} as two packed words, entry b & 7
        const uint32_t ct = (((b & 4) ? 0x03000001u : 0x07000400u) >> (8 * (b & 3))) & 0xffu;
        f |= place(3u & ((b >> 2) ^ (b >> 1)), 2 * (k - i - 1));
        rv |= place(3u & ((ct >> 2) ^ (ct >> 1)), 2 * i);
    }
    if (hash)
    {
        f  = wang_hash64(f);
        rv = wang_hash64(rv);
    }
    rep[p] = f <= rv ? f : rv;
    dir[p] = f <= rv ? 0 : 1;
}

// Window j of a read with nk k-mers covers k-mers [max(0, j-w+1), min(nk-1, j)], j in [0, nk+w-1): the w-1 front-end
// windows, the nk-w+1 central ones and the w-1 back-end ones. Its minimizer is the LAST k-mer of smallest
// representation. A window emits its minimizer when j == 0 or the previous window's minimizer sits elsewhere -- with the
// one exception of central_step() below.
__device__ inline uint32_t window_min(const uint64_t* rep, int64_t j, int64_t nk, int64_t w)
{
    const int64_t lo = j - w + 1 > 0 ? j - w + 1 : 0;
    const int64_t hi = j < nk - 1 ? j : nk - 1;
    uint64_t best    = rep[lo];
    int64_t at       = lo;
    for (int64_t i = lo + 1; i <= hi; ++i)
    {
        const uint64_t v = rep[i];
        if (v <= best)
        {
            best = v;
            at   = i;
        }
    }
    return static_cast<uint32_t>(at);
}

// The reference walks the central windows of a read in steps of 514 - k - w windows (64 threads x 8 bases, held in 16
// bits) and hands the last window's position from step to step through a carry stored by thread `step % 64 - 1`. When
// the step is a multiple of 64 (k + w = 2 mod 64, e.g. k 15 w 51) no thread stores it: the carry keeps its first value,
// the position of the last front-end minimizer (0 when w == 1), and the first window of every later step is compared
// with that instead of with its left neighbour. Such a window sits at a position >= step, the carry at <= w - 2, so it
// always emits as long as w - 2 < step (gwm_index_build refuses the rest).
__device__ inline uint32_t central_step(uint32_t k, uint32_t w)
{
    return static_cast<uint16_t>(static_cast<uint16_t>(512u - (k - 1)) - (w - 1));
}

__global__ void __launch_bounds__(kThreads) window_kernel(const uint64_t* __restrict__ rep,
                                                          const int64_t* __restrict__ base_offsets,
                                                          const int64_t* __restrict__ window_offsets, uint32_t n_reads,
                                                          int64_t total_windows, uint32_t k, uint32_t w,
                                                          uint32_t* __restrict__ min_pos, uint32_t* __restrict__ emit)
{
    const int64_t x = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (x >= total_windows)
        return;
    const uint32_t r  = segment_of(window_offsets, n_reads, x);
    const int64_t j   = x - window_offsets[r];
    const int64_t nk  = base_offsets[r + 1] - base_offsets[r] - k + 1;
    const uint64_t* q = rep + base_offsets[r];
    const uint32_t at = window_min(q, j, nk, w);
    min_pos[x]        = at;
    const uint32_t step = central_step(k, w);
    const int64_t c     = j - (w - 1); // central window number
    if (step % 64 == 0 && c > 0 && c < nk - w + 1 && c % step == 0)
        emit[x] = at != (w > 1 ? window_min(q, w - 2, nk, w) : 0u) ? 1u : 0u;
    else
        emit[x] = (j == 0 || window_min(q, j - 1, nk, w) != at) ? 1u : 0u;
}

// Emitted windows -> (representation, global index) keys for the stable sort, and the rest of the element.
__global__ void __launch_bounds__(kThreads) scatter_minimizers_kernel(
    const uint64_t* __restrict__ rep, const uint8_t* __restrict__ dir, const int64_t* __restrict__ base_offsets,
    const int64_t* __restrict__ window_offsets, uint32_t n_reads, int64_t total_windows,
    const uint32_t* __restrict__ min_pos, const uint32_t* __restrict__ emit, const uint32_t* __restrict__ slot,
    uint32_t first_read_id, uint64_t* __restrict__ keys, uint32_t* __restrict__ order, uint32_t* __restrict__ read_ids,
    uint32_t* __restrict__ positions, uint8_t* __restrict__ dirs)
{
    const int64_t x = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (x >= total_windows || !emit[x])
        return;
    const uint32_t r   = segment_of(window_offsets, n_reads, x);
    const uint32_t o   = slot[x] - 1; // inclusive scan
    const int64_t kmer = base_offsets[r] + min_pos[x];
    keys[o]            = rep[kmer];
    order[o]           = o;
    read_ids[o]        = first_read_id + r;
    positions[o]       = min_pos[x];
    dirs[o]            = dir[kmer];
}

__global__ void __launch_bounds__(kThreads) gather_sorted_kernel(const uint64_t* __restrict__ keys,
                                                                 const uint32_t* __restrict__ order, int64_t n,
                                                                 const uint32_t* __restrict__ rid_in,
                                                                 const uint32_t* __restrict__ pos_in,
                                                                 const uint8_t* __restrict__ dir_in,
                                                                 uint32_t* __restrict__ rid_out,
                                                                 uint32_t* __restrict__ pos_out,
                                                                 uint8_t* __restrict__ dir_out, uint32_t* __restrict__ head)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t o = order[i];
    rid_out[i]       = rid_in[o];
    pos_out[i]       = pos_in[o];
    dir_out[i]       = dir_in[o];
    head[i]          = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// uid: inclusive scan of the head flags (1-based representation number of element i).
__global__ void __launch_bounds__(kThreads) unique_kernel(const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ head,
                                                          const uint32_t* __restrict__ uid, int64_t n,
                                                          uint64_t* __restrict__ unique_rep,
                                                          uint32_t* __restrict__ first_occurrence)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > n)
        return;
    if (i == n)
    {
        first_occurrence[uid[n - 1]] = static_cast<uint32_t>(n);
        return;
    }
    if (head[i])
    {
        unique_rep[uid[i] - 1]       = keys[i];
        first_occurrence[uid[i] - 1] = static_cast<uint32_t>(i);
    }
}

// Frequency filter (index_gpu.cuh filter_out_most_common_representations): a representation with count >= threshold
// goes, threshold = uint64(total elements * filtering_parameter + 0.001).
__global__ void __launch_bounds__(kThreads) filter_flags_kernel(const uint32_t* __restrict__ first_occurrence,
                                                                int64_t n_unique, uint64_t threshold,
                                                                uint32_t* __restrict__ keep_unique)
{
    const int64_t u = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (u >= n_unique)
        return;
    const uint64_t count = first_occurrence[u + 1] - first_occurrence[u];
    keep_unique[u]       = count >= threshold ? 0u : 1u;
}

__global__ void __launch_bounds__(kThreads) element_keep_kernel(const uint32_t* __restrict__ uid,
                                                                const uint32_t* __restrict__ keep_unique, int64_t n,
                                                                uint32_t* __restrict__ keep)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n)
        keep[i] = keep_unique[uid[i] - 1];
}

// new_slot / new_uslot: inclusive scans of keep / keep_unique.
__global__ void __launch_bounds__(kThreads) compress_elements_kernel(
    const uint32_t* __restrict__ keep, const uint32_t* __restrict__ new_slot, int64_t n,
    const uint64_t* __restrict__ rep, const uint32_t* __restrict__ rid, const uint32_t* __restrict__ pos,
    const uint8_t* __restrict__ dir, uint64_t* __restrict__ rep_out, uint32_t* __restrict__ rid_out,
    uint32_t* __restrict__ pos_out, uint8_t* __restrict__ dir_out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i])
        return;
    const uint32_t o = new_slot[i] - 1;
    rep_out[o]       = rep[i];
    rid_out[o]       = rid[i];
    pos_out[o]       = pos[i];
    dir_out[o]       = dir[i];
}

__global__ void __launch_bounds__(kThreads) compress_unique_kernel(
    const uint32_t* __restrict__ keep_unique, const uint32_t* __restrict__ new_uslot, int64_t n_unique,
    const uint64_t* __restrict__ unique_rep, const uint32_t* __restrict__ first_occurrence,
    const uint32_t* __restrict__ new_slot, uint64_t* __restrict__ unique_out, uint32_t* __restrict__ first_out,
    uint32_t n_kept)
{
    const int64_t u = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (u > n_unique)
        return;
    if (u == n_unique)
    {
        first_out[new_uslot[n_unique - 1]] = n_kept;
        return;
    }
    if (!keep_unique[u])
        return;
    const uint32_t o = new_uslot[u] - 1;
    unique_out[o]    = unique_rep[u];
    first_out[o]     = new_slot[first_occurrence[u]] - 1; // the first element of a kept representation is kept
}

// ------------------------------------------------------------------------------------------------------------------
// matcher
// ------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kThreads) lookup_kernel(const uint64_t* __restrict__ q_unique, int64_t n_q,
                                                          const uint32_t* __restrict__ q_first,
                                                          const uint64_t* __restrict__ t_unique, int64_t n_t,
                                                          const uint32_t* __restrict__ t_first,
                                                          int64_t* __restrict__ found, int64_t* __restrict__ count)
{
    const int64_t u = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (u >= n_q)
        return;
    const uint64_t v = q_unique[u];
    int64_t lo = 0, hi = n_t;
    while (lo < hi)
    {
        const int64_t mid = lo + (hi - lo) / 2;
        if (t_unique[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    const bool hit = lo < n_t && t_unique[lo] == v;
    found[u]       = hit ? lo : -1;
    count[u]       = hit ? static_cast<int64_t>(q_first[u + 1] - q_first[u]) * (t_first[lo + 1] - t_first[lo]) : 0;
}

// Anchor a of representation u (first u with cum[u] > a) is the (a - start) / n_t-th query element with that
// representation against the (a - start) % n_t-th target element. Also writes the two sort keys.
__global__ void __launch_bounds__(kThreads) generate_anchors_kernel(
    const int64_t* __restrict__ cum, int64_t n_q, const int64_t* __restrict__ found,
    const uint32_t* __restrict__ q_first, const uint32_t* __restrict__ q_rid, const uint32_t* __restrict__ q_pos,
    const uint32_t* __restrict__ t_first, const uint32_t* __restrict__ t_rid, const uint32_t* __restrict__ t_pos,
    int64_t n_anchors, uint32_t q_smallest, uint32_t t_smallest, uint64_t t_reads, uint64_t t_longest,
    gwm_anchor* __restrict__ anchors, uint64_t* __restrict__ read_key, uint64_t* __restrict__ pos_key,
    uint32_t* __restrict__ order)
{
    const int64_t a = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (a >= n_anchors)
        return;
    int64_t lo = 0, hi = n_q;
    while (lo < hi)
    {
        const int64_t mid = lo + (hi - lo) / 2;
        if (cum[mid] <= a)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int64_t u     = lo;
    const int64_t rel   = a - (u > 0 ? cum[u - 1] : 0);
    const int64_t j     = found[u];
    const int64_t n_t   = t_first[j + 1] - t_first[j];
    const uint32_t qi   = q_first[u] + static_cast<uint32_t>(rel / n_t);
    const uint32_t ti   = t_first[j] + static_cast<uint32_t>(rel % n_t);
    gwm_anchor an;
    an.query_read_id           = q_rid[qi];
    an.target_read_id          = t_rid[ti];
    an.query_position_in_read  = q_pos[qi];
    an.target_position_in_read = t_pos[ti];
    anchors[a]                 = an;
    read_key[a]                = (an.query_read_id - q_smallest) * t_reads + (an.target_read_id - t_smallest);
    pos_key[a]                 = an.query_position_in_read * t_longest + an.target_position_in_read;
    order[a]                   = static_cast<uint32_t>(a);
}

__global__ void __launch_bounds__(kThreads) gather_keys_kernel(const uint64_t* __restrict__ key,
                                                               const uint32_t* __restrict__ order, int64_t n,
                                                               uint64_t* __restrict__ out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = key[order[i]];
}

__global__ void __launch_bounds__(kThreads) gather_anchors_kernel(const gwm_anchor* __restrict__ in,
                                                                  const uint32_t* __restrict__ order, int64_t n,
                                                                  gwm_anchor* __restrict__ out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n)
        out[i] = in[order[i]];
}

// ------------------------------------------------------------------------------------------------------------------
// overlapper
// ------------------------------------------------------------------------------------------------------------------

// (prev, cur) are in one chain: same read pair, cur.q - prev.q < 150 in unsigned arithmetic, |cur.t - prev.t| < 150.
__device__ inline bool same_chain(const gwm_anchor& prev, const gwm_anchor& cur)
{
    const int dt = static_cast<int>(cur.target_position_in_read) - static_cast<int>(prev.target_position_in_read);
    return prev.query_read_id == cur.query_read_id && prev.target_read_id == cur.target_read_id &&
           (cur.query_position_in_read - prev.query_position_in_read) < 150u && abs(dt) < 150;
}

__device__ inline bool same_overlap(const gwm_anchor& a, const gwm_anchor& b)
{
    const int dq = abs(static_cast<int>(a.query_position_in_read) - static_cast<int>(b.query_position_in_read));
    const int dt = abs(static_cast<int>(a.target_position_in_read) - static_cast<int>(b.target_position_in_read));
    return a.target_read_id == b.target_read_id && a.query_read_id == b.query_read_id && abs(dq - dt) < 300;
}

__global__ void __launch_bounds__(kThreads) chain_heads_kernel(const gwm_anchor* __restrict__ a, int64_t n,
                                                               uint32_t* __restrict__ head)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n)
        head[i] = (i == 0 || !same_chain(a[i - 1], a[i])) ? 1u : 0u;
}

__global__ void __launch_bounds__(kThreads) chain_length_kernel(const uint32_t* __restrict__ start, uint32_t n_chains,
                                                                uint32_t n_anchors, uint32_t* __restrict__ length,
                                                                uint32_t* __restrict__ kept)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chains)
        return;
    const uint32_t len = (c + 1 < n_chains ? start[c + 1] : n_anchors) - start[c];
    length[c]          = len;
    kept[c]            = len >= 3 ? 1u : 0u;
}

// kept chain m -> its start and length; fuse head when m == 0 or its first anchor does not match the previous kept
// chain's first anchor.
__global__ void __launch_bounds__(kThreads) fuse_heads_kernel(const gwm_anchor* __restrict__ a,
                                                              const uint32_t* __restrict__ start,
                                                              const uint32_t* __restrict__ length,
                                                              const uint32_t* __restrict__ kept_ids, uint32_t n_kept,
                                                              uint32_t* __restrict__ kept_start,
                                                              uint32_t* __restrict__ kept_length,
                                                              uint32_t* __restrict__ head)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_kept)
        return;
    const uint32_t c = kept_ids[m];
    kept_start[m]    = start[c];
    kept_length[m]   = length[c];
    head[m]          = (m == 0 || !same_overlap(a[start[kept_ids[m - 1]]], a[start[c]])) ? 1u : 0u;
}

// Fused overlap f spans kept chains [fh[f], fh[f+1]): residues = sum of their lengths, anchors [first start, last end).
__global__ void __launch_bounds__(kThreads) create_filter_kernel(
    const gwm_anchor* __restrict__ a, const uint32_t* __restrict__ fh, uint32_t n_fused, uint32_t n_kept,
    const uint32_t* __restrict__ kept_start, const uint32_t* __restrict__ kept_length,
    const uint32_t* __restrict__ length_sum, int32_t all_to_all, uint64_t min_residues, uint64_t min_overlap_len,
    uint64_t min_bases_per_residue, float min_overlap_fraction, gwm_overlap* __restrict__ out,
    uint32_t* __restrict__ keep)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_fused)
        return;
    const uint32_t m0 = fh[f];
    const uint32_t m1 = (f + 1 < n_fused ? fh[f + 1] : n_kept) - 1;
    const uint32_t residues = length_sum[m1] - (m0 > 0 ? length_sum[m0 - 1] : 0);
    const gwm_anchor s = a[kept_start[m0]];
    const gwm_anchor e = a[kept_start[m1] + kept_length[m1] - 1];
    gwm_overlap o;
    o.query_read_id                = e.query_read_id;
    o.target_read_id               = e.target_read_id;
    o.num_residues                 = residues;
    o.query_start_position_in_read = s.query_position_in_read;
    o.query_end_position_in_read   = e.query_position_in_read;
    o.overlap_complete             = 1;
    if (s.target_position_in_read > e.target_position_in_read)
    {
        o.relative_strand               = '-';
        o.target_start_position_in_read = e.target_position_in_read;
        o.target_end_position_in_read   = s.target_position_in_read;
    }
    else
    {
        o.relative_strand               = '+';
        o.target_start_position_in_read = s.target_position_in_read;
        o.target_end_position_in_read   = e.target_position_in_read;
    }
    out[f]  = o;
    keep[f] = passes_overlap_filter(o, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                                    min_overlap_fraction)
                  ? 1u
                  : 0u;
}

void set_empty(gwm_index* out)
{
    std::memset(out, 0, sizeof(*out));
}

} // namespace

void gwm_set_error(const char* text) { g_error = text; }

extern "C" {

const char* gwm_last_error(void) { return g_error.c_str(); }

void gwm_index_free(gwm_index* x)
{
    if (!x)
        return;
    if (x->device_slab)
    {
        // restored by gwm_index_unpack: the arrays lie in this one allocation
        (void)hipFree(x->device_slab);
        set_empty(x);
        return;
    }
    (void)hipFree(x->representations);
    (void)hipFree(x->read_ids);
    (void)hipFree(x->positions_in_reads);
    (void)hipFree(x->directions);
    (void)hipFree(x->unique_representations);
    (void)hipFree(x->first_occurrence_of_representations);
    set_empty(x);
}

int gwm_index_build(const char* bases, const int64_t* offsets, int32_t n_reads, uint32_t first_read_id, int32_t k,
                    int32_t w, int32_t hash_representations, double filtering_parameter, void* stream, gwm_index* out)
{
    set_empty(out);
    try
    {
        if (k < 1 || k > 32 || w < 1 || n_reads < 0)
            throw std::invalid_argument("gwm_index_build: need 1 <= k <= 32, w >= 1, n_reads >= 0");
        {
            const uint32_t step = static_cast<uint16_t>(static_cast<uint16_t>(512 - (k - 1)) - (w - 1));
            if (step % 64 == 0 && static_cast<int64_t>(w) - 2 >= static_cast<int64_t>(step))
                throw std::invalid_argument("gwm_index_build: k + w = 2 (mod 64) needs w - 2 < 514 - k - w");
        }
        hipStream_t s = static_cast<hipStream_t>(stream);
        out->first_read_id = first_read_id;
        // reads of at least k + w - 1 bases, in order
        std::vector<int64_t> base_off{0}, win_off{0};
        std::vector<int32_t> kept;
        uint32_t longest = 0;
        for (int32_t i = 0; i < n_reads; ++i)
        {
            const int64_t len = offsets[i + 1] - offsets[i];
            if (len >= static_cast<int64_t>(w) + k - 1)
            {
                kept.push_back(i);
                base_off.push_back(base_off.back() + len);
                win_off.push_back(win_off.back() + len - k + w);
                longest = std::max<uint32_t>(longest, static_cast<uint32_t>(len));
            }
        }
        const int64_t total_bases = base_off.back(), total_windows = win_off.back();
        if (total_bases == 0)
            return 0; // empty index: number_of_reads 0, no arrays
        if (total_windows >= (int64_t(1) << 32) - 1)
            throw std::invalid_argument("gwm_index_build: more than 2^32 - 2 windows in one index");
        out->number_of_reads                     = static_cast<uint32_t>(n_reads);
        out->number_of_basepairs_in_longest_read = longest;
        const uint32_t nr                        = static_cast<uint32_t>(kept.size());
        std::vector<char> merged(static_cast<size_t>(total_bases));
        for (uint32_t r = 0; r < nr; ++r)
            std::memcpy(merged.data() + base_off[r], bases + offsets[kept[r]], static_cast<size_t>(base_off[r + 1] - base_off[r]));

        Events ev(5);
        Temp temp;
        dbuf<uint32_t> d_count(1);
        ev.record(0, s);
        dbuf<uint8_t> d_bases(total_bases);
        dbuf<int64_t> d_boff(nr + 1), d_woff(nr + 1);
        GWM_CHECK(hipMemcpyAsync(d_bases.p, merged.data(), total_bases, hipMemcpyHostToDevice, s));
        GWM_CHECK(hipMemcpyAsync(d_boff.p, base_off.data(), sizeof(int64_t) * (nr + 1), hipMemcpyHostToDevice, s));
        GWM_CHECK(hipMemcpyAsync(d_woff.p, win_off.data(), sizeof(int64_t) * (nr + 1), hipMemcpyHostToDevice, s));
        dbuf<uint64_t> d_rep(total_bases);
        dbuf<uint8_t> d_dir(total_bases);
        kmer_kernel<<<grid_for(total_bases), kThreads, 0, s>>>(d_bases.p, d_boff.p, nr, total_bases, k,
                                                              hash_representations, d_rep.p, d_dir.p);
        GWM_CHECK(hipGetLastError());
        dbuf<uint32_t> d_minpos(total_windows), d_emit(total_windows), d_slot(total_windows);
        window_kernel<<<grid_for(total_windows), kThreads, 0, s>>>(d_rep.p, d_boff.p, d_woff.p, nr, total_windows, k,
                                                                  w, d_minpos.p, d_emit.p);
        GWM_CHECK(hipGetLastError());
        inclusive_sum(d_emit.p, d_slot.p, total_windows, temp, s);
        const int64_t n = to_host(d_slot.p + total_windows - 1, s);
        dbuf<uint64_t> keys_a(n), keys_b(n);
        dbuf<uint32_t> ord_a(n), ord_b(n), rid_a(n), pos_a(n);
        dbuf<uint8_t> dir_a(n);
        scatter_minimizers_kernel<<<grid_for(total_windows), kThreads, 0, s>>>(
            d_rep.p, d_dir.p, d_boff.p, d_woff.p, nr, total_windows, d_minpos.p, d_emit.p, d_slot.p, first_read_id,
            keys_a.p, ord_a.p, rid_a.p, pos_a.p, dir_a.p);
        GWM_CHECK(hipGetLastError());
        d_bases.reset();
        d_rep.reset();
        d_dir.reset();
        d_minpos.reset();
        d_emit.reset();
        d_slot.reset();
        ev.record(1, s);

        // stable sort by representation: hashed values fit in 32 bits, plain ones in 2k bits below k = 16
        const unsigned bits = hash_representations ? 32u : (k < 16 ? 2u * k : 64u);
        sort_pairs(keys_a.p, keys_b.p, ord_a.p, ord_b.p, n, bits, temp, s);
        dbuf<uint32_t> rid(n), pos(n), head(n);
        dbuf<uint8_t> dir(n);
        gather_sorted_kernel<<<grid_for(n), kThreads, 0, s>>>(keys_b.p, ord_b.p, n, rid_a.p, pos_a.p, dir_a.p, rid.p,
                                                             pos.p, dir.p, head.p);
        GWM_CHECK(hipGetLastError());
        ev.record(2, s);

        dbuf<uint32_t> uid(n);
        inclusive_sum(head.p, uid.p, n, temp, s);
        const int64_t n_unique = to_host(uid.p + n - 1, s);
        dbuf<uint64_t> unique_rep(n_unique);
        dbuf<uint32_t> first(n_unique + 1);
        unique_kernel<<<grid_for(n + 1), kThreads, 0, s>>>(keys_b.p, head.p, uid.p, n, unique_rep.p, first.p);
        GWM_CHECK(hipGetLastError());
        ev.record(3, s);

        int64_t n_out = n, n_unique_out = n_unique;
        if (filtering_parameter < 1.0)
        {
            const uint64_t threshold = static_cast<uint64_t>(static_cast<double>(n) * filtering_parameter + 0.001);
            dbuf<uint32_t> keep_u(n_unique), uslot(n_unique), keep(n), slot(n);
            filter_flags_kernel<<<grid_for(n_unique), kThreads, 0, s>>>(first.p, n_unique, threshold, keep_u.p);
            GWM_CHECK(hipGetLastError());
            element_keep_kernel<<<grid_for(n), kThreads, 0, s>>>(uid.p, keep_u.p, n, keep.p);
            GWM_CHECK(hipGetLastError());
            inclusive_sum(keep_u.p, uslot.p, n_unique, temp, s);
            inclusive_sum(keep.p, slot.p, n, temp, s);
            n_unique_out = to_host(uslot.p + n_unique - 1, s);
            n_out        = to_host(slot.p + n - 1, s);
            dbuf<uint64_t> rep2(n_out), unique2(n_unique_out);
            dbuf<uint32_t> rid2(n_out), pos2(n_out), first2(n_unique_out + 1);
            dbuf<uint8_t> dir2(n_out);
            if (n_out > 0)
            {
                compress_elements_kernel<<<grid_for(n), kThreads, 0, s>>>(keep.p, slot.p, n, keys_b.p, rid.p, pos.p,
                                                                         dir.p, rep2.p, rid2.p, pos2.p, dir2.p);
                GWM_CHECK(hipGetLastError());
            }
            compress_unique_kernel<<<grid_for(n_unique + 1), kThreads, 0, s>>>(
                keep_u.p, uslot.p, n_unique, unique_rep.p, first.p, slot.p, unique2.p, first2.p,
                static_cast<uint32_t>(n_out));
            GWM_CHECK(hipGetLastError());
            GWM_CHECK(hipStreamSynchronize(s));
            std::swap(keys_b.p, rep2.p);
            std::swap(rid.p, rid2.p);
            std::swap(pos.p, pos2.p);
            std::swap(dir.p, dir2.p);
            std::swap(unique_rep.p, unique2.p);
            std::swap(first.p, first2.p);
        }
        ev.record(4, s);
        GWM_CHECK(hipStreamSynchronize(s));
        out->stage_ms[0]                         = ev.ms(0, 1);
        out->stage_ms[1]                         = ev.ms(1, 2);
        out->stage_ms[2]                         = ev.ms(2, 3);
        out->stage_ms[3]                         = ev.ms(3, 4);
        out->n                                   = n_out;
        out->n_unique                            = n_unique_out;
        out->n_first_occurrence                  = n_unique_out + 1;
        out->representations                     = keys_b.release();
        out->read_ids                            = rid.release();
        out->positions_in_reads                  = pos.release();
        out->directions                          = dir.release();
        out->unique_representations              = unique_rep.release();
        out->first_occurrence_of_representations = first.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        g_error = e.what();
        gwm_index_free(out);
        return -1;
    }
}

int gwm_index_from_arrays(int64_t n, const uint32_t* read_ids, const uint32_t* positions_in_reads, int64_t n_unique,
                          const uint64_t* unique_representations, const uint32_t* first_occurrence,
                          uint32_t first_read_id, uint32_t number_of_reads, uint32_t number_of_basepairs_in_longest_read,
                          gwm_index* out)
{
    set_empty(out);
    try
    {
        if (n < 0 || n_unique < 0 || (n_unique > 0 && first_occurrence[n_unique] != static_cast<uint32_t>(n)))
            throw std::invalid_argument("gwm_index_from_arrays: first_occurrence[n_unique] must be n");
        std::vector<uint64_t> rep(static_cast<size_t>(n));
        for (int64_t u = 0; u < n_unique; ++u)
        {
            if (first_occurrence[u] > first_occurrence[u + 1] || (u > 0 && unique_representations[u - 1] >= unique_representations[u]))
                throw std::invalid_argument("gwm_index_from_arrays: sections must ascend");
            for (uint32_t i = first_occurrence[u]; i < first_occurrence[u + 1]; ++i)
                rep[i] = unique_representations[u];
        }
        std::vector<uint8_t> dir(static_cast<size_t>(n), 0);
        dbuf<uint64_t> d_rep(n), d_unique(n_unique);
        dbuf<uint32_t> d_rid(n), d_pos(n), d_first(n_unique > 0 ? n_unique + 1 : 0);
        dbuf<uint8_t> d_dir(n);
        if (n > 0)
        {
            GWM_CHECK(hipMemcpy(d_rep.p, rep.data(), sizeof(uint64_t) * n, hipMemcpyHostToDevice));
            GWM_CHECK(hipMemcpy(d_rid.p, read_ids, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
            GWM_CHECK(hipMemcpy(d_pos.p, positions_in_reads, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
            GWM_CHECK(hipMemcpy(d_dir.p, dir.data(), n, hipMemcpyHostToDevice));
        }
        if (n_unique > 0)
        {
            GWM_CHECK(hipMemcpy(d_unique.p, unique_representations, sizeof(uint64_t) * n_unique, hipMemcpyHostToDevice));
            GWM_CHECK(hipMemcpy(d_first.p, first_occurrence, sizeof(uint32_t) * (n_unique + 1), hipMemcpyHostToDevice));
        }
        out->n                                   = n;
        out->n_unique                            = n_unique;
        out->n_first_occurrence                  = n_unique > 0 ? n_unique + 1 : 0;
        out->first_read_id                       = first_read_id;
        out->number_of_reads                     = number_of_reads;
        out->number_of_basepairs_in_longest_read = number_of_basepairs_in_longest_read;
        out->representations                     = d_rep.release();
        out->read_ids                            = d_rid.release();
        out->positions_in_reads                  = d_pos.release();
        out->directions                          = d_dir.release();
        out->unique_representations              = d_unique.release();
        out->first_occurrence_of_representations = d_first.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        g_error = e.what();
        gwm_index_free(out);
        return -1;
    }
}

void gwm_anchors_free(gwm_anchors* a)
{
    if (!a)
        return;
    (void)hipFree(a->anchors);
    std::memset(a, 0, sizeof(*a));
}

int gwm_match(const gwm_index* q, const gwm_index* t, void* stream, gwm_anchors* out)
{
    std::memset(out, 0, sizeof(*out));
    try
    {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (q->n_unique == 0 || t->n_unique == 0)
            return 0;
        Events ev(3);
        Temp temp;
        ev.record(0, s);
        const int64_t nq = q->n_unique;
        dbuf<int64_t> found(nq), count(nq), cum(nq);
        lookup_kernel<<<grid_for(nq), kThreads, 0, s>>>(q->unique_representations, nq,
                                                       q->first_occurrence_of_representations,
                                                       t->unique_representations, t->n_unique,
                                                       t->first_occurrence_of_representations, found.p, count.p);
        GWM_CHECK(hipGetLastError());
        inclusive_sum(count.p, cum.p, nq, temp, s);
        const int64_t n = to_host(cum.p + nq - 1, s);
        if (n == 0)
            return 0;
        if (n >= (int64_t(1) << 32))
            throw std::invalid_argument("gwm_match: 2^32 anchors or more for one index pair");
        const uint32_t q_small = q->number_of_reads > 0 ? q->first_read_id : 0;
        const uint32_t t_small = t->number_of_reads > 0 ? t->first_read_id : 0;
        dbuf<gwm_anchor> raw(n), sorted(n);
        dbuf<uint64_t> rkey(n), pkey(n), k_a(n), k_b(n);
        dbuf<uint32_t> ord_a(n), ord_b(n);
        generate_anchors_kernel<<<grid_for(n), kThreads, 0, s>>>(
            cum.p, nq, found.p, q->first_occurrence_of_representations, q->read_ids, q->positions_in_reads,
            t->first_occurrence_of_representations, t->read_ids, t->positions_in_reads, n, q_small, t_small,
            t->number_of_reads, t->number_of_basepairs_in_longest_read, raw.p, rkey.p, pkey.p, ord_a.p);
        GWM_CHECK(hipGetLastError());
        ev.record(1, s);
        // LSD over the two compound keys: positions (query * longest target + target), then read pair
        const uint64_t max_r = static_cast<uint64_t>(q->number_of_reads) * t->number_of_reads + t->number_of_reads;
        const uint64_t max_p = static_cast<uint64_t>(q->number_of_basepairs_in_longest_read) *
                                   t->number_of_basepairs_in_longest_read +
                               t->number_of_basepairs_in_longest_read;
        sort_pairs(pkey.p, k_a.p, ord_a.p, ord_b.p, n, bits_for(max_p), temp, s);
        gather_keys_kernel<<<grid_for(n), kThreads, 0, s>>>(rkey.p, ord_b.p, n, k_b.p);
        GWM_CHECK(hipGetLastError());
        sort_pairs(k_b.p, k_a.p, ord_b.p, ord_a.p, n, bits_for(max_r), temp, s);
        gather_anchors_kernel<<<grid_for(n), kThreads, 0, s>>>(raw.p, ord_a.p, n, sorted.p);
        GWM_CHECK(hipGetLastError());
        ev.record(2, s);
        GWM_CHECK(hipStreamSynchronize(s));
        out->stage_ms[0] = ev.ms(0, 1);
        out->stage_ms[1] = ev.ms(1, 2);
        out->n           = n;
        out->anchors     = sorted.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        g_error = e.what();
        gwm_anchors_free(out);
        return -1;
    }
}

static int find_overlaps(const gwm_anchor* anchors, int64_t n, int32_t all_to_all, int64_t min_residues,
                         int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
                         void* stream, gwm_overlap* out, gwm_overlap** device_out, int64_t* count,
                         float* chain_fuse_filter_ms)
{
    *count = 0;
    if (chain_fuse_filter_ms)
        *chain_fuse_filter_ms = 0.f;
    try
    {
        if (min_residues < 0 || min_overlap_len < 0 || min_bases_per_residue < 0)
            throw std::invalid_argument("gwm_find_overlaps: min_residues, min_overlap_len and min_bases_per_residue "
                                        "must be >= 0");
        if (n <= 0)
            return 0;
        if (n >= (int64_t(1) << 32))
            throw std::invalid_argument("gwm_find_overlaps: 2^32 anchors or more");
        hipStream_t s = static_cast<hipStream_t>(stream);
        Events ev(2);
        Temp temp;
        dbuf<uint32_t> d_count(1);
        ev.record(0, s);
        dbuf<uint32_t> head(n), start(n);
        chain_heads_kernel<<<grid_for(n), kThreads, 0, s>>>(anchors, n, head.p);
        GWM_CHECK(hipGetLastError());
        const uint32_t n_chains = select_indices(head.p, n, start.p, d_count.p, temp, s);
        dbuf<uint32_t> length(n_chains), kept(n_chains), kept_ids(n_chains);
        chain_length_kernel<<<grid_for(n_chains), kThreads, 0, s>>>(start.p, n_chains, static_cast<uint32_t>(n),
                                                                   length.p, kept.p);
        GWM_CHECK(hipGetLastError());
        const uint32_t n_kept = select_indices(kept.p, n_chains, kept_ids.p, d_count.p, temp, s);
        int64_t n_out = 0;
        if (n_kept > 0)
        {
            dbuf<uint32_t> kstart(n_kept), klen(n_kept), fhead(n_kept), ksum(n_kept), fh(n_kept);
            fuse_heads_kernel<<<grid_for(n_kept), kThreads, 0, s>>>(anchors, start.p, length.p, kept_ids.p, n_kept,
                                                                   kstart.p, klen.p, fhead.p);
            GWM_CHECK(hipGetLastError());
            inclusive_sum(klen.p, ksum.p, n_kept, temp, s);
            const uint32_t n_fused = select_indices(fhead.p, n_kept, fh.p, d_count.p, temp, s);
            dbuf<gwm_overlap> fused(n_fused), kept_overlaps(n_fused);
            dbuf<uint32_t> keep(n_fused);
            create_filter_kernel<<<grid_for(n_fused), kThreads, 0, s>>>(
                anchors, fh.p, n_fused, n_kept, kstart.p, klen.p, ksum.p, all_to_all,
                static_cast<uint64_t>(min_residues), static_cast<uint64_t>(min_overlap_len),
                static_cast<uint64_t>(min_bases_per_residue), min_overlap_fraction, fused.p, keep.p);
            GWM_CHECK(hipGetLastError());
            size_t bytes = 0;
            GWM_CHECK(rocprim::select(nullptr, bytes, fused.p, keep.p, kept_overlaps.p, d_count.p,
                                      static_cast<size_t>(n_fused), s));
            GWM_CHECK(rocprim::select(temp.get(bytes), bytes, fused.p, keep.p, kept_overlaps.p, d_count.p,
                                      static_cast<size_t>(n_fused), s));
            n_out = to_host(d_count.p, s);
            if (n_out > 0 && out)
                GWM_CHECK(hipMemcpyAsync(out, kept_overlaps.p, sizeof(gwm_overlap) * n_out, hipMemcpyDeviceToHost, s));
            if (n_out > 0 && device_out)
                *device_out = kept_overlaps.release();
        }
        ev.record(1, s);
        GWM_CHECK(hipStreamSynchronize(s));
        if (chain_fuse_filter_ms)
            *chain_fuse_filter_ms = ev.ms(0, 1);
        *count = n_out;
        return 0;
    }
    catch (const std::exception& e)
    {
        g_error = e.what();
        return -1;
    }
}

int gwm_find_overlaps(const gwm_anchor* anchors, int64_t n, int32_t all_to_all, int64_t min_residues, int64_t min_overlap_len,
                int64_t min_bases_per_residue, float min_overlap_fraction, void* stream, gwm_overlap* out,
                int64_t* count, float* chain_fuse_filter_ms)
{
    return find_overlaps(anchors, n, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                         min_overlap_fraction, stream, out, nullptr, count, chain_fuse_filter_ms);
}

int gwm_find_overlaps_device(const gwm_anchor* anchors, int64_t n, int32_t all_to_all, int64_t min_residues,
                             int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
                             void* stream, gwm_overlap** out, int64_t* count, float* chain_fuse_filter_ms)
{
    *out = nullptr;
    return find_overlaps(anchors, n, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                         min_overlap_fraction, stream, nullptr, out, count, chain_fuse_filter_ms);
}

void gwm_device_free(void* p) { (void)hipFree(p); }

} // extern "C"
