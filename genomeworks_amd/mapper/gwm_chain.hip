// gwm_chain.hip -- cudamapper's chaining overlapper on gfx950: anchors of one read pair chained by dynamic programming
// in both orientations, the best chains extracted, turned into overlap records and filtered (rules C1-C8 next to
// gwm_chain_overlaps in include/gwhip_mapper.h; DESIGN.md section 3.11 has the layout).
//
// One wave64 per group of anchors, four groups to a block of 256 threads, no LDS and no barrier. Lane s holds the
// latest anchor j = s (mod 64) of its group -- query and target position and both scores -- so the 64 lanes are the
// look-back window i - 64 .. i - 1 of every step and nothing shifts. Scores and predecessor distances go to global
// scratch; the same wave then extracts the chains from it.
#include "gwhip_mapper.h"

#include "gwm_device_utils.hpp"
#include "gwm_overlap_filter.hpp"

#include <climits>
#include <stdexcept>
#include <string>

namespace
{

constexpr uint32_t kLookBack      = 64;       // == the wave: one candidate predecessor per lane
constexpr uint32_t kMaxGroup      = 1u << 24; // anchors; scores stay below 2^24 * 32 = 2^29
constexpr int32_t kMaxChainsLimit = 64;

struct chain_params
{
    int32_t k;
    uint32_t max_gap, bandwidth;
    int32_t min_score, max_chains;
    int32_t all_to_all;
    uint64_t min_residues, min_overlap_len, min_bases_per_residue;
    float min_overlap_fraction;
};

__device__ __forceinline__ bool other_pair(const gwm_anchor& a, const gwm_anchor& b)
{
    return a.query_read_id != b.query_read_id || a.target_read_id != b.target_read_id;
}

__global__ void __launch_bounds__(kThreads) group_heads_kernel(const gwm_anchor* __restrict__ a, int64_t n,
                                                               uint32_t* __restrict__ head)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n)
        head[i] = (i == 0 || other_pair(a[i - 1], a[i])) ? 1u : 0u;
}

// Group g = anchors [start[g], start[g + 1]): worth a wave unless it is a read against itself (all against all) or
// smaller than min_residues -- the filter drops every record of either. The largest group goes to *longest.
__global__ void __launch_bounds__(kThreads) group_worth_kernel(const gwm_anchor* __restrict__ a,
                                                               const uint32_t* __restrict__ start, uint32_t n_groups,
                                                               uint32_t n_anchors, int32_t all_to_all,
                                                               uint64_t min_residues, uint32_t* __restrict__ worth,
                                                               uint32_t* __restrict__ longest)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups)
        return;
    const uint32_t len   = (g + 1 < n_groups ? start[g + 1] : n_anchors) - start[g];
    const gwm_anchor one = a[start[g]];
    worth[g] = (len >= min_residues && !(all_to_all && one.query_read_id == one.target_read_id)) ? 1u : 0u;
    atomicMax(longest, len);
}

// Worthwhile group w -> its first anchor, its length and its number of record slots: min(max_chains, length) rounds
// per orientation (a round uses up at least one anchor).
__global__ void __launch_bounds__(kThreads) group_slots_kernel(const uint32_t* __restrict__ start,
                                                               const uint32_t* __restrict__ ids, uint32_t n_worth,
                                                               uint32_t n_groups, uint32_t n_anchors,
                                                               uint32_t max_chains, uint32_t* __restrict__ first,
                                                               uint32_t* __restrict__ length,
                                                               int64_t* __restrict__ slots)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_worth)
        return;
    const uint32_t g   = ids[w];
    const uint32_t len = (g + 1 < n_groups ? start[g + 1] : n_anchors) - start[g];
    first[w]           = start[g];
    length[w]          = len;
    slots[w]           = 2 * static_cast<int64_t>(len < max_chains ? len : max_chains);
}

// the gfx9 DPP row-shift / row-broadcast sequence: lane 63 ends with the maximum of the wave
__device__ __forceinline__ int32_t wave_max(int32_t v)
{
    constexpr int32_t ident = INT32_MIN;
#define GWM_DPP_MAX(ctrl, rmask) v = max(v, __builtin_amdgcn_update_dpp(ident, v, ctrl, rmask, 0xf, false))
    GWM_DPP_MAX(0x111, 0xf); // row_shr:1
    GWM_DPP_MAX(0x112, 0xf); // row_shr:2
    GWM_DPP_MAX(0x114, 0xf); // row_shr:4
    GWM_DPP_MAX(0x118, 0xf); // row_shr:8
    GWM_DPP_MAX(0x142, 0xa); // row_bcast:15 into rows 1, 3
    GWM_DPP_MAX(0x143, 0xc); // row_bcast:31 into rows 2, 3
#undef GWM_DPP_MAX
    return __builtin_amdgcn_readlane(v, 63);
}

// C4: cost(0) = 0, cost(d) = d k / 100 + (floor(log2 d) >> 1); d < 2^31, k <= 32
__device__ __forceinline__ int32_t gap_cost(uint32_t d, uint32_t k)
{
    const int32_t linear = static_cast<int32_t>(static_cast<uint64_t>(d) * k / 100u);
    return d == 0 ? 0 : linear + ((31 - __clz(static_cast<int32_t>(d))) >> 1);
}

// f(j) + gain(j, i) of the anchor this lane holds, or INT32_MIN where it may not precede i (C3). dq and dt come in
// as uint32 differences that are exact where `ordered` says that both are positive.
__device__ __forceinline__ int32_t candidate(bool ordered, uint32_t dq, uint32_t dt, int32_t held_f,
                                             const chain_params& c)
{
    const uint32_t d   = dq > dt ? dq - dt : dt - dq;
    const bool ok      = ordered && dq <= c.max_gap && dt <= c.max_gap && d <= c.bandwidth;
    const uint32_t k   = static_cast<uint32_t>(c.k);
    const uint32_t hit = min(min(dq, dt), k);
    return ok ? held_f + static_cast<int32_t>(hit) - gap_cost(d, k) : INT32_MIN;
}

// C5 for one anchor and one orientation from the 64 candidates: f(i) and the distance to p(i) (0: none). Among equal
// candidates the nearest lane behind `step` wins, i.e. the largest j: the mask is rotated so that distance 1 is bit 63.
__device__ __forceinline__ void settle(int32_t v, uint32_t step, int32_t k, int32_t& f, uint32_t& distance)
{
    const int32_t best  = wave_max(v);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(v == best);
    const uint64_t rot  = step == 0 ? mask : (mask >> step) | (mask << (64 - step));
    const bool chained  = best > k; // INT32_MIN when nothing may precede
    f                   = chained ? best : k;
    distance            = chained ? 1u + static_cast<uint32_t>(__builtin_clzll(rot)) : 0u;
}

// C6 + C7 for one group and one orientation, by the whole wave. f, dist, used: this orientation's scratch of the
// group (used starts all zero). Slot r of `records` / `scores` / `keep` is round r. owner, where the caller asked for
// the chains: owner[i] = first_slot + r + 1 for every anchor i that round r visits, this orientation's part of the
// group as `used` is (starts all zero).
__device__ void extract_chains(const gwm_anchor* __restrict__ a, uint32_t m, const int32_t* f, const uint8_t* dist,
                               uint8_t* used, bool forward, const chain_params& c, uint32_t rounds,
                               gwm_overlap* __restrict__ records, int32_t* __restrict__ scores,
                               uint32_t* __restrict__ keep, uint32_t* owner, uint32_t first_slot)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t r = 0; r < rounds; ++r)
    {
        // the unused anchor of largest f, smallest index on ties: per lane over ascending indices, then over the lanes
        int32_t best_f   = -1; // every f is >= k >= 1
        uint32_t best_at = 0;
        for (uint32_t i = lane; i < m; i += 64)
        {
            const int32_t v = f[i];
            if (!used[i] && v > best_f)
            {
                best_f  = v;
                best_at = i;
            }
        }
        long long key = best_f < 0 ? -1ll : (static_cast<long long>(best_f) << 24) | (kMaxGroup - 1 - best_at);
        for (int off = 32; off > 0; off >>= 1)
        {
            const long long other = __shfl_xor(key, off);
            key                   = other > key ? other : key;
        }
        const int32_t end_f = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(key >> 24));
        const uint32_t end  = kMaxGroup - 1 - (static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(
                                                   static_cast<int32_t>(key & (kMaxGroup - 1)))));
        if (end_f < 0 || end_f < c.min_score)
            return;

        // The walk back. The 64 distances and used flags of the block of 64 anchors that holds the current position
        // are loaded at once, one per lane, and the walk goes from lane to lane until it leaves the block.
        uint32_t cur = end, first = end, residues = 0;
        int32_t cut_f = 0;
        bool walking  = true;
        while (walking)
        {
            const uint32_t block = cur & ~63u;
            const uint32_t mine  = block + lane;
            const uint32_t d     = mine < m ? dist[mine] : 0u;
            const uint32_t u     = mine < m ? used[mine] : 0u;
            uint64_t visited     = 0;
            while (true)
            {
                const uint32_t l = cur - block;
                if (__builtin_amdgcn_readlane(u, l) != 0u)
                {
                    cut_f   = f[cur]; // stopped in front of a used anchor
                    walking = false;
                    break;
                }
                visited |= uint64_t(1) << l;
                first = cur;
                ++residues;
                const uint32_t step = __builtin_amdgcn_readlane(d, l);
                if (step == 0u)
                {
                    walking = false;
                    break;
                }
                const bool leaves = step > l;
                cur -= step;
                if (leaves)
                    break;
            }
            if ((visited >> lane) & 1u)
            {
                used[mine] = 1;
                if (owner)
                    owner[mine] = first_slot + r + 1;
            }
        }
        const int32_t score = end_f - cut_f;
        if (lane == 0 && score >= c.min_score)
        {
            const gwm_anchor s = a[first], e = a[end];
            gwm_overlap o;
            o.query_read_id                 = e.query_read_id;
            o.target_read_id                = e.target_read_id;
            o.query_start_position_in_read  = s.query_position_in_read;
            o.query_end_position_in_read    = e.query_position_in_read;
            o.target_start_position_in_read = forward ? s.target_position_in_read : e.target_position_in_read;
            o.target_end_position_in_read   = forward ? e.target_position_in_read : s.target_position_in_read;
            o.relative_strand               = forward ? '+' : '-';
            o.num_residues                  = residues;
            o.overlap_complete              = 1;
            records[r]                      = o;
            scores[r]                       = score;
            keep[r] = passes_overlap_filter(o, c.all_to_all, c.min_residues, c.min_overlap_len, c.min_bases_per_residue,
                                            c.min_overlap_fraction)
                          ? 1u
                          : 0u;
        }
        // the next round's arg-max reads the used flags other lanes wrote
        __threadfence_block();
    }
}

// anchors: all of them; group w is anchors [first[w], first[w] + length[w]) and owns record slots
// [slot_end[w] - slots, slot_end[w]). f / dist / used: two arrays of n_anchors each ('+' then '-'), used all zero.
// owner: null, or laid out as `used` and all zero: the record slot + 1 of every anchor that a chain took.
__global__ void __launch_bounds__(kThreads) chain_dp_kernel(const gwm_anchor* __restrict__ anchors, int64_t n_anchors,
                                                            const uint32_t* __restrict__ first,
                                                            const uint32_t* __restrict__ length,
                                                            const int64_t* __restrict__ slot_end, uint32_t n_groups,
                                                            chain_params c, int32_t* f, uint8_t* dist, uint8_t* used,
                                                            gwm_overlap* __restrict__ records,
                                                            int32_t* __restrict__ scores, uint32_t* __restrict__ keep,
                                                            uint32_t* owner)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w    = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / 64) + threadIdx.x / 64);
    if (w >= n_groups)
        return;
    const uint32_t base = __builtin_amdgcn_readfirstlane(first[w]);
    const uint32_t m    = __builtin_amdgcn_readfirstlane(length[w]);
    const gwm_anchor* a = anchors + base;
    int32_t* f_plus     = f + base;
    int32_t* f_minus    = f + n_anchors + base;
    uint8_t* d_plus     = dist + base;
    uint8_t* d_minus    = dist + n_anchors + base;

    // what this lane holds: the latest anchor j = lane (mod 64), none before the first block reaches the lane
    uint32_t held_q = 0, held_t = 0;
    int32_t held_fp = 0, held_fm = 0;
    bool held = false;
    for (uint32_t i0 = 0; i0 < m; i0 += kLookBack)
    {
        const uint32_t steps = m - i0 < kLookBack ? m - i0 : kLookBack;
        gwm_anchor next      = {0, 0, 0, 0};
        if (lane < steps)
            next = a[i0 + lane];
        uint32_t dist_p = 0, dist_m = 0;
        for (uint32_t s = 0; s < steps; ++s) // anchor i = i0 + s, and i & 63 == s
        {
            const uint32_t qi = __builtin_amdgcn_readlane(next.query_position_in_read, s);
            const uint32_t ti = __builtin_amdgcn_readlane(next.target_position_in_read, s);
            // uint32 differences are exact where the comparison next to them says they are positive
            const uint32_t dq    = qi - held_q;
            const bool behind    = held && qi > held_q;
            const int32_t cand_p = candidate(behind && ti > held_t, dq, ti - held_t, held_fp, c);
            const int32_t cand_m = candidate(behind && held_t > ti, dq, held_t - ti, held_fm, c);
            int32_t fp, fm;
            uint32_t dp, dm;
            settle(cand_p, s, c.k, fp, dp);
            settle(cand_m, s, c.k, fm, dm);
            if (lane == s)
            {
                held_q  = qi;
                held_t  = ti;
                held_fp = fp;
                held_fm = fm;
                held    = true;
                dist_p  = dp;
                dist_m  = dm;
            }
        }
        if (lane < steps) // lane s took anchor i0 + s over at step s and kept it since
        {
            f_plus[i0 + lane]  = held_fp;
            f_minus[i0 + lane] = held_fm;
            d_plus[i0 + lane]  = static_cast<uint8_t>(dist_p);
            d_minus[i0 + lane] = static_cast<uint8_t>(dist_m);
        }
    }
    // the extraction reads scores and distances other lanes wrote
    __threadfence_block();

    const uint32_t rounds = m < static_cast<uint32_t>(c.max_chains) ? m : static_cast<uint32_t>(c.max_chains);
    const int64_t slot    = slot_end[w] - 2 * static_cast<int64_t>(rounds);
    extract_chains(a, m, f_plus, d_plus, used + base, true, c, rounds, records + slot, scores + slot, keep + slot,
                   owner ? owner + base : nullptr, static_cast<uint32_t>(slot));
    extract_chains(a, m, f_minus, d_minus, used + n_anchors + base, false, c, rounds, records + slot + rounds,
                   scores + slot + rounds, keep + slot + rounds, owner ? owner + n_anchors + base : nullptr,
                   static_cast<uint32_t>(slot + rounds));
}

template <typename T>
T* select_kept(const T* in, const uint32_t* keep, int64_t n, uint32_t* d_count, Temp& temp, hipStream_t s,
               dbuf<T>& out)
{
    out.resize(n);
    size_t bytes = 0;
    GWM_CHECK(rocprim::select(nullptr, bytes, in, keep, out.p, d_count, static_cast<size_t>(n), s));
    GWM_CHECK(rocprim::select(temp.get(bytes), bytes, in, keep, out.p, d_count, static_cast<size_t>(n), s));
    return out.p;
}

// Entry e of owner (anchor e of '+', then anchor e - n of '-'): flag[e] says that a kept record took the anchor,
// key[e] is that record's index (kept_through[slot] - 1, the inclusive scan of keep) and value[e] the anchor.
__global__ void __launch_bounds__(kThreads) chain_members_kernel(const uint32_t* __restrict__ owner, int64_t n,
                                                                 const uint32_t* __restrict__ keep,
                                                                 const uint32_t* __restrict__ kept_through,
                                                                 uint32_t* __restrict__ flag, uint32_t* __restrict__ key,
                                                                 uint32_t* __restrict__ value)
{
    const int64_t e = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= 2 * n)
        return;
    const uint32_t own = owner[e];
    const bool member  = own != 0 && keep[own - 1] != 0;
    flag[e]            = member ? 1u : 0u;
    key[e]             = member ? kept_through[own - 1] - 1 : 0u;
    value[e]           = static_cast<uint32_t>(e < n ? e : e - n);
}

// positions[2 i], [2 i + 1] = query and target position of anchor member[i]
__global__ void __launch_bounds__(kThreads) chain_positions_kernel(const gwm_anchor* __restrict__ a,
                                                                   const uint32_t* __restrict__ member, int64_t count,
                                                                   uint32_t* __restrict__ positions)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    const gwm_anchor x   = a[member[i]];
    positions[2 * i]     = x.query_position_in_read;
    positions[2 * i + 1] = x.target_position_in_read;
}

__global__ void __launch_bounds__(kThreads) chain_residues_kernel(const gwm_overlap* __restrict__ o, int64_t count,
                                                                  int64_t* __restrict__ residues)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < count)
        residues[i] = o[i].num_residues;
}

// The anchors of the kept records, in record order and in anchor order within a record, from the slot marks of the
// extraction: offsets[0 .. n_out] and positions; returns their number. A record's anchors all lie in one half of
// owner in ascending order, and the radix sort by record index is stable.
int64_t chain_members(const gwm_anchor* anchors, int64_t n, const uint32_t* owner, const uint32_t* keep, int64_t n_slots,
                      const gwm_overlap* kept_records, int64_t n_out, Temp& temp, hipStream_t s, dbuf<int64_t>& offsets,
                      dbuf<uint32_t>& positions)
{
    dbuf<uint32_t> kept_through(n_slots), flag(2 * n), key(2 * n), value(2 * n), d_count(1);
    inclusive_sum(keep, kept_through.p, n_slots, temp, s);
    chain_members_kernel<<<grid_for(2 * n), kThreads, 0, s>>>(owner, n, keep, kept_through.p, flag.p, key.p, value.p);
    GWM_CHECK(hipGetLastError());
    dbuf<uint32_t> keys, values;
    select_kept(key.p, flag.p, 2 * n, d_count.p, temp, s, keys);
    select_kept(value.p, flag.p, 2 * n, d_count.p, temp, s, values);
    const int64_t members = to_host(d_count.p, s);
    offsets.resize(n_out + 1);
    GWM_CHECK(hipMemsetAsync(offsets.p, 0, sizeof(int64_t), s));
    dbuf<int64_t> residues(n_out);
    chain_residues_kernel<<<grid_for(n_out), kThreads, 0, s>>>(kept_records, n_out, residues.p);
    GWM_CHECK(hipGetLastError());
    inclusive_sum(residues.p, offsets.p + 1, n_out, temp, s);
    if (to_host(offsets.p + n_out, s) != members)
        throw std::runtime_error("gwm_chain_overlaps: the kept records do not own the anchors their chains took");
    positions.resize(2 * members);
    if (members > 0)
    {
        dbuf<uint32_t> sorted_keys(members), sorted_values(members);
        sort_pairs(keys.p, sorted_keys.p, values.p, sorted_values.p, members, bits_for(static_cast<uint64_t>(n_out)), temp, s);
        chain_positions_kernel<<<grid_for(members), kThreads, 0, s>>>(anchors, sorted_values.p, members, positions.p);
        GWM_CHECK(hipGetLastError());
    }
    return members;
}

// what a caller that asked for the chains gets: host arrays of given capacity, or device arrays
struct chain_anchor_output
{
    int64_t* offsets_host      = nullptr;
    uint32_t* positions_host   = nullptr;
    int64_t capacity           = 0; // pairs of positions_host
    int64_t** offsets_device   = nullptr;
    uint32_t** positions_device = nullptr;
    int64_t* count             = nullptr; // pairs of all kept records
};

int chain_overlaps(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                   int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                   float min_overlap_fraction, void* stream, gwm_overlap* out_host, int32_t* scores_host,
                   int64_t capacity, gwm_overlap** out_device, int32_t** scores_device, int64_t* count,
                   float* chain_ms, const chain_anchor_output* chains = nullptr)
{
    *count = 0;
    if (chains && chains->count)
        *chains->count = 0;
    if (chain_ms)
        *chain_ms = 0.f;
    try
    {
        if (!chaining)
            throw std::invalid_argument("gwm_chain_overlaps: no chaining parameters");
        const gwm_chaining& p = *chaining;
        if (p.kmer_size < 1 || p.kmer_size > 32 || p.max_gap < 1 || p.bandwidth < 0 || p.min_chain_score < 0 ||
            p.max_chains < 1 || p.max_chains > kMaxChainsLimit)
            throw std::invalid_argument("gwm_chain_overlaps: need 1 <= kmer_size <= 32, max_gap >= 1, bandwidth >= 0, "
                                        "min_chain_score >= 0 and 1 <= max_chains <= 64");
        if (min_residues < 0 || min_overlap_len < 0 || min_bases_per_residue < 0)
            throw std::invalid_argument("gwm_chain_overlaps: min_residues, min_overlap_len and min_bases_per_residue "
                                        "must be >= 0");
        if (n <= 0)
        {
            if (chains && chains->offsets_host)
                chains->offsets_host[0] = 0;
            return 0;
        }
        if (n >= (int64_t(1) << 32))
            throw std::invalid_argument("gwm_chain_overlaps: 2^32 anchors or more");
        hipStream_t s = static_cast<hipStream_t>(stream);
        Events ev(2);
        Temp temp;
        dbuf<uint32_t> d_count(1), d_longest(1);
        ev.record(0, s);
        dbuf<uint32_t> head(n), start(n);
        group_heads_kernel<<<grid_for(n), kThreads, 0, s>>>(anchors, n, head.p);
        GWM_CHECK(hipGetLastError());
        const uint32_t n_groups = select_indices(head.p, n, start.p, d_count.p, temp, s);
        dbuf<uint32_t> worth(n_groups), ids(n_groups);
        GWM_CHECK(hipMemsetAsync(d_longest.p, 0, sizeof(uint32_t), s));
        group_worth_kernel<<<grid_for(n_groups), kThreads, 0, s>>>(anchors, start.p, n_groups,
                                                                  static_cast<uint32_t>(n), all_to_all,
                                                                  static_cast<uint64_t>(min_residues), worth.p,
                                                                  d_longest.p);
        GWM_CHECK(hipGetLastError());
        const uint32_t n_worth = select_indices(worth.p, n_groups, ids.p, d_count.p, temp, s);
        if (to_host(d_longest.p, s) >= kMaxGroup)
            throw std::invalid_argument("gwm_chain_overlaps: 2^24 anchors or more of one read pair");
        int64_t n_out = 0, n_members = 0;
        dbuf<int64_t> chain_offsets;
        dbuf<uint32_t> chain_positions;
        dbuf<gwm_overlap> kept_records;
        dbuf<int32_t> kept_scores;
        if (n_worth > 0)
        {
            dbuf<uint32_t> first(n_worth), length(n_worth);
            dbuf<int64_t> slots(n_worth), slot_end(n_worth);
            group_slots_kernel<<<grid_for(n_worth), kThreads, 0, s>>>(start.p, ids.p, n_worth, n_groups,
                                                                     static_cast<uint32_t>(n),
                                                                     static_cast<uint32_t>(p.max_chains), first.p,
                                                                     length.p, slots.p);
            GWM_CHECK(hipGetLastError());
            inclusive_sum(slots.p, slot_end.p, n_worth, temp, s);
            const int64_t n_slots = to_host(slot_end.p + n_worth - 1, s); // <= 2 n
            dbuf<int32_t> f(2 * n), slot_scores(n_slots);
            dbuf<uint8_t> dist(2 * n), used(2 * n);
            dbuf<gwm_overlap> slot_records(n_slots);
            dbuf<uint32_t> keep(n_slots), owner;
            if (chains)
            {
                if (n_slots >= (int64_t(1) << 32) - 1)
                    throw std::invalid_argument("gwm_chain_overlaps: 2^32 - 1 record slots or more with the chains asked for");
                owner.resize(2 * n);
                GWM_CHECK(hipMemsetAsync(owner.p, 0, sizeof(uint32_t) * static_cast<size_t>(2 * n), s));
            }
            GWM_CHECK(hipMemsetAsync(used.p, 0, static_cast<size_t>(2 * n), s));
            GWM_CHECK(hipMemsetAsync(keep.p, 0, sizeof(uint32_t) * static_cast<size_t>(n_slots), s));
            const chain_params c{p.kmer_size,
                                 static_cast<uint32_t>(p.max_gap),
                                 static_cast<uint32_t>(p.bandwidth),
                                 p.min_chain_score,
                                 p.max_chains,
                                 all_to_all,
                                 static_cast<uint64_t>(min_residues),
                                 static_cast<uint64_t>(min_overlap_len),
                                 static_cast<uint64_t>(min_bases_per_residue),
                                 min_overlap_fraction};
            const unsigned waves_per_block = kThreads / 64;
            chain_dp_kernel<<<(n_worth + waves_per_block - 1) / waves_per_block, kThreads, 0, s>>>(
                anchors, n, first.p, length.p, slot_end.p, n_worth, c, f.p, dist.p, used.p, slot_records.p,
                slot_scores.p, keep.p, owner.p);
            GWM_CHECK(hipGetLastError());
            select_kept(slot_records.p, keep.p, n_slots, d_count.p, temp, s, kept_records);
            select_kept(slot_scores.p, keep.p, n_slots, d_count.p, temp, s, kept_scores);
            n_out = to_host(d_count.p, s);
            if (chains && n_out > 0)
                n_members = chain_members(anchors, n, owner.p, keep.p, n_slots, kept_records.p, n_out, temp, s, chain_offsets,
                                          chain_positions);
        }
        ev.record(1, s);
        const int64_t n_copy = n_out < capacity ? n_out : capacity;
        if (chains && n_copy > 0)
        {
            if (chains->offsets_host)
                GWM_CHECK(hipMemcpyAsync(chains->offsets_host, chain_offsets.p, sizeof(int64_t) * (n_copy + 1), hipMemcpyDeviceToHost, s));
            // the anchors of the records copied, as far as the room reaches
            const int64_t theirs = n_copy == n_out ? n_members : to_host(chain_offsets.p + n_copy, s);
            const int64_t pairs  = theirs < chains->capacity ? theirs : chains->capacity;
            if (chains->positions_host && pairs > 0)
                GWM_CHECK(hipMemcpyAsync(chains->positions_host, chain_positions.p, sizeof(uint32_t) * 2 * pairs, hipMemcpyDeviceToHost, s));
        }
        else if (chains && chains->offsets_host)
            chains->offsets_host[0] = 0;
        if (n_copy > 0 && out_host)
            GWM_CHECK(hipMemcpyAsync(out_host, kept_records.p, sizeof(gwm_overlap) * n_copy, hipMemcpyDeviceToHost, s));
        if (n_copy > 0 && scores_host)
            GWM_CHECK(hipMemcpyAsync(scores_host, kept_scores.p, sizeof(int32_t) * n_copy, hipMemcpyDeviceToHost, s));
        GWM_CHECK(hipStreamSynchronize(s));
        if (chain_ms)
            *chain_ms = ev.ms(0, 1);
        if (n_out > 0 && out_device)
            *out_device = kept_records.release();
        if (n_out > 0 && scores_device)
            *scores_device = kept_scores.release();
        if (chains && n_out > 0 && chains->offsets_device)
            *chains->offsets_device = chain_offsets.release();
        if (chains && n_out > 0 && chains->positions_device)
            *chains->positions_device = chain_positions.release();
        if (chains && chains->count)
            *chains->count = n_members;
        *count = n_out;
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        return -1;
    }
}

} // namespace

extern "C" {

int gwm_chain_overlaps(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                       int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                       float min_overlap_fraction, void* stream, gwm_overlap* out, int32_t* scores, int64_t capacity,
                       int64_t* count, float* chain_ms)
{
    return chain_overlaps(anchors, n, chaining, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                          min_overlap_fraction, stream, out, scores, capacity, nullptr, nullptr, count, chain_ms);
}

int gwm_chain_overlaps_device(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                              int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                              float min_overlap_fraction, void* stream, gwm_overlap** out, int32_t** scores,
                              int64_t* count, float* chain_ms)
{
    *out = nullptr;
    if (scores)
        *scores = nullptr;
    return chain_overlaps(anchors, n, chaining, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                          min_overlap_fraction, stream, nullptr, nullptr, 0, out, scores, count, chain_ms);
}

int gwm_chain_overlaps_anchored(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                                int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                float min_overlap_fraction, void* stream, gwm_overlap* out, int32_t* scores, int64_t capacity,
                                int64_t* anchor_offsets, uint32_t* anchor_positions, int64_t anchor_capacity, int64_t* count,
                                int64_t* n_chain_anchors, float* chain_ms)
{
    chain_anchor_output chains;
    chains.offsets_host   = anchor_offsets;
    chains.positions_host = anchor_positions;
    chains.capacity       = anchor_capacity;
    chains.count          = n_chain_anchors;
    return chain_overlaps(anchors, n, chaining, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                          min_overlap_fraction, stream, out, scores, capacity, nullptr, nullptr, count, chain_ms, &chains);
}

int gwm_chain_overlaps_anchored_device(const gwm_anchor* anchors, int64_t n, const gwm_chaining* chaining, int32_t all_to_all,
                                       int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                       float min_overlap_fraction, void* stream, gwm_overlap** out, int32_t** scores,
                                       int64_t** anchor_offsets, uint32_t** anchor_positions, int64_t* count,
                                       int64_t* n_chain_anchors, float* chain_ms)
{
    *out = nullptr;
    if (scores)
        *scores = nullptr;
    if (anchor_offsets)
        *anchor_offsets = nullptr;
    if (anchor_positions)
        *anchor_positions = nullptr;
    chain_anchor_output chains;
    chains.offsets_device   = anchor_offsets;
    chains.positions_device = anchor_positions;
    chains.count            = n_chain_anchors;
    return chain_overlaps(anchors, n, chaining, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                          min_overlap_fraction, stream, nullptr, nullptr, 0, out, scores, count, chain_ms, &chains);
}
}
