// gwm_variants.hip -- cudamapper on gfx950: variant calling, the SNVs, deletions and insertion alleles of a target set
// under its aligned overlaps (include/gwhip_mapper.h, gwm_overlap_variants). Three device
// stages, and only the called records cross to the host:
//
// 1. In the chunk callback of gwm_align_chunks.hpp, next to the pileup of gwm_pileup_kernel.hpp: the insertion-run
//    consumer, run_kernel. One wave64 per alignment over tiles of 64 columns by the walk of gwm_column_walk.hpp; the
//    head of a run is found exactly as the pileup kernel finds it, so a run gives a record at the cell the pileup
//    counts it at. The head lane reads its run's length from the state bytes behind it, at most 33 of them, and packs
//    the at most 32 query bytes into the key itself: nothing of an open run is carried between tiles, and a run across
//    a tile boundary is the same code path as any other. A counting pass, an exclusive scan, a writing pass
//    (ChunkedOutput): records land by alignment and column, no atomics.
// 2. The allele vote: the run records sorted by (cell, L, key) (rocPRIM merge_sort), run-length encoded into
//    (cell, L, key, count) and reduced per cell to the best allele -- most records, then shorter, then smaller key
//    (two rocPRIM reduce_by_key over the one record type, whose count starts at 1).
// 3. Calling: one thread per base reads its counters and the target's byte and flags SNV and deletion in one byte, the
//    only per-base array besides the counters; a rocPRIM reduce counts both kinds, rocPRIM selects compact the flagged
//    cells of either kind and the best alleles that pass at the depth of their cell; one thread per selected item
//    writes its record, and two rocPRIM merges give the order of the result.
// Integer counts and total orders throughout: the records are a function of the multiset of alignments.
#include "gwm_pileup_kernel.hpp"

#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <rocprim/iterator/discard_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace
{

constexpr uint32_t kLongestRun = 32; // bases of an allele: two bits each fill the 64-bit key
constexpr uint32_t kSnv = 0, kDeletionKind = 1, kInsertionKind = 2;

// An insertion run of one alignment, and what the vote makes of equal ones (24 B): `count` is 1 as the consumer writes
// it, the number of equal records behind the run-length encoding.
struct gwm_insertion_run
{
    int64_t cell; // offsets[target read] + p
    uint64_t key;
    uint32_t length;
    uint32_t count;
};

// A, C, G, T = 0..3 of a base byte, as the pileup kernel reads it
__device__ __forceinline__ uint32_t channel_of(uint8_t c)
{
    const uint32_t code = (static_cast<uint32_t>(c) >> 1) & 3u; // A, C, T, G = 0, 1, 2, 3
    return code ^ (code >> 1);
}

// One wave64 per alignment of the chunk (states as AlignedChunk lays them out), target role. kWrite false: counts[i] =
// run records of alignment i. kWrite true: the records at runs[offsets[i]] in column order. A record is the head of a
// maximal run of state 3 with target bases on both sides (1 <= b and b + 1 <= target length, the pileup kernel's
// condition) whose length is 1..kLongestRun. Every state byte read lies within the alignment's len columns and every
// query byte within the query slice, which align_chunks() has checked against the read; the run is compared with the
// slice length all the same.
template <bool kWrite>
__global__ void __launch_bounds__(kThreads) run_kernel(const gwm_overlap* __restrict__ o,
                                                       const uint8_t* __restrict__ results,
                                                       const int64_t* __restrict__ starts,
                                                       const int32_t* __restrict__ result_lengths, int64_t m,
                                                       ReadSet qset, ReadSet tset, int64_t* __restrict__ counts,
                                                       const int64_t* __restrict__ offsets,
                                                       gwm_insertion_run* __restrict__ runs)
{
    const int64_t i     = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= m)
        return; // whole waves leave together
    const WaveAlignment w(o, results, starts, result_lengths, i);
    const gwm_overlap& x        = w.x;
    const uint32_t query_length = x.query_end_position_in_read - w.qs, target_length = w.te - w.ts;
    const uint8_t* query        = qset.bases + qset.offsets[x.query_read_id - qset.first_read_id];
    const int64_t target_at     = tset.offsets[x.target_read_id - tset.first_read_id];
    const uint32_t total        = kWrite ? static_cast<uint32_t>(offsets[i + 1] - offsets[i]) : 0u;
    gwm_insertion_run* out      = kWrite ? runs + offsets[i] : nullptr;
    const uint64_t lower        = (1ull << lane) - 1;
    // wave-uniform: columns walked so far that consume a query / a target base, the state of the last one, records
    uint32_t query_run = 0, target_run = 0, last_state = 0, records = 0;
    for (uint32_t base = 0; base < w.len; base += 64)
    {
        const TileColumn c(w, base, lane, lower, query_run, target_run);
        query_run = c.query_run, target_run = c.target_run;
        uint32_t before = __shfl_up(c.state, 1, 64);
        if (lane == 0)
            before = last_state;
        uint32_t length = 0;
        if (c.valid && c.state == 3 && before != 3 && c.b >= 1 && c.b + 1 <= target_length)
        {
            // the run's further columns j + 1, j + 2, ...: column j lies at s[len - 1 - j]
            const uint32_t j = base + lane;
            length           = 1;
            while (length <= kLongestRun && j + length < w.len && w.s[w.len - 1 - j - length] == 3)
                ++length; // kLongestRun + 1: a longer run, which is counted in the pileup and never called
            if (c.a + length > query_length)
                length = 0;
        }
        const bool record       = length >= 1 && length <= kLongestRun;
        const uint64_t recorded = __ballot(record);
        if (kWrite && record)
        {
            const uint32_t r = records + static_cast<uint32_t>(__popcll(recorded & lower));
            if (r < total)
            {
                // the allele in forward target coordinates: the query bases, on '-' their reverse complement
                uint64_t key = 0;
                for (uint32_t k = 0; k < length; ++k)
                {
                    const uint32_t at = w.reverse ? c.q + length - 1 - k : c.q + k;
                    const uint32_t ch = channel_of(query[at]);
                    key               = (key << 2) | (w.reverse ? 3u - ch : ch);
                }
                // c.t is the target position behind the run in column order: the larger neighbour where it ascends
                const uint32_t p = w.reverse ? c.t : c.t - 1;
                out[r]           = gwm_insertion_run{target_at + p, key, length, 1u};
            }
        }
        records += static_cast<uint32_t>(__popcll(recorded));
        last_state = __shfl(c.state, 63, 64);
    }
    if (!kWrite && lane == 0)
        counts[i] = records;
}

// The orders of the vote.
struct SameCellFirst
{
    __device__ bool operator()(const gwm_insertion_run& a, const gwm_insertion_run& b) const
    {
        if (a.cell != b.cell)
            return a.cell < b.cell;
        if (a.length != b.length)
            return a.length < b.length;
        return a.key < b.key;
    }
};
struct SameAllele
{
    __device__ bool operator()(const gwm_insertion_run& a, const gwm_insertion_run& b) const
    {
        return a.cell == b.cell && a.length == b.length && a.key == b.key;
    }
};
struct SameCell
{
    __device__ bool operator()(const gwm_insertion_run& a, const gwm_insertion_run& b) const { return a.cell == b.cell; }
};
struct AddCounts // of equal records
{
    __device__ gwm_insertion_run operator()(const gwm_insertion_run& a, const gwm_insertion_run& b) const
    {
        return {a.cell, a.key, a.length, a.count + b.count};
    }
};
struct BetterAllele // of one cell: most records, then the shorter, then the smaller key -- a total order
{
    __device__ gwm_insertion_run operator()(const gwm_insertion_run& a, const gwm_insertion_run& b) const
    {
        if (a.count != b.count)
            return a.count > b.count ? a : b;
        if (a.length != b.length)
            return a.length < b.length ? a : b;
        return a.key <= b.key ? a : b;
    }
};

// in[0 .. n), sorted so that records equal under `same` are neighbours, folded per group of equal records with `fold`
// into out; returns the number of groups
template <typename Same, typename Fold>
int64_t fold_groups(const gwm_insertion_run* in, int64_t n, gwm_insertion_run* out, size_t* d_count, Same same,
                    Fold fold, Temp& t, hipStream_t s)
{
    rocprim::discard_iterator keys_out;
    size_t bytes = 0;
    GWM_CHECK(rocprim::reduce_by_key(nullptr, bytes, in, in, static_cast<size_t>(n), keys_out, out, d_count, fold, same, s));
    GWM_CHECK(rocprim::reduce_by_key(t.get(bytes), bytes, in, in, static_cast<size_t>(n), keys_out, out, d_count, fold,
                                     same, s));
    return static_cast<int64_t>(to_host(d_count, s));
}

// The thresholds of a call, and what a thread reads of a cell.
struct Thresholds
{
    uint32_t min_count, min_percent;
    __device__ bool passes(uint32_t k, uint64_t d) const
    {
        return k >= min_count && 100ull * k >= static_cast<uint64_t>(min_percent) * d;
    }
};
struct Cell
{
    uint32_t ref, alt, alt_count, deletions;
    uint64_t depth;
    // counts: the pileup's channel-major planes of n_bases cells; bases: the target set's, which share the cells
    __device__ Cell(const uint32_t* counts, int64_t n_bases, const uint8_t* bases, int64_t cell, bool with_alt)
    {
        ref       = channel_of(bases[cell]);
        deletions = counts[static_cast<int64_t>(kDeletion) * n_bases + cell];
        depth     = deletions;
        alt = alt_count = 0;
        bool has_alt    = false;
        for (uint32_t c = 0; c < 4; ++c)
        {
            const uint32_t n = counts[static_cast<int64_t>(c) * n_bases + cell];
            depth += n;
            if (with_alt && c != ref && (!has_alt || n > alt_count)) // the smallest channel on a tie
                alt = c, alt_count = n, has_alt = true;
        }
    }
};

// one thread per base: bit 0 SNV, bit 1 deletion
__global__ void __launch_bounds__(kThreads) flag_kernel(const uint32_t* __restrict__ counts, int64_t n_bases,
                                                        const uint8_t* __restrict__ bases, Thresholds th,
                                                        uint8_t* __restrict__ flags)
{
    const int64_t cell = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (cell >= n_bases)
        return;
    const Cell c(counts, n_bases, bases, cell, true);
    flags[cell] = static_cast<uint8_t>((th.passes(c.alt_count, c.depth) ? 1u : 0u) |
                                       (th.passes(c.deletions, c.depth) ? 2u : 0u));
}

struct HasBit
{
    uint8_t bit;
    __device__ bool operator()(uint8_t flags) const { return (flags & bit) != 0; }
};

// how many cells are flagged for either kind: one reduction sizes the outputs of both selects
struct KindCounts
{
    int64_t snvs, deletions;
};
struct CountKinds
{
    __device__ KindCounts operator()(uint8_t flags) const { return {flags & 1, (flags >> 1) & 1}; }
};
struct AddKinds
{
    __device__ KindCounts operator()(const KindCounts& a, const KindCounts& b) const
    {
        return {a.snvs + b.snvs, a.deletions + b.deletions};
    }
};

// the best allele of a cell is called when its record count passes at the depth of the cell
struct AllelePasses
{
    const uint32_t* counts;
    int64_t n_bases;
    const uint8_t* bases;
    Thresholds th;
    __device__ bool operator()(const gwm_insertion_run& a) const
    {
        return a.cell >= 0 && a.cell < n_bases && th.passes(a.count, Cell(counts, n_bases, bases, a.cell, false).depth);
    }
};

// the read of a cell: the last one that begins at or before it (empty reads own no cell)
__device__ uint32_t read_of(const int64_t* offsets, uint32_t n_reads, int64_t cell)
{
    uint32_t lo = 0, hi = n_reads; // offsets[lo] <= cell < offsets[hi]
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= cell)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ gwm_variant variant_at(const ReadSet& tset, int64_t cell, uint32_t kind, const Cell& c)
{
    gwm_variant v{};
    v.target_read = read_of(tset.offsets, tset.n_reads, cell);
    v.position    = static_cast<uint32_t>(cell - tset.offsets[v.target_read]);
    v.depth       = static_cast<uint32_t>(c.depth);
    v.kind        = static_cast<uint8_t>(kind);
    v.ref         = static_cast<uint8_t>(c.ref);
    return v;
}

// one thread per selected cell of one kind (kSnv or kDeletionKind), cells ascending
__global__ void __launch_bounds__(kThreads) site_records_kernel(const int64_t* __restrict__ cells, int64_t n,
                                                                uint32_t kind, const uint32_t* __restrict__ counts,
                                                                int64_t n_bases, ReadSet tset,
                                                                gwm_variant* __restrict__ out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n)
        return;
    const int64_t cell = cells[i];
    const Cell c(counts, n_bases, tset.bases, cell, kind == kSnv);
    gwm_variant v = variant_at(tset, cell, kind, c);
    v.count       = kind == kSnv ? c.alt_count : c.deletions;
    v.alt         = static_cast<uint8_t>(c.alt);
    out[i]        = v;
}

// one thread per called allele, cells ascending
__global__ void __launch_bounds__(kThreads) insertion_records_kernel(const gwm_insertion_run* __restrict__ called,
                                                                     int64_t n, const uint32_t* __restrict__ counts,
                                                                     int64_t n_bases, ReadSet tset,
                                                                     gwm_variant* __restrict__ out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n)
        return;
    const gwm_insertion_run a = called[i];
    const Cell c(counts, n_bases, tset.bases, a.cell, false);
    gwm_variant v = variant_at(tset, a.cell, kInsertionKind, c);
    v.count       = a.count;
    v.length      = static_cast<uint8_t>(a.length);
    v.key         = a.key;
    out[i]        = v;
}

struct RecordOrder // by cell, then by kind
{
    __device__ bool operator()(const gwm_variant& a, const gwm_variant& b) const
    {
        if (a.target_read != b.target_read)
            return a.target_read < b.target_read;
        if (a.position != b.position)
            return a.position < b.position;
        return a.kind < b.kind;
    }
};

// a[0 .. na) and b[0 .. nb), each in RecordOrder, into out in RecordOrder
void merge_records(const gwm_variant* a, int64_t na, const gwm_variant* b, int64_t nb, gwm_variant* out, Temp& t,
                   hipStream_t s)
{
    if (na == 0 || nb == 0)
    {
        if (na + nb > 0)
            GWM_CHECK(hipMemcpyAsync(out, na ? a : b, sizeof(gwm_variant) * static_cast<size_t>(na + nb),
                                     hipMemcpyDeviceToDevice, s));
        return;
    }
    size_t bytes = 0;
    GWM_CHECK(rocprim::merge(nullptr, bytes, a, b, out, static_cast<size_t>(na), static_cast<size_t>(nb), RecordOrder{}, s));
    GWM_CHECK(rocprim::merge(t.get(bytes), bytes, a, b, out, static_cast<size_t>(na), static_cast<size_t>(nb),
                             RecordOrder{}, s));
}

KindCounts count_kinds(const uint8_t* flags, int64_t n_bases, Temp& t, hipStream_t s)
{
    dbuf<KindCounts> d_sum(1);
    rocprim::transform_iterator<const uint8_t*, CountKinds, KindCounts> kinds(flags, CountKinds{});
    size_t bytes = 0;
    GWM_CHECK(rocprim::reduce(nullptr, bytes, kinds, d_sum.p, KindCounts{0, 0}, static_cast<size_t>(n_bases), AddKinds{}, s));
    GWM_CHECK(rocprim::reduce(t.get(bytes), bytes, kinds, d_sum.p, KindCounts{0, 0}, static_cast<size_t>(n_bases),
                              AddKinds{}, s));
    return to_host(d_sum.p, s);
}

// the cells whose flag byte has `bit`, ascending, into cells, which holds as many as count_kinds() said
void flagged_cells(const uint8_t* flags, int64_t n_bases, uint8_t bit, int64_t* cells, size_t* d_count, Temp& t,
                   hipStream_t s)
{
    rocprim::counting_iterator<int64_t> all(0);
    size_t bytes = 0;
    GWM_CHECK(rocprim::select(nullptr, bytes, all, flags, cells, d_count, static_cast<size_t>(n_bases), HasBit{bit}, s));
    GWM_CHECK(rocprim::select(t.get(bytes), bytes, all, flags, cells, d_count, static_cast<size_t>(n_bases), HasBit{bit}, s));
}

// Stages 2 and 3 over the counters of the target set t (n_bases > 0) and the n_runs run records of the call, which
// are reordered in place: the called records in their final order into `variants`; returns their number.
int64_t vote_and_call(dbuf<gwm_insertion_run>& runs, int64_t n_runs, const uint32_t* counts, int64_t n_bases,
                      const ReadSet& t, Thresholds th, Temp& temp, hipStream_t s, dbuf<gwm_variant>& variants)
{
    dbuf<size_t> d_count(1);
    // the vote: sorted, run-length encoded, the best allele of every cell, those that pass
    int64_t n_called = 0;
    dbuf<gwm_insertion_run> folded(n_runs);
    if (n_runs > 0)
    {
        size_t bytes = 0;
        GWM_CHECK(rocprim::merge_sort(nullptr, bytes, runs.p, folded.p, static_cast<size_t>(n_runs), SameCellFirst{}, s));
        GWM_CHECK(rocprim::merge_sort(temp.get(bytes), bytes, runs.p, folded.p, static_cast<size_t>(n_runs),
                                      SameCellFirst{}, s));
        const int64_t n_alleles = fold_groups(folded.p, n_runs, runs.p, d_count.p, SameAllele{}, AddCounts{}, temp, s);
        const int64_t n_cells   = fold_groups(runs.p, n_alleles, folded.p, d_count.p, SameCell{}, BetterAllele{}, temp, s);
        const AllelePasses passes{counts, n_bases, t.bases, th};
        bytes = 0;
        GWM_CHECK(rocprim::select(nullptr, bytes, folded.p, runs.p, d_count.p, static_cast<size_t>(n_cells), passes, s));
        GWM_CHECK(rocprim::select(temp.get(bytes), bytes, folded.p, runs.p, d_count.p, static_cast<size_t>(n_cells),
                                  passes, s));
        n_called = static_cast<int64_t>(to_host(d_count.p, s)); // runs.p[0 .. n_called): the called alleles by cell
    }
    // SNV and deletion: the flags of every base, the flagged cells of either kind
    dbuf<uint8_t> flags(n_bases);
    flag_kernel<<<grid_for(n_bases), kThreads, 0, s>>>(counts, n_bases, t.bases, th, flags.p);
    GWM_CHECK(hipGetLastError());
    const KindCounts flagged = count_kinds(flags.p, n_bases, temp, s);
    const int64_t n_snv = flagged.snvs, n_deleted = flagged.deletions, total = n_snv + n_deleted + n_called;
    if (total == 0)
        return 0;
    dbuf<int64_t> snv_cells(n_snv), deleted_cells(n_deleted); // no per-base array beyond the counters and the flags
    if (n_snv > 0)
        flagged_cells(flags.p, n_bases, 1, snv_cells.p, d_count.p, temp, s);
    if (n_deleted > 0)
        flagged_cells(flags.p, n_bases, 2, deleted_cells.p, d_count.p, temp, s);
    // the records of the three kinds, each ascending by cell, then the order of the result by two merges
    dbuf<gwm_variant> kinds(total), sites(n_snv + n_deleted);
    gwm_variant *snvs = kinds.p, *deletions = kinds.p + n_snv, *insertions = kinds.p + n_snv + n_deleted;
    if (n_snv > 0)
        site_records_kernel<<<grid_for(n_snv), kThreads, 0, s>>>(snv_cells.p, n_snv, kSnv, counts, n_bases, t, snvs);
    if (n_deleted > 0)
        site_records_kernel<<<grid_for(n_deleted), kThreads, 0, s>>>(deleted_cells.p, n_deleted, kDeletionKind, counts,
                                                                      n_bases, t, deletions);
    if (n_called > 0)
        insertion_records_kernel<<<grid_for(n_called), kThreads, 0, s>>>(runs.p, n_called, counts, n_bases, t, insertions);
    GWM_CHECK(hipGetLastError());
    variants.resize(total);
    merge_records(snvs, n_snv, deletions, n_deleted, sites.p, temp, s);
    merge_records(sites.p, n_snv + n_deleted, insertions, n_called, variants.p, temp, s);
    GWM_CHECK(hipStreamSynchronize(s)); // the buffers of this scope are in use until here
    return total;
}

int overlap_variants(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                     int32_t n_queries, uint32_t first_query_read_id, const char* target_bases, const int64_t* target_offsets,
                     int32_t n_targets, uint32_t first_target_read_id, int32_t min_count, int32_t min_percent,
                     const gwm::Scoring& scoring, int64_t max_device_bytes, void* stream, gwm_variants* out);

} // namespace

extern "C" {

void gwm_variants_free(gwm_variants* variants)
{
    if (!variants)
        return;
    (void)hipFree(variants->variants);
    gwm_pileup_free(&variants->pileup);
    *variants = gwm_variants{};
}

int gwm_overlap_variants(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                         int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                         const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                         int32_t min_count, int32_t min_percent, int64_t max_device_bytes, void* stream,
                         gwm_variants* out)
{
    return gwm_overlap_variants_scored(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id, target_bases,
                                       target_offsets, n_targets, first_target_read_id, min_count, min_percent, nullptr,
                                       max_device_bytes, stream, out);
}

int gwm_overlap_variants_scored(const gwm_overlap* overlaps, int64_t n, const char* query_bases,
                                const int64_t* query_offsets, int32_t n_queries, uint32_t first_query_read_id,
                                const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                                uint32_t first_target_read_id, int32_t min_count, int32_t min_percent,
                                const gwm_scoring* scoring, int64_t max_device_bytes, void* stream, gwm_variants* out)
{
    return overlap_variants(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id, target_bases,
                            target_offsets, n_targets, first_target_read_id, min_count, min_percent, gwm::scoring_of(scoring),
                            max_device_bytes, stream, out);
}

int gwm_overlap_variants_scored2(const gwm_overlap* overlaps, int64_t n, const char* query_bases,
                                 const int64_t* query_offsets, int32_t n_queries, uint32_t first_query_read_id,
                                 const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                                 uint32_t first_target_read_id, int32_t min_count, int32_t min_percent,
                                 const gwm_scoring2* scoring, int64_t max_device_bytes, void* stream, gwm_variants* out)
{
    return overlap_variants(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id, target_bases,
                            target_offsets, n_targets, first_target_read_id, min_count, min_percent, gwm::scoring_of(scoring),
                            max_device_bytes, stream, out);
}

} // extern "C"

namespace
{

int overlap_variants(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                     int32_t n_queries, uint32_t first_query_read_id, const char* target_bases, const int64_t* target_offsets,
                     int32_t n_targets, uint32_t first_target_read_id, int32_t min_count, int32_t min_percent,
                     const gwm::Scoring& scoring, int64_t max_device_bytes, void* stream, gwm_variants* out)
{
    *out = gwm_variants{};
    try
    {
        check_chunk_arguments("gwm_overlap_variants", n_queries, n_targets, max_device_bytes, n);
        check_scoring("gwm_overlap_variants: ", scoring);
        if (min_count < 1)
            throw std::invalid_argument("gwm_overlap_variants: min_count below 1");
        if (min_percent < 0 || min_percent > 100)
            throw std::invalid_argument("gwm_overlap_variants: min_percent outside 0..100");
        hipStream_t s = static_cast<hipStream_t>(stream);
        dbuf<uint32_t> counts;
        dbuf<gwm_variant> variants;
        int64_t n_variants    = 0;
        const int64_t n_bases = zeroed_counts(target_offsets, n_targets, s, counts);
        const ReadSet q = read_set(query_bases, query_offsets, n_queries, first_query_read_id);
        const ReadSet t = read_set(target_bases, target_offsets, n_targets, first_target_read_id);
        if (n > 0)
        {
            ChunkedOutput<gwm_insertion_run> records(n, s);
            Temp temp;
            gwm::align_chunks("gwm_overlap_variants", overlaps, n, q, t, max_device_bytes, scoring, s, out->stage_ms,
                              [&](const AlignedChunk& c) {
                                  add_role<false>(c, q, t, n_bases, counts.p, s);
                                  records.add(
                                      c, temp, s,
                                      [&](int64_t* run_counts) {
                                          run_kernel<false><<<c.m_waves, kThreads, 0, s>>>(
                                              c.overlaps, c.results, c.starts, c.result_lengths, c.m, q, t, run_counts,
                                              nullptr, nullptr);
                                      },
                                      [&](const int64_t* offsets, gwm_insertion_run* runs) {
                                          run_kernel<true><<<c.m_waves, kThreads, 0, s>>>(
                                              c.overlaps, c.results, c.starts, c.result_lengths, c.m, q, t, nullptr,
                                              offsets, runs);
                                      });
                              });
            if (n_bases > 0)
            {
                Events ev(2);
                ev.record(0, s);
                dbuf<int64_t> run_offsets;
                dbuf<gwm_insertion_run> runs;
                const int64_t n_runs = records.finish(n, temp, s, run_offsets, runs);
                n_variants = vote_and_call(runs, n_runs, counts.p, n_bases, t,
                                           Thresholds{static_cast<uint32_t>(min_count), static_cast<uint32_t>(min_percent)},
                                           temp, s, variants);
                ev.record(1, s);
                out->stage_ms[3] = ev.ms(0, 1);
            }
        }
        GWM_CHECK(hipStreamSynchronize(s));
        out->pileup.n_bases = n_bases;
        out->pileup.counts  = counts.release();
        std::copy(out->stage_ms, out->stage_ms + 3, out->pileup.stage_ms);
        out->n_variants = n_variants;
        out->variants   = variants.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        *out = gwm_variants{};
        return -1;
    }
}

} // namespace
