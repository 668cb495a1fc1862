// mapper.cpp -- the flat C API of include/gw_mapper_capi.h (libcudamapper.so): extern "C" adapters over the owning
// Index / Matcher / host copy / result objects of gwm_handles.hpp, the index batcher (gwm_index_batcher.hpp) and the
// batched driver (gwm_driver.hpp).
#include "gw_mapper_capi.h"
#include "gwm_anchor_plan.hpp"
#include "gwm_driver.hpp"
#include "gwm_index_batcher.hpp"

#include <cstring>

namespace
{

using namespace gwm;

thread_local std::string g_capi_error;

template <typename F>
auto guarded(F&& f, decltype(f()) on_error) -> decltype(f())
{
    try
    {
        return f();
    }
    catch (const std::exception& e)
    {
        g_capi_error = e.what();
    }
    catch (...)
    {
        g_capi_error = "unknown exception";
    }
    return on_error;
}

// The read sets and the overlap records of one call on the device, uploaded once: q and t are the device copies of
// the queries and the targets. even_without_overlaps false: with n <= 0 nothing is uploaded and q, t and d are empty.
struct device_call
{
    read_sets reads;
    dbuf<gwm_overlap> d;
    const reads_view &q, &t;
    device_call(const reads_view& queries, const reads_view& targets, const void* overlaps, int64_t n,
                bool even_without_overlaps)
        : reads(queries, targets), q(reads.device_queries), t(reads.device_targets)
    {
        if (even_without_overlaps || n > 0)
        {
            reads.upload();
            d.upload(static_cast<const gwm_overlap*>(overlaps), n);
        }
    }
};

// the entry points that select layers refuse a negative max_depth, which their helpers take for "segments only"
bool refuse_negative_depth(const char* who, int32_t max_depth)
{
    if (max_depth < 0)
        g_capi_error = std::string(who) + ": negative max_depth";
    return max_depth < 0;
}

// The qualities of a weighted call: Phred+33 bytes that share the offsets of the bases, or
// nullptr for a set that has none. weighted false: a call of the entry points without qualities, which has none, is
// not validated and gathers no weights; everything else is one path, on which absent qualities filter nothing.
struct quality_options
{
    bool weighted                = false;
    const char* query_qualities  = nullptr; // in read correction: of the one set
    const char* target_qualities = nullptr;
    int32_t min_mean_quality     = 0;
};

// every byte in 33..126, before anything is uploaded
void check_qualities(const std::string& who, const char* qualities, const reads_view& reads)
{
    if (!qualities)
        return;
    if (reads.n < 0)
        throw std::invalid_argument(who + ": negative number of reads");
    const int64_t bytes = reads.offsets[reads.n];
    for (int64_t i = 0; i < bytes; ++i)
        if (qualities[i] < 33 || qualities[i] > 126)
            throw std::invalid_argument(who + ": quality byte " + std::to_string(i) + " lies outside 33..126");
}

void check_quality_options(const std::string& who, const quality_options& w, const reads_view& queries,
                           const reads_view& targets)
{
    if (w.min_mean_quality < 0)
        throw std::invalid_argument(who + ": negative min_mean_quality");
    check_qualities(who, w.query_qualities, queries);
    check_qualities(who, w.target_qualities, targets);
}

// a device copy of a set's qualities next to its reads; no qualities, no copy
void upload_qualities(dbuf<char>& device, const char* qualities, const reads_view& reads)
{
    if (qualities)
        device.upload(qualities, std::max<int64_t>(reads.offsets[reads.n], 1));
}

// Q1: the quality sums of the records of one role, on the device, and their copy to the host (4 B per record)
void quality_sums_of(const gwm_segments& s, const gwm_overlap* device_overlaps, int64_t n_overlaps, int32_t query_role,
                     const char* device_qualities, const reads_view& device_reads, uint32_t first_read_id, void* stream,
                     std::vector<uint32_t>& sums, float& sums_ms)
{
    sums.assign(static_cast<size_t>(s.n_segments), 0u);
    dbuf<uint32_t> device_sums(s.n_segments);
    float ms = 0.f;
    throw_on(gwm_segment_quality_sums(s.segments, s.n_segments, device_overlaps, n_overlaps, query_role,
                                      device_qualities, device_reads.offsets, device_reads.n, first_read_id,
                                      device_sums.p, stream, &ms));
    copy_out(sums.data(), device_sums.p, s.n_segments);
    sums_ms += ms;
}

// the windows of a selection into h: their table, and their bases gathered on the device and copied out once; with
// `qualities` (the device qualities of q and of t, either may be nullptr) their weights as well (Q3), one byte per base
void gather_windows(gw_mapper_windows& h, window_selection selection, const reads_view& q, const reads_view& t,
                    void* stream, const char* const* qualities = nullptr)
{
    h.windows = std::move(selection.windows);
    const std::vector<gwm_gather_entry>& plan = selection.plan;
    h.sequence_offsets.assign(plan.size() + 1, 0);
    for (size_t i = 0; i < plan.size(); ++i)
        h.sequence_offsets[i + 1] = h.sequence_offsets[i] + (plan[i].end - plan[i].begin);
    const int64_t total = h.sequence_offsets.back();
    h.bases.resize(static_cast<size_t>(total));
    if (total > 0)
    {
        dbuf<gwm_gather_entry> device_plan;
        dbuf<int64_t> device_starts;
        dbuf<char> device_bases(total);
        device_plan.upload(plan.data(), static_cast<int64_t>(plan.size()));
        device_starts.upload(h.sequence_offsets.data(), static_cast<int64_t>(plan.size()));
        throw_on(gwm_gather_sequences(device_plan.p, static_cast<int64_t>(plan.size()), device_starts.p, q.bases,
                                      q.offsets, q.n, t.bases, t.offsets, t.n, device_bases.p, total, stream,
                                      &h.stage_ms[3]));
        copy_out(h.bases.data(), device_bases.p, total);
        if (qualities)
        {
            h.weights.resize(static_cast<size_t>(total));
            dbuf<int8_t> device_weights(total);
            throw_on(gwm_gather_weights(device_plan.p, static_cast<int64_t>(plan.size()), device_starts.p, qualities[0],
                                        q.offsets, q.n, qualities[1], t.offsets, t.n, device_weights.p, total, stream,
                                        &h.quality_ms[1]));
            copy_out(h.weights.data(), device_weights.p, total);
        }
    }
}

struct owned_segments
{
    gwm_segments s{};
    ~owned_segments() { gwm_segments_free(&s); }
};

// the records of one role and their offsets to the host
void copy_segments(const gwm_segments& s, int64_t n, std::vector<gwm_segment>& segments, std::vector<int64_t>& offsets)
{
    segments.resize(static_cast<size_t>(s.n_segments));
    copy_out(segments.data(), s.segments, s.n_segments);
    offsets.assign(static_cast<size_t>(n) + 1, 0);
    copy_out(offsets.data(), s.segment_offsets, s.n > 0 ? s.n + 1 : 0);
}

// gw_mapper_window_overlaps, or with max_depth < 0 its segments pass alone: no selection, no gather, no windows
gw_mapper_windows* window_overlaps(const void* overlaps, int64_t n, const reads_view& query_reads,
                                   uint32_t first_query_read_id, const reads_view& target_reads,
                                   uint32_t first_target_read_id, int32_t window_length, int32_t max_depth,
                                   int64_t max_device_bytes, void* stream, const quality_options& options = {})
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_windows> h(new gw_mapper_windows());
        if (n < 0)
            throw std::invalid_argument("gw_mapper_window_overlaps: negative number of overlaps");
        const gwm_overlap* host_overlaps = static_cast<const gwm_overlap*>(overlaps);
        const bool all_to_all            = target_reads.bases == nullptr;
        quality_options w                = options;
        if (all_to_all) // the targets are the queries, with the queries' qualities
            w.target_qualities = nullptr;
        if (w.weighted)
            check_quality_options("gw_mapper_window_overlaps_weighted", w, query_reads, target_reads);
        // once: the segments pass and the window gather read the same device copies
        device_call c(query_reads, target_reads, overlaps, n, true);
        const read_sets& reads = c.reads;
        dbuf<char> query_qualities, target_qualities; // once as well, next to the reads; none without qualities
        upload_qualities(query_qualities, w.query_qualities, reads.queries);
        upload_qualities(target_qualities, w.target_qualities, reads.targets);
        // segments on the device, their records (24 B each) to the host
        owned_segments device;
        throw_on(gwm_window_segments(c.d.p, n, c.q.bases, c.q.offsets, reads.queries.n, first_query_read_id, c.t.bases,
                                     c.t.offsets, reads.targets.n, first_target_read_id, window_length, max_device_bytes,
                                     stream, &device.s));
        const gwm_segments& s = device.s;
        copy_segments(s, n, h->segments, h->segment_offsets);
        h->edit_distances.resize(static_cast<size_t>(n));
        copy_out(h->edit_distances.data(), s.edit_distances, s.n);
        std::memcpy(h->stage_ms, s.stage_ms, sizeof(s.stage_ms));
        if (max_depth < 0)
            return h.release();
        // the layers of every window, on the host
        std::vector<int64_t> target_lengths(static_cast<size_t>(reads.targets.n));
        for (int32_t r = 0; r < reads.targets.n; ++r)
            target_lengths[r] = reads.targets.offsets[r + 1] - reads.targets.offsets[r];
        // the queries supply every layer: their qualities, where there are any, decide which records are layers (Q2)
        if (query_qualities.p)
            quality_sums_of(s, c.d.p, n, 0, query_qualities.p, c.q, first_query_read_id, stream, h->quality_sums,
                            h->quality_ms[0]);
        window_selection selection = select_layers(
            h->segments.data(), s.n_segments, host_overlaps, n, reads.queries.n, first_query_read_id,
            target_lengths.data(), reads.targets.n, first_target_read_id, window_length, max_depth,
            query_qualities.p ? h->quality_sums.data() : nullptr, w.min_mean_quality);
        const char* const device_qualities[2] = {query_qualities.p, all_to_all ? query_qualities.p : target_qualities.p};
        gather_windows(*h, std::move(selection), c.q, c.t, stream, w.weighted ? device_qualities : nullptr);
        return h.release();
    }, static_cast<gw_mapper_windows*>(nullptr));
}

// gw_mapper_correction_windows; with max_depth < 0 gw_mapper_pair_segments: the records are taken for pairs as they
// stand and nothing is selected or gathered
gw_mapper_windows* correction_windows(const void* overlaps, int64_t n, const reads_view& host_reads,
                                      uint32_t first_read_id, int32_t window_length, int32_t max_depth,
                                      int64_t max_device_bytes, void* stream, const quality_options& w = {})
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_windows> h(new gw_mapper_windows());
        if (n < 0)
            throw std::invalid_argument("gw_mapper_correction_windows: negative number of overlaps");
        if (w.weighted)
            check_quality_options("gw_mapper_correction_windows_weighted", w, host_reads, host_reads);
        const gwm_overlap* given = static_cast<const gwm_overlap*>(overlaps);
        std::vector<gwm_overlap> pairs;
        if (max_depth < 0)
        {
            pairs.assign(given, given + n);
            for (int64_t i = 0; i < n; ++i)
                h->pair_positions.push_back(i);
        }
        else
        {
            h->pair_positions = select_pairs(given, n);
            for (int64_t i : h->pair_positions)
                pairs.push_back(given[i]);
        }
        const int64_t n_pairs = static_cast<int64_t>(pairs.size());
        // once: the segments pass and the window gather read the same device copy
        device_call c(host_reads, reads_view{nullptr, nullptr, 0}, pairs.data(), n_pairs, true);
        dbuf<char> qualities; // once as well, next to the reads; none without qualities
        upload_qualities(qualities, w.query_qualities, host_reads);
        const reads_view& r = c.q;
        owned_segments target_role, query_role;
        throw_on(gwm_pair_segments(c.d.p, n_pairs, r.bases, r.offsets, r.n, first_read_id, window_length,
                                   max_device_bytes, stream, &target_role.s, &query_role.s));
        copy_segments(target_role.s, n_pairs, h->segments, h->segment_offsets);
        copy_segments(query_role.s, n_pairs, h->query_role_segments, h->query_role_offsets);
        h->edit_distances.resize(static_cast<size_t>(n_pairs));
        copy_out(h->edit_distances.data(), target_role.s.edit_distances, target_role.s.n);
        std::memcpy(h->stage_ms, target_role.s.stage_ms, sizeof(target_role.s.stage_ms));
        h->query_role_ms = query_role.s.stage_ms[2];
        if (max_depth < 0)
            return h.release();
        std::vector<int64_t> lengths(static_cast<size_t>(host_reads.n));
        for (int32_t i = 0; i < host_reads.n; ++i)
            lengths[i] = host_reads.offsets[i + 1] - host_reads.offsets[i];
        // a target-role record's layer comes from the pair's query read, a query-role record's from its target read
        if (qualities.p)
        {
            quality_sums_of(target_role.s, c.d.p, n_pairs, 0, qualities.p, r, first_read_id, stream, h->quality_sums,
                            h->quality_ms[0]);
            quality_sums_of(query_role.s, c.d.p, n_pairs, 1, qualities.p, r, first_read_id, stream,
                            h->query_role_quality_sums, h->quality_ms[0]);
        }
        const char* const device_qualities[2] = {qualities.p, qualities.p};
        gather_windows(*h,
                       select_correction_layers(h->segments.data(), target_role.s.n_segments,
                                                h->query_role_segments.data(), query_role.s.n_segments, pairs.data(),
                                                n_pairs, lengths.data(), host_reads.n, first_read_id, window_length,
                                                max_depth, qualities.p ? h->quality_sums.data() : nullptr,
                                                qualities.p ? h->query_role_quality_sums.data() : nullptr,
                                                w.min_mean_quality),
                       r, r, stream, w.weighted ? device_qualities : nullptr);
        return h.release();
    }, static_cast<gw_mapper_windows*>(nullptr));
}

// what the selection entry points of the C API return and write: the number of sequences; the flat plan and window
// table where they are asked for and their capacities suffice
int64_t copy_selection(const window_selection& s, uint32_t* plan, int64_t plan_capacity, int64_t* n_windows,
                       uint32_t* window_table, int64_t window_capacity)
{
    const int64_t sequences = static_cast<int64_t>(s.plan.size()), windows = static_cast<int64_t>(s.windows.size());
    static_assert(sizeof(gwm_gather_entry) == 5 * sizeof(uint32_t) && sizeof(window_record) == 4 * sizeof(uint32_t),
                  "the flat layouts of gw_mapper_select_layers");
    if (plan && sequences <= plan_capacity && sequences > 0)
        std::memcpy(plan, s.plan.data(), sizeof(gwm_gather_entry) * s.plan.size());
    if (window_table && windows <= window_capacity && windows > 0)
        std::memcpy(window_table, s.windows.data(), sizeof(window_record) * s.windows.size());
    if (n_windows)
        *n_windows = windows;
    return sequences;
}

// the five integers of gw_mapper_chain_overlaps as the engine takes them
gwm_chaining chaining_of(const int32_t chaining[5])
{
    if (!chaining)
        throw std::invalid_argument("gw_mapper_chain_overlaps: no chaining parameters");
    return gwm_chaining{chaining[0], chaining[1], chaining[2], chaining[3], chaining[4]};
}

} // namespace

extern "C" {

const char* gw_mapper_last_error(void) { return g_capi_error.c_str(); }

gw_mapper_index* gw_mapper_index_create(const char* bases, const int64_t* offsets, int32_t n_reads,
                                        uint32_t first_read_id, int32_t kmer_size, int32_t window_size,
                                        int32_t hash_representations, double filtering_parameter, void* stream)
{
    return guarded([&] {
        return new gw_mapper_index(bases, offsets, n_reads, first_read_id, kmer_size, window_size, hash_representations,
                                   filtering_parameter, static_cast<hipStream_t>(stream));
    }, static_cast<gw_mapper_index*>(nullptr));
}

void gw_mapper_index_destroy(gw_mapper_index* index) { delete index; }

int gw_mapper_index_info(const gw_mapper_index* index, int64_t* sizes, uint32_t* reads, float* stage_ms)
{
    const gwm_index& x = index->x;
    if (sizes)
    {
        sizes[0] = x.n;
        sizes[1] = x.n_unique;
        sizes[2] = x.n_first_occurrence;
    }
    if (reads)
    {
        reads[0] = x.number_of_reads;
        reads[1] = x.number_of_reads > 0 ? x.first_read_id : 0;
        reads[2] = x.number_of_reads > 0 ? x.first_read_id + x.number_of_reads - 1 : 0;
        reads[3] = x.number_of_basepairs_in_longest_read;
    }
    if (stage_ms)
        std::memcpy(stage_ms, x.stage_ms, sizeof(x.stage_ms));
    return 0;
}

int gw_mapper_index_copy(const gw_mapper_index* index, uint64_t* representations, uint32_t* read_ids,
                         uint32_t* positions_in_reads, uint8_t* directions, uint64_t* unique_representations,
                         uint32_t* first_occurrence_of_representations)
{
    return guarded([&] {
        const gwm_index& x = index->x;
        copy_out(representations, x.representations, x.n);
        copy_out(read_ids, x.read_ids, x.n);
        copy_out(positions_in_reads, x.positions_in_reads, x.n);
        copy_out(directions, x.directions, x.n);
        copy_out(unique_representations, x.unique_representations, x.n_unique);
        copy_out(first_occurrence_of_representations, x.first_occurrence_of_representations, x.n_first_occurrence);
        return 0;
    }, GW_MAPPER_ERROR);
}

gw_mapper_index* gw_mapper_index_from_arrays(int64_t n, const uint32_t* read_ids, const uint32_t* positions_in_reads,
                                             int64_t n_unique, const uint64_t* unique_representations,
                                             const uint32_t* first_occurrence_of_representations,
                                             uint32_t first_read_id, uint32_t number_of_reads,
                                             uint32_t number_of_basepairs_in_longest_read)
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_index> h(new gw_mapper_index());
        throw_on(gwm_index_from_arrays(n, read_ids, positions_in_reads, n_unique, unique_representations,
                                       first_occurrence_of_representations, first_read_id, number_of_reads,
                                       number_of_basepairs_in_longest_read, &h->x));
        return h.release();
    }, static_cast<gw_mapper_index*>(nullptr));
}

gw_mapper_matcher* gw_mapper_matcher_create(const gw_mapper_index* query, const gw_mapper_index* target, void* stream)
{
    return guarded([&] { return new gw_mapper_matcher(*query, *target, static_cast<hipStream_t>(stream)); },
                   static_cast<gw_mapper_matcher*>(nullptr));
}

void gw_mapper_matcher_destroy(gw_mapper_matcher* matcher) { delete matcher; }

int64_t gw_mapper_matcher_anchor_count(const gw_mapper_matcher* matcher) { return matcher->a.n; }

int gw_mapper_matcher_copy_anchors(const gw_mapper_matcher* matcher, void* anchors, int64_t capacity, float* stage_ms)
{
    return guarded([&] {
        const int64_t n = capacity < matcher->a.n ? capacity : matcher->a.n;
        copy_out(static_cast<gwm_anchor*>(anchors), matcher->a.anchors, n);
        if (stage_ms)
            std::memcpy(stage_ms, matcher->a.stage_ms, sizeof(matcher->a.stage_ms));
        return 0;
    }, GW_MAPPER_ERROR);
}

int64_t gw_mapper_get_overlaps(const gw_mapper_matcher* matcher, int32_t all_to_all, int64_t min_residues,
                               int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
                               void* overlaps, float* chain_fuse_filter_ms, void* stream)
{
    return guarded([&] {
        int64_t count = 0;
        throw_on(gwm_find_overlaps(matcher->a.anchors, matcher->a.n, all_to_all, min_residues, min_overlap_len,
                                   min_bases_per_residue, min_overlap_fraction, stream,
                                   static_cast<gwm_overlap*>(overlaps), &count, chain_fuse_filter_ms));
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_get_overlaps_host(const void* anchors, int64_t n, int32_t all_to_all, int64_t min_residues,
                                    int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
                                    void* overlaps, void* stream)
{
    return guarded([&] {
        int64_t count = 0;
        if (n <= 0)
            return count;
        dbuf<gwm_anchor> d;
        d.upload(static_cast<const gwm_anchor*>(anchors), n);
        throw_on(gwm_find_overlaps(d.p, n, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                                   min_overlap_fraction, stream, static_cast<gwm_overlap*>(overlaps), &count, nullptr));
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_chain_overlaps(const gw_mapper_matcher* matcher, const int32_t chaining[5], int32_t all_to_all,
                                 int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                 float min_overlap_fraction, void* overlaps, int32_t* scores, int64_t capacity,
                                 float* chain_ms, void* stream)
{
    return guarded([&] {
        int64_t count        = 0;
        const gwm_chaining c = chaining_of(chaining);
        throw_on(gwm_chain_overlaps(matcher->a.anchors, matcher->a.n, &c, all_to_all, min_residues, min_overlap_len,
                                    min_bases_per_residue, min_overlap_fraction, stream,
                                    static_cast<gwm_overlap*>(overlaps), scores, capacity, &count, chain_ms));
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_chain_overlaps_host(const void* anchors, int64_t n, const int32_t chaining[5], int32_t all_to_all,
                                      int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                      float min_overlap_fraction, void* overlaps, int32_t* scores, int64_t capacity,
                                      float* chain_ms, void* stream)
{
    return guarded([&] {
        int64_t count        = 0;
        const gwm_chaining c = chaining_of(chaining);
        dbuf<gwm_anchor> d;
        if (n > 0 && n < (int64_t(1) << 32)) // the engine refuses the rest before it reads an anchor
            d.upload(static_cast<const gwm_anchor*>(anchors), n);
        throw_on(gwm_chain_overlaps(d.p, n, &c, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                                    min_overlap_fraction, stream, static_cast<gwm_overlap*>(overlaps), scores, capacity,
                                    &count, chain_ms));
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_chain_overlaps_anchored(const gw_mapper_matcher* matcher, const int32_t chaining[5], int32_t all_to_all,
                                          int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                          float min_overlap_fraction, void* overlaps, int32_t* scores, int64_t capacity,
                                          int64_t* anchor_offsets, uint32_t* anchor_positions, int64_t anchor_capacity,
                                          int64_t* n_chain_anchors, float* chain_ms, void* stream)
{
    return guarded([&] {
        int64_t count        = 0;
        const gwm_chaining c = chaining_of(chaining);
        throw_on(gwm_chain_overlaps_anchored(matcher->a.anchors, matcher->a.n, &c, all_to_all, min_residues, min_overlap_len,
                                             min_bases_per_residue, min_overlap_fraction, stream,
                                             static_cast<gwm_overlap*>(overlaps), scores, capacity, anchor_offsets,
                                             anchor_positions, anchor_capacity, &count, n_chain_anchors, chain_ms));
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_chain_overlaps_anchored_host(const void* anchors, int64_t n, const int32_t chaining[5],
                                               int32_t all_to_all, int64_t min_residues, int64_t min_overlap_len,
                                               int64_t min_bases_per_residue, float min_overlap_fraction, void* overlaps,
                                               int32_t* scores, int64_t capacity, int64_t* anchor_offsets,
                                               uint32_t* anchor_positions, int64_t anchor_capacity,
                                               int64_t* n_chain_anchors, float* chain_ms, void* stream)
{
    return guarded([&] {
        int64_t count        = 0;
        const gwm_chaining c = chaining_of(chaining);
        dbuf<gwm_anchor> d;
        if (n > 0 && n < (int64_t(1) << 32)) // the engine refuses the rest before it reads an anchor
            d.upload(static_cast<const gwm_anchor*>(anchors), n);
        throw_on(gwm_chain_overlaps_anchored(d.p, n, &c, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                                             min_overlap_fraction, stream, static_cast<gwm_overlap*>(overlaps), scores,
                                             capacity, anchor_offsets, anchor_positions, anchor_capacity, &count,
                                             n_chain_anchors, chain_ms));
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_map(const char* query_bases, const int64_t* query_offsets, int32_t n_queries,
                      const char* target_bases, const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size,
                      int32_t window_size, double filtering_parameter, int64_t min_residues, int64_t min_overlap_len,
                      int64_t min_bases_per_residue, float min_overlap_fraction, void* overlaps, int64_t capacity,
                      void* stream)
{
    return guarded([&] {
        hipStream_t s = static_cast<hipStream_t>(stream);
        const bool all_to_all = target_bases == nullptr;
        gw_mapper_index q(query_bases, query_offsets, n_queries, 0, kmer_size, window_size, 1, filtering_parameter, s);
        std::unique_ptr<gw_mapper_index> t;
        if (!all_to_all)
            t.reset(new gw_mapper_index(target_bases, target_offsets, n_targets, 0, kmer_size, window_size, 1,
                                        filtering_parameter, s));
        gw_mapper_matcher m(q, all_to_all ? q : *t, s);
        std::vector<gwm_overlap> out(static_cast<size_t>(m.a.n / 3 + 1)); // a kept chain holds >= 3 anchors
        int64_t count = 0;
        throw_on(gwm_find_overlaps(m.a.anchors, m.a.n, all_to_all ? 1 : 0, min_residues, min_overlap_len,
                                   min_bases_per_residue, min_overlap_fraction, s, out.data(), &count, nullptr));
        const int64_t n_copy = count < capacity ? count : capacity;
        if (overlaps && n_copy > 0)
            std::memcpy(overlaps, out.data(), sizeof(gwm_overlap) * static_cast<size_t>(n_copy));
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_post_process_overlaps(const void* overlaps, int64_t n, int32_t drop_fused_overlaps, void* out,
                                        int64_t capacity, void* stream, float* fuse_ms)
{
    return guarded([&] {
        int64_t count = 0;
        if (fuse_ms)
            *fuse_ms = 0.f;
        if (n <= 0)
            return count;
        dbuf<gwm_overlap> in, result;
        in.upload(static_cast<const gwm_overlap*>(overlaps), n);
        result.resize(n + n / 2);
        throw_on(gwm_post_process_overlaps(in.p, n, drop_fused_overlaps, stream, result.p, &count, fuse_ms));
        copy_out(static_cast<gwm_overlap*>(out), result.p, count < capacity ? count : capacity);
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

int gw_mapper_rescue_overlap_ends(void* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                                  int32_t n_queries, const char* target_bases, const int64_t* target_offsets,
                                  int32_t n_targets, uint32_t first_query_read_id, uint32_t first_target_read_id,
                                  int32_t extension, float required_similarity, void* stream, float* rescue_ms)
{
    return guarded([&] {
        if (rescue_ms)
            *rescue_ms = 0.f;
        // without overlaps nothing is uploaded, and the argument checks still apply
        device_call c({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, overlaps, n,
                      false);
        throw_on(gwm_rescue_overlap_ends(c.d.p, n, c.q.bases, c.q.offsets, c.reads.queries.n, first_query_read_id,
                                         c.t.bases, c.t.offsets, c.reads.targets.n, first_target_read_id, extension,
                                         required_similarity, stream, rescue_ms));
        copy_out(static_cast<gwm_overlap*>(overlaps), c.d.p, n);
        return 0;
    }, GW_MAPPER_ERROR);
}

int gw_mapper_extend_overlaps(void* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                              int32_t n_queries, const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                              uint32_t first_query_read_id, uint32_t first_target_read_id, const int32_t* extension,
                              int32_t max_extension, int64_t max_device_bytes, void* stream, int32_t* extensions,
                              int32_t* scores)
{
    return guarded([&] {
        if (extension == nullptr)
            throw std::invalid_argument("gw_mapper_extend_overlaps: no extension parameters");
        const gwm_extension e{extension[0], extension[1], extension[2], extension[3], extension[4], extension[5]};
        // without overlaps nothing is uploaded, and the argument checks still apply
        device_call c({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, overlaps, n,
                      false);
        dbuf<int32_t> moved, score;
        if (n > 0)
        {
            moved.resize(4 * n);
            score.resize(2 * n);
        }
        throw_on(gwm_extend_overlaps(c.d.p, n, c.q.bases, c.q.offsets, c.reads.queries.n, first_query_read_id, c.t.bases,
                                     c.t.offsets, c.reads.targets.n, first_target_read_id, &e, max_extension, max_device_bytes,
                                     stream, moved.p, score.p));
        copy_out(static_cast<gwm_overlap*>(overlaps), c.d.p, n);
        copy_out(extensions, moved.p, 4 * n);
        copy_out(scores, score.p, 2 * n);
        return 0;
    }, GW_MAPPER_ERROR);
}

int64_t gw_mapper_group_reads_into_indices(const int64_t* read_lengths, int64_t n_reads, int64_t max_basepairs_per_index,
                                           uint32_t* out, int64_t capacity)
{
    return guarded([&] {
        if (n_reads < 0)
            throw std::invalid_argument("gw_mapper_group_reads_into_indices: negative number of reads");
        const std::vector<descriptor> d = group_reads(read_lengths, n_reads, max_basepairs_per_index);
        const int64_t count             = static_cast<int64_t>(d.size());
        for (int64_t i = 0; out && i < count && i < capacity; ++i)
        {
            out[2 * i]     = d[i].first_read;
            out[2 * i + 1] = d[i].number_of_reads;
        }
        return count;
    }, int64_t(GW_MAPPER_ERROR));
}

gw_mapper_cigars* gw_mapper_align_overlaps(const void* overlaps, int64_t n, const char* query_bases,
                                           const int64_t* query_offsets, int32_t n_queries,
                                           uint32_t first_query_read_id, const char* target_bases,
                                           const int64_t* target_offsets, int32_t n_targets,
                                           uint32_t first_target_read_id, int64_t max_device_bytes, void* stream)
{
    return gw_mapper_align_overlaps_scored(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id,
                                           target_bases, target_offsets, n_targets, first_target_read_id, nullptr,
                                           max_device_bytes, stream);
}

namespace
{
// scoring[0..3] = mismatch, gap_open, gap_extend, band of the C API as the kernel level takes it; refused here when
// out of range, before anything is uploaded
const gwm_scoring* checked_scoring(const char* who, const int32_t* scoring, gwm_scoring* storage)
{
    if (scoring == nullptr)
        return nullptr;
    *storage = gwm_scoring{scoring[0], scoring[1], scoring[2], scoring[3]};
    if (scoring[0] < 1 || scoring[0] > 255 || scoring[1] < 0 || scoring[1] > 255 || scoring[2] < 1 || scoring[2] > 255 ||
        scoring[3] < 0)
        throw std::invalid_argument(std::string(who) + ": scoring (mismatch " + std::to_string(scoring[0]) + ", gap_open " +
                                    std::to_string(scoring[1]) + ", gap_extend " + std::to_string(scoring[2]) + ", band " +
                                    std::to_string(scoring[3]) + ") outside 1..255, 0..255, 1..255, >= 0");
    return storage;
}

// the same for scoring[0..5] = mismatch, gap_open, gap_extend, gap_open2, gap_extend2, band
const gwm_scoring2* checked_scoring2(const char* who, const int32_t* scoring, gwm_scoring2* storage)
{
    if (scoring == nullptr)
        return nullptr;
    gwm_scoring one_piece{};
    const int32_t first[4] = {scoring[0], scoring[1], scoring[2], scoring[5]};
    checked_scoring(who, first, &one_piece);
    *storage = gwm_scoring2{scoring[0], scoring[1], scoring[2], scoring[3], scoring[4], scoring[5]};
    if (scoring[3] < 0 || scoring[3] > 255 || scoring[4] < 1 || scoring[4] > 255)
        throw std::invalid_argument(std::string(who) + ": scoring (gap_open2 " + std::to_string(scoring[3]) + ", gap_extend2 " +
                                    std::to_string(scoring[4]) + ") outside 0..255, 1..255");
    return storage;
}
} // namespace

gw_mapper_cigars* gw_mapper_align_overlaps_scored(const void* overlaps, int64_t n, const char* query_bases,
                                                  const int64_t* query_offsets, int32_t n_queries,
                                                  uint32_t first_query_read_id, const char* target_bases,
                                                  const int64_t* target_offsets, int32_t n_targets,
                                                  uint32_t first_target_read_id, const int32_t* scoring,
                                                  int64_t max_device_bytes, void* stream)
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_cigars> h(new gw_mapper_cigars());
        gwm_scoring storage{};
        const gwm_scoring* sc = checked_scoring("gw_mapper_align_overlaps_scored", scoring, &storage);
        // without overlaps nothing is uploaded, and the argument checks still apply
        device_call c({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, overlaps, n,
                      false);
        throw_on(gwm_align_overlaps_scored(c.d.p, n, c.q.bases, c.q.offsets, c.reads.queries.n, first_query_read_id,
                                           c.t.bases, c.t.offsets, c.reads.targets.n, first_target_read_id, sc,
                                           max_device_bytes, stream, &h->c));
        return h.release();
    }, static_cast<gw_mapper_cigars*>(nullptr));
}

gw_mapper_cigars* gw_mapper_align_overlaps_scored2(const void* overlaps, int64_t n, const char* query_bases,
                                                   const int64_t* query_offsets, int32_t n_queries,
                                                   uint32_t first_query_read_id, const char* target_bases,
                                                   const int64_t* target_offsets, int32_t n_targets,
                                                   uint32_t first_target_read_id, const int32_t* scoring,
                                                   int64_t max_device_bytes, void* stream)
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_cigars> h(new gw_mapper_cigars());
        gwm_scoring2 storage{};
        const gwm_scoring2* sc = checked_scoring2("gw_mapper_align_overlaps_scored2", scoring, &storage);
        device_call c({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, overlaps, n,
                      false);
        throw_on(gwm_align_overlaps_scored2(c.d.p, n, c.q.bases, c.q.offsets, c.reads.queries.n, first_query_read_id,
                                            c.t.bases, c.t.offsets, c.reads.targets.n, first_target_read_id, sc,
                                            max_device_bytes, stream, &h->c));
        return h.release();
    }, static_cast<gw_mapper_cigars*>(nullptr));
}

gw_mapper_cigars* gw_mapper_align_overlaps_anchored(const void* overlaps, int64_t n, const char* query_bases,
                                                    const int64_t* query_offsets, int32_t n_queries,
                                                    uint32_t first_query_read_id, const char* target_bases,
                                                    const int64_t* target_offsets, int32_t n_targets,
                                                    uint32_t first_target_read_id, const int64_t* anchor_offsets,
                                                    const uint32_t* anchor_positions, int64_t n_anchors,
                                                    int32_t anchor_kmer_size, int32_t anchor_spacing,
                                                    const int32_t* scoring, int32_t scoring_values,
                                                    int64_t max_device_bytes, void* stream)
{
    return guarded([&] {
        const std::string who = "gw_mapper_align_overlaps_anchored";
        std::unique_ptr<gw_mapper_cigars> h(new gw_mapper_cigars());
        if ((scoring_values != 0 && scoring_values != 4 && scoring_values != 6) || (scoring_values != 0 && scoring == nullptr))
            throw std::invalid_argument(who + ": scoring_values must be 0, 4 or 6, with a scoring unless it is 0");
        gwm_scoring one{};
        gwm_scoring2 costs{};
        if (scoring_values == 4)
        {
            checked_scoring(who.c_str(), scoring, &one);
            costs = gwm_scoring2{one.mismatch, one.gap_open, one.gap_extend, 0, 0, one.band};
        }
        else if (scoring_values == 6)
            checked_scoring2(who.c_str(), scoring, &costs);
        // the lists, before anything is uploaded
        if (!gwm_plan::parameters_in_range(anchor_kmer_size, anchor_spacing))
            throw std::invalid_argument(who + ": anchor_kmer_size " + std::to_string(anchor_kmer_size) + ", anchor_spacing " +
                                        std::to_string(anchor_spacing) + " outside 1..32, >= 1");
        if (n_anchors < 0 || n_anchors >= (int64_t(1) << 32) || (n > 0 && anchor_offsets == nullptr) ||
            (n_anchors > 0 && anchor_positions == nullptr))
            throw std::invalid_argument(who + ": anchors without offsets or positions, or their number outside 0..2^32 - 1");
        if (n > 0)
        {
            const int64_t bad = gwm_plan::first_bad_offset(anchor_offsets, n, n_anchors);
            if (bad >= 0)
                throw std::invalid_argument(who + ": anchor offsets must start at 0, never decrease and end at the number of "
                                            "anchors (" + std::to_string(n_anchors) + "): entry " + std::to_string(bad) + " is " +
                                            std::to_string(anchor_offsets[bad]));
        }
        device_call c({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, overlaps, n,
                      false);
        dbuf<int64_t> offsets;
        dbuf<uint32_t> positions;
        if (n > 0)
        {
            offsets.upload(anchor_offsets, n + 1);
            positions.upload(anchor_positions, 2 * n_anchors);
        }
        const gwm_anchor_lists lists{offsets.p, positions.p, n_anchors, anchor_kmer_size, anchor_spacing};
        throw_on(gwm_align_overlaps_anchored(c.d.p, n, c.q.bases, c.q.offsets, c.reads.queries.n, first_query_read_id,
                                             c.t.bases, c.t.offsets, c.reads.targets.n, first_target_read_id, &lists,
                                             scoring_values == 0 ? 0 : scoring_values == 4 ? 1 : 2, &costs, max_device_bytes,
                                             stream, &h->c));
        return h.release();
    }, static_cast<gw_mapper_cigars*>(nullptr));
}

int64_t gw_mapper_cigars_count(const gw_mapper_cigars* cigars) { return cigars->c.n; }

int64_t gw_mapper_cigars_text_bytes(const gw_mapper_cigars* cigars) { return cigars->c.text_bytes; }

int gw_mapper_cigars_copy(const gw_mapper_cigars* cigars, char* text, int64_t* offsets, int32_t* edit_distances,
                          float* stage_ms)
{
    return guarded([&] {
        const gwm_cigars& c = cigars->c;
        copy_out(text, c.text, c.text_bytes);
        if (offsets && c.n == 0)
            offsets[0] = 0;
        copy_out(offsets, c.cigar_offsets, c.n > 0 ? c.n + 1 : 0);
        copy_out(edit_distances, c.edit_distances, c.n);
        if (stage_ms)
            std::memcpy(stage_ms, c.stage_ms, sizeof(c.stage_ms));
        return 0;
    }, GW_MAPPER_ERROR);
}

void gw_mapper_cigars_destroy(gw_mapper_cigars* cigars) { delete cigars; }

gw_mapper_windows* gw_mapper_window_overlaps(const void* overlaps, int64_t n, const char* query_bases,
                                             const int64_t* query_offsets, int32_t n_queries,
                                             uint32_t first_query_read_id, const char* target_bases,
                                             const int64_t* target_offsets, int32_t n_targets,
                                             uint32_t first_target_read_id, int32_t window_length, int32_t max_depth,
                                             int64_t max_device_bytes, void* stream)
{
    if (refuse_negative_depth("gw_mapper_window_overlaps", max_depth))
        return nullptr;
    return window_overlaps(overlaps, n, {query_bases, query_offsets, n_queries}, first_query_read_id,
                           {target_bases, target_offsets, n_targets}, first_target_read_id, window_length, max_depth,
                           max_device_bytes, stream);
}

gw_mapper_windows* gw_mapper_window_segments(const void* overlaps, int64_t n, const char* query_bases,
                                             const int64_t* query_offsets, int32_t n_queries,
                                             uint32_t first_query_read_id, const char* target_bases,
                                             const int64_t* target_offsets, int32_t n_targets,
                                             uint32_t first_target_read_id, int32_t window_length,
                                             int64_t max_device_bytes, void* stream)
{
    return window_overlaps(overlaps, n, {query_bases, query_offsets, n_queries}, first_query_read_id,
                           {target_bases, target_offsets, n_targets}, first_target_read_id, window_length, -1,
                           max_device_bytes, stream);
}

int gw_mapper_windows_counts(const gw_mapper_windows* windows, int64_t* counts)
{
    counts[0] = static_cast<int64_t>(windows->windows.size());
    counts[1] = static_cast<int64_t>(windows->sequence_offsets.size()) - 1;
    counts[2] = static_cast<int64_t>(windows->bases.size());
    counts[3] = static_cast<int64_t>(windows->segments.size());
    return 0;
}

int gw_mapper_windows_copy_segments(const gw_mapper_windows* windows, void* segments, int64_t* segment_offsets,
                                    int32_t* edit_distances, float* stage_ms)
{
    const gw_mapper_windows& w = *windows;
    if (segments && !w.segments.empty())
        std::memcpy(segments, w.segments.data(), sizeof(gwm_segment) * w.segments.size());
    if (segment_offsets)
        std::memcpy(segment_offsets, w.segment_offsets.data(), sizeof(int64_t) * w.segment_offsets.size());
    if (edit_distances && !w.edit_distances.empty())
        std::memcpy(edit_distances, w.edit_distances.data(), sizeof(int32_t) * w.edit_distances.size());
    if (stage_ms)
        std::memcpy(stage_ms, w.stage_ms, sizeof(w.stage_ms));
    return 0;
}

int gw_mapper_windows_copy_windows(const gw_mapper_windows* windows, char* bases, int64_t* sequence_offsets,
                                   int32_t* sequences_per_window, uint32_t* window_target_read, uint32_t* window_index)
{
    const gw_mapper_windows& w = *windows;
    if (bases && !w.bases.empty())
        std::memcpy(bases, w.bases.data(), w.bases.size());
    if (sequence_offsets)
        std::memcpy(sequence_offsets, w.sequence_offsets.data(), sizeof(int64_t) * w.sequence_offsets.size());
    for (size_t i = 0; i < w.windows.size(); ++i)
    {
        if (sequences_per_window)
            sequences_per_window[i] = static_cast<int32_t>(w.windows[i].n_sequences);
        if (window_target_read)
            window_target_read[i] = w.windows[i].target_read;
        if (window_index)
            window_index[i] = w.windows[i].window;
    }
    return 0;
}

void gw_mapper_windows_destroy(gw_mapper_windows* windows) { delete windows; }

int64_t gw_mapper_select_layers(const void* segments, int64_t n_segments, const void* overlaps, int64_t n_overlaps,
                                int32_t n_queries, uint32_t first_query_read_id, const int64_t* target_lengths,
                                int32_t n_targets, uint32_t first_target_read_id, int32_t window_length,
                                int32_t max_depth, uint32_t* plan, int64_t plan_capacity, int64_t* n_windows,
                                uint32_t* window_table, int64_t window_capacity)
{
    return gw_mapper_select_layers_weighted(segments, n_segments, overlaps, n_overlaps, n_queries, first_query_read_id,
                                            target_lengths, n_targets, first_target_read_id, window_length, max_depth,
                                            nullptr, 0, plan, plan_capacity, n_windows, window_table, window_capacity);
}

int64_t gw_mapper_select_layers_weighted(const void* segments, int64_t n_segments, const void* overlaps,
                                         int64_t n_overlaps, int32_t n_queries, uint32_t first_query_read_id,
                                         const int64_t* target_lengths, int32_t n_targets,
                                         uint32_t first_target_read_id, int32_t window_length, int32_t max_depth,
                                         const uint32_t* quality_sums, int32_t min_mean_quality, uint32_t* plan,
                                         int64_t plan_capacity, int64_t* n_windows, uint32_t* window_table,
                                         int64_t window_capacity)
{
    return guarded([&] {
        return copy_selection(select_layers(static_cast<const gwm_segment*>(segments), n_segments,
                                            static_cast<const gwm_overlap*>(overlaps), n_overlaps, n_queries,
                                            first_query_read_id, target_lengths, n_targets, first_target_read_id,
                                            window_length, max_depth, quality_sums, min_mean_quality),
                              plan, plan_capacity, n_windows, window_table, window_capacity);
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_select_pairs(const void* overlaps, int64_t n_overlaps, int64_t* positions, int64_t capacity)
{
    return guarded([&] {
        const std::vector<int64_t> kept = select_pairs(static_cast<const gwm_overlap*>(overlaps), n_overlaps);
        const int64_t n = static_cast<int64_t>(kept.size());
        if (positions && n <= capacity && n > 0)
            std::memcpy(positions, kept.data(), sizeof(int64_t) * kept.size());
        return n;
    }, int64_t(GW_MAPPER_ERROR));
}

int64_t gw_mapper_select_correction_layers(const void* target_role, int64_t n_target_role, const void* query_role,
                                           int64_t n_query_role, const void* pairs, int64_t n_pairs,
                                           const int64_t* read_lengths, int32_t n_reads, uint32_t first_read_id,
                                           int32_t window_length, int32_t max_depth, uint32_t* plan, int64_t plan_capacity,
                                           int64_t* n_windows, uint32_t* window_table, int64_t window_capacity)
{
    return gw_mapper_select_correction_layers_weighted(target_role, n_target_role, query_role, n_query_role, pairs,
                                                       n_pairs, read_lengths, n_reads, first_read_id, window_length,
                                                       max_depth, nullptr, nullptr, 0, plan, plan_capacity, n_windows,
                                                       window_table, window_capacity);
}

int64_t gw_mapper_select_correction_layers_weighted(const void* target_role, int64_t n_target_role,
                                                    const void* query_role, int64_t n_query_role, const void* pairs,
                                                    int64_t n_pairs, const int64_t* read_lengths, int32_t n_reads,
                                                    uint32_t first_read_id, int32_t window_length, int32_t max_depth,
                                                    const uint32_t* target_role_quality_sums,
                                                    const uint32_t* query_role_quality_sums, int32_t min_mean_quality,
                                                    uint32_t* plan, int64_t plan_capacity, int64_t* n_windows,
                                                    uint32_t* window_table, int64_t window_capacity)
{
    return guarded([&] {
        return copy_selection(
            select_correction_layers(static_cast<const gwm_segment*>(target_role), n_target_role,
                                     static_cast<const gwm_segment*>(query_role), n_query_role,
                                     static_cast<const gwm_overlap*>(pairs), n_pairs, read_lengths, n_reads,
                                     first_read_id, window_length, max_depth, target_role_quality_sums,
                                     query_role_quality_sums, min_mean_quality),
            plan, plan_capacity, n_windows, window_table, window_capacity);
    }, int64_t(GW_MAPPER_ERROR));
}

gw_mapper_windows* gw_mapper_correction_windows(const void* overlaps, int64_t n, const char* bases,
                                                const int64_t* offsets, int32_t n_reads, uint32_t first_read_id,
                                                int32_t window_length, int32_t max_depth, int64_t max_device_bytes,
                                                void* stream)
{
    if (refuse_negative_depth("gw_mapper_correction_windows", max_depth))
        return nullptr;
    return correction_windows(overlaps, n, {bases, offsets, n_reads}, first_read_id, window_length, max_depth,
                              max_device_bytes, stream);
}

gw_mapper_windows* gw_mapper_pair_segments(const void* pairs, int64_t n, const char* bases, const int64_t* offsets,
                                           int32_t n_reads, uint32_t first_read_id, int32_t window_length,
                                           int64_t max_device_bytes, void* stream)
{
    return correction_windows(pairs, n, {bases, offsets, n_reads}, first_read_id, window_length, -1, max_device_bytes,
                              stream);
}

int64_t gw_mapper_windows_copy_query_role_segments(const gw_mapper_windows* windows, void* segments, int64_t capacity,
                                                   int64_t* query_role_offsets, int64_t* pair_positions, int64_t* n_pairs,
                                                   float* query_role_ms)
{
    const gw_mapper_windows& w = *windows;
    const int64_t n            = static_cast<int64_t>(w.query_role_segments.size());
    if (segments && n <= capacity && n > 0)
        std::memcpy(segments, w.query_role_segments.data(), sizeof(gwm_segment) * w.query_role_segments.size());
    if (query_role_offsets)
        std::memcpy(query_role_offsets, w.query_role_offsets.data(), sizeof(int64_t) * w.query_role_offsets.size());
    if (pair_positions && !w.pair_positions.empty())
        std::memcpy(pair_positions, w.pair_positions.data(), sizeof(int64_t) * w.pair_positions.size());
    if (n_pairs)
        *n_pairs = static_cast<int64_t>(w.pair_positions.size());
    if (query_role_ms)
        *query_role_ms = w.query_role_ms;
    return n;
}

gw_mapper_pileup* gw_mapper_overlap_pileup(const void* overlaps, int64_t n, const char* query_bases,
                                           const int64_t* query_offsets, int32_t n_queries,
                                           uint32_t first_query_read_id, const char* target_bases,
                                           const int64_t* target_offsets, int32_t n_targets,
                                           uint32_t first_target_read_id, int64_t max_device_bytes, void* stream)
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_pileup> h(new gw_mapper_pileup());
        if (n < 0)
            throw std::invalid_argument("gw_mapper_overlap_pileup: negative number of overlaps");
        // without overlaps too: the counters are those of the target set
        device_call c({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, overlaps, n,
                      true);
        throw_on(gwm_overlap_pileup(c.d.p, n, c.q.bases, c.q.offsets, c.reads.queries.n, first_query_read_id, c.t.bases,
                                    c.t.offsets, c.reads.targets.n, first_target_read_id, max_device_bytes, stream,
                                    &h->p));
        return h.release();
    }, static_cast<gw_mapper_pileup*>(nullptr));
}

gw_mapper_pileup* gw_mapper_pair_pileup(const void* pairs, int64_t n, const char* bases, const int64_t* offsets,
                                        int32_t n_reads, uint32_t first_read_id, int64_t max_device_bytes, void* stream)
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_pileup> h(new gw_mapper_pileup());
        if (n < 0)
            throw std::invalid_argument("gw_mapper_pair_pileup: negative number of pairs");
        device_call c({bases, offsets, n_reads}, reads_view{nullptr, nullptr, 0}, pairs, n, true);
        throw_on(gwm_pair_pileup(c.d.p, n, c.q.bases, c.q.offsets, c.q.n, first_read_id, max_device_bytes, stream, &h->p));
        return h.release();
    }, static_cast<gw_mapper_pileup*>(nullptr));
}

int64_t gw_mapper_pileup_bases(const gw_mapper_pileup* pileup) { return pileup->p.n_bases; }

int gw_mapper_pileup_copy(const gw_mapper_pileup* pileup, uint32_t* counts, float* stage_ms)
{
    return guarded([&] {
        const gwm_pileup& p = pileup->p;
        copy_out(counts, p.counts, 6 * p.n_bases);
        if (stage_ms)
            std::memcpy(stage_ms, p.stage_ms, sizeof(p.stage_ms));
        return 0;
    }, GW_MAPPER_ERROR);
}

void gw_mapper_pileup_destroy(gw_mapper_pileup* pileup) { delete pileup; }

gw_mapper_variants* gw_mapper_overlap_variants(const void* overlaps, int64_t n, const char* query_bases,
                                               const int64_t* query_offsets, int32_t n_queries,
                                               uint32_t first_query_read_id, const char* target_bases,
                                               const int64_t* target_offsets, int32_t n_targets,
                                               uint32_t first_target_read_id, int32_t min_count, int32_t min_percent,
                                               int64_t max_device_bytes, void* stream)
{
    return gw_mapper_overlap_variants_scored(overlaps, n, query_bases, query_offsets, n_queries, first_query_read_id,
                                             target_bases, target_offsets, n_targets, first_target_read_id, min_count,
                                             min_percent, nullptr, max_device_bytes, stream);
}

gw_mapper_variants* gw_mapper_overlap_variants_scored(const void* overlaps, int64_t n, const char* query_bases,
                                                      const int64_t* query_offsets, int32_t n_queries,
                                                      uint32_t first_query_read_id, const char* target_bases,
                                                      const int64_t* target_offsets, int32_t n_targets,
                                                      uint32_t first_target_read_id, int32_t min_count,
                                                      int32_t min_percent, const int32_t* scoring,
                                                      int64_t max_device_bytes, void* stream)
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_variants> h(new gw_mapper_variants());
        gwm_scoring storage{};
        const gwm_scoring* sc = checked_scoring("gw_mapper_overlap_variants_scored", scoring, &storage);
        if (n < 0)
            throw std::invalid_argument("gw_mapper_overlap_variants: negative number of overlaps");
        // refused before the reads are uploaded: nothing reaches the device
        if (min_count < 1)
            throw std::invalid_argument("gw_mapper_overlap_variants: min_count below 1");
        if (min_percent < 0 || min_percent > 100)
            throw std::invalid_argument("gw_mapper_overlap_variants: min_percent outside 0..100");
        // without overlaps too: the counters are those of the target set
        device_call c({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, overlaps, n,
                      true);
        throw_on(gwm_overlap_variants_scored(c.d.p, n, c.q.bases, c.q.offsets, c.reads.queries.n, first_query_read_id,
                                             c.t.bases, c.t.offsets, c.reads.targets.n, first_target_read_id, min_count,
                                             min_percent, sc, max_device_bytes, stream, &h->v));
        return h.release();
    }, static_cast<gw_mapper_variants*>(nullptr));
}

gw_mapper_variants* gw_mapper_overlap_variants_scored2(const void* overlaps, int64_t n, const char* query_bases,
                                                       const int64_t* query_offsets, int32_t n_queries,
                                                       uint32_t first_query_read_id, const char* target_bases,
                                                       const int64_t* target_offsets, int32_t n_targets,
                                                       uint32_t first_target_read_id, int32_t min_count,
                                                       int32_t min_percent, const int32_t* scoring,
                                                       int64_t max_device_bytes, void* stream)
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_variants> h(new gw_mapper_variants());
        gwm_scoring2 storage{};
        const gwm_scoring2* sc = checked_scoring2("gw_mapper_overlap_variants_scored2", scoring, &storage);
        if (n < 0)
            throw std::invalid_argument("gw_mapper_overlap_variants: negative number of overlaps");
        if (min_count < 1)
            throw std::invalid_argument("gw_mapper_overlap_variants: min_count below 1");
        if (min_percent < 0 || min_percent > 100)
            throw std::invalid_argument("gw_mapper_overlap_variants: min_percent outside 0..100");
        device_call c({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, overlaps, n,
                      true);
        throw_on(gwm_overlap_variants_scored2(c.d.p, n, c.q.bases, c.q.offsets, c.reads.queries.n, first_query_read_id,
                                              c.t.bases, c.t.offsets, c.reads.targets.n, first_target_read_id, min_count,
                                              min_percent, sc, max_device_bytes, stream, &h->v));
        return h.release();
    }, static_cast<gw_mapper_variants*>(nullptr));
}

int64_t gw_mapper_variants_count(const gw_mapper_variants* variants) { return variants->v.n_variants; }

int gw_mapper_variants_copy(const gw_mapper_variants* variants, void* records, float* stage_ms)
{
    return guarded([&] {
        const gwm_variants& v = variants->v;
        copy_out(static_cast<gwm_variant*>(records), v.variants, v.n_variants);
        if (stage_ms)
            std::memcpy(stage_ms, v.stage_ms, sizeof(v.stage_ms));
        return 0;
    }, GW_MAPPER_ERROR);
}

int gw_mapper_variants_pileup_copy(const gw_mapper_variants* variants, uint32_t* counts)
{
    return guarded([&] {
        const gwm_pileup& p = variants->v.pileup;
        copy_out(counts, p.counts, 6 * p.n_bases);
        return 0;
    }, GW_MAPPER_ERROR);
}

void gw_mapper_variants_destroy(gw_mapper_variants* variants) { delete variants; }

gw_mapper_windows* gw_mapper_window_overlaps_weighted(const void* overlaps, int64_t n, const char* query_bases,
                                                      const int64_t* query_offsets, int32_t n_queries,
                                                      uint32_t first_query_read_id, const char* target_bases,
                                                      const int64_t* target_offsets, int32_t n_targets,
                                                      uint32_t first_target_read_id, const char* query_qualities,
                                                      const char* target_qualities, int32_t min_mean_quality,
                                                      int32_t window_length, int32_t max_depth,
                                                      int64_t max_device_bytes, void* stream)
{
    if (refuse_negative_depth("gw_mapper_window_overlaps_weighted", max_depth))
        return nullptr;
    return window_overlaps(overlaps, n, {query_bases, query_offsets, n_queries}, first_query_read_id,
                           {target_bases, target_offsets, n_targets}, first_target_read_id, window_length, max_depth,
                           max_device_bytes, stream, {true, query_qualities, target_qualities, min_mean_quality});
}

gw_mapper_windows* gw_mapper_correction_windows_weighted(const void* overlaps, int64_t n, const char* bases,
                                                         const int64_t* offsets, int32_t n_reads,
                                                         uint32_t first_read_id, const char* qualities,
                                                         int32_t min_mean_quality, int32_t window_length,
                                                         int32_t max_depth, int64_t max_device_bytes, void* stream)
{
    if (refuse_negative_depth("gw_mapper_correction_windows_weighted", max_depth))
        return nullptr;
    return correction_windows(overlaps, n, {bases, offsets, n_reads}, first_read_id, window_length, max_depth,
                              max_device_bytes, stream, {true, qualities, nullptr, min_mean_quality});
}

int gw_mapper_windows_copy_weights(const gw_mapper_windows* windows, int8_t* weights, uint32_t* quality_sums,
                                   uint32_t* query_role_quality_sums, float* ms)
{
    const gw_mapper_windows& w = *windows;
    if (weights && !w.weights.empty())
        std::memcpy(weights, w.weights.data(), w.weights.size());
    if (quality_sums && !w.quality_sums.empty())
        std::memcpy(quality_sums, w.quality_sums.data(), sizeof(uint32_t) * w.quality_sums.size());
    if (query_role_quality_sums && !w.query_role_quality_sums.empty())
        std::memcpy(query_role_quality_sums, w.query_role_quality_sums.data(),
                    sizeof(uint32_t) * w.query_role_quality_sums.size());
    if (ms)
        std::memcpy(ms, w.quality_ms, sizeof(w.quality_ms));
    return 0;
}

int gw_mapper_segment_quality_sums(const void* segments, int64_t n_segments, const void* overlaps, int64_t n_overlaps,
                                   int32_t query_role, const char* qualities, const int64_t* offsets, int32_t n_reads,
                                   uint32_t first_read_id, uint32_t* sums, void* stream, float* sums_ms)
{
    return guarded([&] {
        if (sums_ms)
            *sums_ms = 0.f;
        if (n_segments < 0 || n_overlaps < 0 || n_reads < 0)
            throw std::invalid_argument("gw_mapper_segment_quality_sums: a negative count");
        if (!qualities || !offsets)
            throw std::invalid_argument("gw_mapper_segment_quality_sums: no qualities");
        const reads_view reads{qualities, offsets, n_reads};
        check_qualities("gw_mapper_segment_quality_sums", qualities, reads);
        if (n_segments == 0)
            return 0;
        dbuf<char> device_qualities;
        dbuf<int64_t> device_offsets;
        dbuf<gwm_segment> device_segments;
        dbuf<gwm_overlap> device_overlaps;
        dbuf<uint32_t> device_sums(n_segments);
        upload_qualities(device_qualities, qualities, reads);
        device_offsets.upload(offsets, static_cast<int64_t>(n_reads) + 1);
        device_segments.upload(static_cast<const gwm_segment*>(segments), n_segments);
        device_overlaps.upload(static_cast<const gwm_overlap*>(overlaps), n_overlaps);
        throw_on(gwm_segment_quality_sums(device_segments.p, n_segments, device_overlaps.p, n_overlaps, query_role,
                                          device_qualities.p, device_offsets.p, n_reads, first_read_id, device_sums.p,
                                          stream, sums_ms));
        copy_out(sums, device_sums.p, n_segments);
        return 0;
    }, GW_MAPPER_ERROR);
}

gw_mapper_overlaps* gw_mapper_map_batched(const char* query_bases, const int64_t* query_offsets, int32_t n_queries,
                                          const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                                          int32_t kmer_size, int32_t window_size, double filtering_parameter,
                                          int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                          float min_overlap_fraction, int64_t max_basepairs_per_query_index,
                                          int64_t max_basepairs_per_target_index, int32_t post_process,
                                          int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, void* stream)
{
    return gw_mapper_map_batched_cached(query_bases, query_offsets, n_queries, target_bases, target_offsets, n_targets,
                                        kmer_size, window_size, filtering_parameter, min_residues, min_overlap_len,
                                        min_bases_per_residue, min_overlap_fraction, max_basepairs_per_query_index,
                                        max_basepairs_per_target_index, post_process, drop_fused_overlaps,
                                        rescue_overlap_ends, 0, 0, 1, 1, 1, 1, stream);
}

gw_mapper_overlaps* gw_mapper_map_batched_aligned(
    const char* query_bases, const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
    const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size, int32_t window_size, double filtering_parameter,
    int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
    int64_t max_basepairs_per_query_index, int64_t max_basepairs_per_target_index, int32_t post_process,
    int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, int32_t align_overlaps, int64_t max_device_bytes,
    void* stream)
{
    return gw_mapper_map_batched_cached(query_bases, query_offsets, n_queries, target_bases, target_offsets, n_targets,
                                        kmer_size, window_size, filtering_parameter, min_residues, min_overlap_len,
                                        min_bases_per_residue, min_overlap_fraction, max_basepairs_per_query_index,
                                        max_basepairs_per_target_index, post_process, drop_fused_overlaps,
                                        rescue_overlap_ends, align_overlaps, max_device_bytes, 1, 1, 1, 1, stream);
}

gw_mapper_overlaps* gw_mapper_map_batched_cached(
    const char* query_bases, const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
    const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size, int32_t window_size, double filtering_parameter,
    int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
    int64_t max_basepairs_per_query_index, int64_t max_basepairs_per_target_index, int32_t post_process,
    int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, int32_t align_overlaps, int64_t max_device_bytes,
    int32_t query_indices_in_host_memory, int32_t query_indices_in_device_memory, int32_t target_indices_in_host_memory,
    int32_t target_indices_in_device_memory, void* stream)
{
    return guarded([&] {
        const map_options options{kmer_size, window_size, filtering_parameter, min_residues, min_overlap_len,
                                  min_bases_per_residue, min_overlap_fraction, max_basepairs_per_query_index,
                                  max_basepairs_per_target_index, post_process, drop_fused_overlaps, rescue_overlap_ends,
                                  align_overlaps, max_device_bytes, query_indices_in_host_memory,
                                  query_indices_in_device_memory, target_indices_in_host_memory,
                                  target_indices_in_device_memory, 0, gwm_chaining{}};
        return map_batched({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, options,
                           static_cast<hipStream_t>(stream));
    }, static_cast<gw_mapper_overlaps*>(nullptr));
}

gw_mapper_overlaps* gw_mapper_map_batched_chained(
    const char* query_bases, const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
    const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size, int32_t window_size, double filtering_parameter,
    int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
    int64_t max_basepairs_per_query_index, int64_t max_basepairs_per_target_index, int32_t post_process,
    int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, int32_t align_overlaps, int64_t max_device_bytes,
    int32_t query_indices_in_host_memory, int32_t query_indices_in_device_memory, int32_t target_indices_in_host_memory,
    int32_t target_indices_in_device_memory, int32_t max_gap, int32_t bandwidth, int32_t min_chain_score,
    int32_t max_chains, void* stream)
{
    return guarded([&] {
        const map_options options{kmer_size, window_size, filtering_parameter, min_residues, min_overlap_len,
                                  min_bases_per_residue, min_overlap_fraction, max_basepairs_per_query_index,
                                  max_basepairs_per_target_index, post_process, drop_fused_overlaps, rescue_overlap_ends,
                                  align_overlaps, max_device_bytes, query_indices_in_host_memory,
                                  query_indices_in_device_memory, target_indices_in_host_memory,
                                  target_indices_in_device_memory, 1,
                                  gwm_chaining{kmer_size, max_gap, bandwidth, min_chain_score, max_chains}};
        return map_batched({query_bases, query_offsets, n_queries}, {target_bases, target_offsets, n_targets}, options,
                           static_cast<hipStream_t>(stream));
    }, static_cast<gw_mapper_overlaps*>(nullptr));
}

int gw_mapper_overlaps_cache_counts(const gw_mapper_overlaps* result, int64_t* index_builds, int64_t* index_restores,
                                    float* pack_unpack_ms)
{
    if (index_builds)
        *index_builds = result->index_builds;
    if (index_restores)
        *index_restores = result->index_restores;
    if (pack_unpack_ms)
        std::memcpy(pack_unpack_ms, result->cache_ms, sizeof(result->cache_ms));
    return 0;
}

int64_t gw_mapper_generate_batches_of_indices(const int64_t* query_read_lengths, int64_t n_queries,
                                              const int64_t* target_read_lengths, int64_t n_targets,
                                              int64_t query_basepairs_per_index, int64_t target_basepairs_per_index,
                                              int32_t query_indices_in_host_memory,
                                              int32_t query_indices_in_device_memory,
                                              int32_t target_indices_in_host_memory,
                                              int32_t target_indices_in_device_memory, uint32_t* out, int64_t capacity)
{
    return guarded([&] {
        const bool same = target_read_lengths == nullptr;
        if (n_queries < 0 || (!same && n_targets < 0))
            throw std::invalid_argument("gw_mapper_generate_batches_of_indices: negative number of reads");
        if (same && query_basepairs_per_index != target_basepairs_per_index)
            throw std::invalid_argument("generate_batches_of_indices: basepairs_per_index not the same");
        const std::vector<descriptor> qd = group_reads(query_read_lengths, n_queries, query_basepairs_per_index);
        const std::vector<descriptor> td =
            same ? qd : group_reads(target_read_lengths, n_targets, target_basepairs_per_index);
        const std::vector<batch_of_indices> batches =
            generate_batches(qd, td, query_indices_in_host_memory, query_indices_in_device_memory,
                             target_indices_in_host_memory, target_indices_in_device_memory, same);
        std::vector<uint32_t> flat;
        auto put = [&](const index_batch& b) {
            flat.push_back(static_cast<uint32_t>(b.query_indices.size()));
            flat.push_back(static_cast<uint32_t>(b.target_indices.size()));
            for (const std::vector<descriptor>* v : {&b.query_indices, &b.target_indices})
                for (const descriptor& d : *v)
                {
                    flat.push_back(d.first_read);
                    flat.push_back(d.number_of_reads);
                }
        };
        flat.push_back(static_cast<uint32_t>(batches.size()));
        for (const batch_of_indices& b : batches)
        {
            put(b.host_batch);
            flat.push_back(static_cast<uint32_t>(b.device_batches.size()));
            for (const index_batch& d : b.device_batches)
                put(d);
        }
        const int64_t words = static_cast<int64_t>(flat.size());
        if (out && words <= capacity)
            std::memcpy(out, flat.data(), sizeof(uint32_t) * flat.size());
        return words;
    }, int64_t(GW_MAPPER_ERROR));
}

gw_mapper_index_host_copy* gw_mapper_index_host_copy_create(const gw_mapper_index* index, void* stream, float* pack_ms)
{
    return guarded([&] {
        std::unique_ptr<gw_mapper_index_host_copy> h(
            new gw_mapper_index_host_copy(*index, static_cast<hipStream_t>(stream)));
        if (pack_ms)
            *pack_ms = h->c.pack_ms;
        return h.release();
    }, static_cast<gw_mapper_index_host_copy*>(nullptr));
}

int64_t gw_mapper_index_host_copy_bytes(const gw_mapper_index_host_copy* copy)
{
    return gwm_index_host_copy_bytes(&copy->c);
}

gw_mapper_index* gw_mapper_index_host_copy_to_device(const gw_mapper_index_host_copy* copy, void* stream,
                                                     float* restore_ms)
{
    return guarded([&] {
        hipStream_t s = static_cast<hipStream_t>(stream);
        std::unique_ptr<gw_mapper_index> h(new gw_mapper_index());
        Events span(2);
        span.record(0, s);
        throw_on(gwm_index_unpack(&copy->c, s, &h->x));
        span.record(1, s);
        const float ms = span.ms(0, 1); // waits: the index is ready when this returns
        if (restore_ms)
            *restore_ms = ms;
        return h.release();
    }, static_cast<gw_mapper_index*>(nullptr));
}

void gw_mapper_index_host_copy_destroy(gw_mapper_index_host_copy* copy) { delete copy; }

int64_t gw_mapper_overlaps_count(const gw_mapper_overlaps* result) { return static_cast<int64_t>(result->overlaps.size()); }

int gw_mapper_overlaps_copy(const gw_mapper_overlaps* result, void* overlaps, int64_t capacity, float* stage_ms,
                            int64_t* index_pairs)
{
    const int64_t n = std::min<int64_t>(capacity, static_cast<int64_t>(result->overlaps.size()));
    if (overlaps && n > 0)
        std::memcpy(overlaps, result->overlaps.data(), sizeof(gwm_overlap) * static_cast<size_t>(n));
    if (stage_ms)
        std::memcpy(stage_ms, result->stage_ms, sizeof(result->stage_ms));
    if (index_pairs)
        *index_pairs = result->index_pairs;
    return 0;
}

int64_t gw_mapper_overlaps_cigar_text_bytes(const gw_mapper_overlaps* result)
{
    return result->aligned ? static_cast<int64_t>(result->cigar_text.size()) : int64_t(GW_MAPPER_ERROR);
}

int gw_mapper_overlaps_copy_cigars(const gw_mapper_overlaps* result, char* text, int64_t* offsets,
                                   int32_t* edit_distances, float* stage_ms)
{
    if (!result->aligned)
    {
        g_capi_error = "gw_mapper_overlaps_copy_cigars: the overlaps were mapped without alignment";
        return GW_MAPPER_ERROR;
    }
    if (text && !result->cigar_text.empty())
        std::memcpy(text, result->cigar_text.data(), result->cigar_text.size());
    if (offsets)
        std::memcpy(offsets, result->cigar_offsets.data(), sizeof(int64_t) * result->cigar_offsets.size());
    if (edit_distances && !result->edit_distances.empty())
        std::memcpy(edit_distances, result->edit_distances.data(), sizeof(int32_t) * result->edit_distances.size());
    if (stage_ms)
        std::memcpy(stage_ms, result->align_ms, sizeof(result->align_ms));
    return 0;
}

void gw_mapper_overlaps_destroy(gw_mapper_overlaps* result) { delete result; }

} // extern "C"
