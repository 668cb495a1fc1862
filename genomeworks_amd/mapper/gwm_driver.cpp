// gwm_driver.cpp -- the batched driver in its parts: the plan (batches of indices), the stages of one index pair, the
// index cache with its second stream, and the walk over host and device batches that ties them together.
#include "gwm_driver.hpp"

#include "gwm_index_batcher.hpp"

#include <array>
#include <iterator>
#include <map>
#include <string>

namespace
{

using namespace gwm;

std::vector<batch_of_indices> batches_of(const read_sets& reads, const map_options& opt)
{
    const std::vector<int64_t> ql = read_lengths(reads.queries.offsets, reads.queries.n),
                               tl = read_lengths(reads.targets.offsets, reads.targets.n);
    const std::vector<descriptor> qd = group_reads(ql.data(), reads.queries.n, opt.max_basepairs_per_query_index);
    const std::vector<descriptor> td = group_reads(tl.data(), reads.targets.n, opt.max_basepairs_per_target_index);
    // The batches are the upper triangle only where query and target indices are the same list. All against all
    // with two index sizes keeps the whole matrix, and the pair walk drops the lower triangle as it always did.
    const bool same_indices =
        reads.all_to_all && opt.max_basepairs_per_query_index == opt.max_basepairs_per_target_index;
    return generate_batches(qd, td, opt.query_indices_in_host_memory, opt.query_indices_in_device_memory,
                            opt.target_indices_in_host_memory, opt.target_indices_in_device_memory, same_indices);
}

// The index numbers its reads by rank among the reads it kept: behind a read it skipped, read ids no longer name
// positions in the input, and the alignment would pair the wrong sequences without a sign.
void refuse_reads_the_index_skips(const read_sets& reads, const map_options& opt)
{
    const int64_t shortest = static_cast<int64_t>(opt.kmer_size) + opt.window_size - 1;
    for (const reads_view* set : {&reads.queries, &reads.targets})
        for (int32_t i = 0; i < set->n; ++i)
            if (set->offsets[i + 1] - set->offsets[i] < shortest)
                throw std::invalid_argument(
                    "gw_mapper_map_batched_aligned: " + std::string(set == &reads.queries ? "query" : "target") +
                    " read " + std::to_string(i) + " has " + std::to_string(set->offsets[i + 1] - set->offsets[i]) +
                    " bases, fewer than k + w - 1 = " + std::to_string(shortest) +
                    ": the index skips it and numbers the reads behind it by rank, "
                    "so overlap read ids would no longer name input reads and the alignment would pair the "
                    "wrong sequences; remove such reads to align");
}

// The stages of one index pair, as they always were: match and overlaps, then on what they leave post-processing, end
// rescue and alignment as the options ask, all on the mapping stream; what is left is appended to the result.
struct pair_stages
{
    const read_sets& reads_;
    const map_options& opt_;
    const hipStream_t s_;
    gw_mapper_overlaps& result_;

    void map(const gw_mapper_index& qi, const gw_mapper_index& ti)
    {
        dbuf<gwm_overlap> found, fused;
        int64_t count = find(qi, ti, found);
        ++result_.index_pairs;
        if (count == 0)
            return;
        gwm_overlap* current = found.p;
        if (opt_.post_process)
        {
            float ms = 0.f;
            fused.resize(count + count / 2);
            throw_on(gwm_post_process_overlaps(found.p, count, opt_.drop_fused_overlaps, s_, fused.p, &count, &ms));
            result_.stage_ms[1] += ms;
            current = fused.p;
        }
        if (opt_.rescue_overlap_ends && count > 0)
            rescue(current, count);
        if (opt_.align_overlaps && count > 0)
            align(current, count);
        const size_t at = result_.overlaps.size();
        result_.overlaps.resize(at + static_cast<size_t>(count));
        copy_out(result_.overlaps.data() + at, current, count);
    }

    int64_t find(const gw_mapper_index& qi, const gw_mapper_index& ti, dbuf<gwm_overlap>& found)
    {
        int64_t count = 0;
        float ms      = 0.f;
        gw_mapper_matcher m(qi, ti, s_);
        if (opt_.chained)
            throw_on(gwm_chain_overlaps_device(m.a.anchors, m.a.n, &opt_.chaining, reads_.all_to_all ? 1 : 0,
                                               opt_.min_residues, opt_.min_overlap_len, opt_.min_bases_per_residue,
                                               opt_.min_overlap_fraction, s_, &found.p, nullptr, &count, &ms));
        else
            throw_on(gwm_find_overlaps_device(m.a.anchors, m.a.n, reads_.all_to_all ? 1 : 0, opt_.min_residues,
                                              opt_.min_overlap_len, opt_.min_bases_per_residue,
                                              opt_.min_overlap_fraction, s_, &found.p, &count, &ms));
        result_.stage_ms[0] += ms;
        return count;
    }

    void rescue(gwm_overlap* overlaps, int64_t count)
    {
        const reads_view &q = reads_.device_queries, &t = reads_.device_targets;
        float ms = 0.f;
        throw_on(gwm_rescue_overlap_ends(overlaps, count, q.bases, q.offsets, q.n, 0, t.bases, t.offsets, t.n,
                                         0, 50, 0.5f, s_, &ms));
        result_.stage_ms[2] += ms;
    }

    // what is left of this index pair, where it lies: one aligner capacity per pair
    void align(const gwm_overlap* overlaps, int64_t count)
    {
        const reads_view &q = reads_.device_queries, &t = reads_.device_targets;
        gw_mapper_cigars cigars;
        throw_on(gwm_align_overlaps(overlaps, count, q.bases, q.offsets, q.n, 0, t.bases, t.offsets, t.n, 0,
                                    opt_.max_device_bytes, s_, &cigars.c));
        const size_t text_at = result_.cigar_text.size(), n_at = result_.edit_distances.size();
        result_.cigar_text.resize(text_at + static_cast<size_t>(cigars.c.text_bytes));
        copy_out(&result_.cigar_text[0] + text_at, cigars.c.text, cigars.c.text_bytes);
        result_.cigar_offsets.resize(n_at + static_cast<size_t>(count) + 1);
        copy_out(result_.cigar_offsets.data() + n_at, cigars.c.cigar_offsets, count + 1);
        for (size_t i = n_at; i < result_.cigar_offsets.size(); ++i)
            result_.cigar_offsets[i] += static_cast<int64_t>(text_at);
        result_.edit_distances.resize(n_at + static_cast<size_t>(count));
        copy_out(result_.edit_distances.data() + n_at, cigars.c.edit_distances, count);
        for (int k = 0; k < 3; ++k)
            result_.align_ms[k] += cigars.c.stage_ms[k];
    }
};

// The driver's second stream, on which packed indices are restored while the first one maps. settle() puts an event
// behind what was queued and makes the mapping stream wait for it; the host does not wait. The spans around the
// restores are kept, and restore_ms() reads them once, at the end of the run.
struct copy_stream
{
    hipStream_t stream = nullptr;
    hipEvent_t ready   = nullptr;
    std::vector<std::unique_ptr<Events>> spans;
    size_t settled = 0;
    copy_stream()
    {
        check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreateWithFlags");
        if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess)
        {
            (void)hipStreamDestroy(stream);
            throw std::runtime_error("hipEventCreateWithFlags failed");
        }
    }
    copy_stream(const copy_stream&) = delete;
    copy_stream& operator=(const copy_stream&) = delete;
    ~copy_stream()
    {
        (void)hipStreamSynchronize(stream);
        spans.clear();
        (void)hipEventDestroy(ready);
        (void)hipStreamDestroy(stream);
    }
    void settle(hipStream_t mapping_stream)
    {
        if (spans.size() == settled)
            return;
        check(hipEventRecord(ready, stream), "hipEventRecord");
        check(hipStreamWaitEvent(mapping_stream, ready, 0), "hipStreamWaitEvent");
        settled = spans.size();
    }
    float restore_ms()
    {
        float total = 0.f;
        for (const std::unique_ptr<Events>& span : spans)
            total += span->ms(0, 1);
        return total;
    }
};

// The index cache: the indices alive on the device, the packed host copies, the second stream that restores them, and
// the counts and times of building, packing and restoring. An index is named by its descriptor and, unless the two
// read sets are one, by its kind (0 query, 1 target). The walk calls, per host batch,
//     begin_host_batch, then per device batch [prefetch] index()... [advance], then end_host_batch.
// The ordering rules that keep this correct are the contracts of these methods, stated at each.
class index_cache
{
public:
    index_cache(const read_sets& reads, const map_options& options, hipStream_t mapping_stream)
        : reads_(reads), opt_(options), s_(mapping_stream)
    {
    }
    // Also when an exception unwinds, the second stream is drained before any host copy goes: no copy may outlive
    // the slab it reads.
    ~index_cache() { (void)hipStreamSynchronize(restores_.stream); }

    // Makes the indices of the host batch's first device batch current, and gives those a later device batch asks for
    // a packed host copy. Before an index is built it is looked for among the indices still on the device and among
    // the host copies of the previous host batch.
    // Contract: what the previous device batch left and this host batch does not ask for is freed before anything is
    // built, so one index per batch never holds more than the two indices of a pair. On return the mapping stream
    // waits for every restore queued here (settle()), so it may use the current indices. The previous host batch's
    // copies, which such a restore may still read, are kept until end_host_batch().
    void begin_host_batch(const batch_of_indices& batch)
    {
        std::vector<index_key> first, later;
        for (size_t b = 0; b < batch.device_batches.size(); ++b)
            for (const index_key& k : keys_of(batch.device_batches[b]))
                (b == 0 ? first : later).push_back(k);
        std::map<index_key, copy_ptr> copies;
        const std::vector<index_key> asked_for = keys_of(batch.host_batch);
        for (auto it = on_device_.begin(); it != on_device_.end();)
            it = in(asked_for, it->first) ? std::next(it) : on_device_.erase(it);
        for (const index_key& k : asked_for)
        {
            const auto alive = on_device_.find(k);
            const auto kept  = on_host_.find(k);
            index_ptr index  = alive != on_device_.end() ? alive->second : nullptr;
            copy_ptr copy    = kept != on_host_.end() ? kept->second : nullptr;
            on_device_.erase(k); // from here on it lives as long as this batch needs it
            if (!index)
            {
                if (!copy)
                    index = build(k);
                else if (in(first, k))
                    index = restore(copy);
            }
            if (in(later, k))
                copies[k] = copy ? copy : pack(*index); // on the mapping stream, behind the build
            if (in(first, k))
                current_[k] = index;
        }
        restores_.settle(s_);
        on_device_.clear();
        on_host_.swap(copies);
        previous_copies_.swap(copies);
    }

    // Queues, on the second stream, the restores of those indices of the next device batch that are not current.
    // Contract: nothing here makes the mapping stream or the host wait; advance() does, before the indices are used.
    void prefetch(const index_batch& next_device_batch)
    {
        for (const index_key& k : keys_of(next_device_batch))
        {
            const auto here = current_.find(k);
            next_[k]        = here != current_.end() ? here->second : restore(on_host_.at(k));
        }
    }

    // Makes the prefetched indices current and lets go of those only the finished device batch held.
    // Contract: settle() comes first, so the mapping stream uses a restored index only behind its restore.
    void advance()
    {
        restores_.settle(s_);
        current_.swap(next_);
        next_.clear();
    }

    // A current index: of the device batch begin_host_batch() or the last advance() made current.
    const gw_mapper_index& index(uint32_t kind, const descriptor& d) const { return *current_.at(key_of(kind, d)); }

    // Leaves the current indices on the device for the next host batch to find.
    // Contract: the previous host batch's copies are let go only behind a wait on the second stream. (It is idle by
    // now; the wait makes letting them go safe by itself.)
    void end_host_batch()
    {
        on_device_.swap(current_);
        if (!previous_copies_.empty())
            check(hipStreamSynchronize(restores_.stream), "hipStreamSynchronize");
        previous_copies_.clear();
    }

    // The counts and device times of the run into the result; waits for the restores' events.
    void report(gw_mapper_overlaps& result)
    {
        result.index_builds   = builds_;
        result.index_restores = restores_count_;
        result.cache_ms[0]    = pack_ms_;
        result.cache_ms[1]    = restores_.restore_ms();
    }

private:
    using index_key = std::array<uint32_t, 3>;
    using index_ptr = std::shared_ptr<gw_mapper_index>;
    using copy_ptr  = std::shared_ptr<gw_mapper_index_host_copy>;

    index_key key_of(uint32_t kind, const descriptor& d) const
    {
        return index_key{reads_.all_to_all ? 0u : kind, d.first_read, d.number_of_reads};
    }
    static bool in(const std::vector<index_key>& keys, const index_key& k)
    {
        return std::find(keys.begin(), keys.end(), k) != keys.end();
    }
    // the indices of a batch that hold reads, each once, queries first
    std::vector<index_key> keys_of(const index_batch& b) const
    {
        std::vector<index_key> keys;
        for (uint32_t kind = 0; kind < 2; ++kind)
            for (const descriptor& d : kind == 0 ? b.query_indices : b.target_indices)
                if (d.number_of_reads > 0 && !in(keys, key_of(kind, d)))
                    keys.push_back(key_of(kind, d));
        return keys;
    }
    // from the bases: the key holds the descriptor, reads k[1] .. k[1] + k[2] of its set
    index_ptr build(const index_key& k)
    {
        const reads_view& set = k[0] == 1 ? reads_.targets : reads_.queries;
        ++builds_;
        return std::make_shared<gw_mapper_index>(set.bases, set.offsets + k[1], static_cast<int32_t>(k[2]), k[1],
                                                 opt_.kmer_size, opt_.window_size, 1, opt_.filtering_parameter, s_);
    }
    index_ptr restore(const copy_ptr& copy)
    {
        index_ptr index = std::make_shared<gw_mapper_index>();
        restores_.spans.emplace_back(new Events(2));
        Events& span = *restores_.spans.back();
        span.record(0, restores_.stream);
        throw_on(gwm_index_unpack(&copy->c, restores_.stream, &index->x));
        span.record(1, restores_.stream);
        ++restores_count_;
        return index;
    }
    copy_ptr pack(const gw_mapper_index& index)
    {
        copy_ptr copy = std::make_shared<gw_mapper_index_host_copy>(index, s_);
        pack_ms_ += copy->c.pack_ms;
        return copy;
    }

    const read_sets& reads_;
    const map_options& opt_;
    const hipStream_t s_;
    copy_stream restores_; // indices of the next device batch come back on it while this one is mapped
    std::map<index_key, index_ptr> on_device_, current_, next_; // left by the previous device batch; being mapped; next
    std::map<index_key, copy_ptr> on_host_, previous_copies_;   // of this host batch; of the one before
    int64_t builds_ = 0, restores_count_ = 0;
    float pack_ms_ = 0.f;
};

} // namespace

namespace gwm
{

gw_mapper_overlaps* map_batched(const reads_view& queries, const reads_view& targets, const map_options& opt,
                                hipStream_t stream)
{
    read_sets reads(queries, targets);
    if (reads.queries.n < 0 || reads.targets.n < 0)
        throw std::invalid_argument("gw_mapper_map_batched: negative number of reads");
    const std::vector<batch_of_indices> batches = batches_of(reads, opt);
    if (opt.align_overlaps)
        refuse_reads_the_index_skips(reads, opt);
    if (opt.rescue_overlap_ends || opt.align_overlaps)
        reads.upload();
    std::unique_ptr<gw_mapper_overlaps> result(new gw_mapper_overlaps());
    result->aligned = opt.align_overlaps != 0;
    pair_stages stages{reads, opt, stream, *result};
    index_cache cache(reads, opt, stream);

    for (const batch_of_indices& batch : batches)
    {
        cache.begin_host_batch(batch);
        // while one device batch is mapped, the next one's indices are restored on the second stream
        for (size_t b = 0; b < batch.device_batches.size(); ++b)
        {
            const bool more = b + 1 < batch.device_batches.size();
            if (more)
                cache.prefetch(batch.device_batches[b + 1]);
            for (const descriptor& qx : batch.device_batches[b].query_indices)
                for (const descriptor& tx : batch.device_batches[b].target_indices)
                    if (qx.number_of_reads != 0 && tx.number_of_reads != 0 &&
                        !(reads.all_to_all && tx.first_read < qx.first_read))
                        stages.map(cache.index(0, qx), cache.index(1, tx));
            if (more)
                cache.advance();
        }
        cache.end_host_batch();
    }
    cache.report(*result);
    return result.release();
}

} // namespace gwm
