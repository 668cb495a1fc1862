// mapper.cpp -- host side of cudamapper (libcudamapper.so): owning Index and Matcher objects over the stage functions
// of include/gwhip_mapper.h, and the flat C API of include/gw_mapper_capi.h.
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace
{

thread_local std::string g_capi_error;

void throw_on(int rc)
{
    if (rc != 0)
        throw std::runtime_error(gwm_last_error());
}

void hip_check(hipError_t e, const char* what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

template <typename T>
void copy_out(T* dst, const T* src, int64_t n)
{
    if (dst && n > 0)
        hip_check(hipMemcpy(dst, src, sizeof(T) * static_cast<size_t>(n), hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

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

// Owning device copy of a host array.
template <typename T>
struct device_array
{
    T* p = nullptr;
    device_array() = default;
    device_array(const T* host, int64_t n) { upload(host, n); }
    device_array(const device_array&) = delete;
    device_array& operator=(const device_array&) = delete;
    ~device_array() { reset(); }
    void reset()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
    }
    void allocate(int64_t n)
    {
        reset();
        if (n > 0)
            hip_check(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * static_cast<size_t>(n)), "hipMalloc");
    }
    void upload(const T* host, int64_t n)
    {
        allocate(n);
        if (n > 0)
            hip_check(hipMemcpy(p, host, sizeof(T) * static_cast<size_t>(n), hipMemcpyHostToDevice), "hipMemcpy H2D");
    }
};

// A read set on the device, in the layout gwm_rescue_overlap_ends takes.
struct device_reads
{
    device_array<char> bases;
    device_array<int64_t> offsets;
    int32_t n = 0;
    device_reads(const char* host_bases, const int64_t* host_offsets, int32_t n_reads)
        : n(n_reads)
    {
        if (n_reads < 0)
            throw std::invalid_argument("negative number of reads");
        bases.upload(host_bases, std::max<int64_t>(host_offsets[n_reads], 1));
        offsets.upload(host_offsets, n_reads + 1);
    }
};

struct descriptor
{
    uint32_t first_read;
    uint32_t number_of_reads;
};

// group_reads_into_indices of the reference, its loop as it stands (see gw_mapper_capi.h)
std::vector<descriptor> group_reads(const int64_t* lengths, int64_t n, int64_t max_basepairs)
{
    std::vector<descriptor> out;
    uint32_t first = 0, count = 0;
    int64_t bases = 0;
    for (int64_t i = 0; i < n; ++i)
    {
        if (lengths[i] + bases > max_basepairs)
        {
            out.push_back({first, count});
            first = static_cast<uint32_t>(i);
            count = 1;
            bases = lengths[i];
        }
        else
        {
            bases += lengths[i];
            ++count;
        }
    }
    out.push_back({first, count});
    return out;
}

struct device_overlaps
{
    gwm_overlap* p = nullptr;
    device_overlaps() = default;
    device_overlaps(const device_overlaps&) = delete;
    device_overlaps& operator=(const device_overlaps&) = delete;
    ~device_overlaps() { gwm_device_free(p); }
};

} // namespace

struct gw_mapper_index
{
    gwm_index x{};
    gw_mapper_index(const char* bases, const int64_t* offsets, int32_t n_reads, uint32_t first_read_id, int32_t k,
                    int32_t w, int32_t hash, double filtering_parameter, hipStream_t stream)
    {
        throw_on(gwm_index_build(bases, offsets, n_reads, first_read_id, k, w, hash, filtering_parameter, stream, &x));
    }
    gw_mapper_index() = default;
    ~gw_mapper_index() { gwm_index_free(&x); }
    gw_mapper_index(const gw_mapper_index&) = delete;
    gw_mapper_index& operator=(const gw_mapper_index&) = delete;
};

struct gw_mapper_matcher
{
    gwm_anchors a{};
    gw_mapper_matcher(const gw_mapper_index& q, const gw_mapper_index& t, hipStream_t stream)
    {
        throw_on(gwm_match(&q.x, &t.x, stream, &a));
    }
    ~gw_mapper_matcher() { gwm_anchors_free(&a); }
    gw_mapper_matcher(const gw_mapper_matcher&) = delete;
    gw_mapper_matcher& operator=(const gw_mapper_matcher&) = delete;
};

struct gw_mapper_overlaps
{
    std::vector<gwm_overlap> overlaps;
    float stage_ms[3]   = {0.f, 0.f, 0.f};
    int64_t index_pairs = 0;
    // with alignment: the CIGAR of overlap i is cigar_text[cigar_offsets[i] .. cigar_offsets[i + 1])
    bool aligned = false;
    std::string cigar_text;
    std::vector<int64_t> cigar_offsets{0};
    std::vector<int32_t> edit_distances;
    float align_ms[3] = {0.f, 0.f, 0.f};
};

// CIGARs of one gwm_align_overlaps call, on the device until they are copied out
struct gw_mapper_cigars
{
    gwm_cigars c{};
    gw_mapper_cigars() = default;
    ~gw_mapper_cigars() { gwm_cigars_free(&c); }
    gw_mapper_cigars(const gw_mapper_cigars&) = delete;
    gw_mapper_cigars& operator=(const gw_mapper_cigars&) = delete;
};

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
        gwm_anchor* d = nullptr;
        hip_check(hipMalloc(reinterpret_cast<void**>(&d), sizeof(gwm_anchor) * static_cast<size_t>(n)), "hipMalloc");
        std::unique_ptr<gwm_anchor, hipError_t (*)(void*)> hold(d, hipFree);
        hip_check(hipMemcpy(d, anchors, sizeof(gwm_anchor) * static_cast<size_t>(n), hipMemcpyHostToDevice),
                  "hipMemcpy H2D");
        throw_on(gwm_find_overlaps(d, n, all_to_all, min_residues, min_overlap_len, min_bases_per_residue,
                                   min_overlap_fraction, stream, static_cast<gwm_overlap*>(overlaps), &count, nullptr));
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
        device_array<gwm_overlap> in(static_cast<const gwm_overlap*>(overlaps), n), result;
        result.allocate(n + n / 2);
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
        if (n <= 0)
        {
            // the argument checks still apply
            throw_on(gwm_rescue_overlap_ends(nullptr, 0, nullptr, nullptr, n_queries, 0, nullptr, nullptr,
                                             target_bases ? n_targets : n_queries, 0, extension, required_similarity,
                                             stream, nullptr));
            return 0;
        }
        device_reads q(query_bases, query_offsets, n_queries);
        std::unique_ptr<device_reads> t;
        if (target_bases)
            t.reset(new device_reads(target_bases, target_offsets, n_targets));
        const device_reads& tr = t ? *t : q;
        device_array<gwm_overlap> d(static_cast<const gwm_overlap*>(overlaps), n);
        throw_on(gwm_rescue_overlap_ends(d.p, n, q.bases.p, q.offsets.p, q.n, first_query_read_id, tr.bases.p,
                                         tr.offsets.p, tr.n, first_target_read_id, extension, required_similarity,
                                         stream, rescue_ms));
        copy_out(static_cast<gwm_overlap*>(overlaps), d.p, n);
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
    return guarded([&] {
        std::unique_ptr<gw_mapper_cigars> h(new gw_mapper_cigars());
        if (n <= 0)
        {
            // the argument checks still apply
            throw_on(gwm_align_overlaps(nullptr, 0, nullptr, nullptr, n_queries, 0, nullptr, nullptr,
                                        target_bases ? n_targets : n_queries, 0, max_device_bytes, stream, &h->c));
            return h.release();
        }
        device_reads q(query_bases, query_offsets, n_queries);
        std::unique_ptr<device_reads> t;
        if (target_bases)
            t.reset(new device_reads(target_bases, target_offsets, n_targets));
        const device_reads& tr = t ? *t : q;
        device_array<gwm_overlap> d(static_cast<const gwm_overlap*>(overlaps), n);
        throw_on(gwm_align_overlaps(d.p, n, q.bases.p, q.offsets.p, q.n, first_query_read_id, tr.bases.p, tr.offsets.p,
                                    tr.n, first_target_read_id, max_device_bytes, stream, &h->c));
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

gw_mapper_overlaps* gw_mapper_map_batched(const char* query_bases, const int64_t* query_offsets, int32_t n_queries,
                                          const char* target_bases, const int64_t* target_offsets, int32_t n_targets,
                                          int32_t kmer_size, int32_t window_size, double filtering_parameter,
                                          int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue,
                                          float min_overlap_fraction, int64_t max_basepairs_per_query_index,
                                          int64_t max_basepairs_per_target_index, int32_t post_process,
                                          int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, void* stream)
{
    return gw_mapper_map_batched_aligned(query_bases, query_offsets, n_queries, target_bases, target_offsets, n_targets,
                                         kmer_size, window_size, filtering_parameter, min_residues, min_overlap_len,
                                         min_bases_per_residue, min_overlap_fraction, max_basepairs_per_query_index,
                                         max_basepairs_per_target_index, post_process, drop_fused_overlaps,
                                         rescue_overlap_ends, 0, 0, stream);
}

gw_mapper_overlaps* gw_mapper_map_batched_aligned(
    const char* query_bases, const int64_t* query_offsets, int32_t n_queries, const char* target_bases,
    const int64_t* target_offsets, int32_t n_targets, int32_t kmer_size, int32_t window_size, double filtering_parameter,
    int64_t min_residues, int64_t min_overlap_len, int64_t min_bases_per_residue, float min_overlap_fraction,
    int64_t max_basepairs_per_query_index, int64_t max_basepairs_per_target_index, int32_t post_process,
    int32_t drop_fused_overlaps, int32_t rescue_overlap_ends, int32_t align_overlaps, int64_t max_device_bytes,
    void* stream)
{
    return guarded([&] {
        hipStream_t s         = static_cast<hipStream_t>(stream);
        const bool all_to_all = target_bases == nullptr;
        if (all_to_all)
        {
            target_bases   = query_bases;
            target_offsets = query_offsets;
            n_targets      = n_queries;
        }
        if (n_queries < 0 || n_targets < 0)
            throw std::invalid_argument("gw_mapper_map_batched: negative number of reads");
        auto lengths = [](const int64_t* offsets, int32_t n) {
            std::vector<int64_t> v(static_cast<size_t>(n));
            for (int32_t i = 0; i < n; ++i)
                v[i] = offsets[i + 1] - offsets[i];
            return v;
        };
        const std::vector<int64_t> ql = lengths(query_offsets, n_queries), tl = lengths(target_offsets, n_targets);
        const std::vector<descriptor> qd = group_reads(ql.data(), n_queries, max_basepairs_per_query_index);
        const std::vector<descriptor> td = group_reads(tl.data(), n_targets, max_basepairs_per_target_index);
        if (align_overlaps)
        {
            // The index numbers its reads by rank among the reads it kept: behind a read it skipped, read ids no
            // longer name positions in the input, and the alignment would pair the wrong sequences without a sign.
            const int64_t shortest = static_cast<int64_t>(kmer_size) + window_size - 1;
            for (const std::vector<int64_t>* set : {&ql, &tl})
                for (size_t i = 0; i < set->size(); ++i)
                    if ((*set)[i] < shortest)
                        throw std::invalid_argument(
                            "gw_mapper_map_batched_aligned: " + std::string(set == &ql ? "query" : "target") + " read " +
                            std::to_string(i) + " has " + std::to_string((*set)[i]) + " bases, fewer than k + w - 1 = " +
                            std::to_string(shortest) + ": the index skips it and numbers the reads behind it by rank, "
                            "so overlap read ids would no longer name input reads and the alignment would pair the "
                            "wrong sequences; remove such reads to align");
        }
        std::unique_ptr<device_reads> q_reads, t_reads;
        if (rescue_overlap_ends || align_overlaps)
        {
            q_reads.reset(new device_reads(query_bases, query_offsets, n_queries));
            if (!all_to_all)
                t_reads.reset(new device_reads(target_bases, target_offsets, n_targets));
        }
        std::unique_ptr<gw_mapper_overlaps> result(new gw_mapper_overlaps());
        result->aligned = align_overlaps != 0;
        for (const descriptor& qx : qd)
        {
            if (qx.number_of_reads == 0)
                continue;
            // one query index serves the whole row of target indices
            gw_mapper_index qi(query_bases, query_offsets + qx.first_read, static_cast<int32_t>(qx.number_of_reads),
                               qx.first_read, kmer_size, window_size, 1, filtering_parameter, s);
            for (const descriptor& tx : td)
            {
                if (tx.number_of_reads == 0 || (all_to_all && tx.first_read < qx.first_read))
                    continue;
                const bool same = all_to_all && tx.first_read == qx.first_read && tx.number_of_reads == qx.number_of_reads;
                std::unique_ptr<gw_mapper_index> ti;
                if (!same)
                    ti.reset(new gw_mapper_index(target_bases, target_offsets + tx.first_read,
                                                 static_cast<int32_t>(tx.number_of_reads), tx.first_read, kmer_size,
                                                 window_size, 1, filtering_parameter, s));
                int64_t count = 0;
                float ms      = 0.f;
                device_overlaps found;
                {
                    gw_mapper_matcher m(qi, same ? qi : *ti, s);
                    throw_on(gwm_find_overlaps_device(m.a.anchors, m.a.n, all_to_all ? 1 : 0, min_residues,
                                                      min_overlap_len, min_bases_per_residue, min_overlap_fraction, s,
                                                      &found.p, &count, &ms));
                    result->stage_ms[0] += ms;
                }
                ++result->index_pairs;
                if (count == 0)
                    continue;
                device_array<gwm_overlap> fused;
                gwm_overlap* current = found.p;
                if (post_process)
                {
                    fused.allocate(count + count / 2);
                    throw_on(gwm_post_process_overlaps(found.p, count, drop_fused_overlaps, s, fused.p, &count, &ms));
                    result->stage_ms[1] += ms;
                    current = fused.p;
                }
                if (rescue_overlap_ends && count > 0)
                {
                    const device_reads& tr = t_reads ? *t_reads : *q_reads;
                    throw_on(gwm_rescue_overlap_ends(current, count, q_reads->bases.p, q_reads->offsets.p, q_reads->n,
                                                     0, tr.bases.p, tr.offsets.p, tr.n, 0, 50, 0.5f, s, &ms));
                    result->stage_ms[2] += ms;
                }
                if (align_overlaps && count > 0)
                {
                    // what is left of this index pair, where it lies: one aligner capacity per pair
                    const device_reads& tr = t_reads ? *t_reads : *q_reads;
                    gw_mapper_cigars cigars;
                    throw_on(gwm_align_overlaps(current, count, q_reads->bases.p, q_reads->offsets.p, q_reads->n, 0,
                                                tr.bases.p, tr.offsets.p, tr.n, 0, max_device_bytes, s, &cigars.c));
                    const size_t text_at = result->cigar_text.size(), n_at = result->edit_distances.size();
                    result->cigar_text.resize(text_at + static_cast<size_t>(cigars.c.text_bytes));
                    copy_out(&result->cigar_text[0] + text_at, cigars.c.text, cigars.c.text_bytes);
                    result->cigar_offsets.resize(n_at + static_cast<size_t>(count) + 1);
                    copy_out(result->cigar_offsets.data() + n_at, cigars.c.cigar_offsets, count + 1);
                    for (size_t i = n_at; i < result->cigar_offsets.size(); ++i)
                        result->cigar_offsets[i] += static_cast<int64_t>(text_at);
                    result->edit_distances.resize(n_at + static_cast<size_t>(count));
                    copy_out(result->edit_distances.data() + n_at, cigars.c.edit_distances, count);
                    for (int k = 0; k < 3; ++k)
                        result->align_ms[k] += cigars.c.stage_ms[k];
                }
                const size_t at = result->overlaps.size();
                result->overlaps.resize(at + static_cast<size_t>(count));
                copy_out(result->overlaps.data() + at, current, count);
            }
        }
        return result.release();
    }, static_cast<gw_mapper_overlaps*>(nullptr));
}

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
