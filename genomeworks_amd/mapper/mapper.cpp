// mapper.cpp -- host side of cudamapper (libcudamapper.so): owning Index and Matcher objects over the stage functions
// of include/gwhip_mapper.h, and the flat C API of include/gw_mapper_capi.h.
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <iterator>
#include <map>
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

bool operator==(const descriptor& a, const descriptor& b)
{
    return a.first_read == b.first_read && a.number_of_reads == b.number_of_reads;
}

// IndexBatch / BatchOfIndices of the reference's index batcher
struct index_batch
{
    std::vector<descriptor> query_indices, target_indices;
};

struct batch_of_indices
{
    index_batch host_batch;
    std::vector<index_batch> device_batches;
};

// group_into_batches of the reference: blocks of per_query x per_target indices, query blocks outside; with the same
// query and target only the upper triangle, the targets starting at the query block's own position
std::vector<index_batch> group_into_batches(const std::vector<descriptor>& queries, const std::vector<descriptor>& targets,
                                            int64_t per_query, int64_t per_target, bool same_query_and_target)
{
    if (same_query_and_target && per_query != per_target)
        throw std::invalid_argument("group_into_batches: same query and target, but indices per batch not the same");
    std::vector<index_batch> batches;
    const int64_t nq = static_cast<int64_t>(queries.size()), nt = static_cast<int64_t>(targets.size());
    for (int64_t q = 0; q < nq; q += per_query)
        for (int64_t t = same_query_and_target ? q : 0; t < nt; t += per_target)
            batches.push_back({std::vector<descriptor>(queries.begin() + q, queries.begin() + std::min(q + per_query, nq)),
                               std::vector<descriptor>(targets.begin() + t, targets.begin() + std::min(t + per_target, nt))});
    return batches;
}

// generate_batches_of_indices of the reference over descriptors that are already grouped, with the counts checked as
// its application parameters check them
std::vector<batch_of_indices> generate_batches(const std::vector<descriptor>& queries,
                                               const std::vector<descriptor>& targets, int64_t query_host,
                                               int64_t query_device, int64_t target_host, int64_t target_device,
                                               bool same_query_and_target)
{
    if (query_host < 1 || query_device < 1 || target_host < 1 || target_device < 1)
        throw std::invalid_argument("generate_batches_of_indices: every number of indices has to be at least 1");
    if (query_host < query_device)
        throw std::invalid_argument("generate_batches_of_indices: query indices in host memory has to be larger or "
                                    "equal than query indices in device memory");
    if (target_host < target_device)
        throw std::invalid_argument("generate_batches_of_indices: target indices in host memory has to be larger or "
                                    "equal than target indices in device memory");
    if (same_query_and_target)
    {
        if (query_host != target_host)
            throw std::invalid_argument("generate_batches_of_indices: indices_per_host_batch not the same");
        if (query_device != target_device)
            throw std::invalid_argument("generate_batches_of_indices: indices_per_device_batch not the same");
    }
    std::vector<batch_of_indices> all;
    for (index_batch& host : group_into_batches(queries, targets, query_host, target_host, same_query_and_target))
    {
        // device batches are symmetric only where the host batch's query and target indices are the same
        const bool same_in_batch = same_query_and_target && host.query_indices == host.target_indices;
        std::vector<index_batch> device =
            group_into_batches(host.query_indices, host.target_indices, query_device, target_device, same_in_batch);
        all.push_back({std::move(host), std::move(device)});
    }
    return all;
}

std::vector<int64_t> read_lengths(const int64_t* offsets, int32_t n)
{
    std::vector<int64_t> v(static_cast<size_t>(n));
    for (int32_t i = 0; i < n; ++i)
        v[i] = offsets[i + 1] - offsets[i];
    return v;
}

// Two HIP events around a piece of work on one stream.
struct event_span
{
    hipEvent_t a = nullptr, b = nullptr;
    event_span()
    {
        hip_check(hipEventCreate(&a), "hipEventCreate");
        hip_check(hipEventCreate(&b), "hipEventCreate");
    }
    event_span(const event_span&) = delete;
    event_span& operator=(const event_span&) = delete;
    ~event_span()
    {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
    }
    float ms()
    {
        float v = 0.f;
        hip_check(hipEventSynchronize(b), "hipEventSynchronize");
        hip_check(hipEventElapsedTime(&v, a, b), "hipEventElapsedTime");
        return v;
    }
};

// The driver's second stream, on which packed indices are restored while the first one maps. settle() puts an event
// behind what was queued and makes the mapping stream wait for it; the host does not wait. The spans around the
// restores are kept, and restore_ms() reads them once, at the end of the run.
struct copy_stream
{
    hipStream_t stream = nullptr;
    hipEvent_t ready   = nullptr;
    std::vector<std::unique_ptr<event_span>> spans;
    size_t settled = 0;
    copy_stream()
    {
        hip_check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreateWithFlags");
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
    void begin_span()
    {
        spans.emplace_back(new event_span());
        hip_check(hipEventRecord(spans.back()->a, stream), "hipEventRecord");
    }
    void end_span() { hip_check(hipEventRecord(spans.back()->b, stream), "hipEventRecord"); }
    void settle(hipStream_t mapping_stream)
    {
        if (spans.size() == settled)
            return;
        hip_check(hipEventRecord(ready, stream), "hipEventRecord");
        hip_check(hipStreamWaitEvent(mapping_stream, ready, 0), "hipStreamWaitEvent");
        settled = spans.size();
    }
    float restore_ms()
    {
        float total = 0.f;
        for (const std::unique_ptr<event_span>& span : spans)
            total += span->ms();
        return total;
    }
};

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

struct gw_mapper_index_host_copy
{
    gwm_index_host_copy c{};
    gw_mapper_index_host_copy(const gw_mapper_index& index, hipStream_t stream)
    {
        throw_on(gwm_index_pack(&index.x, stream, &c));
    }
    ~gw_mapper_index_host_copy() { gwm_index_host_copy_free(&c); }
    gw_mapper_index_host_copy(const gw_mapper_index_host_copy&) = delete;
    gw_mapper_index_host_copy& operator=(const gw_mapper_index_host_copy&) = delete;
};

struct gw_mapper_overlaps
{
    std::vector<gwm_overlap> overlaps;
    float stage_ms[3]   = {0.f, 0.f, 0.f};
    int64_t index_pairs = 0;
    // the index cache: indices built from bases, indices restored from a packed host copy, device time of both ways
    int64_t index_builds = 0, index_restores = 0;
    float cache_ms[2]    = {0.f, 0.f}; // pack, unpack
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
        const std::vector<int64_t> ql = read_lengths(query_offsets, n_queries), tl = read_lengths(target_offsets, n_targets);
        const std::vector<descriptor> qd = group_reads(ql.data(), n_queries, max_basepairs_per_query_index);
        const std::vector<descriptor> td = group_reads(tl.data(), n_targets, max_basepairs_per_target_index);
        // The batches are the upper triangle only where query and target indices are the same list. All against all
        // with two index sizes keeps the whole matrix, and the pair walk below drops the lower triangle as it always did.
        const bool same_indices = all_to_all && max_basepairs_per_query_index == max_basepairs_per_target_index;
        const std::vector<batch_of_indices> batches =
            generate_batches(qd, td, query_indices_in_host_memory, query_indices_in_device_memory,
                             target_indices_in_host_memory, target_indices_in_device_memory, same_indices);
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

        // ---- the stages of one index pair, as they always were
        auto map_pair = [&](const gw_mapper_index& qi, const gw_mapper_index& ti) {
            int64_t count = 0;
            float ms      = 0.f;
            device_overlaps found;
            {
                gw_mapper_matcher m(qi, ti, s);
                throw_on(gwm_find_overlaps_device(m.a.anchors, m.a.n, all_to_all ? 1 : 0, min_residues, min_overlap_len,
                                                  min_bases_per_residue, min_overlap_fraction, s, &found.p, &count,
                                                  &ms));
                result->stage_ms[0] += ms;
            }
            ++result->index_pairs;
            if (count == 0)
                return;
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
                throw_on(gwm_rescue_overlap_ends(current, count, q_reads->bases.p, q_reads->offsets.p, q_reads->n, 0,
                                                 tr.bases.p, tr.offsets.p, tr.n, 0, 50, 0.5f, s, &ms));
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
        };

        // ---- the index cache. An index is named by its descriptor and, unless the two sets are one, by its kind.
        using index_key = std::array<uint32_t, 3>;
        using index_ptr = std::shared_ptr<gw_mapper_index>;
        using copy_ptr  = std::shared_ptr<gw_mapper_index_host_copy>;
        auto key_of = [&](uint32_t kind, const descriptor& d) {
            return index_key{all_to_all ? 0u : kind, d.first_read, d.number_of_reads};
        };
        // the indices of a batch that hold reads, each once, queries first
        auto keys_of = [&](const index_batch& b) {
            std::vector<std::pair<index_key, descriptor>> keys;
            for (uint32_t kind = 0; kind < 2; ++kind)
                for (const descriptor& d : kind == 0 ? b.query_indices : b.target_indices)
                {
                    const index_key k = key_of(kind, d);
                    if (d.number_of_reads > 0 &&
                        std::none_of(keys.begin(), keys.end(), [&](const auto& e) { return e.first == k; }))
                        keys.push_back({k, d});
                }
            return keys;
        };
        copy_stream restores; // the second stream: indices of the next device batch come back while this one is mapped
        std::map<index_key, index_ptr> on_device; // alive from the previous device batch
        std::map<index_key, copy_ptr> on_host;    // the host copies of the previous host batch
        struct drain
        {
            copy_stream& c;
            ~drain() { (void)hipStreamSynchronize(c.stream); } // no copy may outlive the slab it reads
        } drain_before_the_copies_go{restores};
        auto build = [&](const index_key& k, const descriptor& d) {
            const bool target = !all_to_all && k[0] == 1;
            ++result->index_builds;
            return std::make_shared<gw_mapper_index>(target ? target_bases : query_bases,
                                                     (target ? target_offsets : query_offsets) + d.first_read,
                                                     static_cast<int32_t>(d.number_of_reads), d.first_read, kmer_size,
                                                     window_size, 1, filtering_parameter, s);
        };
        auto restore = [&](const copy_ptr& copy) {
            index_ptr index = std::make_shared<gw_mapper_index>();
            restores.begin_span();
            throw_on(gwm_index_unpack(&copy->c, restores.stream, &index->x));
            restores.end_span();
            ++result->index_restores;
            return index;
        };

        for (const batch_of_indices& batch : batches)
        {
            // 1. the indices of the host batch: those of the first device batch stay on the device, those a later
            //    device batch asks for get a packed host copy. Before one is built it is looked for among the indices
            //    still on the device and among the host copies of the previous host batch.
            std::vector<index_key> first, later;
            for (size_t b = 0; b < batch.device_batches.size(); ++b)
                for (const auto& e : keys_of(batch.device_batches[b]))
                    (b == 0 ? first : later).push_back(e.first);
            auto in = [](const std::vector<index_key>& v, const index_key& k) {
                return std::find(v.begin(), v.end(), k) != v.end();
            };
            std::map<index_key, index_ptr> current;
            std::map<index_key, copy_ptr> copies;
            const auto asked_for = keys_of(batch.host_batch);
            // what the previous device batch left and this host batch does not ask for goes before anything is built,
            // so one index per batch never holds more than the two indices of a pair
            for (auto it = on_device.begin(); it != on_device.end();)
                it = std::none_of(asked_for.begin(), asked_for.end(), [&](const auto& e) { return e.first == it->first; })
                         ? on_device.erase(it)
                         : std::next(it);
            for (const auto& e : asked_for)
            {
                const index_key& k = e.first;
                const auto alive = on_device.find(k);
                const auto kept  = on_host.find(k);
                index_ptr index  = alive != on_device.end() ? alive->second : nullptr;
                copy_ptr copy    = kept != on_host.end() ? kept->second : nullptr;
                if (alive != on_device.end())
                    on_device.erase(alive); // from here on it lives as long as this batch needs it
                if (!index)
                {
                    if (!copy)
                        index = build(k, e.second);
                    else if (in(first, k))
                        index = restore(copy);
                }
                if (in(later, k))
                {
                    if (!copy)
                    {
                        copy = std::make_shared<gw_mapper_index_host_copy>(*index, s);
                        result->cache_ms[0] += copy->c.pack_ms;
                    }
                    copies[k] = copy;
                }
                if (in(first, k))
                    current[k] = index;
            }
            restores.settle(s);
            on_device.clear();
            // `copies` now holds the previous host batch's copies. A restore queued above may still read one of them,
            // so they are let go at the end of this host batch, behind a wait for the second stream.
            on_host.swap(copies);

            // 2. the device batches: while one is mapped, the next one's indices are restored on the second stream
            for (size_t b = 0; b < batch.device_batches.size(); ++b)
            {
                std::map<index_key, index_ptr> next;
                if (b + 1 < batch.device_batches.size())
                    for (const auto& e : keys_of(batch.device_batches[b + 1]))
                    {
                        const auto here = current.find(e.first);
                        next[e.first]   = here != current.end() ? here->second : restore(on_host.at(e.first));
                    }
                for (const descriptor& qx : batch.device_batches[b].query_indices)
                    for (const descriptor& tx : batch.device_batches[b].target_indices)
                    {
                        if (qx.number_of_reads == 0 || tx.number_of_reads == 0 ||
                            (all_to_all && tx.first_read < qx.first_read))
                            continue;
                        map_pair(*current.at(key_of(0, qx)), *current.at(key_of(1, tx)));
                    }
                if (b + 1 < batch.device_batches.size())
                {
                    restores.settle(s);
                    current.swap(next);
                }
            }
            on_device.swap(current);
            if (!copies.empty()) // the second stream is idle by now; this makes letting the old copies go safe by itself
                hip_check(hipStreamSynchronize(restores.stream), "hipStreamSynchronize");
        }
        result->cache_ms[1] = restores.restore_ms();
        return result.release();
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
        event_span span;
        hip_check(hipEventRecord(span.a, s), "hipEventRecord");
        throw_on(gwm_index_unpack(&copy->c, s, &h->x));
        hip_check(hipEventRecord(span.b, s), "hipEventRecord");
        const float ms = span.ms(); // waits: the index is ready when this returns
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
