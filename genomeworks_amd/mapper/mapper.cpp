// mapper.cpp -- host side of cudamapper (libcudamapper.so): owning Index and Matcher objects over the stage functions
// of include/gwhip_mapper.h, and the flat C API of include/gw_mapper_capi.h.
#include "gw_mapper_capi.h"
#include "gwhip_mapper.h"

#include <hip/hip_runtime.h>

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

} // extern "C"
