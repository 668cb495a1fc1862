// gwm_handles.hpp -- what stands behind the opaque pointers of include/gw_mapper_capi.h: owning objects over the stage
// functions of include/gwhip_mapper.h, and the read sets of one call. Shared by mapper.cpp (the extern "C" adapters)
// and gwm_driver.cpp (the batched driver).
#ifndef GWM_HANDLES_HPP
#define GWM_HANDLES_HPP

#include "gwhip_mapper.h"
#include "gwm_host_utils.hpp"
#include "gwm_windows.hpp"

#include <algorithm>
#include <memory>
#include <vector>

namespace gwm
{

inline void throw_on(int rc)
{
    if (rc != 0)
        throw std::runtime_error(gwm_last_error());
}

// A read set as the C API and the stage functions take it, in memory that somebody else keeps, on the host or on the
// device: bases[offsets[i] .. offsets[i + 1]) is read i.
struct reads_view
{
    const char* bases;
    const int64_t* offsets;
    int32_t n;
};

} // namespace gwm

namespace
{

using gwm::reads_view;
using gwm::throw_on;

template <typename T>
void copy_out(T* dst, const T* src, int64_t n)
{
    if (dst && n > 0)
        check(hipMemcpy(dst, src, sizeof(T) * static_cast<size_t>(n), hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

// The queries and targets of one call. Targets without bases mean all against all: the targets are the queries, on
// the host and on the device, and that is settled here once. The device copies, in the layout
// gwm_rescue_overlap_ends and gwm_align_overlaps take, are made by the first upload(), which whoever rescues ends or
// aligns calls before using device_queries / device_targets.
struct read_sets
{
    const reads_view queries, targets;
    const bool all_to_all;
    reads_view device_queries{}, device_targets{};
    read_sets(const reads_view& q, const reads_view& t)
        : queries(q), targets(t.bases ? t : q), all_to_all(t.bases == nullptr)
    {
    }
    void upload()
    {
        if (device_queries.offsets)
            return;
        device_queries = device_targets = upload(queries, bases_[0], offsets_[0]);
        if (!all_to_all)
            device_targets = upload(targets, bases_[1], offsets_[1]);
    }

private:
    static reads_view upload(const reads_view& host, dbuf<char>& bases, dbuf<int64_t>& offsets)
    {
        if (host.n < 0)
            throw std::invalid_argument("negative number of reads");
        bases.upload(host.bases, std::max<int64_t>(host.offsets[host.n], 1));
        offsets.upload(host.offsets, host.n + 1);
        return {bases.p, offsets.p, host.n};
    }
    dbuf<char> bases_[2];
    dbuf<int64_t> offsets_[2];
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

// The counters of one gwm_overlap_pileup or gwm_pair_pileup call, on the device until they are copied out
struct gw_mapper_pileup
{
    gwm_pileup p{};
    gw_mapper_pileup() = default;
    ~gw_mapper_pileup() { gwm_pileup_free(&p); }
    gw_mapper_pileup(const gw_mapper_pileup&) = delete;
    gw_mapper_pileup& operator=(const gw_mapper_pileup&) = delete;
};

// The records and the counters of one gwm_overlap_variants call, on the device until they are copied out
struct gw_mapper_variants
{
    gwm_variants v{};
    gw_mapper_variants() = default;
    ~gw_mapper_variants() { gwm_variants_free(&v); }
    gw_mapper_variants(const gw_mapper_variants&) = delete;
    gw_mapper_variants& operator=(const gw_mapper_variants&) = delete;
};

// The windows of one gw_mapper_window_overlaps or gw_mapper_correction_windows call, on the host
struct gw_mapper_windows
{
    std::vector<gwm_segment> segments; // in read correction: the target-role records of the pairs
    std::vector<int64_t> segment_offsets{0};
    std::vector<int32_t> edit_distances;
    float stage_ms[4] = {0.f, 0.f, 0.f, 0.f}; // gather, align, segments, window gather
    std::vector<gwm::window_record> windows;
    std::vector<int64_t> sequence_offsets{0};
    std::vector<char> bases;
    // read correction only: the input positions of the pairs, their query-role records and those records' device time
    std::vector<int64_t> pair_positions;
    std::vector<gwm_segment> query_role_segments;
    std::vector<int64_t> query_role_offsets{0};
    float query_role_ms = 0.f;
    // weighted calls only: one weight per byte of `bases`, the quality sums of `segments` and of query_role_segments
    // (empty where the supplying set has no qualities), and the device time of the sums and of the weight gather
    std::vector<int8_t> weights;
    std::vector<uint32_t> quality_sums, query_role_quality_sums;
    float quality_ms[2] = {0.f, 0.f};
};

#endif
