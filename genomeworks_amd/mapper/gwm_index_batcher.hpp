// gwm_index_batcher.hpp -- the reference's index batcher on the host, no device involved: reads grouped into index
// descriptors, descriptors into host batches, host batches into device batches (rules in INTEGRATION.md section 3h).
#ifndef GWM_INDEX_BATCHER_HPP
#define GWM_INDEX_BATCHER_HPP

#include <cstdint>
#include <vector>

namespace gwm
{

struct descriptor
{
    uint32_t first_read;
    uint32_t number_of_reads;
};

inline bool operator==(const descriptor& a, const descriptor& b)
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

// group_reads_into_indices of the reference, its loop as it stands (see gw_mapper_capi.h)
std::vector<descriptor> group_reads(const int64_t* lengths, int64_t n, int64_t max_basepairs);

// generate_batches_of_indices of the reference over descriptors that are already grouped, with the counts checked as
// its application parameters check them
std::vector<batch_of_indices> generate_batches(const std::vector<descriptor>& queries,
                                               const std::vector<descriptor>& targets, int64_t query_host,
                                               int64_t query_device, int64_t target_host, int64_t target_device,
                                               bool same_query_and_target);

std::vector<int64_t> read_lengths(const int64_t* offsets, int32_t n);

} // namespace gwm

#endif
