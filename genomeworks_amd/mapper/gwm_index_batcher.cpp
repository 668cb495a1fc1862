// gwm_index_batcher.cpp -- see gwm_index_batcher.hpp
#include "gwm_index_batcher.hpp"

#include <algorithm>
#include <stdexcept>
#include <utility>

namespace gwm
{

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

// group_into_batches of the reference: blocks of per_query x per_target indices, query blocks outside; with the same
// query and target only the upper triangle, the targets starting at the query block's own position
static std::vector<index_batch> group_into_batches(const std::vector<descriptor>& queries, const std::vector<descriptor>& targets,
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

} // namespace gwm
