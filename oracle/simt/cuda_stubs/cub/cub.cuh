// cub/cub.cuh -- TEST INFRASTRUCTURE (oracle/simt): stand-ins for the cub calls of the reference's cudamapper sources
// (cub::DeviceRadixSort::SortPairs is in device/device_radix_sort.cuh), written here as plain sequential loops over host memory.
// Each one states the documented result of the cub call of the same name, nothing is taken from a cub tree; like cub, a call
// with a null temporary storage only reports the storage it wants. Equality is asked of neighbours, predecessor first --
// equality_op(in[i - 1], in[i]) -- which matters to the reference: its operator== of two anchors is neither symmetric nor
// transitive. What these loops cannot show is how cub itself evaluates such an operator.
#pragma once
#include <cstddef>
#include <cstdint>
#include <iterator>

#include "device/device_radix_sort.cuh"
#include "util_type.cuh"
#include <cuda_runtime_api.h>

namespace cub
{
/// it[i] = op(base[i])
template <typename Value, typename Op, typename InputIt, typename Offset = std::ptrdiff_t>
class TransformInputIterator
{
public:
    using value_type        = Value;
    using difference_type   = Offset;
    using reference         = Value;
    using pointer           = Value*;
    using iterator_category = std::random_access_iterator_tag;
    TransformInputIterator(InputIt base, Op op) : base_(base), op_(op) {}
    Value operator*() const { return op_(*base_); }
    Value operator[](Offset i) const { return op_(base_[i]); }
    TransformInputIterator operator+(Offset i) const { return TransformInputIterator(base_ + i, op_); }
    TransformInputIterator& operator++() { ++base_; return *this; }

private:
    InputIt base_;
    Op op_;
};

struct DeviceRunLengthEncode
{
    /// runs of neighbours that compare equal: the first element of every run, the run's length, the number of runs
    template <typename In, typename UniqueOut, typename LengthsOut, typename NumRunsOut>
    static cudaError_t Encode(void* temp, size_t& temp_bytes, In in, UniqueOut unique_out, LengthsOut counts_out, NumRunsOut num_runs_out,
                              int n, cudaStream_t = nullptr)
    {
        if (temp == nullptr)
        {
            temp_bytes = 16;
            return cudaSuccess;
        }
        int runs = 0;
        for (int i = 0; i < n; ++i)
        {
            if (i == 0 || !(in[i - 1] == in[i]))
            {
                unique_out[runs] = in[i];
                counts_out[runs] = 0;
                ++runs;
            }
            counts_out[runs - 1] = counts_out[runs - 1] + 1;
        }
        *num_runs_out = runs;
        return cudaSuccess;
    }
};

struct DeviceScan
{
    /// out[i] = in[0] + ... + in[i - 1]
    template <typename In, typename Out>
    static cudaError_t ExclusiveSum(void* temp, size_t& temp_bytes, In in, Out out, int n, cudaStream_t = nullptr)
    {
        if (temp == nullptr)
        {
            temp_bytes = 16;
            return cudaSuccess;
        }
        typename std::iterator_traits<In>::value_type acc = 0;
        for (int i = 0; i < n; ++i)
        {
            const auto v = in[i];
            out[i]       = acc;
            acc          = acc + v;
        }
        return cudaSuccess;
    }
};

struct DeviceReduce
{
    /// runs of neighbouring keys that compare equal: the first key of every run, its values reduced from left to right, the number of runs
    template <typename KeysIn, typename UniqueOut, typename ValuesIn, typename AggregatesOut, typename NumRunsOut, typename ReductionOp>
    static cudaError_t ReduceByKey(void* temp, size_t& temp_bytes, KeysIn keys_in, UniqueOut unique_out, ValuesIn values_in,
                                   AggregatesOut aggregates_out, NumRunsOut num_runs_out, ReductionOp op, int n, cudaStream_t = nullptr)
    {
        if (temp == nullptr)
        {
            temp_bytes = 16;
            return cudaSuccess;
        }
        int runs = 0;
        for (int i = 0; i < n; ++i)
        {
            if (i == 0 || !(keys_in[i - 1] == keys_in[i]))
            {
                unique_out[runs]     = keys_in[i];
                aggregates_out[runs] = values_in[i];
                ++runs;
            }
            else
                aggregates_out[runs - 1] = op(aggregates_out[runs - 1], values_in[i]);
        }
        *num_runs_out = runs;
        return cudaSuccess;
    }
};
} // namespace cub
