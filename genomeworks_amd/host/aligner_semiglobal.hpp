// aligner_semiglobal.hpp -- the infix / prefix alignment types (AlignmentType::infix_alignment, ::prefix_alignment): the
// query is placed inside its target (infix) or at its start (prefix) instead of end to end. No counterpart in the
// reference, whose only type is global_alignment.
//
// Per pair: a score-only Myers scan on the device finds the edit distance d and the target slice [tb, te)
// (include/gwhip_semiglobal.h states the rules); only (d, tb, te) comes back to the host. A gather kernel then lays the
// queries and their slices out as q0 t0[tb:te] q1 t1[tb:te] ..., and the default global aligner (gwhip_hirschberg_myers
// with this aligner's max_query_length) aligns them as it stands: the states of a pair are exactly those of a
// global_alignment aligner of the same limits on (Q, T[tb:te]). A pair whose slice is empty gets its n deletions
// without that aligner. Limits, statuses and life cycle are AlignerGlobal's (aligner_global.hpp).
#pragma once
#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>
#include <claraparabricks/genomeworks/cudaaligner/alignment.hpp>

#include <vector>

#include "pinned_vector.hpp"

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaaligner
{

class AlignerSemiglobal : public Aligner
{
public:
    AlignerSemiglobal(AlignmentType type, int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                      DefaultDeviceAllocator allocator, cudaStream_t stream, int32_t device_id);
    ~AlignerSemiglobal() override;

    /// The ends scan, a wait for (d, tb, te), then gather and traceback queued on the stream.
    StatusType align_all() override;
    StatusType sync_alignments() override;
    StatusType add_alignment(const char* query, int32_t query_length, const char* target, int32_t target_length,
                             bool reverse_complement_query = false, bool reverse_complement_target = false) override;
    const std::vector<std::shared_ptr<Alignment>>& get_alignments() const override { return alignments_; }
    /// null pointers: the packed run-length form is the banded aligner's (as for AlignerGlobal)
    DeviceAlignmentsPtrs get_alignments_device() const override { return DeviceAlignmentsPtrs{}; }
    void reset() override;
    void free_temporary_device_buffers() override {}
    int32_t num_alignments() const override { return static_cast<int32_t>(alignments_.size()); }
    cudaStream_t get_stream() const override { return stream_; }
    int32_t get_device() const override { return device_id_; }
    DefaultDeviceAllocator get_device_allocator() const override { return allocator_; }

    AlignmentType get_alignment_type() const { return type_; }
    /// measurement aid: HIP-event times of the last align_all() -- the ends scan(s), and gather + traceback; false before one
    bool last_stage_ms(float* ends_ms, float* traceback_ms);

private:
    void free_device();

    AlignmentType type_;
    int32_t max_query_length_, max_target_length_, max_alignments_;
    DefaultDeviceAllocator allocator_;
    cudaStream_t stream_;
    int32_t device_id_;
    PinnedVector<char> seq_h_;
    PinnedVector<int64_t> seq_starts_h_;
    PinnedVector<int32_t> ends_h_;        ///< [3n] d, tb, te
    PinnedVector<int64_t> sub_starts_h_;  ///< [2 n_sub + 1] layout of the gathered pairs
    PinnedVector<int32_t> sub_index_h_;   ///< [n_sub] pair of gathered pair s
    PinnedVector<int8_t> results_h_;
    PinnedVector<int32_t> result_lengths_h_;
    std::vector<std::shared_ptr<Alignment>> alignments_;
    char* ends_block_        = nullptr; ///< sequences, starts, ends, scan workspace
    size_t ends_block_bytes_ = 0;
    char* tb_block_          = nullptr; ///< gathered sequences, their starts and index, states, lengths, aligner workspace
    size_t tb_block_bytes_   = 0;
    void* events_[4]         = {nullptr, nullptr, nullptr, nullptr}; ///< hipEvent_t: around the scan, around gather + traceback
    bool timed_              = false;
    bool launched_           = false;
};

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
