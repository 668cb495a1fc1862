// aligner_semiglobal.hpp -- the infix / prefix alignment types (AlignmentType::infix_alignment, ::prefix_alignment): the
// query is placed inside its target (infix) or at its start (prefix) instead of end to end. No counterpart in the
// reference, whose only type is global_alignment.
//
// Per pair: a score-only Myers scan on the device finds the edit distance d and the target slice [tb, te)
// (include/gwhip_semiglobal.h states the rules); only (d, tb, te) comes back to the host. A gather kernel then lays the
// queries and their slices out as q0 t0[tb:te] q1 t1[tb:te] ..., and the default global aligner (gwhip_hirschberg_myers
// with this aligner's max_query_length) aligns them as it stands: the states of a pair are exactly those of a
// global_alignment aligner of the same limits on (Q, T[tb:te]). A pair whose slice is empty gets its n deletions
// without that aligner. Limits, statuses and life cycle are FixedLimitAligner's (aligner_global.hpp).
#pragma once
#include "aligner_global.hpp"

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaaligner
{

class AlignerSemiglobal : public FixedLimitAligner
{
public:
    AlignerSemiglobal(AlignmentType type, int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                      DefaultDeviceAllocator allocator, cudaStream_t stream, int32_t device_id);
    ~AlignerSemiglobal() override;

    /// The ends scan, a wait for (d, tb, te), then gather and traceback queued on the stream.
    StatusType align_all() override;
    StatusType sync_alignments() override;

    AlignmentType get_alignment_type() const { return type_; }
    /// measurement aid: HIP-event times of the last align_all() -- the ends scan(s), and gather + traceback; false before one
    bool last_stage_ms(float* ends_ms, float* traceback_ms);

private:
    void free_device() override;

    PinnedVector<int32_t> ends_h_;        ///< [3n] d, tb, te
    PinnedVector<int64_t> sub_starts_h_;  ///< [2 n_sub + 1] layout of the gathered pairs
    PinnedVector<int32_t> sub_index_h_;   ///< [n_sub] pair of gathered pair s
    PinnedVector<int8_t> results_h_;
    PinnedVector<int32_t> result_lengths_h_;
    char* ends_block_        = nullptr; ///< sequences, starts, ends, scan workspace
    size_t ends_block_bytes_ = 0;
    char* tb_block_          = nullptr; ///< gathered sequences, their starts and index, states, lengths, aligner workspace
    size_t tb_block_bytes_   = 0;
    hipEvent_t events_[4]    = {nullptr, nullptr, nullptr, nullptr}; ///< around the scan, around gather + traceback
    bool timed_              = false;
};

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
