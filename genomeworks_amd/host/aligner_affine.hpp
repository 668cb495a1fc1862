// aligner_affine.hpp -- global alignment under affine gap costs inside a diagonal band
// (cudaaligner/aligner_affine.hpp): the host side of gwhip_affine_align (include/gwhip_affine.h), whose kernels run
// the forward pass and the traceback and leave the states in the form the default aligner leaves them. Only the
// states, their lengths, the costs and the optimality flags come back. Limits, statuses and life cycle are
// FixedLimitAligner's (aligner_global.hpp); on top of them add_alignment() refuses a pair with exceeded_max_alignments
// when the batch's device buffers (the bit matrix is the bulk: about (n + m) * (|m - n| / 2 + band_width) bytes a
// pair) would exceed the memory the aligner was given.
#pragma once
#include "aligner_global.hpp"
#include "alignment_impl.hpp"

#include <claraparabricks/genomeworks/cudaaligner/aligner_affine.hpp>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaaligner
{

/// what get_alignment_cost() finds
class AffineAlignment : public AlignmentImpl
{
public:
    using AlignmentImpl::AlignmentImpl;
    int32_t cost = -1;
};

class AlignerGlobalAffine : public FixedLimitAligner
{
public:
    /// max_device_memory < 0: the allocator's largest free block
    AlignerGlobalAffine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments, AffineScoring scoring,
                        int32_t band_width, int64_t max_device_memory, DefaultDeviceAllocator allocator, cudaStream_t stream,
                        int32_t device_id);
    /// the same under two-piece gap costs (gwhip_affine2_align)
    AlignerGlobalAffine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments, TwoPieceScoring scoring,
                        int32_t band_width, int64_t max_device_memory, DefaultDeviceAllocator allocator, cudaStream_t stream,
                        int32_t device_id);
    ~AlignerGlobalAffine() override;

    StatusType add_alignment(const char* query, int32_t query_length, const char* target, int32_t target_length,
                             bool reverse_complement_query = false, bool reverse_complement_target = false) override;
    StatusType align_all() override;
    StatusType sync_alignments() override;
    void reset() override;

    /// measurement aid: HIP-event times of the last align_all() -- the forward pass and the traceback; false before one
    bool last_stage_ms(float* forward_ms, float* traceback_ms);

private:
    void free_device() override;
    int64_t device_bytes(int64_t pairs, int64_t bases, int64_t bit_bytes) const;

    size_t workspace_bytes(int32_t pairs, const int64_t* starts) const;

    TwoPieceScoring scoring_; ///< the second piece is read only when two_piece_
    bool two_piece_;
    int32_t band_width_;
    int64_t max_device_memory_;
    int64_t bit_bytes_ = 0; ///< of the queued pairs' bit matrices
    PinnedVector<int8_t> results_h_;
    PinnedVector<int32_t> result_lengths_h_;
    PinnedVector<int32_t> costs_h_;
    PinnedVector<uint8_t> optimal_h_;
    char* device_block_        = nullptr;
    size_t device_block_bytes_ = 0;
    hipEvent_t events_[3]      = {nullptr, nullptr, nullptr}; ///< before the forward pass, between it and the traceback, behind
    bool timed_                = false;
};

/// what get_alignment_extension() finds
class ExtensionAlignment : public AlignmentImpl
{
public:
    using AlignmentImpl::AlignmentImpl;
    Extension extension{-1, -1, -1, false};
};

/// The affine X-drop extension (gwhip_extend of include/gwhip_affine.h) behind FixedLimitAligner's limits, statuses and
/// life cycle; the memory rule of add_alignment() is AlignerGlobalAffine's, with the extension's bit matrix: about
/// min(n + m, 2 min(n, m) + band_width) * band_width bytes a pair.
class AlignerExtension : public FixedLimitAligner
{
public:
    /// max_device_memory < 0: the allocator's largest free block
    AlignerExtension(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments, ExtensionScoring scoring,
                     int32_t band_width, int32_t xdrop, int64_t max_device_memory, DefaultDeviceAllocator allocator,
                     cudaStream_t stream, int32_t device_id);
    ~AlignerExtension() override;

    StatusType add_alignment(const char* query, int32_t query_length, const char* target, int32_t target_length,
                             bool reverse_complement_query = false, bool reverse_complement_target = false) override;
    StatusType align_all() override;
    StatusType sync_alignments() override;
    void reset() override;

    /// measurement aid: HIP-event times of the last align_all() -- the forward pass and the traceback; false before one
    bool last_stage_ms(float* forward_ms, float* traceback_ms);

private:
    void free_device() override;
    int64_t device_bytes(int64_t pairs, int64_t bases, int64_t bit_bytes) const;

    ExtensionScoring scoring_;
    int32_t band_width_, xdrop_;
    int64_t max_device_memory_;
    int64_t bit_bytes_ = 0; ///< of the queued pairs' bit matrices
    PinnedVector<int8_t> results_h_;
    PinnedVector<int32_t> numbers_h_; ///< [4 n]: lengths, scores, query ends, target ends
    PinnedVector<uint8_t> dropped_h_;
    char* device_block_        = nullptr;
    size_t device_block_bytes_ = 0;
    hipEvent_t events_[3]      = {nullptr, nullptr, nullptr};
    bool timed_                = false;
};

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
