// aligner_affine.cpp -- host side of the affine-gap global aligner (see aligner_affine.hpp).
#include "aligner_affine.hpp"

#include <claraparabricks/genomeworks/logging/logging.hpp>
#include <claraparabricks/genomeworks/utils/cudautils.hpp>
#include <claraparabricks/genomeworks/utils/signed_integer_utils.hpp>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "../../include/gwhip_affine.h"
#include "host_common.hpp"

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaaligner
{

namespace
{
AffineScoring checked(AffineScoring s, int32_t band_width)
{
    if (s.mismatch < 1 || s.mismatch > 255 || s.gap_open < 0 || s.gap_open > 255 || s.gap_extend < 1 || s.gap_extend > 255)
        throw std::invalid_argument("affine scoring (mismatch " + std::to_string(s.mismatch) + ", gap_open " + std::to_string(s.gap_open) +
                                    ", gap_extend " + std::to_string(s.gap_extend) + ") outside 1..255, 0..255, 1..255");
    if (band_width < 0) throw std::invalid_argument("band_width must be non-negative.");
    return s;
}

TwoPieceScoring checked(TwoPieceScoring s, int32_t band_width)
{
    checked(AffineScoring{s.mismatch, s.gap_open, s.gap_extend}, band_width);
    if (s.gap_open2 < 0 || s.gap_open2 > 255 || s.gap_extend2 < 1 || s.gap_extend2 > 255)
        throw std::invalid_argument("affine scoring (gap_open2 " + std::to_string(s.gap_open2) + ", gap_extend2 " +
                                    std::to_string(s.gap_extend2) + ") outside 0..255, 1..255");
    return s;
}

// the allocator of max_device_memory bytes (-1: the largest free section of the device, written back)
DefaultDeviceAllocator caching_allocator(cudaStream_t stream, int64_t* max_device_memory)
{
    if (*max_device_memory < -1) throw std::invalid_argument("max_device_memory has to be either -1 (=all available GPU memory) or greater or equal than 0.");
    if (*max_device_memory == -1)
    {
        *max_device_memory = cudautils::find_largest_contiguous_device_memory_section();
        if (*max_device_memory == 0) throw std::runtime_error("No memory available for caching");
    }
    return DefaultDeviceAllocator(static_cast<size_t>(*max_device_memory), stream);
}
} // namespace

AlignerGlobalAffine::AlignerGlobalAffine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                         AffineScoring scoring, int32_t band_width, int64_t max_device_memory,
                                         DefaultDeviceAllocator allocator, cudaStream_t stream, int32_t device_id)
    : FixedLimitAligner(AlignmentType::global_alignment, max_query_length, max_target_length, max_alignments, allocator, stream, device_id)
    , scoring_{checked(scoring, band_width).mismatch, scoring.gap_open, scoring.gap_extend, 0, 0}
    , two_piece_(false)
    , band_width_(band_width)
    , max_device_memory_(max_device_memory < 0 ? get_size_of_largest_free_memory_block(allocator) : max_device_memory)
{
}

AlignerGlobalAffine::AlignerGlobalAffine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                         TwoPieceScoring scoring, int32_t band_width, int64_t max_device_memory,
                                         DefaultDeviceAllocator allocator, cudaStream_t stream, int32_t device_id)
    : FixedLimitAligner(AlignmentType::global_alignment, max_query_length, max_target_length, max_alignments, allocator, stream, device_id)
    , scoring_(checked(scoring, band_width))
    , two_piece_(true)
    , band_width_(band_width)
    , max_device_memory_(max_device_memory < 0 ? get_size_of_largest_free_memory_block(allocator) : max_device_memory)
{
}

size_t AlignerGlobalAffine::workspace_bytes(int32_t pairs, const int64_t* starts) const
{
    return two_piece_ ? gwhip_affine2_workspace_bytes(pairs, starts, band_width_) : gwhip_affine_workspace_bytes(pairs, starts, band_width_);
}

AlignerGlobalAffine::~AlignerGlobalAffine()
{
    drain_and_free_device();
    for (hipEvent_t e : events_)
        if (e != nullptr) (void)hipEventDestroy(e);
}

void AlignerGlobalAffine::free_device()
{
    if (device_block_ != nullptr) allocator_.deallocate(device_block_, device_block_bytes_);
    device_block_       = nullptr;
    device_block_bytes_ = 0;
}

void AlignerGlobalAffine::reset()
{
    FixedLimitAligner::reset();
    bit_bytes_ = 0;
    timed_     = false;
}

// the block of align_all(): sequences, starts, states, lengths, costs, flags, the kernels' workspace (each part on a
// 256-byte boundary at most)
int64_t AlignerGlobalAffine::device_bytes(int64_t pairs, int64_t bases, int64_t bit_bytes) const
{
    return 2 * (bases + 16) + (2 * pairs + 1) * 8 + pairs * (4 + 4 + 1) + 8 * (pairs + 1) + bit_bytes + 8 * 256;
}

StatusType AlignerGlobalAffine::add_alignment(const char* query, int32_t query_length, const char* target, int32_t target_length,
                                              bool reverse_complement_query, bool reverse_complement_target)
{
    int64_t pair_bits = 0;
    if (query_length >= 0 && target_length >= 0 && query_length <= max_query_length_ && target_length <= max_target_length_ &&
        num_alignments() < max_alignments_)
    {
        const int64_t starts[3] = {0, query_length, static_cast<int64_t>(query_length) + target_length};
        pair_bits               = static_cast<int64_t>(workspace_bytes(1, starts)) - 256; // without the offsets
        if (device_bytes(num_alignments() + 1, seq_starts_h_.back() + starts[2], bit_bytes_ + pair_bits) > max_device_memory_)
        {
            GW_LOG_DEBUG("The batch's device buffers would exceed the memory given to the aligner.");
            return StatusType::exceeded_max_alignments;
        }
    }
    const StatusType status =
        FixedLimitAligner::add_alignment(query, query_length, target, target_length, reverse_complement_query, reverse_complement_target);
    if (status != StatusType::success) return status;
    // the object that carries the cost, in place of the one the base class made
    const size_t i      = alignments_.size() - 1;
    const int64_t begin = seq_starts_h_[2 * i];
    auto alignment      = std::make_shared<AffineAlignment>(seq_h_.data() + begin, query_length, seq_h_.data() + begin + query_length, target_length);
    alignment->set_alignment_type(type_);
    alignments_[i] = std::move(alignment);
    bit_bytes_ += pair_bits;
    return status;
}

StatusType AlignerGlobalAffine::align_all()
{
    const int32_t n = num_alignments();
    if (n == 0) return StatusType::success;
    scoped_device_switch dev(device_id_);
    for (hipEvent_t& e : events_)
        if (e == nullptr) GW_CU_CHECK_ERR(hipEventCreate(&e));
    launched_ = false;
    timed_    = false;
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_)); // nothing of an earlier batch still uses the block freed below
    free_device();
    const size_t un      = static_cast<size_t>(n);
    const int64_t total  = seq_starts_h_.back();
    const size_t ws_size = workspace_bytes(n, seq_starts_h_.data());
    gwhost::BlockLayout layout;
    const auto seq       = layout.take<char>(static_cast<size_t>(total) + 16);
    const auto starts    = layout.take<int64_t>(2 * un + 1);
    const auto results   = layout.take<int8_t>(static_cast<size_t>(total) + 16);
    const auto lengths   = layout.take<int32_t>(un);
    const auto costs     = layout.take<int32_t>(un);
    const auto optimal   = layout.take<uint8_t>(un);
    const auto workspace = layout.take<char>(ws_size);
    if (static_cast<int64_t>(layout.bytes) > max_device_memory_) return StatusType::exceeded_max_alignments;
    device_block_bytes_ = layout.bytes;
    device_block_       = allocator_.allocate(device_block_bytes_, {stream_});
    GW_CU_CHECK_ERR(hipMemcpyAsync(seq.in(device_block_), seq_h_.data(), static_cast<size_t>(total), hipMemcpyHostToDevice, stream_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(starts.in(device_block_), seq_starts_h_.data(), seq_starts_h_.size() * 8, hipMemcpyHostToDevice, stream_));
    gwhip_affine_args a{};
    a.n_alignments         = n;
    a.sequences            = seq.in(device_block_);
    a.sequence_starts      = starts.in(device_block_);
    a.sequence_starts_host = seq_starts_h_.data();
    a.mismatch             = scoring_.mismatch;
    a.gap_open             = scoring_.gap_open;
    a.gap_extend           = scoring_.gap_extend;
    a.band                 = band_width_;
    a.results              = results.in(device_block_);
    a.result_lengths       = lengths.in(device_block_);
    a.costs                = costs.in(device_block_);
    a.optimal              = optimal.in(device_block_);
    a.workspace            = workspace.in(device_block_);
    a.workspace_bytes      = ws_size;
    void* const events[3]  = {events_[0], events_[1], events_[2]};
    if (two_piece_)
    {
        gwhip_affine2_args b{};
        b.n_alignments         = n;
        b.sequences            = a.sequences;
        b.sequence_starts      = a.sequence_starts;
        b.sequence_starts_host = a.sequence_starts_host;
        b.mismatch             = scoring_.mismatch;
        b.gap_open             = scoring_.gap_open;
        b.gap_extend           = scoring_.gap_extend;
        b.gap_open2            = scoring_.gap_open2;
        b.gap_extend2          = scoring_.gap_extend2;
        b.band                 = band_width_;
        b.results              = a.results;
        b.result_lengths       = a.result_lengths;
        b.costs                = a.costs;
        b.optimal              = a.optimal;
        b.workspace            = a.workspace;
        b.workspace_bytes      = ws_size;
        if (gwhip_affine2_align_events(&b, stream_, events) != 0) throw std::runtime_error(gwhip_affine_last_error());
    }
    else if (gwhip_affine_align_events(&a, stream_, events) != 0)
        throw std::runtime_error(gwhip_affine_last_error());
    results_h_.resize(static_cast<size_t>(total) + 16);
    result_lengths_h_.resize(un);
    costs_h_.resize(un);
    optimal_h_.resize(un);
    GW_CU_CHECK_ERR(hipMemcpyAsync(results_h_.data(), a.results, static_cast<size_t>(total), hipMemcpyDeviceToHost, stream_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(result_lengths_h_.data(), a.result_lengths, un * 4, hipMemcpyDeviceToHost, stream_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(costs_h_.data(), a.costs, un * 4, hipMemcpyDeviceToHost, stream_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(optimal_h_.data(), a.optimal, un, hipMemcpyDeviceToHost, stream_));
    launched_ = true;
    timed_    = true;
    return StatusType::success;
}

StatusType AlignerGlobalAffine::sync_alignments()
{
    scoped_device_switch dev(device_id_);
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    const size_t n = static_cast<size_t>(num_alignments());
    if (!launched_ || n == 0) return StatusType::success;
    for (size_t i = 0; i < n; ++i)
    {
        const int64_t slot = seq_starts_h_[2 * i + 2] - seq_starts_h_[2 * i];
        const int32_t len  = result_lengths_h_[i];
        if (costs_h_[i] < 0) continue; // no result (a band of more diagonals than the kernels take): the status stays uninitialized
        if (len < 0 || len > slot)
            throw std::runtime_error("affine alignment " + std::to_string(i) + ": the kernels report " + std::to_string(len) +
                                     " columns for a slot of " + std::to_string(slot));
        AffineAlignment* alignment = dynamic_cast<AffineAlignment*>(alignments_[i].get());
        alignment->set_alignment(reversed_states(results_h_.data() + seq_starts_h_[2 * i], static_cast<size_t>(len)), optimal_h_[i] != 0);
        alignment->cost = costs_h_[i];
        alignment->set_status(StatusType::success);
    }
    return StatusType::success;
}

bool AlignerGlobalAffine::last_stage_ms(float* forward_ms, float* traceback_ms)
{
    if (!timed_) return false;
    scoped_device_switch dev(device_id_);
    GW_CU_CHECK_ERR(hipEventSynchronize(events_[2]));
    GW_CU_CHECK_ERR(hipEventElapsedTime(forward_ms, events_[0], events_[1]));
    GW_CU_CHECK_ERR(hipEventElapsedTime(traceback_ms, events_[1], events_[2]));
    return true;
}

std::unique_ptr<Aligner> create_aligner_affine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                               AffineScoring scoring, int32_t band_width, DefaultDeviceAllocator allocator,
                                               cudaStream_t stream, int32_t device_id)
{
    return std::make_unique<AlignerGlobalAffine>(max_query_length, max_target_length, max_alignments, scoring, band_width, int64_t(-1), allocator,
                                                 stream, device_id);
}

std::unique_ptr<Aligner> create_aligner_affine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                               AffineScoring scoring, int32_t band_width, cudaStream_t stream, int32_t device_id,
                                               int64_t max_device_memory)
{
    checked(scoring, band_width); // before the device is touched
    scoped_device_switch device(device_id);
    const DefaultDeviceAllocator allocator = caching_allocator(stream, &max_device_memory);
    return std::make_unique<AlignerGlobalAffine>(max_query_length, max_target_length, max_alignments, scoring, band_width, max_device_memory,
                                                 allocator, stream, device_id);
}

std::unique_ptr<Aligner> create_aligner_affine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                               TwoPieceScoring scoring, int32_t band_width, DefaultDeviceAllocator allocator,
                                               cudaStream_t stream, int32_t device_id)
{
    return std::make_unique<AlignerGlobalAffine>(max_query_length, max_target_length, max_alignments, scoring, band_width, int64_t(-1), allocator,
                                                 stream, device_id);
}

std::unique_ptr<Aligner> create_aligner_affine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                               TwoPieceScoring scoring, int32_t band_width, cudaStream_t stream, int32_t device_id,
                                               int64_t max_device_memory)
{
    checked(scoring, band_width); // before the device is touched
    scoped_device_switch device(device_id);
    const DefaultDeviceAllocator allocator = caching_allocator(stream, &max_device_memory);
    return std::make_unique<AlignerGlobalAffine>(max_query_length, max_target_length, max_alignments, scoring, band_width, max_device_memory,
                                                 allocator, stream, device_id);
}

int32_t get_alignment_cost(const Alignment& alignment)
{
    const auto* affine = dynamic_cast<const AffineAlignment*>(&alignment);
    return affine != nullptr && affine->get_status() == StatusType::success ? affine->cost : -1;
}

// ---- the affine X-drop extension ---------------------------------------------------------------------------------

namespace
{
ExtensionScoring checked(ExtensionScoring s, int32_t band_width, int32_t xdrop)
{
    if (s.match < 1 || s.mismatch < 0 || s.match + int64_t(s.mismatch) > 127 || s.gap_open < 0 || s.gap_open > 127 || s.gap_extend < 1 ||
        s.match + 2 * int64_t(s.gap_extend) > 255)
        throw std::invalid_argument("extension scoring (match " + std::to_string(s.match) + ", mismatch " + std::to_string(s.mismatch) +
                                    ", gap_open " + std::to_string(s.gap_open) + ", gap_extend " + std::to_string(s.gap_extend) +
                                    ") outside match >= 1, mismatch >= 0, match + mismatch <= 127, gap_open 0..127, gap_extend >= 1, "
                                    "match + 2 gap_extend <= 255");
    if (band_width < 0 || band_width > GWHIP_EXTEND_MAX_BAND)
        throw std::invalid_argument("band_width " + std::to_string(band_width) + " outside 0..511");
    if (xdrop < -1 || xdrop > GWHIP_EXTEND_MAX_XDROP) throw std::invalid_argument("xdrop " + std::to_string(xdrop) + " outside -1..2^20");
    return s;
}
} // namespace

AlignerExtension::AlignerExtension(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments, ExtensionScoring scoring,
                                   int32_t band_width, int32_t xdrop, int64_t max_device_memory, DefaultDeviceAllocator allocator,
                                   cudaStream_t stream, int32_t device_id)
    : FixedLimitAligner(AlignmentType::extension_alignment, max_query_length, max_target_length, max_alignments, allocator, stream, device_id)
    , scoring_(checked(scoring, band_width, xdrop))
    , band_width_(band_width)
    , xdrop_(xdrop)
    , max_device_memory_(max_device_memory < 0 ? get_size_of_largest_free_memory_block(allocator) : max_device_memory)
{
}

AlignerExtension::~AlignerExtension()
{
    drain_and_free_device();
    for (hipEvent_t e : events_)
        if (e != nullptr) (void)hipEventDestroy(e);
}

void AlignerExtension::free_device()
{
    if (device_block_ != nullptr) allocator_.deallocate(device_block_, device_block_bytes_);
    device_block_       = nullptr;
    device_block_bytes_ = 0;
}

void AlignerExtension::reset()
{
    FixedLimitAligner::reset();
    bit_bytes_ = 0;
    timed_     = false;
}

// the block of align_all(): sequences, starts, states, four numbers and a flag per pair, the kernels' workspace (each
// part on a 256-byte boundary at most)
int64_t AlignerExtension::device_bytes(int64_t pairs, int64_t bases, int64_t bit_bytes) const
{
    return 2 * (bases + 16) + (2 * pairs + 1) * 8 + pairs * (4 * 4 + 1) + 8 * (pairs + 1) + bit_bytes + 8 * 256;
}

StatusType AlignerExtension::add_alignment(const char* query, int32_t query_length, const char* target, int32_t target_length,
                                           bool reverse_complement_query, bool reverse_complement_target)
{
    int64_t pair_bits = 0;
    if (query_length >= 0 && target_length >= 0 && query_length <= max_query_length_ && target_length <= max_target_length_ &&
        num_alignments() < max_alignments_)
    {
        const int64_t starts[3] = {0, query_length, static_cast<int64_t>(query_length) + target_length};
        pair_bits               = static_cast<int64_t>(gwhip_extend_workspace_bytes(1, starts, band_width_, 1)) - 256; // without the offsets
        if (device_bytes(num_alignments() + 1, seq_starts_h_.back() + starts[2], bit_bytes_ + pair_bits) > max_device_memory_)
        {
            GW_LOG_DEBUG("The batch's device buffers would exceed the memory given to the aligner.");
            return StatusType::exceeded_max_alignments;
        }
    }
    const StatusType status =
        FixedLimitAligner::add_alignment(query, query_length, target, target_length, reverse_complement_query, reverse_complement_target);
    if (status != StatusType::success) return status;
    // the object that carries the ends, in place of the one the base class made
    const size_t i      = alignments_.size() - 1;
    const int64_t begin = seq_starts_h_[2 * i];
    auto alignment = std::make_shared<ExtensionAlignment>(seq_h_.data() + begin, query_length, seq_h_.data() + begin + query_length, target_length);
    alignment->set_alignment_type(type_);
    alignments_[i] = std::move(alignment);
    bit_bytes_ += pair_bits;
    return status;
}

StatusType AlignerExtension::align_all()
{
    const int32_t n = num_alignments();
    if (n == 0) return StatusType::success;
    scoped_device_switch dev(device_id_);
    for (hipEvent_t& e : events_)
        if (e == nullptr) GW_CU_CHECK_ERR(hipEventCreate(&e));
    launched_ = false;
    timed_    = false;
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_)); // nothing of an earlier batch still uses the block freed below
    free_device();
    const size_t un      = static_cast<size_t>(n);
    const int64_t total  = seq_starts_h_.back();
    const size_t ws_size = gwhip_extend_workspace_bytes(n, seq_starts_h_.data(), band_width_, 1);
    gwhost::BlockLayout layout;
    const auto seq       = layout.take<char>(static_cast<size_t>(total) + 16);
    const auto starts    = layout.take<int64_t>(2 * un + 1);
    const auto results   = layout.take<int8_t>(static_cast<size_t>(total) + 16);
    const auto numbers   = layout.take<int32_t>(4 * un);
    const auto dropped   = layout.take<uint8_t>(un);
    const auto workspace = layout.take<char>(ws_size);
    if (static_cast<int64_t>(layout.bytes) > max_device_memory_) return StatusType::exceeded_max_alignments;
    device_block_bytes_ = layout.bytes;
    device_block_       = allocator_.allocate(device_block_bytes_, {stream_});
    GW_CU_CHECK_ERR(hipMemcpyAsync(seq.in(device_block_), seq_h_.data(), static_cast<size_t>(total), hipMemcpyHostToDevice, stream_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(starts.in(device_block_), seq_starts_h_.data(), seq_starts_h_.size() * 8, hipMemcpyHostToDevice, stream_));
    gwhip_extend_args a{};
    a.n_alignments         = n;
    a.sequences            = seq.in(device_block_);
    a.sequence_starts      = starts.in(device_block_);
    a.sequence_starts_host = seq_starts_h_.data();
    a.match                = scoring_.match;
    a.mismatch             = scoring_.mismatch;
    a.gap_open             = scoring_.gap_open;
    a.gap_extend           = scoring_.gap_extend;
    a.band                 = band_width_;
    a.xdrop                = xdrop_;
    a.results              = results.in(device_block_);
    a.result_lengths       = numbers.in(device_block_);
    a.scores               = a.result_lengths + un;
    a.query_ends           = a.scores + un;
    a.target_ends          = a.query_ends + un;
    a.dropped              = dropped.in(device_block_);
    a.workspace            = workspace.in(device_block_);
    a.workspace_bytes      = ws_size;
    void* const events[3]  = {events_[0], events_[1], events_[2]};
    if (gwhip_extend_events(&a, stream_, events) != 0) throw std::runtime_error(gwhip_affine_last_error());
    results_h_.resize(static_cast<size_t>(total) + 16);
    numbers_h_.resize(4 * un);
    dropped_h_.resize(un);
    GW_CU_CHECK_ERR(hipMemcpyAsync(results_h_.data(), a.results, static_cast<size_t>(total), hipMemcpyDeviceToHost, stream_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(numbers_h_.data(), a.result_lengths, 4 * un * 4, hipMemcpyDeviceToHost, stream_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(dropped_h_.data(), a.dropped, un, hipMemcpyDeviceToHost, stream_));
    launched_ = true;
    timed_    = true;
    return StatusType::success;
}

StatusType AlignerExtension::sync_alignments()
{
    scoped_device_switch dev(device_id_);
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    const size_t n = static_cast<size_t>(num_alignments());
    if (!launched_ || n == 0) return StatusType::success;
    for (size_t i = 0; i < n; ++i)
    {
        const int32_t len = numbers_h_[i], score = numbers_h_[n + i], query_end = numbers_h_[2 * n + i], target_end = numbers_h_[3 * n + i];
        if (score < 0) continue; // no result: the status stays uninitialized
        if (len < 0 || query_end < 0 || target_end < 0 || len > static_cast<int64_t>(query_end) + target_end ||
            static_cast<int64_t>(query_end) + target_end > seq_starts_h_[2 * i + 2] - seq_starts_h_[2 * i])
            throw std::runtime_error("extension " + std::to_string(i) + ": the kernels report " + std::to_string(len) + " columns up to (" +
                                     std::to_string(query_end) + ", " + std::to_string(target_end) + ")");
        ExtensionAlignment* alignment = dynamic_cast<ExtensionAlignment*>(alignments_[i].get());
        alignment->set_alignment(reversed_states(results_h_.data() + seq_starts_h_[2 * i], static_cast<size_t>(len)), false);
        alignment->set_target_range(0, target_end);
        alignment->extension = Extension{query_end, target_end, score, dropped_h_[i] != 0};
        alignment->set_status(StatusType::success);
    }
    return StatusType::success;
}

bool AlignerExtension::last_stage_ms(float* forward_ms, float* traceback_ms)
{
    if (!timed_) return false;
    scoped_device_switch dev(device_id_);
    GW_CU_CHECK_ERR(hipEventSynchronize(events_[2]));
    GW_CU_CHECK_ERR(hipEventElapsedTime(forward_ms, events_[0], events_[1]));
    GW_CU_CHECK_ERR(hipEventElapsedTime(traceback_ms, events_[1], events_[2]));
    return true;
}

std::unique_ptr<Aligner> create_aligner_extension(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                                  ExtensionScoring scoring, int32_t band_width, int32_t xdrop,
                                                  DefaultDeviceAllocator allocator, cudaStream_t stream, int32_t device_id)
{
    return std::make_unique<AlignerExtension>(max_query_length, max_target_length, max_alignments, scoring, band_width, xdrop, int64_t(-1),
                                              allocator, stream, device_id);
}

std::unique_ptr<Aligner> create_aligner_extension(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                                  ExtensionScoring scoring, int32_t band_width, int32_t xdrop, cudaStream_t stream,
                                                  int32_t device_id, int64_t max_device_memory)
{
    checked(scoring, band_width, xdrop); // before the device is touched
    scoped_device_switch device(device_id);
    const DefaultDeviceAllocator allocator = caching_allocator(stream, &max_device_memory);
    return std::make_unique<AlignerExtension>(max_query_length, max_target_length, max_alignments, scoring, band_width, xdrop,
                                              max_device_memory, allocator, stream, device_id);
}

Extension get_alignment_extension(const Alignment& alignment)
{
    const auto* extension = dynamic_cast<const ExtensionAlignment*>(&alignment);
    return extension != nullptr && extension->get_status() == StatusType::success ? extension->extension : Extension{-1, -1, -1, false};
}

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
