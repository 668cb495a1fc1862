// aligner_semiglobal.cpp -- host side of the infix / prefix alignment types (see aligner_semiglobal.hpp).
#include "aligner_semiglobal.hpp"

#include <claraparabricks/genomeworks/logging/logging.hpp>
#include <claraparabricks/genomeworks/utils/cudautils.hpp>
#include <claraparabricks/genomeworks/utils/genomeutils.hpp>
#include <claraparabricks/genomeworks/utils/signed_integer_utils.hpp>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "../../include/gwhip.h"
#include "../../include/gwhip_semiglobal.h"
#include "alignment_impl.hpp"
#include "host_common.hpp"

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaaligner
{

AlignerSemiglobal::AlignerSemiglobal(AlignmentType type, int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                     DefaultDeviceAllocator allocator, cudaStream_t stream, int32_t device_id)
    : FixedLimitAligner(type, max_query_length, max_target_length, max_alignments, allocator, stream, device_id)
{
    if (type != AlignmentType::infix_alignment && type != AlignmentType::prefix_alignment)
        throw std::invalid_argument("AlignerSemiglobal aligns infix_alignment or prefix_alignment.");
}

AlignerSemiglobal::~AlignerSemiglobal()
{
    drain_and_free_device();
    for (hipEvent_t e : events_)
        if (e != nullptr) (void)hipEventDestroy(e);
}

void AlignerSemiglobal::free_device()
{
    if (ends_block_ != nullptr) allocator_.deallocate(ends_block_, ends_block_bytes_);
    if (tb_block_ != nullptr) allocator_.deallocate(tb_block_, tb_block_bytes_);
    ends_block_ = tb_block_ = nullptr;
    ends_block_bytes_ = tb_block_bytes_ = 0;
}

StatusType AlignerSemiglobal::align_all()
{
    const int32_t n = num_alignments();
    if (n == 0) return StatusType::success;
    scoped_device_switch dev(device_id_);
    hipStream_t s = stream_;
    for (hipEvent_t& e : events_)
        if (e == nullptr) GW_CU_CHECK_ERR(hipEventCreate(&e));
    launched_ = false;
    timed_    = false;
    GW_CU_CHECK_ERR(hipStreamSynchronize(s)); // nothing of an earlier batch still uses the blocks freed below
    free_device();

    // ---- where every query ends and begins: (d, tb, te) per pair ----
    const size_t un     = static_cast<size_t>(n);
    const int64_t total = seq_starts_h_.back();
    int32_t longest     = 0;
    for (size_t i = 0; i < un; ++i) longest = std::max(longest, static_cast<int32_t>(seq_starts_h_[2 * i + 1] - seq_starts_h_[2 * i]));
    const size_t scan_ws = gwhip_semiglobal_workspace_bytes(n, longest);
    gwhost::BlockLayout ends_layout;
    const auto seq            = ends_layout.take<char>(static_cast<size_t>(total) + 16);
    const auto starts         = ends_layout.take<int64_t>(2 * un + 1);
    const auto ends           = ends_layout.take<int32_t>(3 * un);
    const auto scan_workspace = ends_layout.take<char>(scan_ws);
    ends_block_bytes_ = ends_layout.bytes;
    ends_block_       = allocator_.allocate(ends_block_bytes_, {stream_});
    char* d_seq       = seq.in(ends_block_);
    int64_t* d_starts = starts.in(ends_block_);
    int32_t* d_ends   = ends.in(ends_block_);
    GW_CU_CHECK_ERR(hipMemcpyAsync(d_seq, seq_h_.data(), static_cast<size_t>(total), hipMemcpyHostToDevice, s));
    GW_CU_CHECK_ERR(hipMemcpyAsync(d_starts, seq_starts_h_.data(), seq_starts_h_.size() * 8, hipMemcpyHostToDevice, s));
    gwhip_semiglobal_args scan{};
    scan.n_pairs          = n;
    scan.mode             = type_ == AlignmentType::prefix_alignment ? GWHIP_SEMIGLOBAL_PREFIX : GWHIP_SEMIGLOBAL_INFIX;
    scan.sequences        = d_seq;
    scan.sequence_starts  = d_starts;
    scan.max_query_length = longest;
    scan.ends             = d_ends;
    scan.workspace        = scan_workspace.in(ends_block_);
    scan.workspace_bytes  = scan_ws;
    GW_CU_CHECK_ERR(hipEventRecord(events_[0], s));
    if (gwhip_semiglobal_ends(&scan, s) != 0) throw std::runtime_error(gwhip_semiglobal_last_error());
    GW_CU_CHECK_ERR(hipEventRecord(events_[1], s));
    ends_h_.resize(3 * un);
    GW_CU_CHECK_ERR(hipMemcpyAsync(ends_h_.data(), d_ends, 3 * un * 4, hipMemcpyDeviceToHost, s));
    GW_CU_CHECK_ERR(hipStreamSynchronize(s));

    // ---- the pairs whose slice is not empty go to the default global aligner, gathered on the device ----
    sub_starts_h_.assign(1, 0);
    sub_index_h_.clear();
    for (size_t i = 0; i < un; ++i)
    {
        const int64_t qlen = seq_starts_h_[2 * i + 1] - seq_starts_h_[2 * i], tlen = seq_starts_h_[2 * i + 2] - seq_starts_h_[2 * i + 1];
        const int32_t d = ends_h_[3 * i], tb = ends_h_[3 * i + 1], te = ends_h_[3 * i + 2];
        if (d < 0 || d > qlen || tb < 0 || tb > te || te > tlen)
            throw std::runtime_error("semiglobal ends scan: pair " + std::to_string(i) + " reports d = " + std::to_string(d) + ", slice [" +
                                     std::to_string(tb) + ", " + std::to_string(te) + ") of a target of " + std::to_string(tlen));
        if (te == tb) continue;
        const int64_t at = sub_starts_h_.back();
        sub_starts_h_.push_back(at + qlen);
        sub_starts_h_.push_back(at + qlen + (te - tb));
        sub_index_h_.push_back(static_cast<int32_t>(i));
    }
    const int32_t n_sub = static_cast<int32_t>(sub_index_h_.size());
    GW_CU_CHECK_ERR(hipEventRecord(events_[2], s));
    if (n_sub > 0)
    {
        const size_t us         = static_cast<size_t>(n_sub);
        const int64_t sub_total = sub_starts_h_.back();
        const size_t ws_bytes   = gwhip_hirschberg_myers_workspace_bytes(n_sub, sub_starts_h_.data(), max_query_length_);
        gwhost::BlockLayout tb_layout;
        const auto sub_seq    = tb_layout.take<char>(static_cast<size_t>(sub_total) + 16);
        const auto sub_starts = tb_layout.take<int64_t>(2 * us + 1);
        const auto index      = tb_layout.take<int32_t>(us);
        const auto results    = tb_layout.take<int8_t>(static_cast<size_t>(sub_total) + 16);
        const auto lengths    = tb_layout.take<int32_t>(us);
        const auto workspace  = tb_layout.take<char>(ws_bytes);
        tb_block_bytes_    = tb_layout.bytes;
        tb_block_          = allocator_.allocate(tb_block_bytes_, {stream_});
        char* d_sseq       = sub_seq.in(tb_block_);
        int64_t* d_sstarts = sub_starts.in(tb_block_);
        int32_t* d_index   = index.in(tb_block_);
        int8_t* d_results  = results.in(tb_block_);
        int32_t* d_lengths = lengths.in(tb_block_);
        GW_CU_CHECK_ERR(hipMemcpyAsync(d_sstarts, sub_starts_h_.data(), (2 * us + 1) * 8, hipMemcpyHostToDevice, s));
        GW_CU_CHECK_ERR(hipMemcpyAsync(d_index, sub_index_h_.data(), us * 4, hipMemcpyHostToDevice, s));
        if (gwhip_semiglobal_gather(n_sub, d_index, d_seq, d_starts, d_ends, d_sstarts, d_sseq, s) != 0)
            throw std::runtime_error(gwhip_semiglobal_last_error());
        check_gwhip(launch_hirschberg_myers(d_sseq, d_sstarts, n_sub, max_query_length_, d_results, d_lengths, workspace.in(tb_block_), ws_bytes, s));
        GW_CU_CHECK_ERR(hipEventRecord(events_[3], s));
        results_h_.resize(static_cast<size_t>(sub_total) + 16);
        result_lengths_h_.resize(us);
        GW_CU_CHECK_ERR(hipMemcpyAsync(results_h_.data(), d_results, static_cast<size_t>(sub_total), hipMemcpyDeviceToHost, s));
        GW_CU_CHECK_ERR(hipMemcpyAsync(result_lengths_h_.data(), d_lengths, us * 4, hipMemcpyDeviceToHost, s));
    }
    else
        GW_CU_CHECK_ERR(hipEventRecord(events_[3], s));
    launched_ = true;
    timed_    = true;
    return StatusType::success;
}

StatusType AlignerSemiglobal::sync_alignments()
{
    scoped_device_switch dev(device_id_);
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    const size_t n = static_cast<size_t>(num_alignments());
    if (!launched_ || n == 0) return StatusType::success;
    size_t sub = 0; // next gathered pair
    for (size_t i = 0; i < n; ++i)
    {
        const int64_t qlen       = seq_starts_h_[2 * i + 1] - seq_starts_h_[2 * i];
        const int32_t d = ends_h_[3 * i], tb = ends_h_[3 * i + 1], te = ends_h_[3 * i + 2];
        AlignmentImpl* alignment = dynamic_cast<AlignmentImpl*>(alignments_[i].get());
        alignment->set_target_range(tb, te);
        if (te == tb) // nothing of the target is used: every query base is a deletion
        {
            alignment->set_alignment(std::vector<AlignmentState>(static_cast<size_t>(qlen), AlignmentState::deletion), true);
            alignment->set_status(StatusType::success);
            continue;
        }
        const int32_t len     = result_lengths_h_[sub];
        const size_t count    = static_cast<size_t>(std::abs(len));
        const int8_t* r_begin = results_h_.data() + sub_starts_h_[2 * sub];
        ++sub;
        if (count == 0) continue; // the aligner reported nothing for the pair: it stays uninitialized, as for global_alignment
        std::vector<AlignmentState> states = reversed_states(r_begin, count);
        const int32_t edits                = static_cast<int32_t>(count) - static_cast<int32_t>(std::count(states.begin(), states.end(), AlignmentState::match));
        // a negative length is the default aligner's "not optimal": the issue's contract has no such result here
        if (len < 0)
            throw std::runtime_error("semiglobal alignment " + std::to_string(i) + ": the default global aligner reports a non-optimal traceback");
        if (edits != d)
            throw std::runtime_error("semiglobal alignment " + std::to_string(i) + ": the ends scan found distance " + std::to_string(d) +
                                     ", the traceback of its slice has " + std::to_string(edits) + " edits");
        alignment->set_alignment(std::move(states), true);
        alignment->set_status(StatusType::success);
    }
    return StatusType::success;
}

bool AlignerSemiglobal::last_stage_ms(float* ends_ms, float* traceback_ms)
{
    if (!timed_) return false;
    scoped_device_switch dev(device_id_);
    GW_CU_CHECK_ERR(hipEventSynchronize(events_[3]));
    GW_CU_CHECK_ERR(hipEventElapsedTime(ends_ms, events_[0], events_[1]));
    GW_CU_CHECK_ERR(hipEventElapsedTime(traceback_ms, events_[2], events_[3]));
    return true;
}

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
