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

namespace
{
size_t up256(size_t v) { return (v + 255) & ~size_t(255); }
} // namespace

AlignerSemiglobal::AlignerSemiglobal(AlignmentType type, int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                     DefaultDeviceAllocator allocator, cudaStream_t stream, int32_t device_id)
    : type_(type)
    , max_query_length_(throw_on_negative(max_query_length, "max_query_length must be non-negative."))
    , max_target_length_(throw_on_negative(max_target_length, "max_target_length must be non-negative."))
    , max_alignments_(throw_on_negative(max_alignments, "max_alignments must be non-negative."))
    , allocator_(allocator)
    , stream_(stream)
    , device_id_(device_id)
{
    if (type != AlignmentType::infix_alignment && type != AlignmentType::prefix_alignment)
        throw std::invalid_argument("AlignerSemiglobal aligns infix_alignment or prefix_alignment.");
    if (max_alignments < 1) throw std::runtime_error("Max alignments must be at least 1.");
    seq_starts_h_.assign(1, 0);
}

AlignerSemiglobal::~AlignerSemiglobal()
{
    scoped_device_switch dev(device_id_);
    (void)hipStreamSynchronize(stream_);
    free_device();
    for (void* e : events_)
        if (e != nullptr) (void)hipEventDestroy(static_cast<hipEvent_t>(e));
}

void AlignerSemiglobal::free_device()
{
    if (ends_block_ != nullptr) allocator_.deallocate(ends_block_, ends_block_bytes_);
    if (tb_block_ != nullptr) allocator_.deallocate(tb_block_, tb_block_bytes_);
    ends_block_ = tb_block_ = nullptr;
    ends_block_bytes_ = tb_block_bytes_ = 0;
}

StatusType AlignerSemiglobal::add_alignment(const char* query, int32_t query_length, const char* target, int32_t target_length,
                                            bool reverse_complement_query, bool reverse_complement_target)
{
    // limits and their order as AlignerGlobal::add_alignment
    if (query_length < 0 || target_length < 0)
    {
        GW_LOG_DEBUG("Negative target or query length is not allowed.");
        return StatusType::generic_error;
    }
    if (num_alignments() >= max_alignments_) return StatusType::exceeded_max_alignments;
    if (query_length > max_query_length_ || target_length > max_target_length_) return StatusType::exceeded_max_length;
    if (launched_) // the staging arrays are pinned: a batch still in flight reads them by DMA
    {
        scoped_device_switch dev(device_id_);
        GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    }
    const int64_t begin = seq_starts_h_.back();
    seq_h_.resize(static_cast<size_t>(begin + query_length + target_length));
    genomeutils::copy_sequence(query, query_length, seq_h_.data() + begin, reverse_complement_query);
    genomeutils::copy_sequence(target, target_length, seq_h_.data() + begin + query_length, reverse_complement_target);
    seq_starts_h_.push_back(begin + query_length);
    seq_starts_h_.push_back(begin + query_length + target_length);
    auto alignment = std::make_shared<AlignmentImpl>(seq_h_.data() + begin, query_length, seq_h_.data() + begin + query_length, target_length);
    alignment->set_alignment_type(type_);
    alignments_.push_back(std::move(alignment));
    launched_ = false;
    return StatusType::success;
}

StatusType AlignerSemiglobal::align_all()
{
    const int32_t n = num_alignments();
    if (n == 0) return StatusType::success;
    scoped_device_switch dev(device_id_);
    hipStream_t s = stream_;
    for (void*& e : events_)
        if (e == nullptr)
        {
            hipEvent_t fresh = nullptr;
            GW_CU_CHECK_ERR(hipEventCreate(&fresh));
            e = fresh;
        }
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
    size_t off           = 0;
    auto take            = [&](size_t b) { size_t o = off; off += up256(b); return o; };
    const size_t o_seq = take(static_cast<size_t>(total) + 16), o_starts = take((2 * un + 1) * 8), o_ends = take(3 * un * 4), o_ws = take(scan_ws);
    ends_block_bytes_  = off;
    ends_block_        = allocator_.allocate(ends_block_bytes_, {stream_});
    char* d_seq        = ends_block_ + o_seq;
    int64_t* d_starts  = reinterpret_cast<int64_t*>(ends_block_ + o_starts);
    int32_t* d_ends    = reinterpret_cast<int32_t*>(ends_block_ + o_ends);
    GW_CU_CHECK_ERR(hipMemcpyAsync(d_seq, seq_h_.data(), static_cast<size_t>(total), hipMemcpyHostToDevice, s));
    GW_CU_CHECK_ERR(hipMemcpyAsync(d_starts, seq_starts_h_.data(), seq_starts_h_.size() * 8, hipMemcpyHostToDevice, s));
    gwhip_semiglobal_args scan{};
    scan.n_pairs          = n;
    scan.mode             = type_ == AlignmentType::prefix_alignment ? GWHIP_SEMIGLOBAL_PREFIX : GWHIP_SEMIGLOBAL_INFIX;
    scan.sequences        = d_seq;
    scan.sequence_starts  = d_starts;
    scan.max_query_length = longest;
    scan.ends             = d_ends;
    scan.workspace        = ends_block_ + o_ws;
    scan.workspace_bytes  = scan_ws;
    GW_CU_CHECK_ERR(hipEventRecord(static_cast<hipEvent_t>(events_[0]), s));
    if (gwhip_semiglobal_ends(&scan, s) != 0) throw std::runtime_error(gwhip_semiglobal_last_error());
    GW_CU_CHECK_ERR(hipEventRecord(static_cast<hipEvent_t>(events_[1]), s));
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
    GW_CU_CHECK_ERR(hipEventRecord(static_cast<hipEvent_t>(events_[2]), s));
    if (n_sub > 0)
    {
        const size_t us         = static_cast<size_t>(n_sub);
        const int64_t sub_total = sub_starts_h_.back();
        const size_t ws_bytes   = gwhip_hirschberg_myers_workspace_bytes(n_sub, sub_starts_h_.data(), max_query_length_);
        off                     = 0;
        const size_t o_sseq = take(static_cast<size_t>(sub_total) + 16), o_sstarts = take((2 * us + 1) * 8), o_index = take(us * 4);
        const size_t o_res = take(static_cast<size_t>(sub_total) + 16), o_len = take(us * 4), o_hws = take(ws_bytes);
        tb_block_bytes_     = off;
        tb_block_           = allocator_.allocate(tb_block_bytes_, {stream_});
        char* d_sseq        = tb_block_ + o_sseq;
        int64_t* d_sstarts  = reinterpret_cast<int64_t*>(tb_block_ + o_sstarts);
        int32_t* d_index    = reinterpret_cast<int32_t*>(tb_block_ + o_index);
        int8_t* d_results   = reinterpret_cast<int8_t*>(tb_block_ + o_res);
        int32_t* d_lengths  = reinterpret_cast<int32_t*>(tb_block_ + o_len);
        GW_CU_CHECK_ERR(hipMemcpyAsync(d_sstarts, sub_starts_h_.data(), (2 * us + 1) * 8, hipMemcpyHostToDevice, s));
        GW_CU_CHECK_ERR(hipMemcpyAsync(d_index, sub_index_h_.data(), us * 4, hipMemcpyHostToDevice, s));
        if (gwhip_semiglobal_gather(n_sub, d_index, d_seq, d_starts, d_ends, d_sstarts, d_sseq, s) != 0)
            throw std::runtime_error(gwhip_semiglobal_last_error());
        gwhip_hirschberg_args a{};
        a.n_alignments     = n_sub;
        a.sequences        = d_sseq;
        a.sequence_starts  = d_sstarts;
        a.max_query_length = max_query_length_;
        a.results          = d_results;
        a.result_lengths   = d_lengths;
        a.workspace        = tb_block_ + o_hws;
        a.workspace_bytes  = ws_bytes;
        const int rc       = gwhip_hirschberg_myers(&a, s);
        if (rc != 0)
        {
            char buf[512];
            gwhip_last_error_string(buf, sizeof(buf));
            GW_LOG_ERROR(buf);
            GW_CU_CHECK_ERR(static_cast<hipError_t>(rc));
        }
        GW_CU_CHECK_ERR(hipEventRecord(static_cast<hipEvent_t>(events_[3]), s));
        results_h_.resize(static_cast<size_t>(sub_total) + 16);
        result_lengths_h_.resize(us);
        GW_CU_CHECK_ERR(hipMemcpyAsync(results_h_.data(), d_results, static_cast<size_t>(sub_total), hipMemcpyDeviceToHost, s));
        GW_CU_CHECK_ERR(hipMemcpyAsync(result_lengths_h_.data(), d_lengths, us * 4, hipMemcpyDeviceToHost, s));
    }
    else
        GW_CU_CHECK_ERR(hipEventRecord(static_cast<hipEvent_t>(events_[3]), s));
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
        std::vector<AlignmentState> states(count);
        int32_t edits = 0;
        for (size_t k = 0; k < count; ++k) // the device writes a path back to front
        {
            states[k] = static_cast<AlignmentState>(r_begin[count - 1 - k]);
            edits += states[k] != AlignmentState::match;
        }
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
    GW_CU_CHECK_ERR(hipEventSynchronize(static_cast<hipEvent_t>(events_[3])));
    GW_CU_CHECK_ERR(hipEventElapsedTime(ends_ms, static_cast<hipEvent_t>(events_[0]), static_cast<hipEvent_t>(events_[1])));
    GW_CU_CHECK_ERR(hipEventElapsedTime(traceback_ms, static_cast<hipEvent_t>(events_[2]), static_cast<hipEvent_t>(events_[3])));
    return true;
}

void AlignerSemiglobal::reset()
{
    scoped_device_switch dev(device_id_);
    (void)hipStreamSynchronize(stream_);
    alignments_.clear();
    seq_h_.clear();
    seq_starts_h_.assign(1, 0);
    launched_ = false;
    free_device();
}

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
