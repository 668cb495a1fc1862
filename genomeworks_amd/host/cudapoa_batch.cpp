// cudapoa_batch.cpp -- host side of cudapoa::Batch on MI355X.
//
// Behavioural contract (status codes, quirks, error conventions) follows the reference host code:
//   BatchConfig ctors        cudapoa/src/batch.cu:34-104
//   type selection           cudapoa/src/cudapoa_limits.hpp:34-59
//   create_batch             cudapoa/src/batch.cu:107-232
//   CudapoaBatch methods     cudapoa/src/cudapoa_batch.cuh:103-570
// The memory plan is ours: one device block from the allocator = [inputs | outputs | kernel workspace], with
// the workspace layout owned by libgwhip (gwhip_poa_workspace_bytes); one pinned host block for staging.
// All device work goes through the C-ABI in include/gwhip.h.
#include <claraparabricks/genomeworks/cudapoa/batch.hpp>
#include <claraparabricks/genomeworks/cudapoa/cudapoa.hpp>
#include <claraparabricks/genomeworks/logging/logging.hpp>

#include <algorithm>
#include <thread>
#include <atomic>
#include <climits>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <iomanip>
#include <stdexcept>
#include <tuple>

#include "../../include/gwhip.h"
#include "alignment_impl.hpp" // pinned_acquire / pinned_release (the process-wide cache of pinned buffers, runtime.cpp)
#include "host_common.hpp"
#include "owned_hip.hpp"
#include "poa_batch_impl.hpp"

namespace claraparabricks
{
namespace genomeworks
{
namespace cudapoa
{

namespace
{
constexpr int32_t kCellsPerThread = 4;   // CUDAPOA_CELLS_PER_THREAD
constexpr int32_t kMinBandWidth   = 128; // CUDAPOA_MIN_BAND_WIDTH (API constant, not the hardware wave size)
constexpr int32_t kRightPadding   = 8;   // CUDAPOA_BANDED_MATRIX_RIGHT_PADDING
constexpr uint8_t kKernelError    = 0xFF;
std::atomic<int32_t> g_batch_ids{0};     // one process-wide atomic counter (the reference has six racy ones)

std::runtime_error requires_at_least(int64_t bytes)
{
    return std::runtime_error("Requires at least " + std::to_string(bytes) + " bytes of device memory per CUDAPOA batch to process correctly.");
}
} // namespace

StatusType Init()
{
    logging::initialize_logger(logging::LogLevel::warn);
    return StatusType::success;
}

void decode_error(StatusType error_type, std::string& error_message, std::string& error_hint)
{
    struct Text { const char* msg; const char* hint; };
    static const Text table[] = {
        /* success */ {nullptr, nullptr},
        {"Kernel Error: Number of groups per batch exceeded maximum POAs.",
         "Suggestion  : Evaluate maximum number of groups per batch using BatchBlock::estimate_max_poas()."},
        {"Kernel Error: Input read length or output consensus/MSA sequence length exceeded max sequence size.",
         "Suggestion  : Check BatchConfig::max_sequence_size and BatchConfig::max_consensus_size, increase if necessary."},
        {"Kernel Error: Exceeded maximum number of reads per POA.",
         "Suggestion  : Check BatchConfig::max_sequences_per_poa and increase if necessary."},
        {"Kernel Error: Node count exceeded maximum nodes per POA graph.",
         "Suggestion  : Check BatchConfig::max_nodes_per_graph and increase if necessary."},
        {"Kernel Error: Edge count exceeded maximum edges per graph.",
         "Suggestion  : Check default value of CUDAPOA_MAX_NODE_EDGES, note that increasing this macro would increase memory usage per POA."},
        {"Kernel Error: Allocated buffer for score/traceback matrix in adaptive banding is not large enough.",
         "Suggestion  : Check BatchConfig::matrix_sequence_dimension and increase if necessary."},
        {"Kernel Error: Set value for maximum predecessor distance in Needleman-Wunsch algorithm with traceback buffer is not large enough.",
         "Suggestion  : Check BatchConfig::max_banded_pred_distance and increase if necessary."},
        {"Kernel Error: Traceback in Needleman-Wunsch algorithm failed.", "Suggestion  : You may retry with a different banding mode."},
        {"Kernel Error: Output type not available.", "Suggestion  : Check MSA/Consensus selection for output type."},
        {"Error      : Input sequence has all zero base weights.", "Suggestion : Check base weights of POA group sequences on host."},
        {"Error      : No sequence was added to POA group.", "Suggestion : Check status vector in Batch::add_poa_group()."},
        {"Unknown error.", ""},
    };
    const int idx = static_cast<int>(error_type);
    if (idx <= 0 || idx > static_cast<int>(StatusType::generic_error)) throw std::runtime_error("Unknown error type detected.");
    error_message = table[idx].msg;
    error_hint    = table[idx].hint;
}

// ---- BatchConfig (batch.cu:34-104) ----------------------------------------------------------------
BatchConfig::BatchConfig(int32_t max_seq_sz, int32_t max_seq_per_poa, int32_t band_width, BandMode banding,
                         float adapive_storage_factor, float graph_length_factor, int32_t max_pred_dist)
    : max_sequence_size(max_seq_sz)
    , max_consensus_size(2 * max_seq_sz)
    , alignment_band_width(cudautils::align<int32_t, kMinBandWidth>(band_width))
    , max_sequences_per_poa(max_seq_per_poa)
    , band_mode(banding)
    , max_banded_pred_distance(max_pred_dist > 0 ? max_pred_dist : 2 * cudautils::align<int32_t, kMinBandWidth>(band_width))
{
    max_nodes_per_graph = cudautils::align<int32_t, kCellsPerThread>(static_cast<int32_t>(graph_length_factor * max_sequence_size));
    if (banding == BandMode::full_band)
        matrix_sequence_dimension = cudautils::align<int32_t, kCellsPerThread>(max_sequence_size);
    else if (banding == BandMode::static_band || banding == BandMode::static_band_traceback)
        matrix_sequence_dimension = cudautils::align<int32_t, kCellsPerThread>(alignment_band_width + kRightPadding);
    else
        matrix_sequence_dimension =
            cudautils::align<int32_t, kCellsPerThread>(static_cast<int32_t>(adapive_storage_factor * (alignment_band_width + kRightPadding)));

    throw_on_negative(max_seq_sz, "max_sequence_size cannot be negative.");
    throw_on_negative(max_seq_per_poa, "max_sequences_per_poa cannot be negative.");
    throw_on_negative(band_width, "alignment_band_width cannot be negative.");
    throw_on_negative(max_nodes_per_graph, "max_nodes_per_graph cannot be negative.");
    if (alignment_band_width != band_width)
        std::cerr << "Band-width should be multiple of 128. The input was changed from " << band_width << " to "
                  << alignment_band_width << std::endl;
}

BatchConfig::BatchConfig(int32_t max_seq_sz, int32_t max_consensus_sz, int32_t max_nodes_per_poa, int32_t band_width,
                         int32_t max_seq_per_poa, int32_t matrix_seq_dim, BandMode banding, int32_t max_pred_distance)
    : max_sequence_size(max_seq_sz)
    , max_consensus_size(max_consensus_sz)
    , max_nodes_per_graph(cudautils::align<int32_t, kCellsPerThread>(max_nodes_per_poa))
    , matrix_sequence_dimension(cudautils::align<int32_t, kCellsPerThread>(matrix_seq_dim))
    , alignment_band_width(cudautils::align<int32_t, kMinBandWidth>(band_width))
    , max_sequences_per_poa(max_seq_per_poa)
    , band_mode(banding)
    , max_banded_pred_distance(max_pred_distance)
{
    throw_on_negative(max_seq_sz, "max_sequence_size cannot be negative.");
    throw_on_negative(max_consensus_sz, "max_consensus_size cannot be negative.");
    throw_on_negative(max_nodes_per_poa, "max_nodes_per_graph cannot be negative.");
    throw_on_negative(max_seq_per_poa, "max_sequences_per_poa cannot be negative.");
    throw_on_negative(band_width, "alignment_band_width cannot be negative.");
    throw_on_negative(max_pred_distance, "max_banded_pred_distance cannot be negative.");
    if (max_nodes_per_graph < max_sequence_size)
        throw std::invalid_argument("max_nodes_per_graph should be greater than or equal to max_sequence_size.");
    if (max_consensus_size < max_sequence_size)
        throw std::invalid_argument("max_consensus_size should be greater than or equal to max_sequence_size.");
    if (max_sequence_size < alignment_band_width)
        throw std::invalid_argument("alignment_band_width should not be greater than max_sequence_size.");
    if (alignment_band_width != band_width)
        std::cerr << "Band-width should be multiple of 128. The input was changed from " << band_width << " to "
                  << alignment_band_width << std::endl;
}

// ---- type selection (cudapoa_limits.hpp:34-59) ----------------------------------------------------
gwhip_poa_config make_device_config(const BatchConfig& b, int8_t output_mask, int32_t gap, int32_t mismatch, int32_t match)
{
    gwhip_poa_config c{};
    c.max_sequence_size         = b.max_sequence_size;
    c.max_consensus_size        = b.max_consensus_size;
    c.max_nodes_per_graph       = b.max_nodes_per_graph;
    c.matrix_sequence_dimension = b.matrix_sequence_dimension;
    c.alignment_band_width      = b.alignment_band_width;
    c.max_sequences_per_poa     = b.max_sequences_per_poa;
    c.band_mode                 = static_cast<int32_t>(b.band_mode);
    c.max_banded_pred_distance  = b.max_banded_pred_distance;
    c.gap_score                 = gap;
    c.mismatch_score            = mismatch;
    c.match_score               = match;
    c.output_mask               = output_mask;
    const int32_t upper_bound   = b.max_sequence_size * match;
    const int32_t lower_bound   = b.max_sequence_size * std::max(gap, mismatch) + (b.max_nodes_per_graph - b.max_sequence_size) * gap;
    c.score32                   = (upper_bound > INT16_MAX || (-lower_bound) > (INT16_MAX + 1)) ? 1 : 0;
    int32_t max_length          = std::max(std::max(b.max_consensus_size, b.max_nodes_per_graph), b.matrix_sequence_dimension);
    // "if ScoreT is 16-bit, then it's safe to assume SizeT is 16-bit" (batch.cu:173): size32 only with score32
    c.size32                    = (c.score32 && max_length > INT16_MAX) ? 1 : 0;
    c.trace16                   = (b.max_banded_pred_distance > INT8_MAX) ? 1 : 0;
#ifdef SPOA_ACCURATE
    c.spoa_accurate = 1;
#endif
    // the reference selects the racon-style topological order at build time (-Dspoa_accurate=ON, cudapoa_kernels.cuh:
    // 516-531); the kernels here take it as a run-time flag, so one build serves both -- GW_SPOA_ACCURATE=1 turns it on
    if (const char* e = std::getenv("GW_SPOA_ACCURATE")) c.spoa_accurate = (e[0] == '1') ? 1 : c.spoa_accurate;
    return c;
}

// Batch objects alive per device: with more than one, kernels of different batches may share the device
// (gwhip_poa_args::shared_device).
namespace
{
std::atomic<int32_t>& live_batches(int32_t device)
{
    static std::atomic<int32_t> table[64];
    return table[static_cast<uint32_t>(device) & 63u];
}
} // namespace

// ---- PoaBatch ------------------------------------------------------------------------------------------
PoaBatch::PoaBatch(int32_t device_id, cudaStream_t stream, DefaultDeviceAllocator allocator, int64_t max_mem,
                   int8_t output_mask, const BatchConfig& batch_size, int32_t gap_score, int32_t mismatch_score,
                   int32_t match_score)
    : max_sequences_per_poa_(throw_on_negative(batch_size.max_sequences_per_poa, "Maximum sequences per POA has to be non-negative"))
    , device_id_(throw_on_negative(device_id, "Device ID has to be non-negative"))
    , stream_(stream)
    , output_mask_(output_mask)
    , batch_size_(batch_size)
    , allocator_(allocator)
{
    scoped_device_switch dev(device_id_);
    cfg_ = make_device_config(batch_size_, output_mask_, gap_score, mismatch_score, match_score);
    bid_ = g_batch_ids++;

    // capacity: max_poas = avail / (per_poa + per_matrix)  (allocate_block.hpp:64-89, with our byte counts)
    int64_t per_poa = 0, per_matrix = 0;
    gwhip_poa_bytes_per_window(&cfg_, &per_poa, &per_matrix);
    const int64_t avail_mem = std::min(get_size_of_largest_free_memory_block(allocator_), max_mem);
    const int64_t minimum   = per_poa + per_matrix;
    if (avail_mem < minimum) throw requires_at_least(minimum);
    int64_t guess = std::min<int64_t>(avail_mem / (per_poa + per_matrix), INT32_MAX);
    // window_details.seq_starts and the host write offset are int32 (as in the reference, cudapoa_batch.cuh:456-537): a
    // 288 GB device could otherwise hold more input bases than they can index
    const int64_t per_poa_input = std::max<int64_t>(1, static_cast<int64_t>(max_sequences_per_poa_) *
                                                           cudautils::align<int32_t, 4>(batch_size_.max_sequence_size));
    guess     = std::min<int64_t>(guess, (static_cast<int64_t>(INT32_MAX) - 8192) / per_poa_input);
    max_poas_ = static_cast<int32_t>(std::max<int64_t>(guess, 1));
    while (max_poas_ > 1 && static_cast<int64_t>(plan(max_poas_).block.bytes) > avail_mem) max_poas_--;
    layout_ = plan(max_poas_);
    if (static_cast<int64_t>(layout_.block.bytes) > avail_mem) throw requires_at_least(static_cast<int64_t>(layout_.block.bytes));
    score_buffer_bytes_ = static_cast<size_t>(per_matrix) * static_cast<size_t>(max_poas_);
    workspace_bytes_    = gwhip_poa_workspace_bytes(&cfg_, max_poas_, 0);
    device_block_       = allocator_.allocate(layout_.block.bytes, {stream_});
    d_                  = layout_.in(device_block_);
    input_capacity_     = layout_.sequence_bytes - 4096;
    // the kernels read up to 2 KiB past a read (never consumed): keep that slack zero
    GW_CU_CHECK_ERR(hipMemsetAsync(d_.sequences, 0, layout_.sequence_bytes, stream_));
    GW_CU_CHECK_ERR(hipMemsetAsync(d_.weights, 0, layout_.sequence_bytes, stream_));
    GW_CU_CHECK_ERR(hipMemsetAsync(d_.work_counters, 0, 256, stream_)); // (a launch leaves them at zero again)

    // the pinned staging block: the device block without the workspace, from the process-wide cache of pinned buffers
    // (runtime.cpp): pinning and unpinning 1.2 GB took 200 and 100 ms of every construction and destruction of a
    // BatchConfig(1024, 200) batch with 32 GB of device memory
    host_block_ = cudaaligner::pinned_acquire(layout_.workspace.offset, &host_block_capacity_);
    h_          = layout_.in(host_block_);
    // (the staging arrays are not cleared: an upload covers exactly the bytes add_seq_to_poa() wrote, padding included, and
    // the read-ahead slack is zeroed where the kernel reads it, per launch -- clearing 2 x 600 MB of pinned memory was most of the construction time of
    // a BatchConfig(1024, 200) batch with tens of GB of device memory)

    // Where the graph-build kernel copies every read into LDS once, it can take the reads from this block itself and the
    // upload, a pass over memory with the device idle behind it, falls away (generate_poa()). The block is mapped for the
    // device when it is the runtime's pinned memory.
    if (gwhip_poa_reads_host_sequences(&cfg_) != 0)
    {
        void* mapped = nullptr;
        if (hipHostGetDevicePointer(&mapped, h_.sequences, 0) == hipSuccess)
            host_sequences_dev_ = static_cast<const uint8_t*>(mapped);
        else
            (void)hipGetLastError();
    }

    live_batches(device_id_).fetch_add(1);
    debug_message(" Initializing batch on device ");
    reset();
}

PoaBatch::~PoaBatch()
{
    debug_message(" Destroyed buffers on device ");
    scoped_device_switch dev(device_id_);
    // a launch in flight may still read the pinned block, which pinned_release() can hand to another batch or give back to the
    // system: the stream first, then the launch's own event (a stream that failed to synchronise does not skip it)
    (void)hipStreamSynchronize(stream_);
    if (host_reads_pending_) (void)hipEventSynchronize(static_cast<hipEvent_t>(host_reads_done_));
    host_reads_pending_ = false;
    if (host_reads_done_ != nullptr) (void)hipEventDestroy(static_cast<hipEvent_t>(host_reads_done_));
    live_batches(device_id_).fetch_sub(1);
    if (host_block_ != nullptr) cudaaligner::pinned_release(host_block_, host_block_capacity_);
    if (device_block_ != nullptr) allocator_.deallocate(device_block_, layout_.block.bytes);
}

void PoaBatch::debug_message(const std::string& message)
{
    std::string msg = std::string(static_cast<size_t>(bid_), '\t') + " " + std::to_string(bid_) + " " + message + " " + std::to_string(device_id_);
    GW_LOG_DEBUG(msg.c_str());
}

// The device block of a batch of n windows.
PoaBlockLayout PoaBatch::plan(int32_t n_poas) const
{
    const size_t n     = static_cast<size_t>(n_poas);
    const size_t reads = n * static_cast<size_t>(max_sequences_per_poa_);
    const size_t rows  = n * static_cast<size_t>(batch_size_.max_consensus_size);
    PoaBlockLayout l;
    // every read is padded to a multiple of 4 bytes (add_seq_to_poa)
    l.sequences      = l.block.take<uint8_t>(reads * static_cast<size_t>(cudautils::align<int32_t, 4>(batch_size_.max_sequence_size)) + 4096);
    l.sequence_bytes = l.block.bytes;
    l.weights        = l.block.take<int8_t>(l.sequence_bytes);
    l.lengths        = l.block.take<int32_t>(reads);
    l.windows        = l.block.take<gwhip_window_details>(n);
    l.consensus      = l.block.take<uint8_t>(rows);
    l.coverage       = l.block.take<uint16_t>(rows);
    l.has_msa        = (output_mask_ & OutputType::msa) != 0;
    l.msa            = l.block.take<uint8_t>(l.has_msa ? rows * static_cast<size_t>(max_sequences_per_poa_) : 0);
    l.cells          = l.block.take<uint64_t>(n);
    l.work_counters  = l.block.take<uint32_t>(64); // the two work counters of a persistent launch (gwhip_poa_args::work_counters)
    l.workspace      = l.block.take<char>(gwhip_poa_workspace_bytes(&cfg_, n_poas, 0));
    return l;
}

// A host-input launch reads h_.sequences until its graph-build kernel ends (and the copies in front of it read the other
// staging arrays): whoever rewrites the pinned block, or gives it back, waits for the event recorded behind that kernel first.
// It costs nothing once the results of the launch were fetched.
void PoaBatch::wait_for_host_reads()
{
    if (!host_reads_pending_) return;
    GW_CU_CHECK_ERR(hipEventSynchronize(static_cast<hipEvent_t>(host_reads_done_)));
    host_reads_pending_ = false;
}

void PoaBatch::reset()
{
    wait_for_host_reads();
    device_sequences_current_ = false;
    poa_count_              = 0;
    num_nucleotides_copied_ = 0;
    global_sequence_idx_    = 0;
    next_scores_offset_     = 0;
    avail_buf_mem_          = score_buffer_bytes_;
    unit_weights_only_      = true;
}

// reserve_buf, cudapoa_batch.cuh:545-570
bool PoaBatch::reserve_buf(int32_t max_seq_length)
{
    const int32_t matrix_height = batch_size_.max_nodes_per_graph;
    const int32_t matrix_width  = (batch_size_.band_mode != BandMode::full_band)
                                      ? batch_size_.matrix_sequence_dimension
                                      : cudautils::align<int32_t, 4>(max_seq_length + 1 + kCellsPerThread);
    size_t required_size        = static_cast<size_t>(matrix_width) * static_cast<size_t>(matrix_height);
    const bool tb               = batch_size_.band_mode == static_band_traceback || batch_size_.band_mode == adaptive_band_traceback;
    // (full band with int16 scores: + one move byte per cell, as gwhip_poa_bytes_per_window counts it)
    required_size *= tb ? (cfg_.trace16 ? 2 : 1) : (cfg_.score32 ? 4 : (batch_size_.band_mode == BandMode::full_band ? 3 : 2));
    if (required_size > avail_buf_mem_)
    {
        if (get_total_poas() == 0)
        {
            std::cout << "Memory available " << std::fixed << std::setprecision(2)
                      << (static_cast<double>(avail_buf_mem_)) / 1024. / 1024. / 1024.;
            std::cout << "GB, Memory required " << (static_cast<double>(required_size)) / 1024. / 1024. / 1024.;
            std::cout << "GB (sequence length " << max_seq_length << ", graph length " << matrix_height << ")" << std::endl;
        }
        return false;
    }
    avail_buf_mem_ -= required_size;
    return true;
}

// add_poa, cudapoa_batch.cuh:456-472 (poa_count_ is bumped before any sequence is accepted: reference quirk kept)
StatusType PoaBatch::add_poa()
{
    if (poa_count_ == max_poas_) return StatusType::exceeded_maximum_poas;
    gwhip_window_details wd{};
    wd.seq_len_buffer_offset = global_sequence_idx_;
    wd.seq_starts            = num_nucleotides_copied_;
    wd.scores_width          = 0;
    wd.scores_offset         = next_scores_offset_;
    h_.windows[poa_count_]   = wd;
    poa_count_++;
    return StatusType::success;
}

// add_seq_to_poa, cudapoa_batch.cuh:475-542
StatusType PoaBatch::add_seq_to_poa(const char* seq, const int8_t* weights, int32_t seq_len)
{
    if (seq_len > batch_size_.max_sequence_size) return StatusType::exceeded_maximum_sequence_size;
    if (weights != nullptr)
    {
        bool all_zero = true;
        for (int32_t i = 0; i < seq_len; i++)
        {
            throw_on_negative(weights[i], "Base weights need to be non-negative");
            if (weights[i] > 0) all_zero = false;
        }
        if (all_zero) return StatusType::zero_weighted_poa_sequence;
    }
    gwhip_window_details* wd = &h_.windows[poa_count_ - 1];
    const int32_t scores_width = cudautils::align<int32_t, 4>(seq_len + 1 + kCellsPerThread);
    if (scores_width > wd->scores_width)
    {
        next_scores_offset_ += static_cast<size_t>(scores_width - wd->scores_width);
        wd->scores_width = scores_width;
    }
    if (static_cast<int32_t>(wd->num_seqs) >= max_sequences_per_poa_) return StatusType::exceeded_maximum_sequences_per_poa;
    wd->num_seqs++;
    std::memcpy(&h_.sequences[num_nucleotides_copied_], seq, static_cast<size_t>(seq_len));
    if (weights == nullptr)
        std::memset(&h_.weights[num_nucleotides_copied_], 1, static_cast<size_t>(seq_len));
    else
    {
        std::memcpy(&h_.weights[num_nucleotides_copied_], weights, static_cast<size_t>(seq_len));
        unit_weights_only_ = false;
    }
    // padding to the 4-byte boundary: the reference leaves stale bytes there; we zero them (never consumed)
    const int32_t padded = cudautils::align<int32_t, 4>(seq_len);
    for (int32_t i = seq_len; i < padded; i++)
    {
        h_.sequences[num_nucleotides_copied_ + i] = 0;
        h_.weights[num_nucleotides_copied_ + i]   = 0;
    }
    h_.lengths[global_sequence_idx_] = seq_len;
    num_nucleotides_copied_ += padded;
    global_sequence_idx_++;
    return StatusType::success;
}

StatusType PoaBatch::add_poa_group(std::vector<StatusType>& per_seq_status, const Group& poa_group)
{
    // The reference dereferences max_element of an empty group (UB, cudapoa_batch.cuh:108-113); we report it.
    if (poa_group.empty())
    {
        per_seq_status.clear();
        return StatusType::empty_poa_group;
    }
    const auto longest = std::max_element(poa_group.begin(), poa_group.end(),
                                          [](const Entry& a, const Entry& b) { return a.length < b.length; });
    // input bytes this group can take (reads that will be rejected are counted too: an upper bound)
    {
        int64_t bytes = 0;
        int32_t taken = 0;
        for (const auto& entry : poa_group)
            if (entry.length <= batch_size_.max_sequence_size && taken < max_sequences_per_poa_)
            {
                bytes += cudautils::align<int32_t, 4>(entry.length);
                taken++;
            }
        if (static_cast<int64_t>(num_nucleotides_copied_) + bytes > static_cast<int64_t>(input_capacity_)) return StatusType::exceeded_maximum_poas;
    }
    if (!reserve_buf(longest->length)) return StatusType::exceeded_maximum_poas;
    per_seq_status.clear();
    wait_for_host_reads(); // a refill behind a launch: the kernel may still be reading the block this group is written to
    device_sequences_current_ = false;
    StatusType status = add_poa();
    if (status != StatusType::success) return status;
    bool poa_empty = true;
    for (const auto& entry : poa_group)
    {
        StatusType entry_status = add_seq_to_poa(entry.seq, entry.weights, entry.length);
        if (entry_status == StatusType::success) poa_empty = false;
        per_seq_status.push_back(entry_status);
    }
    return poa_empty ? StatusType::empty_poa_group : StatusType::success;
}

gwhip_poa_args PoaBatch::kernel_args() const
{
    gwhip_poa_args a{};
    a.cfg              = cfg_;
    a.total_windows    = poa_count_;
    a.sequences        = d_.sequences;
    a.base_weights     = d_.weights;
    a.sequence_lengths = d_.lengths;
    a.window_details   = d_.windows;
    a.consensus        = d_.consensus;
    a.coverage         = d_.coverage;
    a.msa              = d_.msa;
    a.workspace        = layout_.workspace.in(device_block_);
    a.workspace_bytes  = workspace_bytes_;
    a.cells            = d_.cells;
    a.work_counters    = d_.work_counters;
    a.shared_device    = live_batches(device_id_).load(std::memory_order_relaxed) > 1 ? 1 : 0;
    return a;
}

// GW_POA_HOST_INPUT=0 (read per call: the same-binary A/B arm) keeps the upload.
bool PoaBatch::use_host_input() const
{
    if (host_sequences_dev_ == nullptr) return false;
    const char* e = std::getenv("GW_POA_HOST_INPUT");
    return !(e != nullptr && e[0] == '0');
}

void PoaBatch::upload_sequences()
{
    GW_CU_CHECK_ERR(hipMemcpyAsync(d_.sequences, h_.sequences, static_cast<size_t>(num_nucleotides_copied_), hipMemcpyHostToDevice, stream_));
    // zero the 2 KiB read-ahead slack behind the last read (it may hold an older batch's bases)
    GW_CU_CHECK_ERR(hipMemsetAsync(d_.sequences + num_nucleotides_copied_, 0, 2048, stream_));
    device_sequences_current_ = true;
}

void PoaBatch::ensure_resident_sequences()
{
    if (!device_sequences_current_) upload_sequences();
}

void PoaBatch::upload_inputs(bool host_input)
{
    if (!host_input)
        GW_CU_CHECK_ERR(hipMemcpyAsync(d_.sequences, h_.sequences, static_cast<size_t>(num_nucleotides_copied_), hipMemcpyHostToDevice, stream_));
    // a batch whose reads all came without base weights (the common case, and the benchmark's) needs no weight upload:
    // every consumed byte is 1 (padding bytes are never read), so the device array is filled in place
    if (unit_weights_only_)
        GW_CU_CHECK_ERR(hipMemsetAsync(d_.weights, 1, static_cast<size_t>(num_nucleotides_copied_), stream_));
    else
        GW_CU_CHECK_ERR(hipMemcpyAsync(d_.weights, h_.weights, static_cast<size_t>(num_nucleotides_copied_), hipMemcpyHostToDevice, stream_));
    // zero the 2 KiB read-ahead slack behind the last read (it may hold an older batch's bases): where the kernel will read
    if (!host_input)
    {
        GW_CU_CHECK_ERR(hipMemsetAsync(d_.sequences + num_nucleotides_copied_, 0, 2048, stream_));
        device_sequences_current_ = true;
    }
    else
        std::memset(h_.sequences + num_nucleotides_copied_, 0, 2048);
    GW_CU_CHECK_ERR(hipMemcpyAsync(d_.windows, h_.windows, static_cast<size_t>(poa_count_) * sizeof(gwhip_window_details), hipMemcpyHostToDevice, stream_));
    restore_lengths();
}

// sequence_lengths[first read of each window] is overwritten with the node count by a launch
void PoaBatch::restore_lengths()
{
    GW_CU_CHECK_ERR(hipMemcpyAsync(d_.lengths, h_.lengths, static_cast<size_t>(global_sequence_idx_) * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
}

void PoaBatch::launch(void* event_after_graph_build, uint64_t* phase_cycles, const uint8_t* sequences)
{
    gwhip_poa_args a          = kernel_args();
    if (sequences != nullptr) a.sequences = sequences;
    a.event_after_graph_build = event_after_graph_build;
    a.phase_cycles            = phase_cycles;
    // (A launch gate that kept concurrent batches from overlapping on the device beyond one wavefront per SIMD was built and
    // measured in round 6 -- it loses: 2048 windows over four batches 154 ms gated, 108-126 ms with the launches left to the
    // hardware; what did matter is the size of a fill, host/multi_device.cpp.)
    const int rc     = gwhip_poa_generate(&a, stream_);
    if (rc != 0)
    {
        char buf[512];
        gwhip_last_error_string(buf, sizeof(buf));
        GW_LOG_ERROR(buf);
        GW_CU_CHECK_ERR(static_cast<hipError_t>(rc));
    }
}

void PoaBatch::generate_poa()
{
    scoped_device_switch dev(device_id_);
    if (poa_count_ == 0)
    {
        debug_message(" No POA was added to compute! ");
        return;
    }
    // Host input: no sequence H2D -- the graph-build kernel fetches every read from the pinned block when it stages it in LDS
    // (the block's device address; gwhip_poa_reads_host_sequences). The block then belongs to the kernel until the event
    // recorded behind it has passed (wait_for_host_reads()).
    const bool host_input    = use_host_input();
    last_generate_read_host_ = host_input;
    if (host_input)
    {
        wait_for_host_reads(); // (a second launch of the same fill: the slack below is rewritten)
        if (host_reads_done_ == nullptr)
        {
            hipEvent_t e = nullptr;
            GW_CU_CHECK_ERR(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            host_reads_done_ = e;
        }
    }
    upload_inputs(host_input);
    debug_message(" Launching kernel for " + std::to_string(poa_count_) + " on device ");
    if (host_input)
    {
        host_reads_pending_ = true; // (before the call: whatever it enqueued before failing may read the block)
        launch(host_reads_done_, nullptr, host_sequences_dev_);
    }
    else
        launch();
    debug_message(" Launched kernel on device ");
}

void PoaBatch::relaunch_resident()
{
    scoped_device_switch dev(device_id_);
    if (poa_count_ == 0) return;
    ensure_resident_sequences();
    restore_lengths();
    launch();
}

void PoaBatch::relaunch_resident_timed(float* graph_build_ms, float* output_ms)
{
    scoped_device_switch dev(device_id_);
    if (poa_count_ == 0) return;
    gwhost::OwnedEvents events;
    const hipEvent_t e0 = events.create(hipEventDefault), e1 = events.create(hipEventDefault), e2 = events.create(hipEventDefault);
    ensure_resident_sequences();
    restore_lengths();
    GW_CU_CHECK_ERR(hipEventRecord(e0, stream_));
    launch(e1);
    GW_CU_CHECK_ERR(hipEventRecord(e2, stream_));
    GW_CU_CHECK_ERR(hipEventSynchronize(e2));
    GW_CU_CHECK_ERR(hipEventElapsedTime(graph_build_ms, e0, e1));
    GW_CU_CHECK_ERR(hipEventElapsedTime(output_ms, e1, e2));
}

void PoaBatch::profile_phases(double out[6])
{
    for (int k = 0; k < 6; k++) out[k] = 0;
    if (poa_count_ == 0) return;
    std::vector<uint64_t> h;
    profile_phases_per_window(h);
    for (size_t i = 0; i < h.size(); i++) out[i % 6] += static_cast<double>(h[i]);
    for (int k = 0; k < 6; k++) out[k] /= poa_count_;
}

void PoaBatch::profile_phases_per_window(std::vector<uint64_t>& ticks)
{
    scoped_device_switch dev(device_id_);
    const size_t n = static_cast<size_t>(poa_count_) * 6;
    ticks.assign(n, 0);
    if (n == 0) return;
    uint64_t* d = nullptr;
    GW_CU_CHECK_ERR(hipMalloc(reinterpret_cast<void**>(&d), n * sizeof(uint64_t)));
    ensure_resident_sequences();
    restore_lengths();
    launch(nullptr, d);
    GW_CU_CHECK_ERR(hipMemcpyAsync(ticks.data(), d, n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    GW_CU_CHECK_ERR(hipFree(d));
}

void PoaBatch::log_kernel_error(StatusType error_type)
{
    std::string message, hint;
    decode_error(error_type, message, hint);
    message += " in batch " + std::to_string(bid_) + "\n" + hint;
    GW_LOG_WARN(message.c_str());
}

void PoaBatch::log_failed_windows(const StatusType* status, size_t count)
{
    for (size_t poa = 0; poa < count; poa++)
        if (status[poa] != StatusType::success) log_kernel_error(status[poa]);
}

// The kernels write consensus and coverage back to front, as the reference's do (cudapoa_generate_consensus.cuh:245-283),
// and mark a failed window with 0xFF and its status code at the start of its consensus row.
StatusType PoaBatch::window_status(size_t poa) const
{
    const uint8_t* c = &h_.consensus[poa * static_cast<size_t>(batch_size_.max_consensus_size)];
    return c[0] == kKernelError ? static_cast<StatusType>(c[1]) : StatusType::success;
}

// D2H of consensus + coverage, then un-reversal into count = poa_count_ slots (strings / vectors whose storage is reused
// when they have any); statuses of failed windows are logged in window order.
void PoaBatch::fetch_consensus(std::string* consensus, std::vector<uint16_t>* coverage, StatusType* output_status, bool presize)
{
    scoped_device_switch dev(device_id_);
    // D2H of the windows actually in the batch (the reference copies the whole capacity: SURVEY Appendix C.4). The two
    // arrays are neighbours on both sides with the same spacing: one copy when the unused tail of the first is small.
    const size_t n        = static_cast<size_t>(poa_count_) * batch_size_.max_consensus_size;
    const size_t cons_cap = layout_.coverage.offset - layout_.consensus.offset; // (on both sides: PoaBlockLayout)
    if (n > 0)
    {
        if (cons_cap - n <= n / 4)
            GW_CU_CHECK_ERR(hipMemcpyAsync(h_.consensus, d_.consensus, cons_cap + n * sizeof(uint16_t), hipMemcpyDeviceToHost, stream_));
        else
        {
            GW_CU_CHECK_ERR(hipMemcpyAsync(h_.consensus, d_.consensus, n, hipMemcpyDeviceToHost, stream_));
            GW_CU_CHECK_ERR(hipMemcpyAsync(h_.coverage, d_.coverage, n * sizeof(uint16_t), hipMemcpyDeviceToHost, stream_));
        }
    }
    const size_t count = static_cast<size_t>(poa_count_);
    const size_t row   = static_cast<size_t>(batch_size_.max_consensus_size);
    if (presize)
    {
        // Fresh (empty) strings and vectors of the caller: their heap blocks are requested NOW, while the kernels and the
        // copies above are still in flight and this thread would only wait -- a consensus is about as long as the window's
        // longest read (an estimate: the resize below corrects it either way).
        for (size_t poa = 0; poa < count; poa++)
        {
            const gwhip_window_details& wd = h_.windows[poa];
            int32_t longest = 0;
            for (int32_t k = 0; k < static_cast<int32_t>(wd.num_seqs); k++) longest = std::max(longest, h_.lengths[wd.seq_len_buffer_offset + k]);
            const size_t hint = std::min(row, static_cast<size_t>(longest) + static_cast<size_t>(longest) / 16 + 16);
            consensus[poa].reserve(hint);
            coverage[poa].reserve(hint);
        }
    }
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    // The staging block is pinned memory, which the host reads slowly (measured: 3 GB/s in 8-byte steps from the far end of a
    // row, 5 GB/s with memcpy): a row goes to a small cached buffer in one forward memcpy and is reversed from there.
    constexpr size_t kLocalRow = 4096;
    auto unpack = [&](size_t first, size_t last) {
        alignas(64) char local_c[kLocalRow];
        alignas(64) uint16_t local_v[kLocalRow];
        for (size_t poa = first; poa < last; poa++)
        {
            const char* c      = reinterpret_cast<const char*>(&h_.consensus[poa * row]);
            const uint16_t* cv = &h_.coverage[poa * row];
            output_status[poa] = window_status(poa);
            if (output_status[poa] != StatusType::success) // logged below, in window order
            {
                consensus[poa].clear();
                coverage[poa].clear();
                continue;
            }
            size_t len;
            if (row <= kLocalRow)
            {
                std::memcpy(local_c, c, row);
                len = ::strnlen(local_c, row);
                std::memcpy(local_v, cv, len * sizeof(uint16_t));
                c  = local_c;
                cv = local_v;
            }
            else
                len = ::strnlen(c, row);
            consensus[poa].resize(len);
            gwhost::reverse_bytes(&consensus[poa][0], c, len);
            coverage[poa].resize(len);
            gwhost::reverse_u16(coverage[poa].data(), cv, len);
        }
    };
    // the windows are independent: 16 at a time on the library's worker pool
    constexpr size_t kPerTask = 16;
    gwhost::parallel_tasks((count + kPerTask - 1) / kPerTask, count >= 256 ? 8 : 1,
                           [&](size_t t) { unpack(t * kPerTask, std::min(count, (t + 1) * kPerTask)); });
    log_failed_windows(output_status, count);
}

StatusType PoaBatch::get_consensus(std::vector<std::string>& consensus, std::vector<std::vector<uint16_t>>& coverage,
                                   std::vector<StatusType>& output_status)
{
    if (!(OutputType::consensus & output_mask_)) return StatusType::output_type_unavailable;
    // the results are appended behind whatever the caller's vectors already hold, as in the reference (cudapoa_batch.cuh:186-249)
    const size_t base_c = consensus.size(), base_v = coverage.size(), base_s = output_status.size();
    const size_t count  = static_cast<size_t>(poa_count_);
    consensus.resize(base_c + count);
    coverage.resize(base_v + count);
    output_status.resize(base_s + count, StatusType::success);
    fetch_consensus(consensus.data() + base_c, coverage.data() + base_v, output_status.data() + base_s, true);
    return StatusType::success;
}

StatusType PoaBatch::get_consensus_in_place(std::vector<std::string>& consensus, std::vector<std::vector<uint16_t>>& coverage,
                                            std::vector<StatusType>& output_status)
{
    if (!(OutputType::consensus & output_mask_)) return StatusType::output_type_unavailable;
    const size_t count = static_cast<size_t>(poa_count_);
    consensus.resize(count); // strings and vectors of an earlier call keep their storage
    coverage.resize(count);
    output_status.resize(count);
    fetch_consensus(consensus.data(), coverage.data(), output_status.data(), false);
    return StatusType::success;
}

StatusType PoaBatch::get_msa(std::vector<std::vector<std::string>>& msa, std::vector<StatusType>& output_status)
{
    if (!(OutputType::msa & output_mask_)) return StatusType::output_type_unavailable;
    scoped_device_switch dev(device_id_);
    const size_t row = static_cast<size_t>(batch_size_.max_consensus_size);
    if (poa_count_ > 0)
    {
        GW_CU_CHECK_ERR(hipMemcpyAsync(h_.msa, d_.msa, static_cast<size_t>(poa_count_) * max_sequences_per_poa_ * row, hipMemcpyDeviceToHost, stream_));
        GW_CU_CHECK_ERR(hipMemcpyAsync(h_.consensus, d_.consensus, static_cast<size_t>(poa_count_) * row, hipMemcpyDeviceToHost, stream_));
    }
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    // rows are unpacked behind whatever the caller's vectors already hold; long-read MSAs are hundreds of megabytes of
    // rows, so the windows are split over a few host threads (statuses are logged afterwards, in window order)
    const size_t base_m = msa.size(), base_s = output_status.size();
    const size_t count  = static_cast<size_t>(poa_count_);
    msa.resize(base_m + count);
    output_status.resize(base_s + count, StatusType::success);
    auto unpack = [&](size_t first, size_t last) {
        for (size_t poa = first; poa < last; poa++)
        {
            output_status[base_s + poa] = window_status(poa);
            if (output_status[base_s + poa] != StatusType::success) continue;
            const uint16_t num_seqs = h_.windows[poa].num_seqs;
            std::vector<std::string>& rows = msa[base_m + poa];
            rows.reserve(num_seqs);
            for (int32_t i = 0; i < num_seqs; i++)
                rows.emplace_back(reinterpret_cast<const char*>(&h_.msa[(poa * max_sequences_per_poa_ + static_cast<size_t>(i)) * row]));
        }
    };
    // long-read MSAs are hundreds of megabytes of rows: the windows go over the library's worker pool in chunks (joined and
    // exception-safe: a bad_alloc in one chunk is rethrown here once every chunk has finished)
    const size_t bytes     = count * static_cast<size_t>(max_sequences_per_poa_) * row;
    const size_t n_threads = bytes >= (size_t(8) << 20) ? std::min<size_t>(8, std::max<size_t>(1, count)) : 1;
    const size_t per_task  = std::max<size_t>(1, (count + 4 * n_threads - 1) / (4 * n_threads));
    gwhost::parallel_tasks((count + per_task - 1) / per_task, n_threads,
                           [&](size_t t) { unpack(t * per_task, std::min(count, (t + 1) * per_task)); });
    log_failed_windows(output_status.data() + base_s, count);
    return StatusType::success;
}

void PoaBatch::get_graphs(std::vector<DirectedGraph>& graphs, std::vector<StatusType>& output_status)
{
    scoped_device_switch dev(device_id_);
    graphs.resize(poa_count_);
    if (poa_count_ == 0) return;
    const size_t mn = static_cast<size_t>(batch_size_.max_nodes_per_graph);
    const size_t W  = static_cast<size_t>(poa_count_);
    const auto up   = gwhost::up256;
    // Temporaries in the reference's array layout (303 bytes per node slot), filled by the export kernel. The batch's
    // pool is normally fully committed to the batch block, so they come straight from the runtime -- in chunks of
    // windows of at most ~1 GiB, so that a batch filled to device capacity can still be exported.
    const size_t per_window   = mn * (1 + 2 + GWHIP_MAX_NODE_EDGES * (4 + 2)) + 4 * 256;
    size_t chunk_budget       = size_t(1) << 30;
    if (const char* e = std::getenv("GW_GRAPH_EXPORT_CHUNK_BYTES")) chunk_budget = std::max<size_t>(1, std::strtoull(e, nullptr, 10)); // tests
    const size_t chunk        = std::max<size_t>(1, std::min(W, chunk_budget / per_window));
    const size_t b_nodes = chunk * mn, b_cnt = chunk * mn * 2, b_edges = chunk * mn * GWHIP_MAX_NODE_EDGES * 4, b_w = chunk * mn * GWHIP_MAX_NODE_EDGES * 2;
    const size_t total = up(b_nodes) + up(b_cnt) + up(b_edges) + up(b_w);
    char* d_tmp = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d_tmp), total) != hipSuccess)
    {
        (void)hipGetLastError();
        throw device_memory_allocation_exception();
    }
    uint8_t* d_nodes   = reinterpret_cast<uint8_t*>(d_tmp);
    uint16_t* d_cnt    = reinterpret_cast<uint16_t*>(d_tmp + up(b_nodes));
    int32_t* d_edges   = reinterpret_cast<int32_t*>(d_tmp + up(b_nodes) + up(b_cnt));
    uint16_t* d_w      = reinterpret_cast<uint16_t*>(d_tmp + up(b_nodes) + up(b_cnt) + up(b_edges));
    gwhip_poa_args a   = kernel_args();
    std::vector<uint8_t> nodes(b_nodes);
    std::vector<uint16_t> cnt(chunk * mn), w(chunk * mn * GWHIP_MAX_NODE_EDGES);
    std::vector<int32_t> edges(chunk * mn * GWHIP_MAX_NODE_EDGES);
    std::vector<int32_t> lens(static_cast<size_t>(global_sequence_idx_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(lens.data(), d_.lengths, lens.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    GW_CU_CHECK_ERR(hipMemcpyAsync(h_.consensus, d_.consensus, W * batch_size_.max_consensus_size, hipMemcpyDeviceToHost, stream_));
    for (size_t first = 0; first < W; first += chunk)
    {
        const size_t n_here = std::min(chunk, W - first);
        const int rc = gwhip_poa_export_graphs_range(&a, static_cast<int32_t>(first), static_cast<int32_t>(n_here), d_nodes, d_edges,
                                                     d_w, d_cnt, nullptr, nullptr, stream_);
        if (rc != 0)
        {
            (void)hipFree(d_tmp);
            GW_CU_CHECK_ERR(static_cast<hipError_t>(rc));
        }
        GW_CU_CHECK_ERR(hipMemcpyAsync(nodes.data(), d_nodes, n_here * mn, hipMemcpyDeviceToHost, stream_));
        GW_CU_CHECK_ERR(hipMemcpyAsync(cnt.data(), d_cnt, n_here * mn * 2, hipMemcpyDeviceToHost, stream_));
        GW_CU_CHECK_ERR(hipMemcpyAsync(edges.data(), d_edges, n_here * mn * GWHIP_MAX_NODE_EDGES * 4, hipMemcpyDeviceToHost, stream_));
        GW_CU_CHECK_ERR(hipMemcpyAsync(w.data(), d_w, n_here * mn * GWHIP_MAX_NODE_EDGES * 2, hipMemcpyDeviceToHost, stream_));
        GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
        for (size_t k = 0; k < n_here; k++)
        {
            const size_t poa = first + k;
            output_status.emplace_back(window_status(poa));
            if (output_status.back() != StatusType::success)
            {
                log_kernel_error(output_status.back());
                continue;
            }
            DirectedGraph& graph    = graphs[poa];
            const int32_t num_nodes = lens[static_cast<size_t>(h_.windows[poa].seq_len_buffer_offset)];
            for (int32_t n = 0; n < num_nodes; n++)
            {
                graph.set_node_label(n, std::string(1, static_cast<char>(nodes[k * mn + n])));
                const uint16_t ne = cnt[k * mn + n];
                for (int32_t e = 0; e < ne; e++)
                {
                    const size_t idx = (k * mn + n) * GWHIP_MAX_NODE_EDGES + e;
                    graph.add_edge(edges[idx], n, w[idx]);
                }
            }
        }
    }
    GW_CU_CHECK_ERR(hipFree(d_tmp));
}

uint64_t PoaBatch::total_cells()
{
    scoped_device_switch dev(device_id_);
    if (poa_count_ == 0) return 0;
    GW_CU_CHECK_ERR(hipMemcpyAsync(h_.cells, d_.cells, static_cast<size_t>(poa_count_) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream_));
    GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    uint64_t t = 0;
    for (int32_t i = 0; i < poa_count_; i++) t += h_.cells[i];
    return t;
}

// ---- factories (batch.cu:107-232) ----------------------------------------------------------------------
std::unique_ptr<Batch> create_batch(int32_t device_id, cudaStream_t stream, DefaultDeviceAllocator allocator,
                                    int64_t max_mem, int8_t output_mask, const BatchConfig& batch_size,
                                    int16_t gap_score, int16_t mismatch_score, int16_t match_score)
{
    return std::make_unique<PoaBatch>(device_id, stream, allocator, max_mem, output_mask, batch_size, gap_score,
                                      mismatch_score, match_score);
}

std::unique_ptr<Batch> create_batch(int32_t device_id, cudaStream_t stream, int64_t max_mem, int8_t output_mask,
                                    const BatchConfig& batch_size, int16_t gap_score, int16_t mismatch_score,
                                    int16_t match_score)
{
    if (max_mem < -1)
        throw std::invalid_argument("max_mem has to be either -1 (=all available GPU memory) or greater or equal than 0.");
    scoped_device_switch dev(device_id);
    if (max_mem == -1)
    {
        max_mem = cudautils::find_largest_contiguous_device_memory_section();
        if (max_mem == 0) throw std::runtime_error("No memory available for caching");
    }
    if (max_mem == 0)
    {
        // BatchBlock throws "Requires at least N bytes" for a zero budget (Test_CudapoaBatch.cu:70-97)
        gwhip_poa_config c = make_device_config(batch_size, output_mask, gap_score, mismatch_score, match_score);
        int64_t per_poa = 0, per_matrix = 0;
        gwhip_poa_bytes_per_window(&c, &per_poa, &per_matrix);
        throw requires_at_least(per_poa + per_matrix);
    }
    DefaultDeviceAllocator allocator(static_cast<size_t>(max_mem), stream);
    return create_batch(device_id, stream, allocator, max_mem, output_mask, batch_size, gap_score, mismatch_score, match_score);
}

} // namespace cudapoa
} // namespace genomeworks
} // namespace claraparabricks
