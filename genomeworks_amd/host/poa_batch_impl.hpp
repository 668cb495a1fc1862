// poa_batch_impl.hpp -- concrete cudapoa::Batch for MI355X (declaration; see cudapoa_batch.cpp).
#pragma once
#include <claraparabricks/genomeworks/cudapoa/batch.hpp>

#include "../../include/gwhip.h"
#include "host_common.hpp"

namespace claraparabricks
{
namespace genomeworks
{
namespace cudapoa
{

gwhip_poa_config make_device_config(const BatchConfig& b, int8_t output_mask, int32_t gap, int32_t mismatch, int32_t match);

/// The binning rule of get_multi_batch_sizes on its own (cudapoa_utils.cpp; exposed to the tests through the C API).
void bin_poa_groups(std::vector<BatchConfig>& list_of_batch_sizes, std::vector<std::vector<int32_t>>& list_of_groups_per_batch,
                    const std::vector<int32_t>& capacity, const std::vector<int32_t>& longest, const std::vector<int32_t>& reads,
                    int32_t band_width, BandMode band_mode, float adaptive_storage_factor, float graph_length_factor,
                    int32_t max_pred_distance, const std::vector<int32_t>* bins_capacity);

/// The arrays of a batch, in the order they lie in its block.
struct PoaSections
{
    uint8_t* sequences            = nullptr;
    int8_t* weights               = nullptr;
    int32_t* lengths              = nullptr;
    gwhip_window_details* windows = nullptr;
    uint8_t* consensus            = nullptr;
    uint16_t* coverage            = nullptr;
    uint8_t* msa                  = nullptr; // null unless the batch produces MSAs
    uint64_t* cells               = nullptr;
    uint32_t* work_counters       = nullptr; // 256 bytes behind the cell counters: the window counter of a persistent launch
};

/// Where those arrays start in the device block of a batch of some number of windows: [sequences | weights | lengths |
/// windows | consensus | coverage | msa | cells | work counters | kernel workspace]. The pinned staging block is the same
/// without the workspace, so consensus and coverage are neighbours with the same spacing on both sides (fetch_consensus()).
struct PoaBlockLayout
{
    gwhost::BlockLayout block;
    size_t sequence_bytes = 0; // of `sequences`, and of `weights`: the reads padded to 4 bytes, 4096 bytes of slack, rounded up
    gwhost::BlockLayout::Slot<uint8_t> sequences;
    gwhost::BlockLayout::Slot<int8_t> weights;
    gwhost::BlockLayout::Slot<int32_t> lengths;
    gwhost::BlockLayout::Slot<gwhip_window_details> windows;
    gwhost::BlockLayout::Slot<uint8_t> consensus;
    gwhost::BlockLayout::Slot<uint16_t> coverage;
    gwhost::BlockLayout::Slot<uint8_t> msa;
    bool has_msa = false;
    gwhost::BlockLayout::Slot<uint64_t> cells;
    gwhost::BlockLayout::Slot<uint32_t> work_counters;
    gwhost::BlockLayout::Slot<char> workspace;

    PoaSections in(char* b) const
    {
        return PoaSections{sequences.in(b), weights.in(b), lengths.in(b), windows.in(b),      consensus.in(b),
                           coverage.in(b),  has_msa ? msa.in(b) : nullptr, cells.in(b), work_counters.in(b)};
    }
};

class PoaBatch : public Batch
{
public:
    PoaBatch(int32_t device_id, cudaStream_t stream, DefaultDeviceAllocator allocator, int64_t max_mem, int8_t output_mask,
             const BatchConfig& batch_size, int32_t gap_score = -8, int32_t mismatch_score = -6, int32_t match_score = 8);
    ~PoaBatch() override;

    StatusType add_poa_group(std::vector<StatusType>& per_seq_status, const Group& poa_group) override;
    int32_t get_total_poas() const override { return poa_count_; }
    void generate_poa() override;
    StatusType get_consensus(std::vector<std::string>& consensus, std::vector<std::vector<uint16_t>>& coverage,
                             std::vector<StatusType>& output_status) override;
    StatusType get_msa(std::vector<std::vector<std::string>>& msa, std::vector<StatusType>& output_status) override;
    void get_graphs(std::vector<DirectedGraph>& graphs, std::vector<StatusType>& output_status) override;
    int32_t batch_id() const override { return bid_; }
    void reset() override;

    // extensions used by the benchmark / tests (not part of the reference interface)
    /// get_consensus() that overwrites its arguments (resized to the batch's windows) instead of appending to them, so that a
    /// caller who passes the vectors of its previous call gets the results without a heap allocation per window.
    StatusType get_consensus_in_place(std::vector<std::string>& consensus, std::vector<std::vector<uint16_t>>& coverage,
                                      std::vector<StatusType>& output_status);
    int32_t max_poas() const { return max_poas_; }
    /// The last generate_poa() let the graph-build kernel read the pinned staging block (no sequence upload).
    bool last_generate_read_host() const { return last_generate_read_host_; }
    uint64_t total_cells();    ///< DP cells computed by the last generate_poa() (device counters)
    /// Re-run the kernels on the inputs resident in HBM (no H2D -- but for the reads of a fill that generate_poa() let the kernel
    /// take from the pinned block: the first relaunch of such a fill uploads them once).
    void relaunch_resident();
    /// Same, timed with HIP events on the batch's stream: graph-build kernel and output kernel (milliseconds).
    void relaunch_resident_timed(float* graph_build_ms, float* output_ms);
    /// Profiling aid: relaunch with per-phase cycle accounting; out[6] = mean ticks per window of
    /// {row table, NW forward, sink+traceback, graph merge, topsort, other}.
    void profile_phases(double out[6]);
    void profile_phases_per_window(std::vector<uint64_t>& ticks); // six phase counters per window, in window order
    const gwhip_poa_config& device_config() const { return cfg_; }
    cudaStream_t stream() const { return stream_; }

private:
    void debug_message(const std::string& message);
    bool reserve_buf(int32_t max_seq_length);
    StatusType add_poa();
    StatusType add_seq_to_poa(const char* seq, const int8_t* weights, int32_t seq_len);
    void upload_inputs(bool host_input);
    void upload_sequences();         ///< the reads and the zeroed read-ahead slack behind them, into HBM
    void ensure_resident_sequences(); ///< upload_sequences() unless the device copy already holds this fill's reads
    void restore_lengths(); ///< a launch overwrote the length of each window's first read with its node count
    /// `sequences`: where the graph-build kernel takes the reads from (null: the device copy).
    void launch(void* event_after_graph_build = nullptr, uint64_t* phase_cycles = nullptr, const uint8_t* sequences = nullptr);
    bool use_host_input() const;     ///< this call of generate_poa() lets the kernel read the pinned block (see cudapoa_batch.cpp)
    void wait_for_host_reads();      ///< until no launch in flight reads the pinned block
    gwhip_poa_args kernel_args() const;
    StatusType window_status(size_t poa) const; ///< of the fetched consensus row: success, or the code behind the kernels' error marker
    void log_kernel_error(StatusType error_type);
    void log_failed_windows(const StatusType* status, size_t count); ///< in window order
    void fetch_consensus(std::string* consensus, std::vector<uint16_t>* coverage, StatusType* output_status, bool presize);
    PoaBlockLayout plan(int32_t n_poas) const;

    int32_t max_sequences_per_poa_ = 0;
    int32_t device_id_             = 0;
    cudaStream_t stream_           = nullptr;
    int8_t output_mask_            = 0;
    BatchConfig batch_size_;
    DefaultDeviceAllocator allocator_;
    gwhip_poa_config cfg_{};
    int32_t bid_      = 0;
    int32_t max_poas_ = 0;

    // host-side counters (reset() zeroes them)
    int32_t poa_count_              = 0;
    int32_t num_nucleotides_copied_ = 0;
    bool unit_weights_only_         = true; ///< no read of the batch carried base weights so far
    int32_t global_sequence_idx_    = 0;
    size_t avail_buf_mem_           = 0;
    size_t next_scores_offset_      = 0;
    size_t score_buffer_bytes_      = 0;

    PoaBlockLayout layout_;
    size_t workspace_bytes_ = 0;
    size_t input_capacity_  = 0;
    char* device_block_     = nullptr;
    PoaSections d_;
    char* host_block_           = nullptr; // pinned staging
    size_t host_block_capacity_ = 0;       // what the pinned cache handed out (pinned_release wants it back)
    PoaSections h_;

    // Host input: the graph-build kernel takes the reads from the pinned block itself (generate_poa()).
    const uint8_t* host_sequences_dev_ = nullptr; ///< device address of h_.sequences; null when the configuration's kernel needs
                                                  ///< the reads in HBM or the pinned block is not mapped for the device
    bool device_sequences_current_ = false;       ///< d_.sequences holds this fill's reads (and the zeroed slack)
    void* host_reads_done_         = nullptr;     ///< hipEvent_t behind the graph-build kernel of a host-input launch
    bool host_reads_pending_       = false;       ///< recorded and not yet waited for
    bool last_generate_read_host_  = false;
};

} // namespace cudapoa
} // namespace genomeworks
} // namespace claraparabricks
