// aligner_impl.hpp -- concrete banded / unbanded Myers aligner for MI355X (see cudaaligner.cpp).
#pragma once
#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>
#include <claraparabricks/genomeworks/cudaaligner/alignment.hpp>

#include <string>
#include <vector>

#include "pinned_vector.hpp"

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaaligner
{

class BandedAligner : public FixedBandAligner
{
public:
    /// expand_results: materialise per-position states (the fixed-stride factories) instead of run lengths.
    /// max_query_length >= 0 switches on the fixed-stride limits (exceeded_max_length / exceeded_max_alignments).
    BandedAligner(int64_t max_device_memory, int32_t max_bandwidth, DefaultDeviceAllocator allocator, cudaStream_t stream,
                  int32_t device_id, bool expand_results, int32_t max_query_length, int32_t max_target_length,
                  int32_t max_alignments);
    ~BandedAligner() override;

    StatusType align_all() override;
    StatusType sync_alignments() override;
    StatusType add_alignment(const char* query, int32_t query_length, const char* target, int32_t target_length,
                             bool reverse_complement_query = false, bool reverse_complement_target = false) override;
    StatusType add_alignment(int32_t max_bandwidth, const char* query, int32_t query_length, const char* target,
                             int32_t target_length, bool reverse_complement_query = false,
                             bool reverse_complement_target = false) override;
    const std::vector<std::shared_ptr<Alignment>>& get_alignments() const override { return alignments_; }
    DeviceAlignmentsPtrs get_alignments_device() const override;
    void reset() override;
    void free_temporary_device_buffers() override;
    int32_t num_alignments() const override { return static_cast<int32_t>(seq_starts_h_.size() / 2); } // [2n + 1] offsets
    cudaStream_t get_stream() const override { return stream_; }
    int32_t get_device() const override { return device_id_; }
    DefaultDeviceAllocator get_device_allocator() const override { return allocator_; }
    void reset_max_bandwidth(int32_t max_bandwidth) override;

    // benchmark helpers (not part of the reference interface)
    void relaunch_resident();     ///< run the kernels again on the inputs already resident in HBM
    float relaunch_resident_timed(); ///< same; returns the kernels' time in ms (HIP events on the aligner's stream)
    bool expands_results() const { return expand_results_; }
    uint64_t total_band_cells();  ///< 32 * band words * target length, summed over band attempts and pairs

private:
    struct Chunk;
    /// The GW_ALIGNER_* environment switches, read at the top of every align_all(): a process may change them
    /// between batches, and the tests do.
    struct Switches
    {
        int32_t chunks      = 0;     ///< GW_ALIGNER_CHUNKS: >= 1 when set (the batch's size caps it); 0: the size rule decides
        bool raw_upload     = false; ///< GW_ALIGNER_RAW_UPLOAD (A/B switch): characters instead of packed bases over the link
        int64_t mirror_runs = 0;     ///< GW_ALIGNER_MIRROR_RUNS (tests: a capacity the batch exceeds): >= 1 when set; 0: sized from the batch
        bool trace          = false; ///< GW_ALIGNER_TRACE: host-side timeline of align_all() / sync_alignments() on stderr
        static Switches read();
    };
    /// One buffer of the process-wide pinned cache (alignment_impl.hpp); it goes back there with its owner.
    struct PinnedBuffer
    {
        char* data   = nullptr;
        size_t bytes = 0; ///< capacity (pinned_acquire)
        PinnedBuffer()                    = default;
        PinnedBuffer(const PinnedBuffer&) = delete;
        PinnedBuffer& operator=(const PinnedBuffer&) = delete;
        ~PinnedBuffer() { release(); }
        void release()
        {
            if (data != nullptr) pinned_release(data, bytes);
            data  = nullptr;
            bytes = 0;
        }
        void acquire(size_t want)
        {
            release();
            data = pinned_acquire(want, &bytes);
        }
        /// sync_alignments() hands the buffer to the views' block (which returns it with pinned_release(p, *capacity)): this
        /// side is empty afterwards, and the next batch acquires a fresh buffer
        char* detach(size_t* capacity)
        {
            char* p   = data;
            *capacity = bytes;
            data      = nullptr;
            bytes     = 0;
            return p;
        }
    };
    /// operations[runs] | run lengths[runs] (from the next multiple of 64 bytes): the packed runs of a batch on the host, written
    /// by the kernels of a chunked batch (gwhip_myers_args::results_host) or copied by sync_alignments()
    struct RunsMirror : PinnedBuffer
    {
        int64_t runs = 0; ///< capacity in runs
        int8_t* ops() const { return reinterpret_cast<int8_t*>(data); }
        int32_t* counts() const { return reinterpret_cast<int32_t*>(data + ((runs + 63) & ~int64_t(63))); }
        void acquire_runs(int64_t want)
        {
            runs = 0;
            acquire(static_cast<size_t>((want + 63) & ~int64_t(63)) + static_cast<size_t>(want) * 4 + 64);
            runs = want;
        }
        char* detach(size_t* capacity)
        {
            runs = 0;
            return PinnedBuffer::detach(capacity);
        }
    };
    /// result_starts[pairs + 1] | metadata[pairs] of the last launch
    struct ResultsHead : PinnedBuffer
    {
        int32_t pairs = 0;
        int32_t* offsets() const { return reinterpret_cast<int32_t*>(data); }
        uint32_t* metadata() const { return reinterpret_cast<uint32_t*>(data) + static_cast<size_t>(pairs) + 1; }
        void prepare(int32_t n) // (sync_alignments() hands the buffer to the views' block)
        {
            const size_t need = (2 * static_cast<size_t>(n) + 1) * 4;
            if (data == nullptr || bytes < need) acquire(need);
            pairs = n;
        }
    };

    void reset_data();
    void free_device();
    void launch(hipEvent_t event_before = nullptr, hipEvent_t event_after = nullptr); ///< every chunk's kernels again and the head
    void launch_chunk(const Chunk& c, int32_t phases = 0);
    /// every chunk's kernels, pipelined over the aligner's stream and the side stream; `order` (host, pinned) goes up chunk by
    /// chunk when given, and workspaces are allocated when `allocate`
    void run_chunks(const int32_t* order, bool allocate);
    /// chunk k on stream `s`, which has waited for the chunk's inputs: its part of `order` goes up and its bases are expanded
    /// (when `order` is given), its workspace is allocated (when `allocate`), then its kernels of `phases`
    void queue_chunk(size_t k, const int32_t* order, bool allocate, hipStream_t s, int32_t phases);
    void enqueue_inputs(size_t k); ///< chunk k's bases, offsets and band widths on the upload stream, and its event
    void fetch_head_slice(const Chunk& c, hipStream_t s); ///< the chunk's offsets and metadata follow its kernels to the host
    void drain_streams();                                 ///< host waits for the aligner's, the upload and the side stream (unchecked)

    cudaStream_t stream_;
    int32_t device_id_;
    DefaultDeviceAllocator allocator_;
    int32_t max_bandwidth_;
    int64_t max_device_memory_;
    bool expand_results_;
    int32_t max_query_length_, max_target_length_, max_alignments_;

    // staging arrays in pinned host memory: uploaded asynchronously at link speed
    PinnedVector<char> seq_h_;
    /// the same bases two per byte (include/gwhip.h, gwhip_unpack_bases): what align_all() uploads -- half the bytes over the
    /// link; the characters above stay for the Alignment objects
    PinnedVector<uint8_t> packed_h_;
    PinnedVector<int64_t> seq_starts_h_;
    PinnedVector<int32_t> max_bandwidths_h_;
    PinnedVector<int32_t> order_h_;
    std::vector<std::shared_ptr<Alignment>> alignments_;
    size_t workspace_bytes_estimate_ = 0;
    size_t largest_wave_ws_          = 0;
    int32_t longest_query_           = 0;
    int64_t longest_pair_            = 0; ///< query + target of the longest pair (buckets of the counting sort in align_all())
    int32_t widest_band_             = 0;
    bool launched_                   = false;
    bool uploads_in_flight_          = false;
    int64_t total_length_h_          = 0;
    int32_t n_last_                  = 0;
    Switches switches_;  ///< of the last align_all()
    RunsMirror mirror_;  ///< where the kernels of a chunked batch put its runs
    ResultsHead head_;

    char* device_block_        = nullptr; ///< inputs and outputs (allocated first: the uploads start before the batch is sorted)
    size_t device_block_bytes_ = 0;
    /// A batch is processed as one chunk, or -- large batches -- as several chunks of consecutive pairs whose uploads run on a
    /// stream of their own: the upload of chunk k + 1 overlaps the kernels of chunk k (include/gwhip.h, gwhip_myers_args).
    /// Every chunk has its own workspace (sized once its processing order is known).
    struct Chunk
    {
        int32_t lo = 0, hi = 0;
        int64_t first_offset = 0, span = 0; ///< sequence offset of the first pair, bytes of the chunk's sequences
        char* workspace        = nullptr;
        size_t workspace_bytes = 0, block_bytes = 0;
    };
    std::vector<Chunk> chunks_;
    int64_t launched_total_length_ = 0;   ///< bases of the launched batch (the host arrays move to the views at sync_alignments())
    // Streams and events of chunked batches, created with the first one (timing disabled) and kept for the aligner's life.
    hipStream_t upload_stream_ = nullptr;
    hipStream_t side_stream_   = nullptr; ///< sizing / compaction kernels and result offsets (gwhip_myers_args::side_stream)
    hipEvent_t begin_          = nullptr; ///< on stream_: what the other two streams start a round behind
    hipEvent_t side_joined_    = nullptr; ///< on the side stream: everything a round queued there
    std::vector<hipEvent_t> uploaded_;    ///< [chunk] on the upload stream: the chunk's inputs are up
    std::vector<hipEvent_t> sized_;       ///< [chunk] on the side stream: the chunk's workspace is sized
    char* d_seq_               = nullptr;
    uint8_t* d_packed_         = nullptr; ///< upload staging of packed_h_ (unpacked into d_seq_ on the device)
    int64_t* d_starts_         = nullptr;
    int32_t* d_bw_             = nullptr;
    int32_t* d_order_          = nullptr;
    int8_t* d_results_         = nullptr;
    int32_t* d_result_counts_  = nullptr;
    int32_t* d_result_starts_  = nullptr;
    uint32_t* d_metadata_      = nullptr;
    uint64_t* d_cells_         = nullptr;
};

/// a non-zero return code of a gwhip_* call: logs the kernels' error string and raises the HIP error
void check_gwhip(int rc);

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
