// extender.cpp -- cudaextender's host side: the Extender object (cudaextender/extender.hpp) over the kernel-level
// C-ABI of gwhip_extender.h, and the flat C API of gw_extender_capi.h.
#include <claraparabricks/genomeworks/cudaextender/cudaextender.hpp>
#include <claraparabricks/genomeworks/cudaextender/extender.hpp>
#include <claraparabricks/genomeworks/logging/logging.hpp>
#include <claraparabricks/genomeworks/utils/cudautils.hpp>
#include <claraparabricks/genomeworks/utils/device_buffer.hpp>

#include <gw_extender_capi.h>
#include <gwhip_extender.h>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaextender
{

static_assert(sizeof(SeedPair) == sizeof(gwx_seed) && sizeof(SeedPair) == 8, "SeedPair layout");
static_assert(sizeof(ScoredSegmentPair) == sizeof(gwx_segment) && sizeof(ScoredSegmentPair) == 16,
              "ScoredSegmentPair layout");

StatusType Init()
{
    logging::initialize_logger(logging::LogLevel::warn);
    return StatusType::success;
}

namespace
{

constexpr int32_t kScoreMatrixSize = 64;

class UngappedXDrop : public Extender
{
public:
    UngappedXDrop(const int32_t* h_score_mat, int32_t xdrop_threshold, bool no_entropy, cudaStream_t stream,
                  int32_t device_id, DefaultDeviceAllocator allocator)
        : score_mat_(h_score_mat, h_score_mat + kScoreMatrixSize)
        , xdrop_threshold_(xdrop_threshold)
        , no_entropy_(no_entropy)
        , stream_(stream)
        , device_id_(device_id)
        , allocator_(allocator)
    {
        scoped_device_switch dev(device_id_);
        hipDeviceProp_t prop;
        GW_CU_CHECK_ERR(hipGetDeviceProperties(&prop, device_id_));
        // seeds per chunk: 4 Mi per whole GiB of device memory
        const int64_t gib = static_cast<int64_t>(static_cast<double>(prop.totalGlobalMem) / 1073741824.0);
        chunk_            = static_cast<int32_t>(std::min<int64_t>(std::max<int64_t>(gib, 1) * 4194304, INT32_MAX));
        d_score_mat_      = device_buffer<int32_t>(kScoreMatrixSize, allocator_, stream_);
        cudautils::device_copy_n_async(score_mat_.data(), kScoreMatrixSize, d_score_mat_.data(), stream_);
        GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
    }

    ~UngappedXDrop() override
    {
        for (hipEvent_t e : events_)
            if (e != nullptr) (void)hipEventDestroy(e);
    }

    StatusType extend_async(const int8_t* d_query, int32_t query_length, const int8_t* d_target, int32_t target_length,
                            int32_t score_threshold, const SeedPair* d_seed_pairs, int32_t num_seed_pairs,
                            ScoredSegmentPair* d_scored_segment_pairs, int32_t* d_num_scored_segment_pairs) override
    {
        if (d_query == nullptr || d_target == nullptr || d_seed_pairs == nullptr || d_scored_segment_pairs == nullptr ||
            d_num_scored_segment_pairs == nullptr)
        {
            GW_LOG_ERROR("cudaextender: null input or output pointer");
            return StatusType::invalid_input;
        }
        if (query_length < 0 || target_length < 0 || num_seed_pairs < 0)
        {
            GW_LOG_ERROR("cudaextender: negative length or seed count");
            return StatusType::invalid_input;
        }
        scoped_device_switch dev(device_id_);
        kernel_ms_ = post_ms_ = 0.0;
        positions_            = 0;
        int32_t total         = 0;
        if (num_seed_pairs > 0)
        {
            const int32_t chunk = std::min(chunk_, num_seed_pairs);
            const size_t bytes  = gwx_workspace_bytes(chunk);
            device_buffer<char> workspace(static_cast<std::ptrdiff_t>(bytes), allocator_, stream_);
            const gwx_problem problem{d_target, target_length, d_query, query_length, d_score_mat_.data(),
                                      xdrop_threshold_, score_threshold, no_entropy_ ? 1 : 0};
            void* const* events = nullptr;
            if (timing_)
            {
                for (hipEvent_t& e : events_)
                    if (e == nullptr) GW_CU_CHECK_ERR(hipEventCreate(&e));
                events = reinterpret_cast<void* const*>(events_);
            }
            for (int32_t start = 0; start < num_seed_pairs; start += chunk)
            {
                const int32_t n = std::min(chunk, num_seed_pairs - start);
                int32_t count   = 0;
                if (gwx_extend_chunk(&problem, reinterpret_cast<const gwx_seed*>(d_seed_pairs) + start, n,
                                     reinterpret_cast<gwx_segment*>(d_scored_segment_pairs) + total, &count,
                                     workspace.data(), bytes, stream_, events) != 0)
                {
                    GW_LOG_ERROR(gwx_last_error());
                    return StatusType::generic_error;
                }
                total += count;
                positions_ += gwx_last_positions();
                if (timing_)
                {
                    float a = 0.f, b = 0.f;
                    GW_CU_CHECK_ERR(hipEventElapsedTime(&a, events_[0], events_[1]));
                    GW_CU_CHECK_ERR(hipEventElapsedTime(&b, events_[1], events_[2]));
                    kernel_ms_ += a;
                    post_ms_ += b;
                }
            }
        }
        if (gwx_store_count(d_num_scored_segment_pairs, total, stream_) != 0)
        {
            GW_LOG_ERROR(gwx_last_error());
            return StatusType::generic_error;
        }
        return StatusType::success;
    }

    StatusType extend_async(const int8_t* h_query, int32_t query_length, const int8_t* h_target, int32_t target_length,
                            int32_t score_threshold, const std::vector<SeedPair>& h_seed_pairs) override
    {
        if (h_query == nullptr || h_target == nullptr)
        {
            GW_LOG_ERROR("cudaextender: null input pointer");
            return StatusType::invalid_input;
        }
        if (query_length < 0 || target_length < 0 || h_seed_pairs.size() > static_cast<size_t>(INT32_MAX))
        {
            GW_LOG_ERROR("cudaextender: negative length or too many seeds");
            return StatusType::invalid_input;
        }
        reset();
        scoped_device_switch dev(device_id_);
        const int32_t n = static_cast<int32_t>(h_seed_pairs.size());
        // at least one element each, so a zero-length input still has a device address
        d_query_   = device_buffer<int8_t>(std::max(query_length, 1), allocator_, stream_);
        d_target_  = device_buffer<int8_t>(std::max(target_length, 1), allocator_, stream_);
        d_seeds_   = device_buffer<SeedPair>(std::max(n, 1), allocator_, stream_);
        d_ssp_     = device_buffer<ScoredSegmentPair>(std::max(n, 1), allocator_, stream_);
        d_num_ssp_ = device_buffer<int32_t>(1, allocator_, stream_);
        cudautils::device_copy_n_async(h_query, query_length, d_query_.data(), stream_);
        cudautils::device_copy_n_async(h_target, target_length, d_target_.data(), stream_);
        cudautils::device_copy_n_async(h_seed_pairs.data(), h_seed_pairs.size(), d_seeds_.data(), stream_);
        host_ptr_api_mode_ = true;
        return extend_async(d_query_.data(), query_length, d_target_.data(), target_length, score_threshold,
                            d_seeds_.data(), n, d_ssp_.data(), d_num_ssp_.data());
    }

    StatusType sync() override
    {
        if (!host_ptr_api_mode_) return StatusType::invalid_operation;
        scoped_device_switch dev(device_id_);
        const int32_t n = cudautils::get_value_from_device(d_num_ssp_.data(), stream_);
        h_ssp_.resize(n);
        if (n > 0)
        {
            cudautils::device_copy_n_async(d_ssp_.data(), static_cast<size_t>(n), h_ssp_.data(), stream_);
            GW_CU_CHECK_ERR(hipStreamSynchronize(stream_));
        }
        return StatusType::success;
    }

    const std::vector<ScoredSegmentPair>& get_scored_segment_pairs() const override
    {
        if (!host_ptr_api_mode_)
            throw std::runtime_error("cudaextender: get_scored_segment_pairs() without a host-pointer extend_async");
        return h_ssp_;
    }

    void reset() override
    {
        h_ssp_.clear();
        host_ptr_api_mode_ = false;
        d_query_.free();
        d_target_.free();
        d_seeds_.free();
        d_ssp_.free();
        d_num_ssp_.free();
    }

    // instrumentation and test hooks of the C API
    void set_chunk(int32_t chunk) { chunk_ = std::max(chunk, 1); }
    void set_timing(bool on) { timing_ = on; }
    double kernel_ms() const { return kernel_ms_; }
    double post_ms() const { return post_ms_; }
    int64_t positions() const { return positions_; }

private:
    std::vector<int32_t> score_mat_;
    int32_t xdrop_threshold_;
    bool no_entropy_;
    cudaStream_t stream_;
    int32_t device_id_;
    DefaultDeviceAllocator allocator_;
    int32_t chunk_ = 1;
    device_buffer<int32_t> d_score_mat_;
    // host-pointer API state
    bool host_ptr_api_mode_ = false;
    device_buffer<int8_t> d_query_, d_target_;
    device_buffer<SeedPair> d_seeds_;
    device_buffer<ScoredSegmentPair> d_ssp_;
    device_buffer<int32_t> d_num_ssp_;
    std::vector<ScoredSegmentPair> h_ssp_;
    // instrumentation
    bool timing_           = false;
    hipEvent_t events_[3]  = {nullptr, nullptr, nullptr};
    double kernel_ms_ = 0, post_ms_ = 0;
    int64_t positions_ = 0;
};

} // namespace

std::unique_ptr<Extender> create_extender(const int32_t* h_score_mat, int32_t score_mat_dim, int32_t xdrop_threshold,
                                          bool no_entropy, cudaStream_t stream, int32_t device_id,
                                          DefaultDeviceAllocator allocator, ExtensionType type)
{
    if (type != ExtensionType::ungapped_xdrop)
    {
        GW_LOG_ERROR("cudaextender: unknown ExtensionType");
        return nullptr;
    }
    if (h_score_mat == nullptr || score_mat_dim != kScoreMatrixSize)
    {
        GW_LOG_ERROR("cudaextender: the score matrix must have 64 entries");
        return nullptr;
    }
    return std::make_unique<UngappedXDrop>(h_score_mat, xdrop_threshold, no_entropy, stream, device_id, allocator);
}

} // namespace cudaextender
} // namespace genomeworks
} // namespace claraparabricks

// ---------------------------------------------------------------------------------------------------------------
// flat C API (gw_extender_capi.h)
// ---------------------------------------------------------------------------------------------------------------
using namespace claraparabricks::genomeworks;

struct gw_extender
{
    std::unique_ptr<cudaextender::Extender> ext;
    cudaextender::UngappedXDrop* impl() { return static_cast<cudaextender::UngappedXDrop*>(ext.get()); }
};

namespace
{
thread_local std::string g_capi_error;

template <typename F>
int guarded(F&& f)
{
    try
    {
        return f();
    }
    catch (const std::exception& e)
    {
        g_capi_error = e.what();
    }
    catch (...)
    {
        g_capi_error = "unknown exception";
    }
    return GW_EXTENDER_ERROR;
}
} // namespace

extern "C" {

const char* gw_extender_last_error(void) { return g_capi_error.c_str(); }

gw_extender* gw_extender_create(const int32_t* score_matrix, int32_t score_matrix_dim, int32_t xdrop_threshold,
                                int32_t no_entropy, void* stream, int32_t device_id, int64_t max_device_memory,
                                int32_t extension_type)
{
    gw_extender* h = nullptr;
    guarded([&] {
        const size_t pool = max_device_memory > 0 ? static_cast<size_t>(max_device_memory) : 2ull << 30;
        auto ext = cudaextender::create_extender(score_matrix, score_matrix_dim, xdrop_threshold, no_entropy != 0,
                                                 static_cast<cudaStream_t>(stream), device_id,
                                                 create_default_device_allocator(pool, static_cast<cudaStream_t>(stream)),
                                                 static_cast<cudaextender::ExtensionType>(extension_type));
        if (!ext)
        {
            g_capi_error = "create_extender: unsupported score matrix size or extension type";
            return GW_EXTENDER_ERROR;
        }
        h = new gw_extender{std::move(ext)};
        return 0;
    });
    return h;
}

int gw_extender_extend_host(gw_extender* h, const int8_t* query, int32_t query_length, const int8_t* target,
                            int32_t target_length, int32_t score_threshold, const void* seed_pairs, int64_t num_seed_pairs)
{
    return guarded([&] {
        if (num_seed_pairs < 0 || num_seed_pairs > INT32_MAX || (num_seed_pairs > 0 && seed_pairs == nullptr))
            return static_cast<int>(cudaextender::StatusType::invalid_input);
        const auto* s = static_cast<const cudaextender::SeedPair*>(seed_pairs);
        const std::vector<cudaextender::SeedPair> seeds(s, s + num_seed_pairs);
        return static_cast<int>(h->ext->extend_async(query, query_length, target, target_length, score_threshold, seeds));
    });
}

int gw_extender_extend_device(gw_extender* h, const int8_t* d_query, int32_t query_length, const int8_t* d_target,
                              int32_t target_length, int32_t score_threshold, const void* d_seed_pairs,
                              int32_t num_seed_pairs, void* d_scored_segment_pairs, int32_t* d_num_scored_segment_pairs)
{
    return guarded([&] {
        return static_cast<int>(h->ext->extend_async(
            d_query, query_length, d_target, target_length, score_threshold,
            static_cast<const cudaextender::SeedPair*>(d_seed_pairs), num_seed_pairs,
            static_cast<cudaextender::ScoredSegmentPair*>(d_scored_segment_pairs), d_num_scored_segment_pairs));
    });
}

int gw_extender_sync(gw_extender* h)
{
    return guarded([&] { return static_cast<int>(h->ext->sync()); });
}

int64_t gw_extender_result_count(gw_extender* h)
{
    int64_t n = -1;
    guarded([&] {
        n = static_cast<int64_t>(h->ext->get_scored_segment_pairs().size());
        return 0;
    });
    return n;
}

int gw_extender_copy_results(gw_extender* h, void* out, int64_t capacity)
{
    return guarded([&] {
        const auto& r = h->ext->get_scored_segment_pairs();
        if (static_cast<int64_t>(r.size()) > capacity) throw std::runtime_error("gw_extender_copy_results: buffer too small");
        std::copy(r.begin(), r.end(), static_cast<cudaextender::ScoredSegmentPair*>(out));
        return 0;
    });
}

void gw_extender_reset(gw_extender* h) { guarded([&] { h->ext->reset(); return 0; }); }

void gw_extender_destroy(gw_extender* h) { delete h; }

int gw_extender_set_chunk_size(gw_extender* h, int32_t seeds_per_chunk)
{
    return guarded([&] {
        h->impl()->set_chunk(seeds_per_chunk);
        return 0;
    });
}

int gw_extender_set_instrumentation(gw_extender* h, int32_t enable)
{
    return guarded([&] {
        h->impl()->set_timing(enable != 0);
        gwx_count_positions(enable);
        return 0;
    });
}

int gw_extender_last_timing(gw_extender* h, double* kernel_ms, double* sort_unique_ms, int64_t* positions)
{
    return guarded([&] {
        *kernel_ms      = h->impl()->kernel_ms();
        *sort_unique_ms = h->impl()->post_ms();
        *positions      = h->impl()->positions();
        return 0;
    });
}

int gw_extender_sort_unique_hook(const void* d_segments, const uint8_t* d_keep, int32_t n, void* d_out, int32_t* count,
                                 void* stream)
{
    return guarded([&] {
        void* ws          = nullptr;
        const size_t bytes = gwx_workspace_bytes(n);
        GW_CU_CHECK_ERR(hipMalloc(&ws, bytes));
        const int rc = gwx_sort_unique(static_cast<const gwx_segment*>(d_segments), d_keep, n,
                                       static_cast<gwx_segment*>(d_out), count, ws, bytes, stream);
        if (rc != 0) g_capi_error = gwx_last_error();
        GW_CU_CHECK_ERR(hipFree(ws));
        return rc == 0 ? 0 : GW_EXTENDER_ERROR;
    });
}

} // extern "C"
