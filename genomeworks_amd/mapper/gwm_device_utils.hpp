// gwm_device_utils.hpp -- helpers shared by the cudamapper translation units (gwm_mapper.hip, gwm_postprocess.hip,
// gwm_align.hip, gwm_index_cache.hip):
// checked HIP calls, owning device buffers, the rocPRIM scan / select / sort wrappers and HIP-event stage timers.
// Everything here has internal linkage; the one shared object is the error text behind gwm_last_error().
#ifndef GWM_DEVICE_UTILS_HPP
#define GWM_DEVICE_UTILS_HPP

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

// sets the text gwm_last_error() returns on the calling thread (defined in gwm_mapper.hip)
void gwm_set_error(const char* text);

namespace
{

void check(hipError_t e, const char* what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#define GWM_CHECK(x) check((x), #x)

constexpr int kThreads = 256;

inline unsigned grid_for(int64_t n) { return static_cast<unsigned>((n + kThreads - 1) / kThreads); }

// Owning device allocation.
template <typename T>
struct dbuf
{
    T* p       = nullptr;
    int64_t n  = 0;
    dbuf()     = default;
    explicit dbuf(int64_t count) { resize(count); }
    dbuf(const dbuf&) = delete;
    dbuf& operator=(const dbuf&) = delete;
    ~dbuf() { reset(); }
    void resize(int64_t count)
    {
        reset();
        n = count;
        if (count > 0)
            GWM_CHECK(hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * static_cast<size_t>(count)));
    }
    void reset()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    T* release()
    {
        T* r = p;
        p    = nullptr;
        n    = 0;
        return r;
    }
};

// Scratch for the rocPRIM calls of one stage, grown on demand.
struct Temp
{
    dbuf<char> buf;
    void* get(size_t bytes)
    {
        if (static_cast<int64_t>(bytes) > buf.n)
            buf.resize(static_cast<int64_t>(std::max<size_t>(bytes, 256)));
        return buf.p;
    }
};

template <typename T>
T to_host(const T* d, hipStream_t s)
{
    T h{};
    GWM_CHECK(hipMemcpyAsync(&h, d, sizeof(T), hipMemcpyDeviceToHost, s));
    GWM_CHECK(hipStreamSynchronize(s));
    return h;
}

template <typename In, typename Out>
void inclusive_sum(In in, Out out, int64_t n, Temp& t, hipStream_t s)
{
    size_t bytes = 0;
    GWM_CHECK(rocprim::inclusive_scan(nullptr, bytes, in, out, static_cast<size_t>(n), rocprim::plus<>(), s));
    GWM_CHECK(rocprim::inclusive_scan(t.get(bytes), bytes, in, out, static_cast<size_t>(n), rocprim::plus<>(), s));
}

// Indices i in [0, n) with flags[i] != 0, in order, into out; returns their number.
uint32_t select_indices(const uint32_t* flags, int64_t n, uint32_t* out, uint32_t* d_count, Temp& t, hipStream_t s)
{
    rocprim::counting_iterator<uint32_t> idx(0);
    size_t bytes = 0;
    GWM_CHECK(rocprim::select(nullptr, bytes, idx, flags, out, d_count, static_cast<size_t>(n), s));
    GWM_CHECK(rocprim::select(t.get(bytes), bytes, idx, flags, out, d_count, static_cast<size_t>(n), s));
    return to_host(d_count, s);
}

// Stable LSD radix sort of (key, index) pairs over key bits [0, bits).
template <typename K>
void sort_pairs(K* keys_in, K* keys_out, uint32_t* vals_in, uint32_t* vals_out, int64_t n, unsigned bits, Temp& t,
                hipStream_t s)
{
    size_t bytes = 0;
    GWM_CHECK(rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out,
                                        static_cast<unsigned>(n), 0u, bits, s));
    GWM_CHECK(rocprim::radix_sort_pairs(t.get(bytes), bytes, keys_in, keys_out, vals_in, vals_out,
                                        static_cast<unsigned>(n), 0u, bits, s));
}

unsigned bits_for(uint64_t max_value)
{
    unsigned b = 1;
    while (b < 64 && (max_value >> b) != 0)
        ++b;
    return b;
}

// A read set on the device: bases[offsets[i] .. offsets[i + 1]) is read first_read_id + i.
struct ReadSet
{
    const uint8_t* bases;
    const int64_t* offsets;
    uint32_t n_reads;
    uint32_t first_read_id;
};

struct Events
{
    hipEvent_t e[6] = {};
    int n           = 0;
    explicit Events(int count)
        : n(count)
    {
        for (int i = 0; i < n; ++i)
            GWM_CHECK(hipEventCreate(&e[i]));
    }
    ~Events()
    {
        for (int i = 0; i < n; ++i)
            (void)hipEventDestroy(e[i]);
    }
    void record(int i, hipStream_t s) { GWM_CHECK(hipEventRecord(e[i], s)); }
    float ms(int a, int b)
    {
        float v = 0.f;
        GWM_CHECK(hipEventSynchronize(e[b]));
        GWM_CHECK(hipEventElapsedTime(&v, e[a], e[b]));
        return v;
    }
};

} // namespace

#endif
