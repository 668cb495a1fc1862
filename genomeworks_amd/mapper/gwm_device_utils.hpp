// gwm_device_utils.hpp -- helpers shared by the cudamapper translation units (gwm_mapper.hip, gwm_postprocess.hip,
// gwm_align.hip, gwm_index_cache.hip): what gwm_host_utils.hpp holds (checked HIP calls, owning device buffers,
// HIP-event stage timers, the device read set) and, on top of it, the rocPRIM scan / select / sort wrappers, the timer
// around a single launch and the slice copy of the gather kernels.
// Everything here has internal linkage; the one shared object is the error text behind gwm_last_error().
#ifndef GWM_DEVICE_UTILS_HPP
#define GWM_DEVICE_UTILS_HPP

#include "gwm_host_utils.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>

// sets the text gwm_last_error() returns on the calling thread (defined in gwm_mapper.hip)
void gwm_set_error(const char* text);

namespace
{

constexpr int kThreads = 256;

inline unsigned grid_for(int64_t n) { return static_cast<unsigned>((n + kThreads - 1) / kThreads); }

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

// a device read set from the four arguments the stage functions take it as
inline ReadSet read_set(const char* bases, const int64_t* offsets, int32_t n_reads, uint32_t first_read_id)
{
    return {reinterpret_cast<const uint8_t*>(bases), offsets, static_cast<uint32_t>(n_reads), first_read_id};
}

// One launch (or several) on s between two HIP events: waits for it, and *ms_out = its device time where asked for.
template <typename F>
void timed_launch(hipStream_t s, float* ms_out, F&& launch)
{
    Events ev(2);
    ev.record(0, s);
    launch();
    GWM_CHECK(hipGetLastError());
    ev.record(1, s);
    const float ms = ev.ms(0, 1); // waits
    if (ms_out)
        *ms_out = ms;
}

// The byte maps of copy_slice: a base as it is, and through the aligner's complement table.
struct AsItIs
{
    __device__ __forceinline__ uint8_t operator()(uint8_t c) const { return c; }
};
struct Complement
{
    __device__ __forceinline__ uint8_t operator()(uint8_t c) const { return static_cast<uint8_t>("TGAC"[(c >> 1) & 3]); }
};

// A block copies the slice src[0 .. len) to dst: forward through `forward`, or with `reversed` back to front through
// `backward`. Thread L of a pass takes output byte L: ascending addresses on both sides, or descending ones on the
// read side when reversed -- one segment per wave either way.
template <typename Out, typename Length, typename Forward, typename Backward>
__device__ __forceinline__ void copy_slice(Out* dst, const uint8_t* src, Length len, bool reversed, Forward forward,
                                           Backward backward)
{
    if (reversed)
    {
        for (Length j = threadIdx.x; j < len; j += kThreads)
            dst[j] = static_cast<Out>(backward(src[len - 1 - j]));
    }
    else
    {
        for (Length j = threadIdx.x; j < len; j += kThreads)
            dst[j] = static_cast<Out>(forward(src[j]));
    }
}

// copy_slice by one wave64, for slices of a few hundred bytes: lane L of a pass takes output byte L
template <typename Out, typename Length, typename Forward, typename Backward>
__device__ __forceinline__ void copy_slice_wave(Out* dst, const uint8_t* src, Length len, bool reversed, Forward forward,
                                                Backward backward)
{
    const Length lane = threadIdx.x & 63u;
    if (reversed)
    {
        for (Length j = lane; j < len; j += 64)
            dst[j] = static_cast<Out>(backward(src[len - 1 - j]));
    }
    else
    {
        for (Length j = lane; j < len; j += 64)
            dst[j] = static_cast<Out>(forward(src[j]));
    }
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

} // namespace

#endif
