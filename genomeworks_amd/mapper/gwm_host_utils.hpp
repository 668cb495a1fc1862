// gwm_host_utils.hpp -- the part of the cudamapper helpers that needs nothing but hip_runtime.h, so the host sources
// (mapper.cpp, gwm_driver.cpp) share it with the .hip translation units, which get it through gwm_device_utils.hpp:
// checked HIP calls, the owning device buffer, HIP-event timers and the device read set.
// Everything here but the read set has internal linkage; what a translation unit does not use is `inline` and so
// warns nowhere.
#ifndef GWM_HOST_UTILS_HPP
#define GWM_HOST_UTILS_HPP

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

namespace gwm
{

// A read set on the device: bases[offsets[i] .. offsets[i + 1]) is read first_read_id + i. Not in the unnamed
// namespace below: align_chunks() (gwm_align_chunks.hpp) takes it across translation units.
struct ReadSet
{
    const uint8_t* bases;
    const int64_t* offsets;
    uint32_t n_reads;
    uint32_t first_read_id;
};

} // namespace gwm

namespace
{

using gwm::ReadSet;

inline void check(hipError_t e, const char* what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#define GWM_CHECK(x) check((x), #x)

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
    // a device copy of host[0 .. count), ready when this returns
    void upload(const T* host, int64_t count)
    {
        resize(count);
        if (count > 0)
            check(hipMemcpy(p, host, sizeof(T) * static_cast<size_t>(count), hipMemcpyHostToDevice), "hipMemcpy H2D");
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
