// gwhip_device_facts.h -- what the launch code asks the current device: how many CUs it has (grids that fill the device,
// kernel choices by occupancy) and how much LDS one block may ask for.
//
// device_facts() answers for the device that is current on the calling thread. The answers are cached per device id below
// kCachedDevices, filled by whichever host thread asks first (every thread would store the same values); a higher id is asked
// every time. A query that fails leaves its fallback (256 CUs, 64 KiB) and clears HIP's sticky error, so that the launch that
// follows does not report it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace gwhip
{

struct DeviceFacts
{
    int cus;               // hipDeviceAttributeMultiprocessorCount
    int max_lds_per_block; // hipDeviceAttributeMaxSharedMemoryPerBlock, bytes
};

inline DeviceFacts device_facts()
{
    constexpr int kCachedDevices = 64;
    static std::atomic<int> cus_of[kCachedDevices], lds_of[kCachedDevices]; // zero-initialised: 0 = not asked yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
    {
        (void)hipGetLastError();
        return {256, 64 * 1024};
    }
    const bool cached = dev >= 0 && dev < kCachedDevices;
    if (cached)
        if (const int cus = cus_of[dev].load(std::memory_order_acquire)) return {cus, lds_of[dev].load(std::memory_order_relaxed)};
    DeviceFacts f{0, 0};
    if (hipDeviceGetAttribute(&f.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || f.cus <= 0)
    {
        (void)hipGetLastError();
        f.cus = 256;
    }
    if (hipDeviceGetAttribute(&f.max_lds_per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || f.max_lds_per_block <= 0)
    {
        (void)hipGetLastError();
        f.max_lds_per_block = 64 * 1024;
    }
    if (cached)
    {
        lds_of[dev].store(f.max_lds_per_block, std::memory_order_relaxed);
        cus_of[dev].store(f.cus, std::memory_order_release); // last: a reader that sees it sees an LDS figure too
    }
    return f;
}

} // namespace gwhip
