// owned_hip.hpp -- streams, events and threads owned for the length of a call, released on every exit path.
#pragma once
#include <claraparabricks/genomeworks/utils/cudautils.hpp>

#include <thread>
#include <utility>
#include <vector>

namespace gwhost
{
using claraparabricks::genomeworks::scoped_device_switch;

struct OwnedStreams // (the device is switched per stream)
{
    std::vector<std::pair<int32_t, hipStream_t>> items;
    OwnedStreams()                               = default;
    OwnedStreams(const OwnedStreams&)            = delete;
    OwnedStreams& operator=(const OwnedStreams&) = delete;
    hipStream_t create(int32_t device, bool with_priority = false, int priority = 0)
    {
        scoped_device_switch dev(device);
        hipStream_t s = nullptr;
        if (with_priority) GW_CU_CHECK_ERR(hipStreamCreateWithPriority(&s, hipStreamDefault, priority));
        else GW_CU_CHECK_ERR(hipStreamCreate(&s));
        items.emplace_back(device, s);
        return s;
    }
    ~OwnedStreams()
    {
        for (auto& it : items)
        {
            scoped_device_switch dev(it.first);
            (void)hipStreamDestroy(it.second);
        }
    }
};
struct OwnedEvents
{
    std::vector<hipEvent_t> items;
    OwnedEvents()                              = default;
    OwnedEvents(const OwnedEvents&)            = delete;
    OwnedEvents& operator=(const OwnedEvents&) = delete;
    hipEvent_t create(unsigned flags = hipEventDisableTiming)
    {
        hipEvent_t e = nullptr;
        GW_CU_CHECK_ERR(hipEventCreateWithFlags(&e, flags));
        items.push_back(e);
        return e;
    }
    ~OwnedEvents()
    {
        for (hipEvent_t e : items) (void)hipEventDestroy(e);
    }
};
// joins whatever was started, also when spawning the next thread throws
struct JoinAll
{
    std::vector<std::thread>& threads;
    ~JoinAll()
    {
        for (std::thread& t : threads)
            if (t.joinable()) t.join();
    }
};
} // namespace gwhost
