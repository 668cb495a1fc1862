// host_common.hpp -- small shared helpers of the host library.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>

namespace gwhost
{
inline std::string& last_error()
{
    static thread_local std::string e;
    return e;
}
inline void set_last_error(const std::string& s) { last_error() = s; }

/// Runs task(0) .. task(n_tasks - 1), each exactly once, on the calling thread and up to max_threads - 1 workers of a
/// process-wide pool (created on first use, parked on a condition variable in between; runtime.cpp). The pool serves one
/// caller at a time: a second caller that arrives meanwhile runs its tasks itself. An exception thrown by a task is
/// rethrown here once every task has finished. The un-reversal of a batch's results takes a few hundred microseconds; starting and joining
/// std::threads for it cost as much as the work.
void parallel_tasks(size_t n_tasks, size_t max_threads, const std::function<void(size_t)>& task);

inline size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

/// The arrays of one device block, back to back, each on a 256-byte boundary: take<T>(count) reserves count elements and
/// says where they start, `bytes` is the size of the block once everything is taken.
struct BlockLayout
{
    template <typename T>
    struct Slot
    {
        size_t offset;
        T* in(char* block) const { return reinterpret_cast<T*>(block + offset); }
    };
    size_t bytes = 0;
    template <typename T>
    Slot<T> take(size_t count)
    {
        const Slot<T> slot{bytes};
        bytes += up256(count * sizeof(T));
        return slot;
    }
};

/// dst[k] = src[count - 1 - k] (the aligner kernels write a path back to front): eight bytes at a time as one byte-swapped
/// 64-bit word, the tail byte by byte. The ranges must not overlap.
inline void reverse_bytes(void* dst, const void* src, size_t count)
{
    uint8_t* d       = static_cast<uint8_t*>(dst);
    const uint8_t* s = static_cast<const uint8_t*>(src);
    size_t k         = 0;
    for (; k + 8 <= count; k += 8)
    {
        uint64_t v;
        std::memcpy(&v, s + count - 8 - k, 8);
        v = __builtin_bswap64(v);
        std::memcpy(d + k, &v, 8);
    }
    for (; k < count; ++k) d[k] = s[count - 1 - k];
}

/// The same for 16-bit values (cudapoa's coverage counters): four at a time through a 64-bit word.
inline void reverse_u16(uint16_t* dst, const uint16_t* src, size_t count)
{
    size_t k = 0;
    for (; k + 4 <= count; k += 4)
    {
        uint64_t v;
        std::memcpy(&v, src + count - 4 - k, 8);
        v = (v >> 48) | ((v >> 16) & 0xffff0000ull) | ((v << 16) & 0xffff00000000ull) | (v << 48);
        std::memcpy(dst + k, &v, 8);
    }
    for (; k < count; ++k) dst[k] = src[count - 1 - k];
}
} // namespace gwhost
