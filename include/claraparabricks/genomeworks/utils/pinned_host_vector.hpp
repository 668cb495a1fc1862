// pinned_host_vector.hpp -- std::vector in page-locked host memory, so copies to and from the device run
// asynchronously at link speed.
#pragma once

#include <claraparabricks/genomeworks/utils/exceptions.hpp>

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <new>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace details
{

/// Allocator of page-locked host memory (hipHostMalloc / hipHostFree).
template <typename T>
struct pinned_allocator
{
    using value_type = T;
    pinned_allocator() = default;
    template <typename U>
    pinned_allocator(const pinned_allocator<U>&) noexcept
    {
    }
    T* allocate(std::size_t n)
    {
        void* p = nullptr;
        if (n == 0) return nullptr;
        if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess)
        {
            (void)hipGetLastError();
            throw std::bad_alloc();
        }
        return static_cast<T*>(p);
    }
    void deallocate(T* p, std::size_t) noexcept
    {
        if (p != nullptr) (void)hipHostFree(p);
    }
};
template <typename T, typename U>
bool operator==(const pinned_allocator<T>&, const pinned_allocator<U>&) { return true; }
template <typename T, typename U>
bool operator!=(const pinned_allocator<T>&, const pinned_allocator<U>&) { return false; }

} // namespace details

/// A vector whose storage is pinned host memory.
template <typename T>
using pinned_host_vector = std::vector<T, details::pinned_allocator<T>>;

} // namespace genomeworks
} // namespace claraparabricks
