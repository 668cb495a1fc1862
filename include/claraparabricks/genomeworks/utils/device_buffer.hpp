// device_buffer.hpp -- an owning, fixed-size array in device memory, taken from a DefaultDeviceAllocator (or any
// allocator with allocate(n, streams) / deallocate(p, n)). Elements are not constructed or destroyed.
#pragma once

#include <claraparabricks/genomeworks/utils/allocator.hpp>

#include <cstddef>
#include <type_traits>
#include <utility>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace details
{

template <typename T, typename Allocator>
class buffer
{
    static_assert(std::is_trivially_copyable<T>::value, "device buffers hold trivially copyable types only");

public:
    using value_type     = T;
    using size_type      = std::ptrdiff_t;
    using iterator       = value_type*;
    using const_iterator = const value_type*;
    using allocator_type = Allocator;

    buffer() = default;

    /// n elements from `allocator`, associated with `streams` (the allocator's default stream when none is given).
    template <typename AllocatorIn, typename... Streams>
    explicit buffer(size_type n, AllocatorIn allocator, Streams... streams)
        : size_(n)
        , streams_({streams...})
        , allocator_(allocator)
    {
        if (size_ > 0) data_ = allocator_.allocate(static_cast<std::size_t>(size_), streams_);
    }

    /// An empty buffer bound to `allocator`.
    template <typename AllocatorIn, std::enable_if_t<std::is_class<AllocatorIn>::value, int> = 0>
    explicit buffer(AllocatorIn allocator)
        : allocator_(allocator)
    {
    }

    buffer(const buffer&) = delete;
    buffer& operator=(const buffer&) = delete;
    buffer(buffer&& rhs) noexcept { swap(rhs); }
    buffer& operator=(buffer&& rhs) noexcept
    {
        if (this != &rhs)
        {
            free();
            swap(rhs);
        }
        return *this;
    }
    ~buffer() { free(); }

    value_type* data() { return data_; }
    const value_type* data() const { return data_; }
    size_type size() const { return size_; }
    iterator begin() { return data_; }
    iterator end() { return data_ + size_; }
    const_iterator begin() const { return data_; }
    const_iterator end() const { return data_ + size_; }
    allocator_type get_allocator() const { return allocator_; }

    /// Returns the memory to the allocator; the buffer becomes empty.
    void free()
    {
        if (data_ != nullptr) allocator_.deallocate(data_, static_cast<std::size_t>(size_));
        data_ = nullptr;
        size_ = 0;
    }

    /// Drops the contents and holds new_size (uninitialised) elements.
    void clear_and_resize(size_type new_size)
    {
        if (new_size == size_) return;
        free();
        size_ = new_size;
        if (size_ > 0) data_ = allocator_.allocate(static_cast<std::size_t>(size_), streams_);
    }

    void swap(buffer& o) noexcept
    {
        using std::swap;
        swap(data_, o.data_);
        swap(size_, o.size_);
        swap(streams_, o.streams_);
        swap(allocator_, o.allocator_);
    }

private:
    value_type* data_ = nullptr;
    size_type size_   = 0;
    std::vector<cudaStream_t> streams_;
    allocator_type allocator_;
};

template <typename T, typename A>
void swap(buffer<T, A>& a, buffer<T, A>& b) noexcept
{
    a.swap(b);
}

} // namespace details

/// Device array on the default (caching) allocator.
template <typename T>
using device_buffer = details::buffer<T, CachingDeviceAllocator<T>>;

} // namespace genomeworks
} // namespace claraparabricks
