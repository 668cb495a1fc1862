// thrust/simt_algorithms.h -- TEST INFRASTRUCTURE (oracle/simt): stand-ins for the thrust calls of the reference's cudamapper
// sources, written here as plain sequential loops over host memory ("device" memory of the emulator is host memory). Each one
// states the documented result of the thrust algorithm of the same name; nothing is taken from a thrust tree. The execution
// policy `thrust::cuda::par(allocator).on(stream)` is accepted and ignored. Every thrust/*.h of this directory includes this file.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <numeric>
#include <type_traits>
#include <utility>
#include <vector>

#include <cuda_runtime_api.h>

namespace thrust
{
// ---- execution policy ----------------------------------------------------------------------------------------------
struct simt_policy
{
    simt_policy on(cudaStream_t) const { return *this; }
};
namespace cuda
{
struct par_t : simt_policy
{
    template <typename Allocator>
    simt_policy operator()(const Allocator&) const
    {
        return simt_policy{};
    }
};
static const par_t par{};
} // namespace cuda
static const simt_policy device{};
static const simt_policy host{};

// ---- functors, iterators, containers ---------------------------------------------------------------------------------
template <typename T>
struct plus
{
    T operator()(const T& a, const T& b) const { return a + b; }
};

template <typename T>
class counting_iterator
{
public:
    using value_type        = T;
    using difference_type   = std::ptrdiff_t;
    using reference         = T;
    using pointer           = const T*;
    using iterator_category = std::random_access_iterator_tag;
    counting_iterator() = default;
    explicit counting_iterator(T v) : v_(v) {}
    T operator*() const { return v_; }
    T operator[](difference_type i) const { return static_cast<T>(v_ + i); }
    counting_iterator& operator++() { ++v_; return *this; }
    counting_iterator operator++(int) { counting_iterator c = *this; ++v_; return c; }
    counting_iterator operator+(difference_type i) const { return counting_iterator(static_cast<T>(v_ + i)); }
    difference_type operator-(const counting_iterator& o) const { return static_cast<difference_type>(v_) - static_cast<difference_type>(o.v_); }
    bool operator==(const counting_iterator& o) const { return v_ == o.v_; }
    bool operator!=(const counting_iterator& o) const { return v_ != o.v_; }
    bool operator<(const counting_iterator& o) const { return v_ < o.v_; }

private:
    T v_{};
};
template <typename T>
counting_iterator<T> make_counting_iterator(T v)
{
    return counting_iterator<T>(v);
}

template <typename T>
using host_vector = std::vector<T>;

// ---- algorithms -------------------------------------------------------------------------------------------------------
// out[i] = in[0] + ... + in[i]; `out` may be `first`
template <typename Policy, typename In, typename Out>
Out inclusive_scan(const Policy&, In first, In last, Out out)
{
    if (first == last) return out;
    auto acc = *first;
    *out++   = acc;
    for (++first; first != last; ++first)
    {
        acc    = acc + *first;
        *out++ = acc;
    }
    return out;
}
// out[i] = 0 + in[0] + ... + in[i - 1]
template <typename Policy, typename In, typename Out>
Out exclusive_scan(const Policy&, In first, In last, Out out)
{
    typename std::iterator_traits<In>::value_type acc = 0;
    for (; first != last; ++first)
    {
        const auto v = *first; // (read before the store: `out` may be `first`)
        *out++       = acc;
        acc          = acc + v;
    }
    return out;
}
// out[i] = op(... op(f(in[0]), f(in[1])) ..., f(in[i]))
template <typename Policy, typename In, typename Out, typename Unary, typename Binary>
Out transform_inclusive_scan(const Policy&, In first, In last, Out out, Unary f, Binary op)
{
    if (first == last) return out;
    using Acc = std::decay_t<decltype(op(f(*first), f(*first)))>;
    Acc acc   = f(*first);
    *out++    = acc;
    for (++first; first != last; ++first)
    {
        acc    = op(acc, f(*first));
        *out++ = acc;
    }
    return out;
}
// out[i] = op(... op(init, f(in[0])) ..., f(in[i - 1]))
template <typename Policy, typename In, typename Out, typename Unary, typename Init, typename Binary>
Out transform_exclusive_scan(const Policy&, In first, In last, Out out, Unary f, Init init, Binary op)
{
    using Acc = std::decay_t<decltype(op(f(*first), f(*first)))>;
    Acc acc   = static_cast<Acc>(init);
    for (; first != last; ++first)
    {
        const auto v = f(*first);
        *out++       = acc;
        acc          = op(acc, v);
    }
    return out;
}
// keys ascending, equal keys in their input order, the values moved with their keys
template <typename Policy, typename KeyIt, typename ValueIt>
void stable_sort_by_key(const Policy&, KeyIt kfirst, KeyIt klast, ValueIt vfirst)
{
    const size_t n = static_cast<size_t>(klast - kfirst);
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), size_t(0));
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return kfirst[a] < kfirst[b]; });
    std::vector<typename std::iterator_traits<KeyIt>::value_type> keys(n);
    std::vector<typename std::iterator_traits<ValueIt>::value_type> values(n);
    for (size_t i = 0; i < n; ++i)
    {
        keys[i]   = kfirst[order[i]];
        values[i] = vfirst[order[i]];
    }
    for (size_t i = 0; i < n; ++i)
    {
        kfirst[i] = keys[i];
        vfirst[i] = values[i];
    }
}
// out[0] = in[0], out[i] = in[i] - in[i - 1]
template <typename Policy, typename In, typename Out>
Out adjacent_difference(const Policy&, In first, In last, Out out)
{
    if (first == last) return out;
    auto prev = *first;
    *out++    = prev;
    for (++first; first != last; ++first)
    {
        const auto cur = *first;
        *out++         = cur - prev;
        prev           = cur;
    }
    return out;
}
template <typename Policy, typename It, typename Pred, typename T>
void replace_if(const Policy&, It first, It last, Pred pred, const T& value)
{
    for (; first != last; ++first)
        if (pred(*first)) *first = value;
}
// the elements with pred(element), in their order
template <typename Policy, typename In, typename Out, typename Pred>
Out copy_if(const Policy&, In first, In last, Out out, Pred pred)
{
    for (; first != last; ++first)
        if (pred(*first)) *out++ = *first;
    return out;
}
// the elements with pred(stencil element), in their order
template <typename Policy, typename In, typename Stencil, typename Out, typename Pred>
Out copy_if(const Policy&, In first, In last, Stencil stencil, Out out, Pred pred)
{
    for (; first != last; ++first, ++stencil)
        if (pred(*stencil)) *out++ = *first;
    return out;
}
template <typename Policy, typename In, typename Out, typename Op>
Out transform(const Policy&, In first, In last, Out out, Op op)
{
    for (; first != last; ++first) *out++ = op(*first);
    return out;
}
// first[i] = i
template <typename Policy, typename It>
void sequence(const Policy&, It first, It last)
{
    typename std::iterator_traits<It>::value_type i = 0;
    for (; first != last; ++first) *first = i++;
}
// out[i] = input[map[i]]
template <typename Policy, typename MapIt, typename In, typename Out>
Out gather(const Policy&, MapIt map_first, MapIt map_last, In input, Out out)
{
    for (; map_first != map_last; ++map_first) *out++ = input[*map_first];
    return out;
}
template <typename Policy, typename It>
bool is_sorted(const Policy&, It first, It last)
{
    return std::is_sorted(first, last);
}
template <typename Policy, typename It, typename Compare>
bool is_sorted(const Policy&, It first, It last, Compare comp)
{
    return std::is_sorted(first, last, comp);
}
} // namespace thrust
