// gwm_index_cache.hip -- packed host copies of cudamapper indices (libcudamapper.so, gfx950): gwm_index_pack moves an
// index into one pinned host slab, gwm_index_unpack brings it back into one device allocation. The restore replaces an
// index build on every pair the driver's index cache serves, and it is bound by the host link, so the slab holds only
// what cannot be recomputed: read ids, positions, one direction bit per element and the unique-representation tables.
// The 8 B representation of every element is redundant with unique_representations / first_occurrence and is expanded
// on the device again. Layout and rules: include/gwhip_mapper.h.
#include "gwhip_mapper.h"

#include "gwm_device_utils.hpp"

#include <cstddef>
#include <cstring>

namespace
{

constexpr int64_t kHeaderBytes = 64;
constexpr uint64_t kMagic      = 0x3158444950574d47ull; // "GWMPIDX1"

// what the slab starts with; the arrays follow in slab_layout's order
struct slab_header
{
    uint64_t magic;
    int64_t n;
    int64_t n_unique;
    int64_t n_first_occurrence;
    uint32_t first_read_id;
    uint32_t number_of_reads;
    uint32_t number_of_basepairs_in_longest_read;
    uint32_t bad_direction; // set by the pack kernel: a direction byte other than 0 or 1
    uint8_t reserved[16];
};
static_assert(sizeof(slab_header) == kHeaderBytes, "slab header");

inline int64_t align16(int64_t x) { return (x + 15) & ~int64_t(15); }

// Byte offsets of the sections. The host slab ends at `host_bytes`; the device allocation of a restored index is the
// same bytes followed by the two arrays that are expanded on the device.
struct slab_layout
{
    int64_t read_ids, positions, bitmap, unique, first, host_bytes, representations, directions, device_bytes;
    slab_layout(int64_t n, int64_t n_unique, int64_t n_first)
    {
        read_ids        = kHeaderBytes;
        positions       = align16(read_ids + 4 * n);
        bitmap          = align16(positions + 4 * n);
        unique          = align16(bitmap + 8 * ((n + 63) / 64));
        first           = align16(unique + 8 * n_unique);
        host_bytes      = first + 4 * n_first;
        representations = align16(host_bytes);
        directions      = align16(representations + 8 * n);
        device_bytes    = directions + n;
    }
};

// Consecutive lanes take consecutive elements; the wave's ballot of direction != 0 is bitmap word i / 64. Lanes beyond n
// vote 0, so the tail word carries zero bits there. A byte other than 0 or 1 raises *bad (every such lane stores the
// same 1).
__global__ void __launch_bounds__(kThreads) pack_directions_kernel(const uint8_t* __restrict__ directions, int64_t n,
                                                                  uint64_t* __restrict__ bitmap,
                                                                  uint32_t* __restrict__ bad)
{
    const int64_t i         = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const uint8_t d         = i < n ? directions[i] : uint8_t(0);
    const uint64_t word     = __ballot(d != 0);
    if (d > 1)
        *bad = 1u;
    if ((threadIdx.x & 63) == 0 && i < n)
        bitmap[i >> 6] = word;
}

// Element i takes the representation of the section it lies in: the last u with first_occurrence[u] <= i, which skips
// empty sections (first_occurrence[u] == first_occurrence[u + 1]). An element that no section covers gets 0, as
// gwm_index_from_arrays leaves it.
__global__ void __launch_bounds__(kThreads) expand_representations_kernel(
    const uint64_t* __restrict__ unique, const uint32_t* __restrict__ first_occurrence, int64_t n_unique, int64_t n,
    uint64_t* __restrict__ representations)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n)
        return;
    // upper bound of i in first_occurrence[0 .. n_unique]
    int64_t lo = 0, hi = n_unique > 0 ? n_unique + 1 : 0;
    while (lo < hi)
    {
        const int64_t mid = lo + (hi - lo) / 2;
        if (static_cast<int64_t>(first_occurrence[mid]) <= i)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int64_t u    = lo - 1;
    representations[i] = (u >= 0 && u < n_unique) ? unique[u] : uint64_t(0);
}

__global__ void __launch_bounds__(kThreads) unpack_directions_kernel(const uint64_t* __restrict__ bitmap, int64_t n,
                                                                    uint8_t* __restrict__ directions)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (i < n)
        directions[i] = static_cast<uint8_t>((bitmap[i >> 6] >> (i & 63)) & 1u);
}

void check_grid(int64_t n)
{
    if (n < 0 || n >= (int64_t(1) << 32) - 1)
        throw std::invalid_argument("an index holds at most 2^32 - 2 elements");
}

} // namespace

extern "C" {

void gwm_index_host_copy_free(gwm_index_host_copy* copy)
{
    if (!copy)
        return;
    if (copy->slab)
        (void)hipHostFree(copy->slab);
    std::memset(copy, 0, sizeof(*copy));
}

int64_t gwm_index_host_copy_bytes(const gwm_index_host_copy* copy) { return copy ? copy->bytes : 0; }

int gwm_index_pack(const gwm_index* x, void* stream, gwm_index_host_copy* out)
{
    std::memset(out, 0, sizeof(*out));
    try
    {
        hipStream_t s = static_cast<hipStream_t>(stream);
        check_grid(x->n);
        if (x->n_unique < 0 || x->n_first_occurrence < 0)
            throw std::invalid_argument("gwm_index_pack: negative array size");
        if (x->n_first_occurrence != 0 && x->n_first_occurrence != x->n_unique + 1)
            throw std::invalid_argument("gwm_index_pack: first_occurrence has to hold n_unique + 1 entries, or none");
        const slab_layout at(x->n, x->n_unique, x->n_first_occurrence);
        GWM_CHECK(hipHostMalloc(&out->slab, static_cast<size_t>(at.host_bytes), hipHostMallocDefault));
        out->bytes = at.host_bytes;
        char* slab = static_cast<char*>(out->slab);
        slab_header h{};
        h.magic                               = kMagic;
        h.n                                   = x->n;
        h.n_unique                            = x->n_unique;
        h.n_first_occurrence                  = x->n_first_occurrence;
        h.first_read_id                       = x->first_read_id;
        h.number_of_reads                     = x->number_of_reads;
        h.number_of_basepairs_in_longest_read = x->number_of_basepairs_in_longest_read;
        std::memcpy(slab, &h, sizeof(h));

        Events ev(2);
        ev.record(0, s);
        dbuf<uint64_t> bitmap;
        dbuf<uint32_t> bad;
        if (x->n > 0)
        {
            bitmap.resize((x->n + 63) / 64);
            bad.resize(1);
            GWM_CHECK(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
            pack_directions_kernel<<<grid_for(x->n), kThreads, 0, s>>>(x->directions, x->n, bitmap.p, bad.p);
            GWM_CHECK(hipGetLastError());
            GWM_CHECK(hipMemcpyAsync(slab + at.read_ids, x->read_ids, 4 * x->n, hipMemcpyDeviceToHost, s));
            GWM_CHECK(hipMemcpyAsync(slab + at.positions, x->positions_in_reads, 4 * x->n, hipMemcpyDeviceToHost, s));
            GWM_CHECK(hipMemcpyAsync(slab + at.bitmap, bitmap.p, 8 * bitmap.n, hipMemcpyDeviceToHost, s));
            GWM_CHECK(hipMemcpyAsync(slab + offsetof(slab_header, bad_direction), bad.p, sizeof(uint32_t),
                                     hipMemcpyDeviceToHost, s));
        }
        if (x->n_unique > 0)
            GWM_CHECK(hipMemcpyAsync(slab + at.unique, x->unique_representations, 8 * x->n_unique,
                                     hipMemcpyDeviceToHost, s));
        if (x->n_first_occurrence > 0)
            GWM_CHECK(hipMemcpyAsync(slab + at.first, x->first_occurrence_of_representations,
                                     4 * x->n_first_occurrence, hipMemcpyDeviceToHost, s));
        ev.record(1, s);
        out->pack_ms = ev.ms(0, 1); // waits for the last copy: the slab is complete when this returns
        std::memcpy(&h, slab, sizeof(h));
        if (h.bad_direction != 0)
            throw std::invalid_argument("gwm_index_pack: a direction is neither 0 nor 1; one bit cannot hold it");
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        gwm_index_host_copy_free(out);
        return -1;
    }
}

int gwm_index_unpack(const gwm_index_host_copy* copy, void* stream, gwm_index* out)
{
    std::memset(out, 0, sizeof(*out));
    try
    {
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (!copy || !copy->slab || copy->bytes < kHeaderBytes)
            throw std::invalid_argument("gwm_index_unpack: not a packed index");
        slab_header h;
        std::memcpy(&h, copy->slab, sizeof(h));
        if (h.magic != kMagic || h.n_unique < 0 || h.n_first_occurrence < 0 ||
            (h.n_first_occurrence != 0 && h.n_first_occurrence != h.n_unique + 1))
            throw std::invalid_argument("gwm_index_unpack: not a packed index");
        check_grid(h.n);
        const slab_layout at(h.n, h.n_unique, h.n_first_occurrence);
        if (at.host_bytes != copy->bytes)
            throw std::invalid_argument("gwm_index_unpack: the slab size does not match its header");
        out->n                                   = h.n;
        out->n_unique                            = h.n_unique;
        out->n_first_occurrence                  = h.n_first_occurrence;
        out->first_read_id                       = h.first_read_id;
        out->number_of_reads                     = h.number_of_reads;
        out->number_of_basepairs_in_longest_read = h.number_of_basepairs_in_longest_read;
        if (h.n == 0 && h.n_unique == 0 && h.n_first_occurrence == 0)
            return 0; // nothing on the device, as gwm_index_build leaves an empty index
        dbuf<char> d(at.device_bytes);
        // one copy: the device allocation starts with the slab's bytes
        GWM_CHECK(hipMemcpyAsync(d.p, copy->slab, static_cast<size_t>(at.host_bytes), hipMemcpyHostToDevice, s));
        const uint64_t* unique = reinterpret_cast<const uint64_t*>(d.p + at.unique);
        const uint32_t* first  = reinterpret_cast<const uint32_t*>(d.p + at.first);
        uint64_t* rep          = reinterpret_cast<uint64_t*>(d.p + at.representations);
        uint8_t* dir           = reinterpret_cast<uint8_t*>(d.p + at.directions);
        if (h.n > 0)
        {
            expand_representations_kernel<<<grid_for(h.n), kThreads, 0, s>>>(
                unique, first, h.n_first_occurrence > 0 ? h.n_unique : 0, h.n, rep);
            GWM_CHECK(hipGetLastError());
            unpack_directions_kernel<<<grid_for(h.n), kThreads, 0, s>>>(
                reinterpret_cast<const uint64_t*>(d.p + at.bitmap), h.n, dir);
            GWM_CHECK(hipGetLastError());
        }
        out->representations    = h.n > 0 ? rep : nullptr;
        out->read_ids           = h.n > 0 ? reinterpret_cast<uint32_t*>(d.p + at.read_ids) : nullptr;
        out->positions_in_reads = h.n > 0 ? reinterpret_cast<uint32_t*>(d.p + at.positions) : nullptr;
        out->directions         = h.n > 0 ? dir : nullptr;
        out->unique_representations              = h.n_unique > 0 ? const_cast<uint64_t*>(unique) : nullptr;
        out->first_occurrence_of_representations = h.n_first_occurrence > 0 ? const_cast<uint32_t*>(first) : nullptr;
        out->device_slab                         = d.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        gwm_index_free(out);
        return -1;
    }
}

} // extern "C"
