// gwx_ungapped_xdrop.hip -- cudaextender's ungapped X-drop extension on gfx950 (include/gwhip_extender.h).
//
// One wave64 per seed. A direction is walked in 64-column tiles; per tile the wave does
//   s    = inclusive add-scan of the column scores + the carried prefix score       (DPP, 6 steps)
//   m    = inclusive max-scan of s, combined with the carried best score m >= 0     (DPP, 6 steps)
//   stop = first lane with m - s > X (ballot), clipped to the lanes inside the sequences
//   best = m at lane stop-1; if it grew, its first position = first lane with s == best (ballot)
// All carried state (prefix, best, position) is wave-uniform and lives in SGPRs (readlane / readfirstlane). The
// entropy counts are a second pass over [t - lpos, t + rpos], taken only for seeds whose total is in [thr, 3 thr]:
// per tile one ballot per base and a popcount. The result is sequential by construction: it does not depend on
// the tile width (tests/oracle_extender.c is the position-at-a-time statement).
//
// Then: rocPRIM select (compaction in seed order), two stable radix sorts (key ~length:~score, then diagonal:target), a
// gather, the adjacent-overlap flags of thrust::unique_copy and a second select.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>

#include "gwhip_extender.h"

namespace
{

thread_local std::string g_error;
bool g_count_positions = false;
int64_t g_last_positions = 0;

constexpr int kWave  = 64;
constexpr int kBlock = 256; // 4 waves

int fail(const std::string& what)
{
    g_error = what;
    return -1;
}
#define GWX_CHECK(call)                                                                                               \
    do                                                                                                                \
    {                                                                                                                 \
        hipError_t e_ = (call);                                                                                       \
        if (e_ != hipSuccess) return fail(std::string(#call) + ": " + hipGetErrorString(e_));                        \
    } while (0)

// ---- wave64 scans (gfx9 DPP row-shift / row-broadcast sequence, as in csrc/poa_device.h) ----
__device__ __forceinline__ int32_t wave_inclusive_add(int32_t v)
{
#define GWX_DPP_ADD(ctrl, rmask) v += __builtin_amdgcn_update_dpp(0, v, ctrl, rmask, 0xf, false)
    GWX_DPP_ADD(0x111, 0xf); // row_shr:1
    GWX_DPP_ADD(0x112, 0xf); // row_shr:2
    GWX_DPP_ADD(0x114, 0xf); // row_shr:4
    GWX_DPP_ADD(0x118, 0xf); // row_shr:8
    GWX_DPP_ADD(0x142, 0xa); // row_bcast:15 into rows 1,3
    GWX_DPP_ADD(0x143, 0xc); // row_bcast:31 into rows 2,3
#undef GWX_DPP_ADD
    return v;
}
__device__ __forceinline__ int32_t wave_inclusive_max(int32_t v)
{
    constexpr int32_t ident = INT32_MIN;
#define GWX_DPP_MAX(ctrl, rmask) v = max(v, __builtin_amdgcn_update_dpp(ident, v, ctrl, rmask, 0xf, false))
    GWX_DPP_MAX(0x111, 0xf);
    GWX_DPP_MAX(0x112, 0xf);
    GWX_DPP_MAX(0x114, 0xf);
    GWX_DPP_MAX(0x118, 0xf);
    GWX_DPP_MAX(0x142, 0xa);
    GWX_DPP_MAX(0x143, 0xc);
#undef GWX_DPP_MAX
    return v;
}
__device__ __forceinline__ int32_t uniform(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int32_t lane_value(int32_t v, int32_t lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ int32_t first_lane(uint64_t mask) { return mask ? (int32_t)__builtin_ctzll(mask) : kWave; }

struct Walk
{
    int32_t best; // max(0, prefix scores before the X-drop stop)
    int32_t pos;  // offset of its first occurrence, or the caller's "none" value
    int32_t cols; // columns examined
};

// One direction from (t, q). dir = +1: offsets k = 0, 1, ... (column t+k, q+k); dir = -1: offsets k = 1, 2, ...
// (column t-k, q-k). `avail` = number of columns inside both sequences in that direction.
__device__ __forceinline__ Walk walk(const int8_t* __restrict__ T, const int8_t* __restrict__ Q, const int32_t* sub,
                                     int32_t t, int32_t q, int32_t dir, int32_t avail, int32_t xdrop, int32_t none_pos,
                                     int32_t lane)
{
    const int32_t k0 = dir > 0 ? 0 : 1;
    int32_t carry = 0, best = 0, pos = none_pos, base = 0;
    while (true)
    {
        const int32_t idx  = base + lane;            // 0-based column index in this direction
        const bool inside  = idx < avail;
        const int32_t k    = k0 + idx;
        int32_t v          = 0;
        if (inside) v = sub[8 * T[t + dir * k] + Q[q + dir * k]];
        const int32_t s    = wave_inclusive_add(v) + carry;
        const int32_t m    = max(wave_inclusive_max(s), best);
        const uint64_t drop = __ballot(inside && m - s > xdrop);
        const int32_t n_in = min(avail - base, kWave); // wave-uniform, may be <= 0 only when avail == base == 0
        const int32_t stop = min(first_lane(drop), n_in);
        if (stop > 0)
        {
            const int32_t cand = lane_value(m, stop - 1);
            if (cand > best)
            {
                const uint64_t hit = __ballot(s == cand && lane < stop);
                best = cand;
                pos  = k0 + base + first_lane(hit);
            }
        }
        if (drop != 0 || n_in < kWave || avail - base == kWave)
            return Walk{best, pos, base + max(stop, 0) + (drop != 0 ? 1 : 0)};
        carry = lane_value(s, kWave - 1);
        best  = uniform(max(best, lane_value(m, kWave - 1)));
        base += kWave;
    }
}

__global__ __launch_bounds__(kBlock) void ungapped_xdrop_kernel(gwx_problem p, const gwx_seed* __restrict__ seeds,
                                                                int32_t n, gwx_segment* __restrict__ segments,
                                                                uint8_t* __restrict__ keep,
                                                                unsigned long long* positions)
{
    __shared__ int32_t sub[64];
    if (threadIdx.x < 64) sub[threadIdx.x] = p.score_matrix[threadIdx.x];
    __syncthreads();
    const int32_t lane   = threadIdx.x & (kWave - 1);
    const int32_t waves  = gridDim.x * (kBlock / kWave);
    const int8_t* T      = p.target;
    const int8_t* Q      = p.query;
    unsigned long long cols = 0;
    for (int32_t i = uniform(blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave); i < n; i += waves)
    {
        const uint32_t tu = seeds[i].target, qu = seeds[i].query;
        const int32_t t = uniform((int32_t)tu), q = uniform((int32_t)qu);
        // outside the sequences (either coordinate): no segment and no read (the reference reads out of bounds)
        if (tu >= (uint32_t)p.target_length || qu >= (uint32_t)p.query_length)
        {
            if (lane == 0) keep[i] = 0;
            continue;
        }
        const Walk r = walk(T, Q, sub, t, q, +1, min(p.target_length - t, p.query_length - q), p.xdrop_threshold, -1, lane);
        const Walk l = walk(T, Q, sub, t, q, -1, min(t, q), p.xdrop_threshold, 0, lane);
        cols += (unsigned long long)(r.cols + l.cols);
        const int32_t total  = r.best + l.best;
        const int32_t extent = r.pos + l.pos;
        double entropy       = 1.0;
        if (!p.no_entropy && total >= p.score_threshold && total <= 3 * p.score_threshold)
        {
            // matching columns per base over [t - lpos, t + rpos]
            int32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
            const int32_t t0 = t - l.pos, q0 = q - l.pos;
            for (int32_t base = 0; base <= extent; base += kWave)
            {
                const int32_t j = base + lane;
                int32_t a = -1, b = -2;
                if (j <= extent)
                {
                    a = T[t0 + j];
                    b = Q[q0 + j];
                }
                const bool same = a == b;
                c0 += __popcll(__ballot(same && a == 0));
                c1 += __popcll(__ballot(same && a == 1));
                c2 += __popcll(__ballot(same && a == 2));
                c3 += __popcll(__ballot(same && a == 3));
            }
            if (c0 + c1 + c2 + c3 >= 20)
            {
                const double denom = (double)(extent + 1);
                double acc         = 0.0;
                if (c0 > 0) acc += ((double)c0 / denom) * log((double)c0 / denom);
                if (c1 > 0) acc += ((double)c1 / denom) * log((double)c1 / denom);
                if (c2 > 0) acc += ((double)c2 / denom) * log((double)c2 / denom);
                if (c3 > 0) acc += ((double)c3 / denom) * log((double)c3 / denom);
                entropy = -acc / (double)logf(4.0f);
            }
        }
        const int32_t score = (int32_t)((double)total * entropy);
        const bool kept     = score >= p.score_threshold;
        if (lane == 0)
        {
            keep[i] = kept ? 1 : 0;
            if (kept) segments[i] = gwx_segment{qu - (uint32_t)l.pos, tu - (uint32_t)l.pos, extent, score};
        }
    }
    if (positions != nullptr && lane == 0 && cols != 0) atomicAdd(positions, cols);
}

// sort keys: pass 1 orders by (length, score) descending (signed), pass 2 by (unsigned diagonal, target) ascending;
// both passes are stable, so together they give the comparator's full order
__global__ void length_score_keys(const gwx_segment* __restrict__ s, int32_t n, uint64_t* __restrict__ key,
                                  uint32_t* __restrict__ idx)
{
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const uint32_t l = ~((uint32_t)s[i].length ^ 0x80000000u), sc = ~((uint32_t)s[i].score ^ 0x80000000u);
        key[i] = ((uint64_t)l << 32) | sc;
        idx[i] = (uint32_t)i;
    }
}
__global__ void diagonal_keys(const gwx_segment* __restrict__ s, const uint32_t* __restrict__ perm, int32_t n,
                              uint64_t* __restrict__ key)
{
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const gwx_segment x = s[perm[i]];
        key[i]              = ((uint64_t)(x.target - x.query) << 32) | x.target;
    }
}
// gather into sorted order and flag the elements thrust::unique_copy keeps: i = 0, or i does not overlap input i-1
__global__ void gather_unique_flags(const gwx_segment* __restrict__ s, const uint32_t* __restrict__ perm, int32_t n,
                                    gwx_segment* __restrict__ sorted, uint8_t* __restrict__ keep)
{
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const gwx_segment y = s[perm[i]];
        sorted[i]           = y;
        bool dup            = false;
        if (i > 0)
        {
            const gwx_segment x = s[perm[i - 1]];
            if (x.target - x.query == y.target - y.query)
            {
                const uint32_t xe = x.target + (uint32_t)x.length, ye = y.target + (uint32_t)y.length;
                dup = (x.target >= y.target && xe <= ye) || (y.target >= x.target && ye <= xe);
            }
        }
        keep[i] = dup ? 0 : 1;
    }
}
__global__ void store_count(int32_t* dst, int32_t v) { *dst = v; }

int grid_for(int64_t n, int per_block, int cap)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, cap));
}

size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// Workspace layout (byte offsets) for up to n seeds.
struct Layout
{
    size_t seg_a, seg_b, keep, key64_a, key64_b, idx_a, idx_b, counter, positions, temp, temp_bytes, total;
};

Layout layout(int32_t n)
{
    Layout L{};
    const size_t un = (size_t)std::max(n, 1);
    size_t select_bytes = 0, sort64 = 0;
    (void)rocprim::select((void*)nullptr, select_bytes, (const gwx_segment*)nullptr, (const uint8_t*)nullptr,
                    (gwx_segment*)nullptr, (uint32_t*)nullptr, un);
    (void)rocprim::radix_sort_pairs((void*)nullptr, sort64, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr,
                              (uint32_t*)nullptr, (unsigned int)un);
    L.temp_bytes = std::max({select_bytes, sort64, size_t(1)});
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o += align256(bytes);
        return at;
    };
    L.seg_a     = take(un * sizeof(gwx_segment));
    L.seg_b     = take(un * sizeof(gwx_segment));
    L.keep      = take(un);
    L.key64_a   = take(un * 8);
    L.key64_b   = take(un * 8);
    L.idx_a     = take(un * 4);
    L.idx_b     = take(un * 4);
    L.counter   = take(sizeof(uint32_t));
    L.positions = take(sizeof(unsigned long long));
    L.temp      = take(L.temp_bytes);
    L.total     = o;
    return L;
}

// compaction of `in` by `flags` into `out`, count read back to the host (the stream is waited for)
int select_to_host(const gwx_segment* in, const uint8_t* flags, int32_t n, gwx_segment* out, int32_t* count, char* ws,
                   const Layout& L, hipStream_t stream)
{
    size_t bytes = L.temp_bytes;
    uint32_t* d_count = (uint32_t*)(ws + L.counter);
    GWX_CHECK(rocprim::select(ws + L.temp, bytes, in, flags, out, d_count, (size_t)n, stream));
    uint32_t h = 0;
    GWX_CHECK(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, stream));
    GWX_CHECK(hipStreamSynchronize(stream));
    *count = (int32_t)h;
    return 0;
}

// sort + unique of seg[0..k) (compacted, seed order) into out; `sorted` (k entries) and the keys / indices / flags
// of the workspace are scratch
int sort_unique(const gwx_segment* seg, int32_t k, gwx_segment* sorted, gwx_segment* out, int32_t* count, char* ws,
                const Layout& L, hipStream_t stream)
{
    if (k <= 0)
    {
        *count = 0;
        return 0;
    }
    uint64_t* k64a = (uint64_t*)(ws + L.key64_a);
    uint64_t* k64b = (uint64_t*)(ws + L.key64_b);
    uint32_t* ia   = (uint32_t*)(ws + L.idx_a);
    uint32_t* ib   = (uint32_t*)(ws + L.idx_b);
    uint8_t* keep  = (uint8_t*)(ws + L.keep);
    const int g = grid_for(k, 256, 4096);
    length_score_keys<<<g, 256, 0, stream>>>(seg, k, k64a, ia);
    GWX_CHECK(hipGetLastError());
    size_t bytes = L.temp_bytes;
    GWX_CHECK(rocprim::radix_sort_pairs(ws + L.temp, bytes, k64a, k64b, ia, ib, (unsigned int)k, 0, 64, stream));
    diagonal_keys<<<g, 256, 0, stream>>>(seg, ib, k, k64a);
    GWX_CHECK(hipGetLastError());
    bytes = L.temp_bytes;
    GWX_CHECK(rocprim::radix_sort_pairs(ws + L.temp, bytes, k64a, k64b, ib, ia, (unsigned int)k, 0, 64, stream));
    gather_unique_flags<<<g, 256, 0, stream>>>(seg, ia, k, sorted, keep);
    GWX_CHECK(hipGetLastError());
    return select_to_host(sorted, keep, k, out, count, ws, L, stream);
}

} // namespace

extern "C" {

size_t gwx_workspace_bytes(int32_t max_seeds) { return layout(max_seeds).total; }

const char* gwx_last_error(void) { return g_error.c_str(); }

int gwx_count_positions(int32_t enable)
{
    g_count_positions = enable != 0;
    return 0;
}

int64_t gwx_last_positions(void) { return g_last_positions; }

int gwx_store_count(int32_t* d_dst, int32_t value, void* stream)
{
    store_count<<<1, 1, 0, (hipStream_t)stream>>>(d_dst, value);
    GWX_CHECK(hipGetLastError());
    return 0;
}

int gwx_extend_chunk(const gwx_problem* problem, const gwx_seed* seeds, int32_t n, gwx_segment* out, int32_t* count,
                     void* workspace, size_t workspace_bytes, void* stream_, void* const* events)
{
    hipStream_t stream = (hipStream_t)stream_;
    *count             = 0;
    g_last_positions   = 0;
    if (n <= 0) return 0;
    const Layout L = layout(n);
    if (workspace == nullptr || workspace_bytes < L.total) return fail("gwx_extend_chunk: workspace too small");
    char* ws = (char*)workspace;
    unsigned long long* positions = nullptr;
    if (g_count_positions)
    {
        positions = (unsigned long long*)(ws + L.positions);
        GWX_CHECK(hipMemsetAsync(positions, 0, sizeof(*positions), stream));
    }
    if (events) GWX_CHECK(hipEventRecord((hipEvent_t)events[0], stream));
    gwx_segment* seg_a = (gwx_segment*)(ws + L.seg_a);
    gwx_segment* seg_b = (gwx_segment*)(ws + L.seg_b);
    uint8_t* keep      = (uint8_t*)(ws + L.keep);
    ungapped_xdrop_kernel<<<grid_for(n, kBlock / kWave, 8192), kBlock, 0, stream>>>(*problem, seeds, n, seg_a, keep,
                                                                                     positions);
    GWX_CHECK(hipGetLastError());
    if (events) GWX_CHECK(hipEventRecord((hipEvent_t)events[1], stream));
    int32_t k = 0;
    if (select_to_host(seg_a, keep, n, seg_b, &k, ws, L, stream)) return -1;
    if (sort_unique(seg_b, k, seg_a, out, count, ws, L, stream)) return -1;
    if (events) GWX_CHECK(hipEventRecord((hipEvent_t)events[2], stream));
    if (positions)
    {
        unsigned long long h = 0;
        GWX_CHECK(hipMemcpyAsync(&h, positions, sizeof(h), hipMemcpyDeviceToHost, stream));
        GWX_CHECK(hipStreamSynchronize(stream));
        g_last_positions = (int64_t)h;
    }
    return 0;
}

int gwx_sort_unique(const gwx_segment* segments, const uint8_t* keep, int32_t n, gwx_segment* out, int32_t* count,
                    void* workspace, size_t workspace_bytes, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    *count             = 0;
    if (n <= 0) return 0;
    const Layout L = layout(n);
    if (workspace == nullptr || workspace_bytes < L.total) return fail("gwx_sort_unique: workspace too small");
    char* ws = (char*)workspace;
    int32_t k = 0;
    gwx_segment* seg_a = (gwx_segment*)(ws + L.seg_a);
    gwx_segment* seg_b = (gwx_segment*)(ws + L.seg_b);
    if (select_to_host(segments, keep, n, seg_b, &k, ws, L, stream)) return -1;
    return sort_unique(seg_b, k, seg_a, out, count, ws, L, stream);
}

} // extern "C"
