// gwaffine.hip -- the affine-gap global aligner on gfx950 (include/gwhip_affine.h; the rules are gwaffine_rules.h).
//
// Forward pass: one wave64 per pair, an anti-diagonal wavefront over the band's W diagonals. Lane l owns the K
// neighbouring diagonals l K .. l K + K - 1 and keeps H, E and F of each in registers (3 K VGPRs); one kernel instance
// per K in 1, 2, 4, 8, 16, 32, picked from the batch's widest band. Anti-diagonal a = i + j holds a cell only on the
// diagonals of a's parity, and such a cell reads its own diagonal's H (from a - 2) and H, E / H, F of the two
// neighbouring diagonals (from a - 1), which are of the other parity: the three values are updated in place. Only the
// lane's edge diagonals cross lanes, one pair of one-lane shuffles per step. The query and target bases of a lane's
// K / 2 cells are two register windows that slide by one base every second step; the base that enters is loaded one
// step ahead. A cell's choices (gwaffine_rules.h: src, Eext, Fext, mismatch) are one byte, stored anti-diagonal-major,
// so a step's stores are contiguous across the lanes (dwords from K = 8). No LDS in the forward pass.
//
// Traceback: one wave64 per pair walks the bytes from (n, m), 64 rows of the bit matrix at a time through LDS, and
// writes the states back to front into the pair's result slot, the form gwhip_hirschberg_myers leaves there.
//
// Every kernel is a template over a rules policy: OnePiece (gwaffine_rules.h; a gap run of L columns costs o + L e, three
// values a diagonal, K up to 32) and TwoPiece (gwaffine2_rules.h; min(o1 + L e1, o2 + L e2), five values a diagonal,
// H, E1, F1, E2, F2, K up to 16, three values across a lane's edge per step instead of two). The policy names the costs,
// the band's capacity, the cell update, the optimality bound and the traceback step; the wavefront, the base windows,
// the stores, the tiles and the guards are written once.
//
// The affine X-drop extension (gwhip_extend) is the one-piece wavefront in another geometry with a stop rule on top;
// its kernels are in gwaffine_extend.h, included below, its rules in gwaffine_extend_rules.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gwhip_affine.h"

#include "gwaffine2_rules.h"
#include "gwaffine_extend_rules.h"
#include "gwaffine_rules.h"

namespace
{

using namespace gwaffine;

constexpr int kWavesPerBlock = 4;
constexpr int kThreads       = 64 * kWavesPerBlock;
constexpr int kScanThreads   = 256;

thread_local std::string g_error;

int fail(hipError_t e, const std::string& what)
{
    g_error = what + ": " + hipGetErrorString(e);
    return static_cast<int>(e);
}

inline int64_t round256(int64_t v) { return (v + 255) & ~int64_t(255); }

// The one-piece rules: G = 1 pair of gap matrices.
struct OnePiece
{
    static constexpr int G = 1;
    using CostsT          = Costs;
    using WalkT           = Walk;
    struct Out
    {
        int32_t h, e[1], f[1];
        uint32_t bits;
    };
    static __host__ __device__ __forceinline__ Band band(int64_t n, int64_t m, int64_t B) { return band_of(n, m, B); }
    static __device__ __forceinline__ Out update(int32_t h_diag, int32_t h_left, const int32_t (&e_left)[1], int32_t h_up,
                                                 const int32_t (&f_up)[1], bool match, const Costs& c)
    {
        const Cell r = cell_update(h_diag, h_left, e_left[0], h_up, f_up[0], match, c);
        return Out{r.h, {r.e}, {r.f}, r.bits};
    }
    static __device__ __forceinline__ bool optimal(int64_t cost, int64_t n, int64_t m, int64_t B, const Costs& c)
    {
        return cost_is_optimal(cost, n, m, B, c);
    }
    static __device__ __forceinline__ int32_t step(Walk& w, uint32_t bits) { return walk_step(w, bits); }
};

// The two-piece rules: G = 2, matrices E1, E2 and F1, F2.
struct TwoPiece
{
    static constexpr int G = 2;
    using CostsT          = Costs2;
    using WalkT           = Walk2;
    struct Out
    {
        int32_t h, e[2], f[2];
        uint32_t bits;
    };
    static __host__ __device__ __forceinline__ Band band(int64_t n, int64_t m, int64_t B) { return band_of2(n, m, B); }
    static __device__ __forceinline__ Out update(int32_t h_diag, int32_t h_left, const int32_t (&e_left)[2], int32_t h_up,
                                                 const int32_t (&f_up)[2], bool match, const Costs2& c)
    {
        const Cell2 r = cell_update2(h_diag, h_left, e_left[0], e_left[1], h_up, f_up[0], f_up[1], match, c);
        return Out{r.h, {r.e1, r.e2}, {r.f1, r.f2}, r.bits};
    }
    static __device__ __forceinline__ bool optimal(int64_t cost, int64_t n, int64_t m, int64_t B, const Costs2& c)
    {
        return cost_is_optimal2(cost, n, m, B, c);
    }
    static __device__ __forceinline__ int32_t step(Walk2& w, uint32_t bits) { return walk_step2(w, bits); }
};

template <class R>
struct PairArgs
{
    const char* sequences;
    const int64_t* starts;
    const int64_t* offsets; // [n + 1] of the pairs' bit matrices in `bits`
    uint8_t* bits;
    int64_t bits_capacity;
    int8_t* results;
    int32_t* result_lengths;
    int32_t* costs;
    uint8_t* optimal;
    int32_t n;
    int32_t band;
    typename R::CostsT c;
};

template <class R>
__device__ __forceinline__ Band pair_band(const PairArgs<R>& A, int64_t pair)
{
    const int64_t q0 = A.starts[2 * pair], t0 = A.starts[2 * pair + 1], t1 = A.starts[2 * pair + 2];
    return R::band(t0 - q0, t1 - t0, A.band);
}

// offsets[p] = bytes of the bit matrices of the pairs before p, offsets[n] their total: one block, every thread a run
// of consecutive pairs; bytes_of(p) is pair p's
template <class BytesOf>
__device__ __forceinline__ void scan_offsets(int32_t n, BytesOf bytes_of, int64_t* __restrict__ offsets)
{
    __shared__ int64_t partial[kScanThreads];
    const int64_t per   = (static_cast<int64_t>(n) + kScanThreads - 1) / kScanThreads;
    const int64_t first = min(static_cast<int64_t>(n), threadIdx.x * per), last = min(static_cast<int64_t>(n), first + per);
    int64_t sum = 0;
    for (int64_t p = first; p < last; ++p)
        sum += bytes_of(p);
    partial[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        int64_t run = 0;
        for (int k = 0; k < kScanThreads; ++k)
        {
            const int64_t v = partial[k];
            partial[k]      = run;
            run += v;
        }
        offsets[n] = run;
    }
    __syncthreads();
    int64_t run = partial[threadIdx.x];
    for (int64_t p = first; p < last; ++p)
    {
        offsets[p] = run;
        run += bytes_of(p);
    }
}

template <class R>
__global__ void __launch_bounds__(kScanThreads) offsets_kernel(PairArgs<R> A, int64_t* __restrict__ offsets)
{
    scan_offsets(A.n, [&](int64_t p) { return bits_bytes(pair_band(A, p)); }, offsets);
}

// what the wavefront needs of a pair, in 32 bits (n + m < 2^21, W <= 2048)
struct Pair32
{
    int32_t n, m, lo, W, stride;
};

// One anti-diagonal a for the lane's cells of parity PAR (K >= 2): cell t is diagonal index k0 + PAR + 2 t at
// (i0 - t, j0 + t); qw[t] / tw[t] are its query base and its target base (translated), 0 / 1 where there is none.
// kStore = false (the extension's score-only mode) writes no row of the bit matrix.
template <class R, int K, int PAR, bool kStore = true>
__device__ __forceinline__ void wave_step(int32_t (&H)[K], int32_t (&E)[R::G][K], int32_t (&F)[R::G][K],
                                          const char (&qw)[K / 2], const char (&tw)[K / 2], int32_t a, int32_t k0,
                                          const Pair32& p, const typename R::CostsT& c, uint8_t* __restrict__ row, int lane)
{
    constexpr int C = K / 2, G = R::G;
    // the neighbour across the lane's edge: diagonal k0 - 1 (H and the E's) for PAR 0, diagonal k0 + K (H and the F's)
    // for PAR 1
    int32_t hx, gx[G];
    if (PAR == 0)
    {
        hx = __shfl_up(H[K - 1], 1, 64);
#pragma unroll
        for (int g = 0; g < G; ++g)
            gx[g] = __shfl_up(E[g][K - 1], 1, 64);
    }
    else
    {
        hx = __shfl_down(H[0], 1, 64);
#pragma unroll
        for (int g = 0; g < G; ++g)
            gx[g] = __shfl_down(F[g][0], 1, 64);
    }
    if (lane == (PAR == 0 ? 0 : 63))
    {
        hx = kInf;
#pragma unroll
        for (int g = 0; g < G; ++g)
            gx[g] = kInf;
    }
    uint32_t packed[(C + 3) / 4];
#pragma unroll
    for (int w = 0; w < (C + 3) / 4; ++w)
        packed[w] = 0;
#pragma unroll
    for (int t = 0; t < C; ++t)
    {
        const int kk       = PAR + 2 * t;
        const int32_t k    = k0 + kk;
        const int32_t d    = p.lo + k;
        const int32_t i    = (a - d) >> 1;
        const int32_t j    = (a + d) >> 1;
        const bool valid   = k < p.W && i >= 0 && j >= 0 && i <= p.n && j <= p.m;
        const int32_t hl   = kk > 0 ? H[kk > 0 ? kk - 1 : 0] : hx;
        const int32_t hu   = kk < K - 1 ? H[kk < K - 1 ? kk + 1 : 0] : hx;
        int32_t el[G], fu[G];
#pragma unroll
        for (int g = 0; g < G; ++g)
        {
            el[g] = kk > 0 ? E[g][kk > 0 ? kk - 1 : 0] : gx[g];
            fu[g] = kk < K - 1 ? F[g][kk < K - 1 ? kk + 1 : 0] : gx[g];
        }
        const bool match         = i > 0 && j > 0 && qw[t] == tw[t];
        const typename R::Out r  = R::update(H[kk], hl, el, hu, fu, match, c);
        H[kk]                    = valid ? r.h : kInf;
#pragma unroll
        for (int g = 0; g < G; ++g)
        {
            E[g][kk] = valid ? r.e[g] : kInf;
            F[g][kk] = valid ? r.f[g] : kInf;
        }
        packed[t / 4] |= r.bits << (8 * (t % 4));
    }
    if (!kStore)
        return;
    const int32_t at = lane * C; // (k0 + PAR + 2 t) >> 1 = lane * C + t
    if (C >= 4)
    {
#pragma unroll
        for (int w = 0; w < C / 4; ++w)
            if (at + 4 * w < p.stride) // the stride is a multiple of 4
                *reinterpret_cast<uint32_t*>(row + at + 4 * w) = packed[w];
    }
    else if (C == 2)
    {
        if (at < p.stride)
            *reinterpret_cast<uint16_t*>(row + at) = static_cast<uint16_t>(packed[0]);
    }
    else if (at < p.stride)
        row[at] = static_cast<uint8_t>(packed[0]);
}

template <class R, int K>
__global__ void __launch_bounds__(kThreads) forward_kernel(PairArgs<R> A)
{
    const int64_t pair = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const int lane     = threadIdx.x & 63;
    if (pair >= A.n)
        return; // whole waves leave together
    const int64_t q0 = A.starts[2 * pair], t0 = A.starts[2 * pair + 1];
    const Band b       = pair_band(A, pair);
    const int64_t off  = A.offsets[pair];
    if (!b.aligned || b.W > 64 * K || off + bits_bytes(b) > A.bits_capacity)
    {
        if (lane == 0)
        {
            A.costs[pair]   = -1;
            A.optimal[pair] = 0;
        }
        return;
    }
    const Pair32 p{static_cast<int32_t>(b.n), static_cast<int32_t>(b.m), static_cast<int32_t>(b.lo),
                   static_cast<int32_t>(b.W), static_cast<int32_t>(b.stride)};
    constexpr int G   = R::G;
    const typename R::CostsT c = A.c;
    const char* Q     = A.sequences + q0;
    const char* T     = A.sequences + t0;
    uint8_t* bits     = A.bits + off;
    const int32_t k0  = lane * K;
    const int32_t end = p.n + p.m;
    // a base of the query / the target as the match test takes it; 0 / 1 outside the sequence never match
    auto query_base  = [&](int32_t at) -> char { return at >= 0 && at < p.n ? Q[at] : char(0); };
    auto target_base = [&](int32_t at) -> char {
        return at >= 0 && at < p.m ? "ACTG"[(static_cast<unsigned char>(T[at]) >> 1) & 3] : char(1);
    };

    int32_t H[K], E[G][K], F[G][K];
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
    {
        H[kk] = kInf;
#pragma unroll
        for (int g = 0; g < G; ++g)
            E[g][kk] = F[g][kk] = kInf;
        if (k0 + kk == -p.lo) // cell (0, 0)
            H[kk] = 0;
    }
    if (lane == 0)
        bits[(-p.lo) >> 1] = 0;

    if constexpr (K == 1)
    {
        for (int32_t a = 1; a <= end; ++a)
        {
            const int32_t par = (a + p.lo) & 1;
            int32_t hl = __shfl_up(H[0], 1, 64), hu = __shfl_down(H[0], 1, 64), el[G], fu[G];
            if (lane == 0)
                hl = kInf;
            if (lane == 63)
                hu = kInf;
#pragma unroll
            for (int g = 0; g < G; ++g)
            {
                el[g] = __shfl_up(E[g][0], 1, 64);
                fu[g] = __shfl_down(F[g][0], 1, 64);
                if (lane == 0)
                    el[g] = kInf;
                if (lane == 63)
                    fu[g] = kInf;
            }
            if ((lane & 1) == par)
            {
                const int32_t d  = p.lo + lane;
                const int32_t i  = (a - d) >> 1;
                const int32_t j  = (a + d) >> 1;
                const bool valid = lane < p.W && i >= 0 && j >= 0 && i <= p.n && j <= p.m;
                const bool match = valid && i > 0 && j > 0 && query_base(i - 1) == target_base(j - 1);
                const typename R::Out r = R::update(H[0], hl, el, hu, fu, match, c);
                H[0]                    = valid ? r.h : kInf;
#pragma unroll
                for (int g = 0; g < G; ++g)
                {
                    E[g][0] = valid ? r.e[g] : kInf;
                    F[g][0] = valid ? r.f[g] : kInf;
                }
                if (valid)
                    bits[static_cast<int64_t>(a) * p.stride + (lane >> 1)] = static_cast<uint8_t>(r.bits);
            }
        }
    }
    else
    {
        constexpr int C = K / 2;
        // cell 0 of the lane on anti-diagonal a: diagonal lo + k0 + par(a)
        auto i0 = [&](int32_t a) { return (a - p.lo - k0 - ((a + p.lo) & 1)) >> 1; };
        auto j0 = [&](int32_t a) { return (a + p.lo + k0 + ((a + p.lo) & 1)) >> 1; };
        char qw[C], tw[C];
#pragma unroll
        for (int t = 0; t < C; ++t)
        {
            qw[t] = query_base(i0(1) - t - 1);
            tw[t] = target_base(j0(1) + t - 1);
        }
        for (int32_t a = 1; a <= end; ++a)
        {
            uint8_t* row = bits + static_cast<int64_t>(a) * p.stride;
            if (((a + p.lo) & 1) == 0)
            {
                // the next step has the same query bases and every target base one further
                const char entering = target_base(j0(a + 1) + C - 2);
                wave_step<R, K, 0>(H, E, F, qw, tw, a, k0, p, c, row, lane);
#pragma unroll
                for (int t = 0; t + 1 < C; ++t)
                    tw[t] = tw[t + 1];
                tw[C - 1] = entering;
            }
            else
            {
                // the next step has the same target bases and every query base one further
                const char entering = query_base(i0(a + 1) - 1);
                wave_step<R, K, 1>(H, E, F, qw, tw, a, k0, p, c, row, lane);
#pragma unroll
                for (int t = C - 1; t > 0; --t)
                    qw[t] = qw[t - 1];
                qw[0] = entering;
            }
        }
    }

    // H[n][m] lies on diagonal m - n
    const int32_t k_end = p.m - p.n - p.lo;
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
        if (k0 + kk == k_end)
        {
            A.costs[pair]   = H[kk];
            A.optimal[pair] = R::optimal(H[kk], p.n, p.m, A.band, c) ? 1 : 0;
        }
}

// Traceback: one wave64 (one block) per pair. The walk from (n, m) is serial, so what the wave shares is the fetching:
// lane r loads kTileBytes cells of row a - r of the bit matrix around the walk's cell into LDS, one tile of 64 rows at
// a time, and every lane then walks the tile with the same wave-uniform steps (walk_step of the rules header); lane 0
// writes the states. A step lowers the row by one or two and moves the cell index by at most one for every two rows,
// so a tile that starts 40 cells below the walk's cell holds all 64 rows of the walk.
constexpr int kTileRows  = 64;
constexpr int kTileBytes = 80;

// The walk from (i, j) in H back to (0, 0) through the tiles: the states back to front at out[0 .. cap), their number in
// len. True: bits that lead out of the band or past the slot, a defect and never an input's property.
template <class R>
__device__ __forceinline__ bool walk_tiles(const Band& b, const uint8_t* __restrict__ bits, int8_t* __restrict__ out, int64_t i,
                                           int64_t j, int64_t cap, int lane, uint32_t* tile, int64_t& len)
{
    typename R::WalkT w{i, j, 0};
    len       = 0;
    bool lost = false;
    while (!lost && (w.i != 0 || w.j != 0 || w.matrix != 0))
    {
        const int64_t a_top = w.i + w.j;
        const int64_t c0    = max(int64_t(0), ((w.j - w.i - b.lo) >> 1) - 40) & ~int64_t(3);
        __syncthreads(); // the tile before this one has been walked
        {
            const int64_t row = a_top - lane;
#pragma unroll
            for (int q = 0; q < kTileBytes / 4; ++q)
            {
                const int64_t col = c0 + 4 * q; // the stride is a multiple of 4: a dword lies inside its row or outside
                tile[lane * (kTileBytes / 4) + q] =
                    row >= 0 && col < b.stride ? *reinterpret_cast<const uint32_t*>(bits + row * b.stride + col) : 0u;
            }
        }
        __syncthreads();
        const uint8_t* cells = reinterpret_cast<const uint8_t*>(tile);
        while (w.i != 0 || w.j != 0 || w.matrix != 0)
        {
            const int64_t k = w.j - w.i - b.lo;
            if (w.i < 0 || w.j < 0 || k < 0 || k >= b.W)
            {
                lost = true;
                break;
            }
            const int64_t r = a_top - (w.i + w.j), cc = (k >> 1) - c0;
            if (r >= kTileRows || cc < 0 || cc >= kTileBytes)
                break; // the next tile
            const int32_t state = R::step(w, cells[r * kTileBytes + cc]);
            if (state >= 0)
            {
                if (len >= cap)
                {
                    lost = true;
                    break;
                }
                if (lane == 0)
                    out[len] = static_cast<int8_t>(state);
                ++len;
            }
        }
    }
    return lost;
}

template <class R>
__global__ void __launch_bounds__(64) traceback_kernel(PairArgs<R> A)
{
    __shared__ uint32_t tile[kTileRows * kTileBytes / 4];
    const int64_t pair = blockIdx.x;
    const int lane     = threadIdx.x;
    if (A.costs[pair] < 0) // the forward pass gave no result
    {
        if (lane == 0)
            A.result_lengths[pair] = 0;
        return;
    }
    const Band b    = pair_band(A, pair);
    int64_t len     = 0;
    const bool lost = walk_tiles<R>(b, A.bits + A.offsets[pair], A.results + A.starts[2 * pair], b.n, b.m, b.n + b.m, lane, tile, len);
    if (lane == 0)
    {
        A.result_lengths[pair] = lost ? 0 : static_cast<int32_t>(len);
        if (lost)
        {
            A.costs[pair]   = -1;
            A.optimal[pair] = 0;
        }
    }
}

// what the host reads of the batch: bytes of the workspace, the widest band among the pairs that are aligned;
// false: starts that do not ascend
template <class R>
bool size_batch(int32_t n, const int64_t* starts, int32_t band, int64_t* bytes, int64_t* widest)
{
    *bytes  = round256(8 * (static_cast<int64_t>(n) + 1));
    *widest = 1;
    for (int64_t i = 0; i < n; ++i)
    {
        const int64_t ql = starts[2 * i + 1] - starts[2 * i], tl = starts[2 * i + 2] - starts[2 * i + 1];
        if (ql < 0 || tl < 0)
            return false;
        const Band b = R::band(ql, tl, band);
        *bytes += bits_bytes(b);
        if (b.aligned)
            *widest = std::max(*widest, b.W);
    }
    return true;
}

// the costs of a call's arguments as its rules take them, and the text that refuses them when out of range ("" in range)
Costs costs_of(const gwhip_affine_args& a) { return Costs{a.mismatch, a.gap_open, a.gap_extend}; }
Costs2 costs_of(const gwhip_affine2_args& a) { return Costs2{a.mismatch, a.gap_open, a.gap_extend, a.gap_open2, a.gap_extend2}; }

std::string out_of_range(const gwhip_affine_args& a)
{
    if (costs_in_range(a.mismatch, a.gap_open, a.gap_extend, a.band))
        return "";
    return "mismatch " + std::to_string(a.mismatch) + ", gap_open " + std::to_string(a.gap_open) + ", gap_extend " +
           std::to_string(a.gap_extend) + ", band " + std::to_string(a.band) + " outside 1..255, 0..255, 1..255, >= 0";
}

std::string out_of_range(const gwhip_affine2_args& a)
{
    if (costs2_in_range(a.mismatch, a.gap_open, a.gap_extend, a.gap_open2, a.gap_extend2, a.band))
        return "";
    return "mismatch " + std::to_string(a.mismatch) + ", gap_open " + std::to_string(a.gap_open) + ", gap_extend " +
           std::to_string(a.gap_extend) + ", gap_open2 " + std::to_string(a.gap_open2) + ", gap_extend2 " +
           std::to_string(a.gap_extend2) + ", band " + std::to_string(a.band) +
           " outside 1..255, 0..255, 1..255, 0..255, 1..255, >= 0";
}

// the forward pass of the narrowest variant that holds `per_lane` diagonals a lane
template <class R>
void launch_forward(int64_t per_lane, unsigned blocks, hipStream_t s, const PairArgs<R>& A)
{
    if (per_lane <= 1)
        forward_kernel<R, 1><<<blocks, kThreads, 0, s>>>(A);
    else if (per_lane <= 2)
        forward_kernel<R, 2><<<blocks, kThreads, 0, s>>>(A);
    else if (per_lane <= 4)
        forward_kernel<R, 4><<<blocks, kThreads, 0, s>>>(A);
    else if (per_lane <= 8)
        forward_kernel<R, 8><<<blocks, kThreads, 0, s>>>(A);
    else if (per_lane <= 16 || R::G == 2) // no pair of the two-piece rules is wider
        forward_kernel<R, 16><<<blocks, kThreads, 0, s>>>(A);
    else if constexpr (R::G == 1)
        forward_kernel<R, 32><<<blocks, kThreads, 0, s>>>(A);
}

template <class R, class Args>
int run(const char* name, const Args* a, hipStream_t s, hipEvent_t* events)
{
    const std::string who = std::string(name) + ": ";
    if (a == nullptr || a->n_alignments < 0)
        return fail(hipErrorInvalidValue, who + "no arguments, or a negative number of alignments");
    const std::string refused = out_of_range(*a);
    if (!refused.empty())
        return fail(hipErrorInvalidValue, who + refused);
    const int32_t n = a->n_alignments;
    if (n == 0)
        return 0;
    if (!a->sequences || !a->sequence_starts || !a->sequence_starts_host || !a->results || !a->result_lengths || !a->costs ||
        !a->optimal || !a->workspace)
        return fail(hipErrorInvalidValue, who + "a null pointer among the arguments");
    int64_t need = 0, widest = 0;
    if (!size_batch<R>(n, a->sequence_starts_host, a->band, &need, &widest))
        return fail(hipErrorInvalidValue, who + "sequence_starts_host does not ascend");
    if (a->workspace_bytes < static_cast<size_t>(need))
        return fail(hipErrorInvalidValue, who + "the workspace has " + std::to_string(a->workspace_bytes) +
                                              " bytes, the batch needs " + std::to_string(need));
    const int64_t head = round256(8 * (static_cast<int64_t>(n) + 1));
    PairArgs<R> A{};
    A.sequences      = a->sequences;
    A.starts         = a->sequence_starts;
    A.offsets        = static_cast<const int64_t*>(a->workspace);
    A.bits           = static_cast<uint8_t*>(a->workspace) + head;
    A.bits_capacity  = static_cast<int64_t>(a->workspace_bytes) - head;
    A.results        = a->results;
    A.result_lengths = a->result_lengths;
    A.costs          = a->costs;
    A.optimal        = a->optimal;
    A.n              = n;
    A.band           = a->band;
    A.c              = costs_of(*a);

    offsets_kernel<R><<<1, kScanThreads, 0, s>>>(A, static_cast<int64_t*>(a->workspace));
    const unsigned blocks = static_cast<unsigned>((static_cast<int64_t>(n) + kWavesPerBlock - 1) / kWavesPerBlock);
    if (events && hipEventRecord(events[0], s) != hipSuccess)
        return fail(hipGetLastError(), who + "hipEventRecord");
    launch_forward<R>((widest + 63) / 64, blocks, s, A);
    if (events && hipEventRecord(events[1], s) != hipSuccess)
        return fail(hipGetLastError(), who + "hipEventRecord");
    traceback_kernel<R><<<static_cast<unsigned>(n), 64, 0, s>>>(A);
    if (events && hipEventRecord(events[2], s) != hipSuccess)
        return fail(hipGetLastError(), who + "hipEventRecord");
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(e, who + "launch");
    return 0;
}

template <class R>
size_t workspace_bytes(int32_t n_alignments, const int64_t* sequence_starts_host, int32_t band)
{
    int64_t bytes = 0, widest = 0;
    if (n_alignments <= 0 || sequence_starts_host == nullptr || band < 0 ||
        !size_batch<R>(n_alignments, sequence_starts_host, band, &bytes, &widest))
        return 256;
    return static_cast<size_t>(bytes);
}

template <class R, class Args>
int run_events(const char* name, const Args* args, void* stream, void* const events[3])
{
    if (events == nullptr || !events[0] || !events[1] || !events[2])
        return fail(hipErrorInvalidValue, std::string(name) + "_events: three events are needed");
    hipEvent_t e[3] = {static_cast<hipEvent_t>(events[0]), static_cast<hipEvent_t>(events[1]), static_cast<hipEvent_t>(events[2])};
    return run<R>(name, args, static_cast<hipStream_t>(stream), e);
}

#include "gwaffine_extend.h"

} // namespace

extern "C" {

size_t gwhip_affine_workspace_bytes(int32_t n_alignments, const int64_t* sequence_starts_host, int32_t band)
{
    return workspace_bytes<OnePiece>(n_alignments, sequence_starts_host, band);
}

int gwhip_affine_align(const gwhip_affine_args* args, void* stream)
{
    return run<OnePiece>("gwhip_affine_align", args, static_cast<hipStream_t>(stream), nullptr);
}

int gwhip_affine_align_events(const gwhip_affine_args* args, void* stream, void* const events[3])
{
    return run_events<OnePiece>("gwhip_affine_align", args, stream, events);
}

size_t gwhip_affine2_workspace_bytes(int32_t n_alignments, const int64_t* sequence_starts_host, int32_t band)
{
    return workspace_bytes<TwoPiece>(n_alignments, sequence_starts_host, band);
}

int gwhip_affine2_align(const gwhip_affine2_args* args, void* stream)
{
    return run<TwoPiece>("gwhip_affine2_align", args, static_cast<hipStream_t>(stream), nullptr);
}

int gwhip_affine2_align_events(const gwhip_affine2_args* args, void* stream, void* const events[3])
{
    return run_events<TwoPiece>("gwhip_affine2_align", args, stream, events);
}

size_t gwhip_extend_workspace_bytes(int32_t n_alignments, const int64_t* sequence_starts_host, int32_t band, int32_t with_traceback)
{
    int64_t bytes = 0;
    if (!with_traceback)
        return 0;
    if (n_alignments <= 0 || sequence_starts_host == nullptr || band < 0 || band > kMaxExtendBand ||
        !size_extend_batch(n_alignments, sequence_starts_host, band, &bytes))
        return 256;
    return static_cast<size_t>(bytes);
}

int gwhip_extend(const gwhip_extend_args* args, void* stream) { return run_extend(args, static_cast<hipStream_t>(stream), nullptr); }

int gwhip_extend_events(const gwhip_extend_args* args, void* stream, void* const events[3])
{
    if (events == nullptr || !events[0] || !events[1] || !events[2])
        return fail(hipErrorInvalidValue, "gwhip_extend_events: three events are needed");
    hipEvent_t e[3] = {static_cast<hipEvent_t>(events[0]), static_cast<hipEvent_t>(events[1]), static_cast<hipEvent_t>(events[2])};
    return run_extend(args, static_cast<hipStream_t>(stream), e);
}

const char* gwhip_affine_last_error(void) { return g_error.c_str(); }

} // extern "C"
