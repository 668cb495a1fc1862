// gws_ends.hip -- cudaaligner's infix / prefix alignment types on gfx950: where a query ends and begins in its target
// (include/gwhip_semiglobal.h). Score-only Myers bit-vector scans, one wave64 per pair, no matrix stored:
//
//   * lane l holds 32-bit word l of the column (pv, mv) and the four pattern words of its 32 query bases, so a wave
//     covers 2 048 query bases per ROUND; a longer query takes R rounds per column, lane l owning words l, 64 + l, ...
//     Up to 8 words per lane stay in registers (queries of up to 16 384 bases, one kernel instance per power of two);
//     longer queries keep the same six words per query word in the workspace, [round][array][lane], one coalesced
//     256-byte row per access;
//   * the multi-word addition of Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq is the two-ballot carry look-ahead of gwhip_myers.hip:
//     every lane adds its word alone and reports "generates a carry" / "would pass one on", and one 64-bit scalar
//     addition of the two ballots yields every lane's carry-in. The carry out of lane 63 and the top bits of ph / mh
//     cross to the next round as wave-uniform values;
//   * the bit shifted into word 0 is the top row's horizontal delta: +1 for prefix (D[0][j] = j), 0 for infix;
//   * the lane that owns query bit n - 1 keeps the running bottom score D[n][j], its minimum and the first column that
//     reached it (column 0, score n, counts);
//   * the target's bases arrive 64 columns at a time, one per lane, as 2-bit codes, and are handed to the column loop by
//     v_readlane (the column index is wave-uniform).
//
// The same scan run over the reversed query and the reversed T[0:te] with the +1 top row, stopped at the first column
// whose bottom score equals d, gives the begin: that column j' is the shortest suffix of T[0:te] at global distance d,
// tb = te - j', and j' <= n + d bounds the scan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gwhip_semiglobal.h"

namespace
{

constexpr int kWord          = 32;
constexpr int kWavesPerBlock = 4;
constexpr int kThreads       = 64 * kWavesPerBlock;
constexpr int kMaxRegWords   = GWHIP_SEMIGLOBAL_REGISTER_QUERY / (64 * kWord); // words per lane held in registers

thread_local std::string g_error;

int fail(hipError_t e, const char* what)
{
    g_error = std::string(what) + ": " + hipGetErrorString(e);
    return static_cast<int>(e);
}

struct EndsArgs
{
    const char* sequences;
    const int64_t* starts;
    int32_t* ends;
    uint32_t* workspace;    // W == 0 only: words_per_pair words per pair
    int64_t words_per_pair; // 6 * 64 * max_rounds
    int32_t n;
    int32_t max_rounds;
    int32_t prefix;  // top row +1 in the forward scan
    int32_t reverse; // the anchored scan for tb
};

__device__ __forceinline__ uint32_t select4(uint32_t ci, uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3)
{
    const uint32_t a = (ci & 1u) ? e1 : e0, b = (ci & 1u) ? e3 : e2;
    return (ci & 2u) ? b : a;
}

// One round of one column: lane l advances its word. carry / ph_top / mh_top (wave-uniform) come from the round below --
// the carry into lane 0's addition and the bits shifted into lane 0's word -- and leave for the round above.
__device__ __forceinline__ void round_advance(int lane, uint32_t eq, uint32_t& pv, uint32_t& mv, uint32_t& ph_out, uint32_t& mh_out,
                                              uint32_t& carry, uint32_t& ph_top, uint32_t& mh_top)
{
    const uint32_t xv  = eq | mv;
    const uint32_t a   = eq & pv;
    const uint32_t s0  = a + pv;
    const uint64_t gen = __ballot(s0 < a), prp = __ballot(s0 == 0xffffffffu);
    // bit 63 stays out of the addition: its carry-out is the next round's carry-in, taken separately
    const uint64_t top = 1ull << 63;
    const uint64_t A = (gen | prp) & ~top, B = gen & ~top;
    const uint64_t cin = (A + B + static_cast<uint64_t>(carry)) ^ (prp & ~top);
    const uint32_t sum = s0 + static_cast<uint32_t>((cin >> lane) & 1u);
    carry              = static_cast<uint32_t>(((gen >> 63) | ((prp >> 63) & (cin >> 63))) & 1u);
    const uint32_t xh  = (sum ^ pv) | eq;
    const uint32_t ph  = mv | ~(xh | pv);
    const uint32_t mh  = pv & xh;
    uint32_t ph_lo     = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int32_t>(ph >> 31), 0x138, 0xf, 0xf, false)); // wave_shr:1
    uint32_t mh_lo     = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int32_t>(mh >> 31), 0x138, 0xf, 0xf, false));
    if (lane == 0)
    {
        ph_lo = ph_top;
        mh_lo = mh_top;
    }
    ph_top             = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int32_t>(ph >> 31), 63));
    mh_top             = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int32_t>(mh >> 31), 63));
    const uint32_t phs = (ph << 1) | ph_lo, mhs = (mh << 1) | mh_lo;
    pv                 = mhs | ~(xv | phs);
    mv                 = phs & xv;
    ph_out             = ph;
    mh_out             = mh;
}

// the pattern words of query word w: bit b of e[c] = (base 32 w + b == "ACTG"[c]); `reverse` reads the query back to front
__device__ __forceinline__ void build_patterns(const char* q, int32_t n, bool reverse, int32_t w, uint32_t e[4])
{
    e[0] = e[1] = e[2] = e[3] = 0u;
    const int32_t first       = w * kWord;
    const int32_t count       = min(kWord, n - first);
    for (int32_t b = 0; b < count; ++b)
    {
        const char c = q[reverse ? n - 1 - (first + b) : first + b];
        e[0] |= static_cast<uint32_t>(c == 'A') << b;
        e[1] |= static_cast<uint32_t>(c == 'C') << b;
        e[2] |= static_cast<uint32_t>(c == 'T') << b;
        e[3] |= static_cast<uint32_t>(c == 'G') << b;
    }
}

// W > 0: W words per lane in registers. W == 0: any number of rounds, state and patterns in the workspace.
template <int W>
__global__ void __launch_bounds__(kThreads) semiglobal_ends_kernel(EndsArgs a)
{
    constexpr int R    = W > 0 ? W : 1;
    const int lane     = threadIdx.x & 63;
    const int32_t pair = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
    if (pair >= a.n)
        return; // whole waves leave together
    const int64_t q0 = a.starts[2 * pair], t0 = a.starts[2 * pair + 1], t1 = a.starts[2 * pair + 2];
    const int32_t n = static_cast<int32_t>(t0 - q0), m = static_cast<int32_t>(t1 - t0);
    const char* q = a.sequences + q0;
    const char* t = a.sequences + t0;
    int32_t* e    = a.ends + 3 * static_cast<int64_t>(pair);
    const bool reverse = a.reverse != 0;

    int32_t cols, d_known = 0, te = 0;
    if (!reverse)
    {
        if (n == 0 || m == 0) // d = n at column 0: nothing to scan
        {
            if (lane == 0)
            {
                e[0] = n;
                e[1] = 0;
                e[2] = 0;
            }
            return;
        }
        cols = m;
    }
    else
    {
        d_known = e[0];
        te      = e[2];
        if (d_known < 0)
            return; // the forward scan refused the pair
        if (d_known == n) // column 0 of the reversed scan: the empty slice is at distance n
        {
            if (lane == 0)
                e[1] = te;
            return;
        }
        cols = static_cast<int32_t>(min(static_cast<int64_t>(te), static_cast<int64_t>(n) + d_known));
    }
    const int32_t n_words = (n + kWord - 1) / kWord;
    const int32_t rounds  = (n_words + 63) / 64;
    if (rounds > (W > 0 ? W : a.max_rounds)) // a query beyond the declared max_query_length: refused, not scanned
    {
        if (lane == 0 && !reverse)
        {
            e[0] = -1;
            e[1] = -1;
            e[2] = -1;
        }
        return;
    }
    const int32_t owner_word  = (n - 1) / kWord;
    const int32_t owner_round = owner_word >> 6, owner_lane = owner_word & 63;
    const uint32_t owner_bit  = static_cast<uint32_t>(n - 1) & 31u;
    const uint32_t top        = (reverse || a.prefix) ? 1u : 0u;

    uint32_t pv[R], mv[R], eq[R][4];
    uint32_t* ws = nullptr;
    if constexpr (W > 0)
    {
#pragma unroll
        for (int r = 0; r < R; ++r)
        {
            pv[r] = 0xffffffffu;
            mv[r] = 0u;
            eq[r][0] = eq[r][1] = eq[r][2] = eq[r][3] = 0u;
            if (r < rounds)
                build_patterns(q, n, reverse, r * 64 + lane, eq[r]);
        }
    }
    else
    {
        ws = a.workspace + static_cast<int64_t>(pair) * a.words_per_pair;
        for (int32_t r = 0; r < rounds; ++r)
        {
            uint32_t p[4];
            build_patterns(q, n, reverse, r * 64 + lane, p);
            uint32_t* row = ws + static_cast<int64_t>(r) * 6 * 64 + lane;
            row[0 * 64]   = 0xffffffffu;
            row[1 * 64]   = 0u;
            row[2 * 64]   = p[0];
            row[3 * 64]   = p[1];
            row[4 * 64]   = p[2];
            row[5 * 64]   = p[3];
        }
    }

    int32_t score = n, best = n, best_col = 0; // the owner lane's are the pair's
    int32_t found = -1;                        // reverse: the first column at distance d_known (wave-uniform)
    for (int32_t j0 = 0; j0 < cols && found < 0; j0 += 64)
    {
        uint32_t code = 0;
        if (j0 + lane < cols)
            code = (static_cast<uint32_t>(static_cast<unsigned char>(reverse ? t[te - 1 - (j0 + lane)] : t[j0 + lane])) >> 1) & 3u;
        const int32_t count = min(64, cols - j0);
        for (int32_t k = 0; k < count; ++k)
        {
            const uint32_t ci = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int32_t>(code), k));
            uint32_t carry = 0u, ph_top = top, mh_top = 0u, ph, mh;
            if constexpr (W > 0)
            {
#pragma unroll
                for (int r = 0; r < R; ++r)
                {
                    if (r < rounds)
                    {
                        round_advance(lane, select4(ci, eq[r][0], eq[r][1], eq[r][2], eq[r][3]), pv[r], mv[r], ph, mh, carry, ph_top, mh_top);
                        if (r == owner_round)
                            score += static_cast<int32_t>((ph >> owner_bit) & 1u) - static_cast<int32_t>((mh >> owner_bit) & 1u);
                    }
                }
            }
            else
            {
                for (int32_t r = 0; r < rounds; ++r)
                {
                    uint32_t* row = ws + static_cast<int64_t>(r) * 6 * 64 + lane;
                    uint32_t p = row[0], v = row[64];
                    round_advance(lane, row[(2 + ci) * 64], p, v, ph, mh, carry, ph_top, mh_top);
                    row[0]  = p;
                    row[64] = v;
                    if (r == owner_round)
                        score += static_cast<int32_t>((ph >> owner_bit) & 1u) - static_cast<int32_t>((mh >> owner_bit) & 1u);
                }
            }
            if (!reverse)
            {
                if (score < best)
                {
                    best     = score;
                    best_col = j0 + k + 1;
                }
            }
            else if (__builtin_amdgcn_readlane(score, owner_lane) == d_known)
            {
                found = j0 + k + 1;
                break;
            }
        }
    }
    if (lane == owner_lane)
    {
        if (!reverse)
        {
            e[0] = best;
            e[1] = 0;
            e[2] = best_col;
        }
        else
            e[1] = found < 0 ? -1 : te - found;
    }
}

// Block b writes slice b: even, the query of pair pair_index[b / 2]; odd, its T[tb:te].
__global__ void __launch_bounds__(kThreads) semiglobal_gather_kernel(const int32_t* __restrict__ pair_index, const char* __restrict__ sequences,
                                                                     const int64_t* __restrict__ starts, const int32_t* __restrict__ ends,
                                                                     const int64_t* __restrict__ out_starts, char* __restrict__ out)
{
    const int64_t b    = blockIdx.x;
    const int32_t pair = pair_index[b >> 1];
    const int64_t at   = out_starts[b];
    int64_t len        = out_starts[b + 1] - at;
    const char* src;
    if ((b & 1) == 0)
    {
        src = sequences + starts[2 * pair];
        len = min(len, starts[2 * pair + 1] - starts[2 * pair]);
    }
    else
    {
        const int64_t tb = ends[3 * static_cast<int64_t>(pair) + 1], te = ends[3 * static_cast<int64_t>(pair) + 2];
        const int64_t m  = starts[2 * pair + 2] - starts[2 * pair + 1];
        if (tb < 0 || tb > te || te > m) // never reads outside the pair's target
            return;
        src = sequences + starts[2 * pair + 1] + tb;
        len = min(len, te - tb);
    }
    for (int64_t j = threadIdx.x; j < len; j += kThreads)
        out[at + j] = src[j];
}

int32_t rounds_of(int32_t query_length)
{
    const int32_t words = (std::max(query_length, 1) + kWord - 1) / kWord;
    return (words + 63) / 64;
}

} // namespace

extern "C" {

const char* gwhip_semiglobal_last_error(void)
{
    return g_error.c_str();
}

size_t gwhip_semiglobal_workspace_bytes(int32_t n_pairs, int32_t max_query_length)
{
    const int32_t rounds = rounds_of(max_query_length);
    if (n_pairs <= 0 || rounds <= kMaxRegWords)
        return 256;
    return 256 + static_cast<size_t>(n_pairs) * 6 * 64 * static_cast<size_t>(rounds) * sizeof(uint32_t);
}

int gwhip_semiglobal_ends(const gwhip_semiglobal_args* args, void* stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!args || args->n_pairs < 0 || args->max_query_length < 0 || (args->mode != GWHIP_SEMIGLOBAL_INFIX && args->mode != GWHIP_SEMIGLOBAL_PREFIX) ||
        (args->n_pairs > 0 && (!args->sequences || !args->sequence_starts || !args->ends)))
    {
        g_error = "gwhip_semiglobal_ends: invalid arguments";
        return static_cast<int>(hipErrorInvalidValue);
    }
    if (args->n_pairs == 0)
        return 0;
    const int32_t rounds = rounds_of(args->max_query_length);
    EndsArgs a{};
    a.sequences  = args->sequences;
    a.starts     = args->sequence_starts;
    a.ends       = args->ends;
    a.n          = args->n_pairs;
    a.max_rounds = rounds;
    a.prefix     = args->mode == GWHIP_SEMIGLOBAL_PREFIX ? 1 : 0;
    if (rounds > kMaxRegWords)
    {
        if (!args->workspace || args->workspace_bytes < gwhip_semiglobal_workspace_bytes(args->n_pairs, args->max_query_length))
        {
            g_error = "gwhip_semiglobal_ends: workspace too small";
            return static_cast<int>(hipErrorInvalidValue);
        }
        a.workspace      = reinterpret_cast<uint32_t*>(static_cast<char*>(args->workspace) + 256);
        a.words_per_pair = static_cast<int64_t>(6) * 64 * rounds;
    }
    const dim3 grid(static_cast<unsigned>((args->n_pairs + kWavesPerBlock - 1) / kWavesPerBlock)), block(kThreads);
    for (int pass = 0; pass < (a.prefix ? 1 : 2); ++pass)
    {
        a.reverse = pass;
        if (rounds <= 1)
            hipLaunchKernelGGL(semiglobal_ends_kernel<1>, grid, block, 0, stream, a);
        else if (rounds <= 2)
            hipLaunchKernelGGL(semiglobal_ends_kernel<2>, grid, block, 0, stream, a);
        else if (rounds <= 4)
            hipLaunchKernelGGL(semiglobal_ends_kernel<4>, grid, block, 0, stream, a);
        else if (rounds <= 8)
            hipLaunchKernelGGL(semiglobal_ends_kernel<8>, grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL(semiglobal_ends_kernel<0>, grid, block, 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return fail(e, "semiglobal_ends_kernel launch");
    }
    return 0;
}

int gwhip_semiglobal_gather(int32_t n_sub, const int32_t* pair_index, const char* sequences, const int64_t* sequence_starts,
                            const int32_t* ends, const int64_t* out_starts, char* out, void* stream)
{
    if (n_sub < 0 || (n_sub > 0 && (!pair_index || !sequences || !sequence_starts || !ends || !out_starts || !out)))
    {
        g_error = "gwhip_semiglobal_gather: invalid arguments";
        return static_cast<int>(hipErrorInvalidValue);
    }
    if (n_sub == 0)
        return 0;
    hipLaunchKernelGGL(semiglobal_gather_kernel, dim3(2u * static_cast<unsigned>(n_sub)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       pair_index, sequences, sequence_starts, ends, out_starts, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(e, "semiglobal_gather_kernel launch");
}

} // extern "C"
