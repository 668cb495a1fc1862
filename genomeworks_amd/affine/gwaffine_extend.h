// gwaffine_extend.h -- the affine X-drop extension on gfx950 (gwhip_extend of include/gwhip_affine.h; the rules are
// gwaffine_extend_rules.h). Included by gwaffine.hip behind its wavefront and its tile walk, which this file
// instantiates for the extension's geometry: lo = -B whatever the lengths are, rows up to a_max, one wave64 per pair.
//
// Forward pass: wave_step of the one-piece rules under the derived costs, K diagonals a lane, K in 1 .. 16. On top of
// a step, every lane takes the smallest H' among the cells it has just computed (the largest doubled score
// D = a A - H' of the anti-diagonal, as far as the lane sees it) and keeps its own best cell so far; one wave-wide
// minimum a step (four DPP moves inside the rows of 16 lanes, four lane reads across them) gives top(A), from which
// the running best and the stop test are wave-uniform scalars. The loop leaves at A_stop exactly, so nothing behind it
// is ever computed or counted. The lanes' best cells are reduced once, behind the loop, in the rules' order of end
// cells. kStore = false writes no bit and needs no workspace: scores, ends and flags only.
//
// Traceback: walk_tiles from the pair's own end cell instead of (n, m).

struct ExtendArgs
{
    const char* sequences;
    const int64_t* starts;
    const int64_t* offsets; // [n + 1] of the pairs' bit matrices in `bits`
    uint8_t* bits;
    int64_t bits_capacity;
    int8_t* results;
    int32_t* result_lengths;
    int32_t* scores;
    int32_t* query_ends;
    int32_t* target_ends;
    uint8_t* dropped;
    int32_t n;
    int32_t band;
    int32_t xdrop;
    ExtendScores s;
};

__device__ __forceinline__ Band extend_pair_band(const ExtendArgs& A, int64_t pair)
{
    const int64_t q0 = A.starts[2 * pair], t0 = A.starts[2 * pair + 1], t1 = A.starts[2 * pair + 2];
    return extend_band_of(t0 - q0, t1 - t0, A.band);
}

__global__ void __launch_bounds__(kScanThreads) extend_offsets_kernel(ExtendArgs A, int64_t* __restrict__ offsets)
{
    scan_offsets(A.n, [&](int64_t p) { return extend_bits_bytes(extend_pair_band(A, p)); }, offsets);
}

__device__ __forceinline__ void extend_no_result(const ExtendArgs& A, int64_t pair)
{
    A.scores[pair]      = -1;
    A.query_ends[pair]  = -1;
    A.target_ends[pair] = -1;
    A.dropped[pair]     = 0;
}

// the minimum of v over the 64 lanes, in every lane (all of them active)
__device__ __forceinline__ int32_t wave_min(int32_t v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, true));  // quad_perm:[1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, true));  // quad_perm:[2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, true)); // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, true)); // row_mirror: every lane has its row's
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// what the loop carries besides the wavefront's values: the lane's best cell, and the wave-uniform state of the stop rule
struct ExtendTrack
{
    EndCell mine;
    int32_t best, top_before;
};

// After anti-diagonal a, whose smallest H' in this lane is h at diagonal index k (kInf: the lane has no cell):
// true when the extension stops here.
__device__ __forceinline__ bool extend_track(ExtendTrack& tr, int32_t h, int32_t k, int32_t a, int32_t match, int32_t xdrop)
{
    const int32_t D = doubled_score(match, a, h);
    if (D > tr.mine.D) // an earlier anti-diagonal, and in it a smaller diagonal, keeps a tie
        tr.mine = EndCell{D, a, k};
    const int32_t top = doubled_score(match, a, wave_min(h));
    tr.best           = max(tr.best, top);
    const bool stops  = extend_stops(top, tr.top_before, tr.best, xdrop);
    tr.top_before     = top;
    return stops;
}

// the lane's smallest H' among its cells of parity PAR, and where
template <int K, int PAR>
__device__ __forceinline__ void lane_min(const int32_t (&H)[K], int32_t k0, int32_t& h, int32_t& k)
{
    h = kInf;
    k = k0 + PAR;
#pragma unroll
    for (int kk = PAR; kk < K; kk += 2)
        if (H[kk] < h)
        {
            h = H[kk];
            k = k0 + kk;
        }
}

template <int K, bool kStore>
__global__ void __launch_bounds__(kThreads) extend_forward_kernel(ExtendArgs A)
{
    const int64_t pair = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    const int lane     = threadIdx.x & 63;
    if (pair >= A.n)
        return; // whole waves leave together
    const int64_t q0 = A.starts[2 * pair], t0 = A.starts[2 * pair + 1];
    const Band b      = extend_pair_band(A, pair);
    const int64_t off = kStore ? A.offsets[pair] : 0;
    if (!b.aligned || b.W > 64 * K || (kStore && off + extend_bits_bytes(b) > A.bits_capacity))
    {
        if (lane == 0)
            extend_no_result(A, pair);
        return;
    }
    const Pair32 p{static_cast<int32_t>(b.n), static_cast<int32_t>(b.m), static_cast<int32_t>(b.lo),
                   static_cast<int32_t>(b.W), static_cast<int32_t>(b.stride)};
    const Costs c     = derived_costs(A.s);
    const char* Q     = A.sequences + q0;
    const char* T     = A.sequences + t0;
    uint8_t* bits     = kStore ? A.bits + off : nullptr;
    const int32_t k0  = lane * K;
    const int32_t end = static_cast<int32_t>(extend_a_max(b));
    const int32_t match = A.s.match, xdrop = A.xdrop;
    auto query_base  = [&](int32_t at) -> char { return at >= 0 && at < p.n ? Q[at] : char(0); };
    auto target_base = [&](int32_t at) -> char {
        return at >= 0 && at < p.m ? "ACTG"[(static_cast<unsigned char>(T[at]) >> 1) & 3] : char(1);
    };

    int32_t H[K], E[1][K], F[1][K];
    ExtendTrack tr{EndCell{kNoTop, 0, 0}, 0, 0};
#pragma unroll
    for (int kk = 0; kk < K; ++kk)
    {
        H[kk] = E[0][kk] = F[0][kk] = kInf;
        if (k0 + kk == -p.lo) // cell (0, 0), always a candidate
        {
            H[kk]   = 0;
            tr.mine = EndCell{0, 0, k0 + kk};
        }
    }
    if (kStore && lane == 0)
        bits[(-p.lo) >> 1] = 0;
    int32_t dropped = 0;

    if constexpr (K == 1)
    {
        for (int32_t a = 1; a <= end; ++a)
        {
            const int32_t par = (a + p.lo) & 1;
            int32_t hl = __shfl_up(H[0], 1, 64), hu = __shfl_down(H[0], 1, 64);
            int32_t el[1] = {__shfl_up(E[0][0], 1, 64)}, fu[1] = {__shfl_down(F[0][0], 1, 64)};
            if (lane == 0)
                hl = el[0] = kInf;
            if (lane == 63)
                hu = fu[0] = kInf;
            const bool mine = (lane & 1) == par;
            if (mine)
            {
                const int32_t d  = p.lo + lane;
                const int32_t i  = (a - d) >> 1;
                const int32_t j  = (a + d) >> 1;
                const bool valid = lane < p.W && i >= 0 && j >= 0 && i <= p.n && j <= p.m;
                const bool same  = valid && i > 0 && j > 0 && query_base(i - 1) == target_base(j - 1);
                const OnePiece::Out r = OnePiece::update(H[0], hl, el, hu, fu, same, c);
                H[0]                  = valid ? r.h : kInf;
                E[0][0]               = valid ? r.e[0] : kInf;
                F[0][0]               = valid ? r.f[0] : kInf;
                if (kStore && valid)
                    bits[static_cast<int64_t>(a) * p.stride + (lane >> 1)] = static_cast<uint8_t>(r.bits);
            }
            if (extend_track(tr, mine ? H[0] : kInf, lane, a, match, xdrop))
            {
                dropped = 1;
                break;
            }
        }
    }
    else
    {
        constexpr int C = K / 2;
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
            uint8_t* row = kStore ? bits + static_cast<int64_t>(a) * p.stride : nullptr;
            int32_t h, k;
            if (((a + p.lo) & 1) == 0)
            {
                const char entering = target_base(j0(a + 1) + C - 2);
                wave_step<OnePiece, K, 0, kStore>(H, E, F, qw, tw, a, k0, p, c, row, lane);
#pragma unroll
                for (int t = 0; t + 1 < C; ++t)
                    tw[t] = tw[t + 1];
                tw[C - 1] = entering;
                lane_min<K, 0>(H, k0, h, k);
            }
            else
            {
                const char entering = query_base(i0(a + 1) - 1);
                wave_step<OnePiece, K, 1, kStore>(H, E, F, qw, tw, a, k0, p, c, row, lane);
#pragma unroll
                for (int t = C - 1; t > 0; --t)
                    qw[t] = qw[t - 1];
                qw[0] = entering;
                lane_min<K, 1>(H, k0, h, k);
            }
            if (extend_track(tr, h, k, a, match, xdrop))
            {
                dropped = 1;
                break;
            }
        }
    }

    // the end cell of the wave: the first of the lanes' in the rules' order
    EndCell cell = tr.mine;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1)
    {
        const EndCell other{__shfl_xor(cell.D, step, 64), __shfl_xor(cell.a, step, 64), __shfl_xor(cell.k, step, 64)};
        if (end_cell_before(other, cell))
            cell = other;
    }
    if (lane == 0)
    {
        const int32_t d     = cell.k + p.lo;
        A.query_ends[pair]  = (cell.a - d) >> 1;
        A.target_ends[pair] = (cell.a + d) >> 1;
        A.scores[pair]      = cell.D / 2;
        A.dropped[pair]     = static_cast<uint8_t>(dropped);
    }
}

__global__ void __launch_bounds__(64) extend_traceback_kernel(ExtendArgs A)
{
    __shared__ uint32_t tile[kTileRows * kTileBytes / 4];
    const int64_t pair = blockIdx.x;
    const int lane     = threadIdx.x;
    if (A.scores[pair] < 0) // the forward pass gave no result
    {
        if (lane == 0)
            A.result_lengths[pair] = 0;
        return;
    }
    const Band b     = extend_pair_band(A, pair);
    const int64_t i  = A.query_ends[pair], j = A.target_ends[pair];
    int64_t len      = 0;
    const bool lost  = i < 0 || j < 0 || i > b.n || j > b.m ||
                      walk_tiles<OnePiece>(b, A.bits + A.offsets[pair], A.results + A.starts[2 * pair], i, j, i + j, lane, tile, len);
    if (lane == 0)
    {
        A.result_lengths[pair] = lost ? 0 : static_cast<int32_t>(len);
        if (lost)
            extend_no_result(A, pair);
    }
}

template <bool kStore>
void launch_extend_forward(int64_t per_lane, unsigned blocks, hipStream_t s, const ExtendArgs& A)
{
    if (per_lane <= 1)
        extend_forward_kernel<1, kStore><<<blocks, kThreads, 0, s>>>(A);
    else if (per_lane <= 2)
        extend_forward_kernel<2, kStore><<<blocks, kThreads, 0, s>>>(A);
    else if (per_lane <= 4)
        extend_forward_kernel<4, kStore><<<blocks, kThreads, 0, s>>>(A);
    else if (per_lane <= 8)
        extend_forward_kernel<8, kStore><<<blocks, kThreads, 0, s>>>(A);
    else // B <= 511: no band is wider
        extend_forward_kernel<16, kStore><<<blocks, kThreads, 0, s>>>(A);
}

// bytes of the workspace of a call with traceback; false: starts that do not ascend
bool size_extend_batch(int32_t n, const int64_t* starts, int32_t band, int64_t* bytes)
{
    *bytes = round256(8 * (static_cast<int64_t>(n) + 1));
    for (int64_t i = 0; i < n; ++i)
    {
        const int64_t ql = starts[2 * i + 1] - starts[2 * i], tl = starts[2 * i + 2] - starts[2 * i + 1];
        if (ql < 0 || tl < 0)
            return false;
        *bytes += extend_bits_bytes(extend_band_of(ql, tl, band));
    }
    return true;
}

int run_extend(const gwhip_extend_args* a, hipStream_t s, hipEvent_t* events)
{
    const std::string who = "gwhip_extend: ";
    if (a == nullptr || a->n_alignments < 0)
        return fail(hipErrorInvalidValue, who + "no arguments, or a negative number of alignments");
    if (!extend_in_range(a->match, a->mismatch, a->gap_open, a->gap_extend, a->band, a->xdrop))
        return fail(hipErrorInvalidValue,
                    who + "match " + std::to_string(a->match) + ", mismatch " + std::to_string(a->mismatch) + ", gap_open " +
                        std::to_string(a->gap_open) + ", gap_extend " + std::to_string(a->gap_extend) + ", band " +
                        std::to_string(a->band) + ", xdrop " + std::to_string(a->xdrop) +
                        " outside match >= 1, mismatch >= 0, match + mismatch <= 127, gap_open 0..127, gap_extend >= 1, "
                        "match + 2 gap_extend <= 255, band 0..511, xdrop -1..2^20");
    const int32_t n = a->n_alignments;
    if (n == 0)
        return 0;
    const bool store = a->results != nullptr;
    if (!a->sequences || !a->sequence_starts || !a->sequence_starts_host || !a->scores || !a->query_ends || !a->target_ends ||
        !a->dropped || (store && (!a->result_lengths || !a->workspace)))
        return fail(hipErrorInvalidValue, who + "a null pointer among the arguments");
    int64_t need = 0;
    if (!size_extend_batch(n, a->sequence_starts_host, a->band, &need))
        return fail(hipErrorInvalidValue, who + "sequence_starts_host does not ascend");
    if (store && a->workspace_bytes < static_cast<size_t>(need))
        return fail(hipErrorInvalidValue, who + "the workspace has " + std::to_string(a->workspace_bytes) +
                                              " bytes, the batch needs " + std::to_string(need));
    const int64_t head = round256(8 * (static_cast<int64_t>(n) + 1));
    ExtendArgs A{};
    A.sequences      = a->sequences;
    A.starts         = a->sequence_starts;
    A.offsets        = store ? static_cast<const int64_t*>(a->workspace) : nullptr;
    A.bits           = store ? static_cast<uint8_t*>(a->workspace) + head : nullptr;
    A.bits_capacity  = store ? static_cast<int64_t>(a->workspace_bytes) - head : 0;
    A.results        = a->results;
    A.result_lengths = a->result_lengths;
    A.scores         = a->scores;
    A.query_ends     = a->query_ends;
    A.target_ends    = a->target_ends;
    A.dropped        = a->dropped;
    A.n              = n;
    A.band           = a->band;
    A.xdrop          = a->xdrop;
    A.s              = ExtendScores{a->match, a->mismatch, a->gap_open, a->gap_extend};

    if (store)
        extend_offsets_kernel<<<1, kScanThreads, 0, s>>>(A, static_cast<int64_t*>(a->workspace));
    const unsigned blocks  = static_cast<unsigned>((static_cast<int64_t>(n) + kWavesPerBlock - 1) / kWavesPerBlock);
    const int64_t per_lane = (2 * static_cast<int64_t>(a->band) + 1 + 63) / 64;
    if (events && hipEventRecord(events[0], s) != hipSuccess)
        return fail(hipGetLastError(), who + "hipEventRecord");
    if (store)
        launch_extend_forward<true>(per_lane, blocks, s, A);
    else
        launch_extend_forward<false>(per_lane, blocks, s, A);
    if (events && hipEventRecord(events[1], s) != hipSuccess)
        return fail(hipGetLastError(), who + "hipEventRecord");
    if (store)
        extend_traceback_kernel<<<static_cast<unsigned>(n), 64, 0, s>>>(A);
    if (events && hipEventRecord(events[2], s) != hipSuccess)
        return fail(hipGetLastError(), who + "hipEventRecord");
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(e, who + "launch");
    return 0;
}
