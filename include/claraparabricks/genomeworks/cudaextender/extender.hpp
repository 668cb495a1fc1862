// extender.hpp -- the Extender interface of cudaextender: ungapped X-drop extension of seed pairs on the GPU
// (libcudaextender.so, HIP kernels for gfx950).
//
// Contract, for a seed (t, q) on encoded sequences T (target) and Q (query), score matrix M[8 * T[.] + Q[.]]:
//  - right: prefix scores s_k over columns (t+k, q+k), k = 0, 1, ...; the walk stops at the first k with
//    max(0, s_0..s_k) - s_k > xdrop_threshold, or at the end of either sequence. R = max(0, s before the stop); rpos =
//    first offset reaching R, -1 if R == 0. Left: the same over (t-k, q-k), k = 1, 2, ... giving L and lpos (0 if L == 0).
//  - total = R + L, length = rpos + lpos (so a segment may have length -1, as in SegAlign/GenomeWorks).
//  - unless no_entropy, a total in [score_threshold, 3 * score_threshold] is scaled by the base-4 entropy of the
//    matching A/C/G/T columns of the segment when there are at least 20 of them.
//  - a seed gives ScoredSegmentPair {(q - lpos, t - lpos), length, (int32)(total * entropy)} if that score reaches
//    score_threshold. Segments are sorted by unsigned diagonal (target - query), target, length descending, score
//    descending; a segment is dropped when it and the segment right before it in that order lie on one diagonal and
//    one contains the other (adjacent comparison, as thrust::unique_copy).
//
// Behaviour defined here where the original implementation leaves it undefined:
//  - a seed with target position >= target length or query position >= query length gives no segment and reads
//    nothing outside the sequences;
//  - a kept segment whose entropy is 0 has score 0;
//  - seeds are processed in chunks of floor(device memory / 1 GiB) * 4 194 304; each chunk is sorted and
//    de-duplicated on its own and its segments are appended after the previous chunk's;
//  - device scratch is taken from the allocator per call, sized to the chunk in use;
//  - create_extender() returns nullptr for score_mat_dim != 64 or an unknown ExtensionType;
//  - null pointers and negative lengths or counts return StatusType::invalid_input.
#pragma once

#include <claraparabricks/genomeworks/cudaextender/cudaextender.hpp>
#include <claraparabricks/genomeworks/types.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>

#include <cstdint>
#include <memory>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaextender
{

/// A seed: one position in the query and one in the target (8 bytes).
struct SeedPair
{
    position_in_read_t query_position_in_read;
    position_in_read_t target_position_in_read;
};

/// An extended segment: its first column, its length (see the contract above) and its score (16 bytes).
struct ScoredSegmentPair
{
    SeedPair start_coord;
    int32_t length;
    int32_t score;
};

/// Field-wise equality.
__host__ __device__ inline bool operator==(const ScoredSegmentPair& x, const ScoredSegmentPair& y)
{
    return x.start_coord.target_position_in_read == y.start_coord.target_position_in_read &&
           x.start_coord.query_position_in_read == y.start_coord.query_position_in_read && x.length == y.length &&
           x.score == y.score;
}

/// Seed extension on one device and stream.
class Extender
{
public:
    virtual ~Extender() = default;

    /// Host-pointer API: copies the encoded sequences and seeds to the device and extends them on the extender's
    /// stream. Results are read with sync() and get_scored_segment_pairs(). Resets earlier host-pointer results.
    virtual StatusType extend_async(const int8_t* h_query, int32_t query_length, const int8_t* h_target,
                                    int32_t target_length, int32_t score_threshold,
                                    const std::vector<SeedPair>& h_seed_pairs) = 0;

    /// Device-pointer API: everything lives on the device. d_scored_segment_pairs must hold num_seed_pairs
    /// entries; the segment count is written to *d_num_scored_segment_pairs on the extender's stream.
    virtual StatusType extend_async(const int8_t* d_query, int32_t query_length, const int8_t* d_target,
                                    int32_t target_length, int32_t score_threshold, const SeedPair* d_seed_pairs,
                                    int32_t num_seed_pairs, ScoredSegmentPair* d_scored_segment_pairs,
                                    int32_t* d_num_scored_segment_pairs) = 0;

    /// Waits for a host-pointer extend_async and copies its results to the host. invalid_operation if there was none.
    virtual StatusType sync() = 0;

    /// Results of the last host-pointer extend_async after sync(). Throws std::runtime_error if there was none.
    virtual const std::vector<ScoredSegmentPair>& get_scored_segment_pairs() const = 0;

    /// Drops host-pointer results and device buffers held for them.
    virtual void reset() = 0;
};

/// Creates an Extender. h_score_mat: score_mat_dim (= 64) int32 scores, M[8 * target + query]. Device scratch comes
/// from `allocator`. Returns nullptr for an unsupported score_mat_dim or ExtensionType.
std::unique_ptr<Extender> create_extender(const int32_t* h_score_mat, int32_t score_mat_dim, int32_t xdrop_threshold,
                                          bool no_entropy, cudaStream_t stream, int32_t device_id,
                                          DefaultDeviceAllocator allocator,
                                          ExtensionType type = ExtensionType::ungapped_xdrop);

} // namespace cudaextender
} // namespace genomeworks
} // namespace claraparabricks
