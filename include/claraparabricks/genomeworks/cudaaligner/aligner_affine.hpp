// aligner_affine.hpp -- global alignment under affine gap costs inside a diagonal band. No counterpart in the
// reference, whose aligners are unit-cost. The rules are stated in include/gwhip_affine.h.
#pragma once

#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>
#include <claraparabricks/genomeworks/cudaaligner/alignment.hpp>

#include <cstdint>
#include <memory>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaaligner
{

/// Costs are minimised and a match costs 0; a gap run of L columns costs gap_open + L * gap_extend.
/// 1 <= mismatch <= 255, 0 <= gap_open <= 255, 1 <= gap_extend <= 255. The defaults are conventions, not tuned on data.
struct AffineScoring
{
    int32_t mismatch   = 4;
    int32_t gap_open   = 6;
    int32_t gap_extend = 2;
};

/// An aligner with the limits and statuses of create_aligner(max_query_length, max_target_length, max_alignments, ...)
/// whose alignments are global_alignment under `scoring`, restricted to the diagonals
/// [min(0, m - n) - band_width, max(0, m - n) + band_width] of every pair. An alignment's is_optimal() says that its
/// cost is the optimum of the full matrix; a pair whose band has more than 2048 diagonals keeps the status
/// uninitialized. Throws std::invalid_argument for a scoring or band_width out of range.
std::unique_ptr<Aligner> create_aligner_affine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                               AffineScoring scoring, int32_t band_width, DefaultDeviceAllocator allocator,
                                               cudaStream_t stream, int32_t device_id);
/// The same with an allocator of max_device_memory bytes (-1: the largest free section of the device); a batch whose
/// device buffers would exceed them is refused by add_alignment with exceeded_max_alignments.
std::unique_ptr<Aligner> create_aligner_affine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                               AffineScoring scoring, int32_t band_width, cudaStream_t stream,
                                               int32_t device_id, int64_t max_device_memory = -1);

/// Two-piece gap costs: a gap run of L columns costs min(gap_open + L * gap_extend, gap_open2 + L * gap_extend2), so a
/// short gap and a long one are each priced by the piece that suits it. Ranges as AffineScoring's, for both pieces; no
/// order between the pieces is required. The defaults are minimap2's -A2 -B4 -O4,24 -E2,1 in cost form for a global
/// alignment (INTEGRATION.md section 3p derives them); the pieces cross at L = 20.
struct TwoPieceScoring
{
    int32_t mismatch    = 6;
    int32_t gap_open    = 4;
    int32_t gap_extend  = 3;
    int32_t gap_open2   = 24;
    int32_t gap_extend2 = 2;
};

/// As the two above under two-piece costs; here a pair whose band has more than 1024 diagonals keeps the status
/// uninitialized. get_alignment_cost, is_optimal and the statuses behave as for the one-piece aligner.
std::unique_ptr<Aligner> create_aligner_affine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                               TwoPieceScoring scoring, int32_t band_width, DefaultDeviceAllocator allocator,
                                               cudaStream_t stream, int32_t device_id);
std::unique_ptr<Aligner> create_aligner_affine(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                               TwoPieceScoring scoring, int32_t band_width, cudaStream_t stream,
                                               int32_t device_id, int64_t max_device_memory = -1);

/// The cost of an alignment made by an affine aligner; -1 for one without a result and for other aligners' alignments.
int32_t get_alignment_cost(const Alignment& alignment);

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
