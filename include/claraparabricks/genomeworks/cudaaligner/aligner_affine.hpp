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

/// Scores of the affine X-drop extension, maximised: a match scores +match, a mismatch -mismatch, a gap run of L columns
/// -(gap_open + L * gap_extend). match >= 1, mismatch >= 0, match + mismatch <= 127, 0 <= gap_open <= 127,
/// gap_extend >= 1, match + 2 * gap_extend <= 255. The defaults are minimap2's -A2 -B4 -O4 -E2, conventions and not tuned.
struct ExtensionScoring
{
    int32_t match      = 2;
    int32_t mismatch   = 4;
    int32_t gap_open   = 4;
    int32_t gap_extend = 2;
};

/// An aligner with the limits and statuses of create_aligner(max_query_length, max_target_length, max_alignments, ...)
/// whose alignments are extension_alignment: from the first base of both sequences a prefix of the query is aligned with
/// a prefix of the target, within band_width (0 .. 511) diagonals on either side of the start's, and the extension
/// stops once the best score of two neighbouring anti-diagonals lies more than xdrop (0 .. 2^20; -1: never) below the
/// best score so far (include/gwhip_affine.h states the rules). An alignment has status success, is_optimal() false
/// (nothing is proven), the count of its non-match columns as edit distance, and a CIGAR over the aligned prefixes only;
/// get_alignment_extension names them. Throws std::invalid_argument for a scoring, band_width or xdrop out of range.
std::unique_ptr<Aligner> create_aligner_extension(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                                  ExtensionScoring scoring, int32_t band_width, int32_t xdrop,
                                                  DefaultDeviceAllocator allocator, cudaStream_t stream, int32_t device_id);
/// The same with an allocator of max_device_memory bytes (-1: the largest free section of the device).
std::unique_ptr<Aligner> create_aligner_extension(int32_t max_query_length, int32_t max_target_length, int32_t max_alignments,
                                                  ExtensionScoring scoring, int32_t band_width, int32_t xdrop, cudaStream_t stream,
                                                  int32_t device_id, int64_t max_device_memory = -1);

/// Where an extension ended: query[0:query_end] is aligned with target[0:target_end] at `score`; dropped says that the
/// stop rule ended it before the band's last anti-diagonal.
struct Extension
{
    int32_t query_end, target_end, score;
    bool dropped;
};

/// Of an alignment made by an extension aligner; all -1 (dropped false) for one without a result and for other
/// aligners' alignments.
Extension get_alignment_extension(const Alignment& alignment);

} // namespace cudaaligner
} // namespace genomeworks
} // namespace claraparabricks
