// types.hpp -- the integer types GenomeWorks' public headers share (read ids, positions inside a read).
// cudamapper/overlap_alignment.hpp declares the same two position / id types in its own namespace; both are
// std::uint32_t.
#pragma once

#include <cstdint>

namespace claraparabricks
{
namespace genomeworks
{

/// Index of a read in a read set.
using read_id_t = std::uint32_t;
/// Number of reads in a read set.
using number_of_reads_t = read_id_t;
/// 0-based position of a base inside a read.
using position_in_read_t = std::uint32_t;
/// Length of a sequence, in bases.
using number_of_basepairs_t = position_in_read_t;

} // namespace genomeworks
} // namespace claraparabricks
