// fasta_parser.hpp -- read-only access to the records of a FASTA file (libgenomeworks_amd.so). The records are read
// with the project's own FASTA reader (the one align_overlaps uses); no kseq.
#pragma once

#include <claraparabricks/genomeworks/types.hpp>

#include <memory>
#include <string>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace io
{

/// One FASTA record: the header's first word and the sequence lines joined.
struct FastaSequence
{
    std::string name;
    std::string seq;
};

/// The records of one FASTA file.
class FastaParser
{
public:
    virtual ~FastaParser() = default;
    /// Number of records kept.
    virtual number_of_reads_t get_num_seqences() const = 0;
    /// Record `sequence_id` (0-based; throws std::out_of_range past the end).
    virtual const FastaSequence& get_sequence_by_id(read_id_t sequence_id) const = 0;
};

/// Reads `fasta_file`, keeps the records with at least min_sequence_length bases, and shuffles them (fixed seed)
/// when `shuffle` is set. Throws std::runtime_error if the file cannot be read.
std::unique_ptr<FastaParser> create_kseq_fasta_parser(const std::string& fasta_file,
                                                      number_of_basepairs_t min_sequence_length = 0,
                                                      bool shuffle                              = true);

} // namespace io
} // namespace genomeworks
} // namespace claraparabricks
