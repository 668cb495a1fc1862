// fasta_parser.cpp -- io::create_kseq_fasta_parser on top of cudamapper::read_fasta (overlap_alignment.cpp).
#include <claraparabricks/genomeworks/cudamapper/overlap_alignment.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>

#include <algorithm>
#include <random>
#include <stdexcept>

namespace claraparabricks
{
namespace genomeworks
{
namespace io
{
namespace
{

class FileFastaParser : public FastaParser
{
public:
    FileFastaParser(const std::string& path, number_of_basepairs_t min_length, bool shuffle)
    {
        for (auto& r : cudamapper::read_fasta(path))
            if (r.seq.size() >= min_length) records_.push_back(FastaSequence{std::move(r.name), std::move(r.seq)});
        if (shuffle)
        {
            std::mt19937 rng(0);
            std::shuffle(records_.begin(), records_.end(), rng);
        }
    }
    number_of_reads_t get_num_seqences() const override { return static_cast<number_of_reads_t>(records_.size()); }
    const FastaSequence& get_sequence_by_id(read_id_t sequence_id) const override { return records_.at(sequence_id); }

private:
    std::vector<FastaSequence> records_;
};

} // namespace

std::unique_ptr<FastaParser> create_kseq_fasta_parser(const std::string& fasta_file,
                                                      number_of_basepairs_t min_sequence_length, bool shuffle)
{
    return std::make_unique<FileFastaParser>(fasta_file, min_sequence_length, shuffle);
}

} // namespace io
} // namespace genomeworks
} // namespace claraparabricks
