// utils.hpp -- encoding constants and small file readers for cudaextender callers.
#pragma once

#include <claraparabricks/genomeworks/cudaextender/extender.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>

#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaextender
{

/// Symbol codes of an encoded sequence (index into the 8 x 8 score matrix).
constexpr int8_t A_NT = 0; ///< A
constexpr int8_t C_NT = 1; ///< C
constexpr int8_t G_NT = 2; ///< G
constexpr int8_t T_NT = 3; ///< T
constexpr int8_t L_NT = 4; ///< lower-case a, c, g, t
constexpr int8_t N_NT = 5; ///< N, n
constexpr int8_t X_NT = 6; ///< any other character
constexpr int8_t E_NT = 7; ///< '&'
constexpr int8_t NUC  = 8;         ///< symbols per axis of the score matrix
constexpr int8_t NUC2 = NUC * NUC; ///< entries of the score matrix

namespace details
{
inline int32_t next_csv_int(std::istream& in, char sep, bool& ok)
{
    std::string field;
    ok = static_cast<bool>(std::getline(in, field, sep));
    return std::atoi(field.c_str());
}
} // namespace details

/// Appends the seed pairs of a CSV file with rows `target_position,query_position`.
inline void parse_seed_pairs(const std::string& filepath, std::vector<SeedPair>& seed_pairs)
{
    std::ifstream in(filepath);
    if (!in.is_open()) throw std::runtime_error("Cannot open file " + filepath);
    bool ok = true;
    while (true)
    {
        SeedPair s;
        s.target_position_in_read = static_cast<position_in_read_t>(details::next_csv_int(in, ',', ok));
        if (!ok) break;
        s.query_position_in_read = static_cast<position_in_read_t>(details::next_csv_int(in, '\n', ok));
        seed_pairs.push_back(s);
    }
}

/// Appends the segments of a CSV file with rows `target_position,query_position,length,score`.
inline void parse_scored_segment_pairs(const std::string& filepath, std::vector<ScoredSegmentPair>& scored_segment_pairs)
{
    std::ifstream in(filepath);
    if (!in.is_open()) throw std::runtime_error("Cannot open file " + filepath);
    bool ok = true;
    while (true)
    {
        ScoredSegmentPair s;
        s.start_coord.target_position_in_read = static_cast<position_in_read_t>(details::next_csv_int(in, ',', ok));
        if (!ok) break;
        s.start_coord.query_position_in_read = static_cast<position_in_read_t>(details::next_csv_int(in, ',', ok));
        s.length                             = details::next_csv_int(in, ',', ok);
        s.score                              = details::next_csv_int(in, '\n', ok);
        scored_segment_pairs.push_back(s);
    }
}

/// Encodes `length` characters of src_seq into dst_seq (A_NT ... E_NT).
inline void encode_sequence(int8_t* dst_seq, const char* src_seq, const int32_t length)
{
    for (int32_t i = 0; i < length; i++)
    {
        int8_t code = X_NT;
        switch (src_seq[i])
        {
        case 'A': code = A_NT; break;
        case 'C': code = C_NT; break;
        case 'G': code = G_NT; break;
        case 'T': code = T_NT; break;
        case 'a':
        case 'c':
        case 'g':
        case 't': code = L_NT; break;
        case 'N':
        case 'n': code = N_NT; break;
        case '&': code = E_NT; break;
        default: break;
        }
        dst_seq[i] = code;
    }
}

} // namespace cudaextender
} // namespace genomeworks
} // namespace claraparabricks
