// select_correction_sanitized.cpp -- a stand-alone caller of read correction's host rules (genomeworks_amd/mapper/
// gwm_windows.cpp: select_pairs and select_correction_layers), built by tests/test_correct_oracle.py together with
// that source under -fsanitize=address,undefined. It reads cases from the file named on the command line and prints
// what the rules return; the test compares the text with the hand cases' expected answers.
//
// A case:  pairs n_overlaps
//          per overlap:  query_read target_read query_start target_start query_end target_end strand(+|-)
// Answer:  pairs <kept> / one position per line, or "error".
// A case:  layers W D n_reads first_read_id n_pairs n_target_role n_query_role
//          the read lengths
//          per pair:     as per overlap above
//          per segment:  overlap window target_first target_last query_begin query_end  (target role, then query role)
// Answer:  layers <sequences> <windows> / p set read begin end reversed / w read window first_sequence sequences,
//          or "error" where the selection throws.
#include "../../genomeworks_amd/mapper/gwm_windows.hpp"

#include <cstdio>
#include <exception>
#include <fstream>
#include <string>

namespace
{

void read_overlaps(std::istream& in, std::vector<gwm_overlap>& overlaps)
{
    for (gwm_overlap& o : overlaps)
    {
        char strand;
        o = gwm_overlap{};
        in >> o.query_read_id >> o.target_read_id >> o.query_start_position_in_read >> o.target_start_position_in_read >>
            o.query_end_position_in_read >> o.target_end_position_in_read >> strand;
        o.relative_strand = static_cast<uint8_t>(strand);
    }
}

void read_segments(std::istream& in, std::vector<gwm_segment>& segments)
{
    for (gwm_segment& s : segments)
        in >> s.overlap >> s.window >> s.target_first >> s.target_last >> s.query_begin >> s.query_end;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 2)
        return 2;
    std::ifstream in(argv[1]);
    std::string word;
    while (in >> word)
    {
        if (word == "pairs")
        {
            int64_t no;
            in >> no;
            std::vector<gwm_overlap> overlaps(static_cast<size_t>(no));
            read_overlaps(in, overlaps);
            if (!in)
                return 4;
            try
            {
                const std::vector<int64_t> kept = gwm::select_pairs(overlaps.data(), no);
                std::printf("pairs %zu\n", kept.size());
                for (int64_t i : kept)
                    std::printf("%lld\n", static_cast<long long>(i));
            }
            catch (const std::exception&)
            {
                std::printf("error\n");
            }
            continue;
        }
        if (word != "layers")
            return 3;
        int32_t W, D, nr;
        uint32_t first;
        int64_t np, nt, nq;
        in >> W >> D >> nr >> first >> np >> nt >> nq;
        std::vector<int64_t> lengths(static_cast<size_t>(nr));
        for (int64_t& l : lengths)
            in >> l;
        std::vector<gwm_overlap> pairs(static_cast<size_t>(np));
        read_overlaps(in, pairs);
        std::vector<gwm_segment> target_role(static_cast<size_t>(nt)), query_role(static_cast<size_t>(nq));
        read_segments(in, target_role);
        read_segments(in, query_role);
        if (!in)
            return 4;
        try
        {
            const gwm::window_selection r = gwm::select_correction_layers(
                target_role.data(), nt, query_role.data(), nq, pairs.data(), np, lengths.data(), nr, first, W, D);
            std::printf("layers %zu %zu\n", r.plan.size(), r.windows.size());
            for (const gwm_gather_entry& e : r.plan)
                std::printf("p %u %u %u %u %u\n", e.set, e.read, e.begin, e.end, e.reversed);
            for (const gwm::window_record& w : r.windows)
                std::printf("w %u %u %u %u\n", w.target_read, w.window, w.first_sequence, w.n_sequences);
        }
        catch (const std::exception&)
        {
            std::printf("error\n");
        }
    }
    return 0;
}
