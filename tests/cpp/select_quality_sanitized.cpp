// select_quality_sanitized.cpp -- a stand-alone caller of the host selection with quality sums (genomeworks_amd/mapper/
// gwm_windows.cpp, rule Q2 of INTEGRATION.md section 3l), built by tests/test_polish_quality_oracle.py together with that
// source under -fsanitize=address,undefined. It reads cases from the file named on the command line and prints what
// the selection returns; the test compares the text with the oracle's answers.
//
// A case:  polish W D Q n_queries n_targets n_overlaps n_segments has_sums
//          or  correct W D Q n_reads n_pairs n_target_role n_query_role has_sums
//          the target (read) lengths
//          per overlap:  query_read target_read query_start target_start query_end target_end strand(+|-)
//          per segment:  overlap window target_first target_last query_begin query_end   (correct: target role first)
//          has_sums 1: one quality sum per segment, in the same order; 0: nullptr
// Answer:  case <sequences> <windows> / p set read begin end reversed / w target_read window first_sequence sequences,
//          or "error" where the selection throws. Read ids count from 0.
#include "../../genomeworks_amd/mapper/gwm_windows.hpp"

#include <cstdio>
#include <exception>
#include <fstream>
#include <string>

int main(int argc, char** argv)
{
    if (argc != 2)
        return 2;
    std::ifstream in(argv[1]);
    std::string word;
    while (in >> word)
    {
        const bool correct = word == "correct";
        if (!correct && word != "polish")
            return 3;
        int32_t W, D, Q, n_first, n_second;
        int64_t no, na, nb = 0;
        int has_sums;
        if (correct)
        {
            in >> W >> D >> Q >> n_first >> no >> na >> nb >> has_sums;
            n_second = n_first;
        }
        else
            in >> W >> D >> Q >> n_first >> n_second >> no >> na >> has_sums;
        std::vector<int64_t> lengths(static_cast<size_t>(n_second));
        for (int64_t& l : lengths)
            in >> l;
        std::vector<gwm_overlap> overlaps(static_cast<size_t>(no));
        for (gwm_overlap& o : overlaps)
        {
            char strand;
            o = gwm_overlap{};
            in >> o.query_read_id >> o.target_read_id >> o.query_start_position_in_read >>
                o.target_start_position_in_read >> o.query_end_position_in_read >> o.target_end_position_in_read >> strand;
            o.relative_strand = static_cast<uint8_t>(strand);
        }
        std::vector<gwm_segment> segments(static_cast<size_t>(na + nb));
        for (gwm_segment& s : segments)
            in >> s.overlap >> s.window >> s.target_first >> s.target_last >> s.query_begin >> s.query_end;
        std::vector<uint32_t> sums(has_sums ? segments.size() : 0);
        for (uint32_t& s : sums)
            in >> s;
        if (!in)
            return 4;
        // exactly as many sums as records, so that a read past either end is the sanitizer's to find
        const uint32_t* of_first  = has_sums ? sums.data() : nullptr;
        const uint32_t* of_second = has_sums ? sums.data() + na : nullptr;
        try
        {
            const gwm::window_selection r =
                correct ? gwm::select_correction_layers(segments.data(), na, segments.data() + na, nb, overlaps.data(), no,
                                                        lengths.data(), n_first, 0, W, D, of_first, of_second, Q)
                        : gwm::select_layers(segments.data(), na, overlaps.data(), no, n_first, 0, lengths.data(),
                                             n_second, 0, W, D, of_first, Q);
            std::printf("case %zu %zu\n", r.plan.size(), r.windows.size());
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
