// select_layers_sanitized.cpp -- a stand-alone caller of polishing's host selection (genomeworks_amd/mapper/
// gwm_windows.cpp), built by tests/test_polish_oracle.py together with that source under -fsanitize=address,undefined.
// It reads cases from the file named on the command line and prints what the selection returns; the test compares
// the text with the hand cases' expected answers.
//
// A case:  case W D n_queries first_query_id n_targets first_target_id n_overlaps n_segments
//          the target lengths
//          per overlap:  query_read target_read query_start target_start query_end target_end strand(+|-)
//          per segment:  overlap window target_first target_last query_begin query_end
// Answer:  case <sequences> <windows> / p set read begin end reversed / w target_read window first_sequence sequences,
//          or "error" where the selection throws.
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
        if (word != "case")
            return 3;
        int32_t W, D, nq, nt;
        uint32_t fq, ft;
        int64_t no, ns;
        in >> W >> D >> nq >> fq >> nt >> ft >> no >> ns;
        std::vector<int64_t> lengths(static_cast<size_t>(nt));
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
        std::vector<gwm_segment> segments(static_cast<size_t>(ns));
        for (gwm_segment& s : segments)
            in >> s.overlap >> s.window >> s.target_first >> s.target_last >> s.query_begin >> s.query_end;
        if (!in)
            return 4;
        try
        {
            const gwm::window_selection r = gwm::select_layers(segments.data(), ns, overlaps.data(), no, nq, fq,
                                                               lengths.data(), nt, ft, W, D);
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
