// anchor_plan_sanitized.cpp -- the rules header of anchored overlap alignment
// (genomeworks_amd/mapper/gwm_anchor_plan.hpp) run serially on the host: the slice coordinates, the valid test, the
// order check, the cut rule and the pieces that the kernels of gwm_anchored.hip compile, here under AddressSanitizer
// and UBSan (tests/test_mapper_anchored_oracle.py builds and runs it).
//
// usage: anchor_plan_sanitized CASES
//   CASES holds one case per line:
//     R QUERY_START QUERY_END TARGET_START TARGET_END STRAND K S COUNT Q0 T0 Q1 T1 ...   a record and its anchors
//     O N N_ANCHORS OFFSET_0 ... OFFSET_N                                               the offsets of a call
//   Per R line one line on stdout: "PIECES U V QUERY_LENGTH TARGET_LENGTH ..." for every piece, or "-1" when the valid
//   anchors are not strictly increasing, or "range" for K or S out of range. Per O line the first bad entry, or -1.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "gwm_anchor_plan.hpp"

int main(int argc, char** argv)
{
    if (argc != 2)
    {
        std::fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in)
    {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    while (std::getline(in, line))
    {
        if (line.empty())
            continue;
        std::istringstream fields(line);
        std::string kind;
        fields >> kind;
        if (kind == "O")
        {
            int64_t n = 0, n_anchors = 0;
            fields >> n >> n_anchors;
            std::vector<int64_t> offsets(static_cast<size_t>(n + 1)); // exactly n + 1: the sanitizer sees a read beyond
            for (int64_t& v : offsets)
                fields >> v;
            if (!fields)
            {
                std::fprintf(stderr, "malformed case: %s\n", line.c_str());
                return 2;
            }
            std::printf("%lld\n", static_cast<long long>(gwm_plan::first_bad_offset(offsets.data(), n, n_anchors)));
            continue;
        }
        gwm_plan::Record r{};
        std::string strand;
        int64_t k = 0, spacing = 0, count = 0;
        if (kind != "R" ||
            !(fields >> r.query_start >> r.query_end >> r.target_start >> r.target_end >> strand >> k >> spacing >> count))
        {
            std::fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        r.minus = strand == "-";
        std::vector<uint32_t> anchors(static_cast<size_t>(2 * count));
        for (uint32_t& v : anchors)
            fields >> v;
        if (!fields)
        {
            std::fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        if (!gwm_plan::parameters_in_range(k, spacing))
        {
            std::puts("range");
            continue;
        }
        // first the count alone, then exactly that many pieces
        const int64_t pieces = gwm_plan::plan_record_serial(r, anchors.data(), count, k, spacing, nullptr);
        if (pieces < 0)
        {
            std::puts("-1");
            continue;
        }
        std::vector<gwm_plan::Piece> out(static_cast<size_t>(pieces));
        if (gwm_plan::plan_record_serial(r, anchors.data(), count, k, spacing, out.data()) != pieces)
            return 3;
        std::printf("%lld", static_cast<long long>(pieces));
        for (const gwm_plan::Piece& p : out)
            std::printf(" %lld %lld %lld %lld", static_cast<long long>(p.u), static_cast<long long>(p.v),
                        static_cast<long long>(p.query_length), static_cast<long long>(p.target_length));
        std::puts("");
    }
    return 0;
}
