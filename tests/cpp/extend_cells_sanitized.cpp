// extend_cells_sanitized.cpp -- the affine X-drop extension's rules header
// (genomeworks_amd/affine/gwaffine_extend_rules.h) run serially on the host: the derived costs, the extension band and
// its bit matrix, the stop rule, the end cell and the traceback from it that the kernels of gwaffine.hip compile, here
// under AddressSanitizer and UBSan (tests/test_extend_oracle.py builds and runs it).
//
// usage: extend_cells_sanitized CASES
//   CASES holds one case per line: QUERY TARGET MATCH MISMATCH GAP_OPEN GAP_EXTEND BAND XDROP ("-" is an empty
//   sequence). Per case one line on stdout: QUERY_END TARGET_END SCORE DROPPED LENGTH STATES (states in forward order,
//   "-" for none); "-1 -1 -1 0 0 -" for a pair that gets no result.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gwaffine_extend_rules.h"

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
        std::string q, t;
        gwaffine::ExtendScores s{};
        int64_t B = 0, X = 0;
        if (!(fields >> q >> t >> s.match >> s.mismatch >> s.gap_open >> s.gap_extend >> B >> X))
        {
            std::fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        if (q == "-")
            q.clear();
        if (t == "-")
            t.clear();
        if (!gwaffine::extend_in_range(s.match, s.mismatch, s.gap_open, s.gap_extend, B, X))
        {
            std::fprintf(stderr, "case out of range: %s\n", line.c_str());
            return 2;
        }
        const gwaffine::Band b = gwaffine::extend_band_of(static_cast<int64_t>(q.size()), static_cast<int64_t>(t.size()), B);
        if (!b.aligned)
        {
            std::puts("-1 -1 -1 0 0 -");
            continue;
        }
        // exactly the sizes the rules name: the sanitizer sees any access beyond them
        std::vector<int32_t> h(static_cast<size_t>(b.W)), e(static_cast<size_t>(b.W)), f(static_cast<size_t>(b.W));
        std::vector<uint8_t> bits(static_cast<size_t>(gwaffine::extend_bits_bytes(b)));
        const gwaffine::Extended r =
            gwaffine::extend_serial(b, q.data(), t.data(), s, static_cast<int32_t>(X), h.data(), e.data(), f.data(), bits.data());
        const gwaffine::Extended alone =
            gwaffine::extend_serial(b, q.data(), t.data(), s, static_cast<int32_t>(X), h.data(), e.data(), f.data(), nullptr);
        if (alone.query_end != r.query_end || alone.target_end != r.target_end || alone.score != r.score || alone.dropped != r.dropped)
        {
            std::puts("-3 -3 -3 0 0 -"); // the score alone differs from the full call
            continue;
        }
        std::vector<int8_t> out(static_cast<size_t>(r.query_end + r.target_end));
        const int32_t len = gwaffine::walk_back_from(b, bits.data(), r.query_end, r.target_end, out.data());
        if (len < 0)
        {
            std::puts("-2 -2 -2 0 0 -");
            continue;
        }
        std::string states;
        for (int32_t k = len; k-- > 0;)
            states += static_cast<char>('0' + out[static_cast<size_t>(k)]);
        std::printf("%d %d %d %d %d %s\n", r.query_end, r.target_end, r.score, r.dropped, len, states.empty() ? "-" : states.c_str());
    }
    return 0;
}
