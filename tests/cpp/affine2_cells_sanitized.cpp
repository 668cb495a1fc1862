// affine2_cells_sanitized.cpp -- the two-piece affine-gap aligner's rules header
// (genomeworks_amd/affine/gwaffine2_rules.h) run serially on the host: the band and its capacity, the five-matrix cell
// update, the optimality bound, the serial forward pass and the traceback that the kernels of gwaffine.hip compile,
// here under AddressSanitizer and UBSan (tests/test_affine2_oracle.py builds and runs it).
//
// usage: affine2_cells_sanitized CASES
//   CASES holds one case per line: QUERY TARGET MISMATCH GAP_OPEN GAP_EXTEND GAP_OPEN2 GAP_EXTEND2 BAND ("-" is an
//   empty sequence). Per case one line on stdout: COST OPTIMAL LENGTH STATES (states in forward order, "-" for none);
//   "-1 0 0 -" for a pair that gets no result.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gwaffine2_rules.h"

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
        gwaffine::Costs2 c{};
        int64_t B = 0;
        if (!(fields >> q >> t >> c.mismatch >> c.gap_open >> c.gap_extend >> c.gap_open2 >> c.gap_extend2 >> B))
        {
            std::fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        if (q == "-")
            q.clear();
        if (t == "-")
            t.clear();
        if (!gwaffine::costs2_in_range(c.mismatch, c.gap_open, c.gap_extend, c.gap_open2, c.gap_extend2, B))
        {
            std::fprintf(stderr, "case out of range: %s\n", line.c_str());
            return 2;
        }
        const int64_t n = static_cast<int64_t>(q.size()), m = static_cast<int64_t>(t.size());
        const gwaffine::Band b = gwaffine::band_of2(n, m, B);
        if (!b.aligned)
        {
            std::puts("-1 0 0 -");
            continue;
        }
        // exactly the sizes the rules name: the sanitizer sees any access beyond them
        std::vector<int32_t> values(static_cast<size_t>(5 * b.W));
        std::vector<uint8_t> bits(static_cast<size_t>(gwaffine::bits_bytes(b)));
        std::vector<int8_t> out(q.size() + t.size());
        const int32_t cost = gwaffine::forward_serial2(b, q.data(), t.data(), c, values.data(), bits.data());
        const int32_t len  = gwaffine::walk_back2(b, bits.data(), out.data());
        if (len < 0)
        {
            std::puts("-2 0 0 -");
            continue;
        }
        std::string states;
        for (int32_t k = len; k-- > 0;)
            states += static_cast<char>('0' + out[static_cast<size_t>(k)]);
        std::printf("%d %d %d %s\n", cost, gwaffine::cost_is_optimal2(cost, n, m, B, c) ? 1 : 0, len,
                    states.empty() ? "-" : states.c_str());
    }
    return 0;
}
