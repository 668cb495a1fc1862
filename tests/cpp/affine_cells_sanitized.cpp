// affine_cells_sanitized.cpp -- the affine-gap aligner's shared rules header (genomeworks_amd/affine/gwaffine_rules.h)
// run serially on the host: the band geometry, the layout of the bit matrix, the per-cell update, the optimality bound
// and the traceback that the kernels of gwaffine.hip compile, here under AddressSanitizer and UBSan
// (tests/test_affine_oracle.py builds and runs it).
//
// usage: affine_cells_sanitized CASES
//   CASES holds one case per line: QUERY TARGET MISMATCH GAP_OPEN GAP_EXTEND BAND ("-" is an empty sequence).
//   Per case one line on stdout: COST OPTIMAL LENGTH STATES (states in forward order, "-" for none); "-1 0 0 -" for a
//   pair that gets no result.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gwaffine_rules.h"

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
        gwaffine::Costs c{};
        int64_t B = 0;
        if (!(fields >> q >> t >> c.mismatch >> c.gap_open >> c.gap_extend >> B))
        {
            std::fprintf(stderr, "malformed case: %s\n", line.c_str());
            return 2;
        }
        if (q == "-")
            q.clear();
        if (t == "-")
            t.clear();
        if (!gwaffine::costs_in_range(c.mismatch, c.gap_open, c.gap_extend, B))
        {
            std::fprintf(stderr, "case out of range: %s\n", line.c_str());
            return 2;
        }
        const gwaffine::Band b = gwaffine::band_of(static_cast<int64_t>(q.size()), static_cast<int64_t>(t.size()), B);
        if (!b.aligned)
        {
            std::puts("-1 0 0 -");
            continue;
        }
        // exactly the sizes the rules name: the sanitizer sees any access beyond them
        std::vector<int32_t> h(static_cast<size_t>(b.W)), e(static_cast<size_t>(b.W)), f(static_cast<size_t>(b.W));
        std::vector<uint8_t> bits(static_cast<size_t>(gwaffine::bits_bytes(b)));
        std::vector<int8_t> out(q.size() + t.size());
        const int32_t cost = gwaffine::forward_serial(b, q.data(), t.data(), c, h.data(), e.data(), f.data(), bits.data());
        const int32_t len  = gwaffine::walk_back(b, bits.data(), out.data());
        if (len < 0)
        {
            std::puts("-2 0 0 -");
            continue;
        }
        std::string states;
        for (int32_t k = len; k-- > 0;)
            states += static_cast<char>('0' + out[static_cast<size_t>(k)]);
        std::printf("%d %d %d %s\n", cost,
                    gwaffine::cost_is_optimal(cost, static_cast<int64_t>(q.size()), static_cast<int64_t>(t.size()), B, c) ? 1 : 0,
                    len, states.empty() ? "-" : states.c_str());
    }
    return 0;
}
