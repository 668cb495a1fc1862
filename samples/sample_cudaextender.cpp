// sample_cudaextender.cpp -- ungapped X-drop extension of seed pairs through the C++ Extender interface, with either
// the host-pointer API (default) or the device-pointer API (-d). Prints the segments as CSV rows
// target,query,length,score with -p, and their count on stderr.
//
//   sample_cudaextender [-d] [-p] [-m scores.txt] [-x xdrop] [-t threshold] <target.fa> <query.fa> <seed_pairs.csv>
//
// scores.txt holds the 8 x 8 substitution scores (A C G T L N X E; row = target symbol) as 64 integers.
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I include -I /opt/rocm/include samples/sample_cudaextender.cpp
//        -L genomeworks_amd/lib -lcudaextender -lgenomeworks_amd -lgwhip -L /opt/rocm/lib -lamdhip64
#include <claraparabricks/genomeworks/cudaextender/extender.hpp>
#include <claraparabricks/genomeworks/cudaextender/utils.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/utils/cudautils.hpp>
#include <claraparabricks/genomeworks/utils/device_buffer.hpp>
#include <claraparabricks/genomeworks/utils/pinned_host_vector.hpp>
#include <claraparabricks/genomeworks/utils/signed_integer_utils.hpp>

#include <getopt.h>

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudaextender;

namespace
{

// Default scores: +100 for equal A/C/G/T, -100 for A/C/G/T mismatches, -1000 against L/N/X, -10000 against E.
std::vector<int32_t> default_scores()
{
    std::vector<int32_t> m(NUC2);
    for (int32_t t = 0; t < NUC; t++)
        for (int32_t q = 0; q < NUC; q++)
            m[t * NUC + q] = (t == E_NT || q == E_NT) ? -10000 : (t >= L_NT || q >= L_NT) ? -1000 : (t == q ? 100 : -100);
    return m;
}

// 64 whitespace-separated integers, row-major (row: target symbol, column: query symbol)
std::vector<int32_t> read_scores(const std::string& path)
{
    std::ifstream in(path);
    std::vector<int32_t> m;
    int32_t v;
    while (in >> v)
        m.push_back(v);
    if (m.size() != static_cast<size_t>(NUC2)) throw std::runtime_error("score matrix file needs 64 integers: " + path);
    return m;
}

pinned_host_vector<int8_t> read_encoded(const std::string& path)
{
    const std::string seq = io::create_kseq_fasta_parser(path, 0, false)->get_sequence_by_id(0).seq;
    pinned_host_vector<int8_t> encoded(seq.size());
    encode_sequence(encoded.data(), seq.c_str(), get_size<int32_t>(seq));
    return encoded;
}

} // namespace

int main(int argc, char* argv[])
{
    bool print = false, device_api = false;
    int32_t xdrop_threshold = 910, score_threshold = 3000;
    const bool no_entropy   = false;
    std::vector<int32_t> scores = default_scores();
    int c;
    while ((c = getopt(argc, argv, "pdm:x:t:h")) != -1)
    {
        if (c == 'p')
            print = true;
        else if (c == 'd')
            device_api = true;
        else if (c == 'm')
            scores = read_scores(optarg);
        else if (c == 'x')
            xdrop_threshold = std::atoi(optarg);
        else if (c == 't')
            score_threshold = std::atoi(optarg);
        else
        {
            std::cerr << "usage: " << argv[0]
                      << " [-d] [-p] [-m scores.txt] [-x xdrop] [-t threshold] <target.fa> <query.fa> <seed_pairs.csv>\n"
                      << "  -d  device-pointer API (default: host-pointer API)\n  -p  print the segments\n";
            return c == 'h' ? 0 : 1;
        }
    }
    if (argc - optind != 3)
    {
        std::cerr << "expected <target.fa> <query.fa> <seed_pairs.csv>" << std::endl;
        return 1;
    }

    Init();
    const pinned_host_vector<int8_t> target = read_encoded(argv[optind]);
    const pinned_host_vector<int8_t> query  = read_encoded(argv[optind + 1]);
    std::vector<SeedPair> seeds;
    parse_seed_pairs(argv[optind + 2], seeds);
    std::cerr << "seed pairs: " << seeds.size() << std::endl;

    CudaStream stream                = make_cuda_stream();
    DefaultDeviceAllocator allocator = create_default_device_allocator(1ull << 30, stream.get());
    std::unique_ptr<Extender> extender =
        create_extender(scores.data(), NUC2, xdrop_threshold, no_entropy, stream.get(), 0, allocator);

    std::vector<ScoredSegmentPair> segments;
    if (!device_api)
    {
        if (extender->extend_async(query.data(), get_size<int32_t>(query), target.data(), get_size<int32_t>(target),
                                   score_threshold, seeds) != StatusType::success ||
            extender->sync() != StatusType::success)
        {
            std::cerr << "extension failed" << std::endl;
            return 1;
        }
        segments = extender->get_scored_segment_pairs();
    }
    else
    {
        device_buffer<int8_t> d_query(get_size(query), allocator, stream.get());
        device_buffer<int8_t> d_target(get_size(target), allocator, stream.get());
        device_buffer<SeedPair> d_seeds(get_size(seeds), allocator, stream.get());
        device_buffer<ScoredSegmentPair> d_segments(get_size(seeds), allocator, stream.get());
        device_buffer<int32_t> d_count(1, allocator, stream.get());
        cudautils::device_copy_n_async(query.data(), query.size(), d_query.data(), stream.get());
        cudautils::device_copy_n_async(target.data(), target.size(), d_target.data(), stream.get());
        cudautils::device_copy_n_async(seeds.data(), seeds.size(), d_seeds.data(), stream.get());
        if (extender->extend_async(d_query.data(), get_size<int32_t>(d_query), d_target.data(),
                                   get_size<int32_t>(d_target), score_threshold, d_seeds.data(),
                                   get_size<int32_t>(d_seeds), d_segments.data(), d_count.data()) != StatusType::success)
        {
            std::cerr << "extension failed" << std::endl;
            return 1;
        }
        const int32_t n = cudautils::get_value_from_device(d_count.data(), stream.get());
        segments.resize(n);
        cudautils::device_copy_n_async(d_segments.data(), segments.size(), segments.data(), stream.get());
        GW_CU_CHECK_ERR(hipStreamSynchronize(stream.get()));
    }
    std::cerr << "scored segment pairs: " << segments.size() << std::endl;
    if (print)
        for (const ScoredSegmentPair& s : segments)
            std::cout << s.start_coord.target_position_in_read << "," << s.start_coord.query_position_in_read << ","
                      << s.length << "," << s.score << "\n";
    return 0;
}
