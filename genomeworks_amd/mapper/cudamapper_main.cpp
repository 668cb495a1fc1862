// cudamapper_main.cpp -- the `cudamapper` command-line tool: a thin main over gw_mapper_map_batched_cached
// (include/gw_mapper_capi.h), the project's FASTA reader and its PAF writer (cudamapper/overlap_alignment.hpp).
//
//   cudamapper [options] query.fasta target.fasta > overlaps.paf
//
// Option letters and defaults are those of the reference's cudamapper (application_parameters.cpp) for
// -k -w -i -t -F -r -l -b -z -R -D -Q -q -C -c -h -v. One device; options that ask for anything else are refused
// with a message instead of being ignored. --cigar (no letter) aligns the printed records on the device and adds the
// cg:Z: column. -Q -q -C -c size the index cache as in the reference, with its checks and its two notes about -C / -c;
// a run without any of them walks one index pair at a time (1, 1, 1, 1), which keeps the order of the PAF lines that
// this tool has always printed. The reference's defaults (10, 5) apply to those not given once one of them is.
// --chain (no letter) finds the overlaps of every index pair with the chaining overlapper instead of the triggered
// one; --chain-max-gap, --chain-bandwidth, --chain-min-score and --chain-max-chains set its parameters.
#include "gw_mapper_capi.h"

#include <claraparabricks/genomeworks/cudamapper/overlap_alignment.hpp>

#include <getopt.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <iostream>
#include <string>
#include <vector>

namespace
{

using namespace claraparabricks::genomeworks::cudamapper;

// gwhip_mapper.h's gwm_overlap, == cudamapper::Overlap of the reference (36 B)
struct overlap_record
{
    uint32_t query_read_id;
    uint32_t target_read_id;
    uint32_t query_start_position_in_read;
    uint32_t target_start_position_in_read;
    uint32_t query_end_position_in_read;
    uint32_t target_end_position_in_read;
    uint8_t relative_strand;
    uint32_t num_residues;
    uint8_t overlap_complete;
};
static_assert(sizeof(overlap_record) == 36, "overlap layout");

void help(std::FILE* f)
{
    std::fputs(
        "Usage: cudamapper [options ...] <query_sequences> <target_sequences>\n"
        "     <sequences> FASTA files; the same path twice maps all against all\n"
        "  -k, --kmer-size              length of kmer to use for minimizers [15] (Max=32)\n"
        "  -w, --window-size            length of window to use for minimizers [10]\n"
        "  -i, --index-size             length of batch size used for query in MB [30] (a decimal fraction is accepted)\n"
        "  -t, --target-index-size      length of batch sized used for target in MB [30]\n"
        "  -F, --filtering-parameter    remove representations with frequency >= this value; 1.0 disables [1e-5];\n"
        "                               off by default for less than 0.5 Mbp of input\n"
        "  -r, --min-residues           minimum number of matching residues in an overlap [3]\n"
        "  -l, --min-overlap-length     minimum length for an overlap [250]\n"
        "  -b, --min-bases-per-residue  minimum number of bases in overlap per match [1000]\n"
        "  -z, --min-overlap-fraction   minimum ratio of overlap length to alignment length [0.8]\n"
        "  -R, --rescue-overlap-ends    extend the ends of overlaps over similar flanks\n"
        "  -D, --drop-fused-overlaps    remove overlaps which are joined into larger overlaps\n"
        "      --cigar                  align every printed overlap on the device and add its CIGAR as a cg:Z: column\n"
        "      --chain                  chain the anchors of every read pair by dynamic programming, both strands,\n"
        "                               instead of the triggered overlapper\n"
        "      --chain-max-gap          largest step of a chain in query and in target [5000] (needs --chain)\n"
        "      --chain-bandwidth        largest difference of the two steps [500] (needs --chain)\n"
        "      --chain-min-score        smallest score of a chain [40] (needs --chain)\n"
        "      --chain-max-chains       chains per read pair and strand [4] (1..64, needs --chain)\n"
        "  -Q, --query-indices-in-host-memory    query indices kept as packed copies in host memory [10]\n"
        "  -q, --query-indices-in-device-memory  query indices kept in device memory [5]\n"
        "  -C, --target-indices-in-host-memory   target indices kept in host memory [as -Q]\n"
        "  -c, --target-indices-in-device-memory target indices kept in device memory [as -q]\n"
        "                               without any of -Q -q -C -c one index pair is walked at a time (all four 1);\n"
        "                               the order of the output lines follows the batches\n"
        "  -v, --version                version information\n"
        "  -h, --help                   this message\n"
        "Not in this tool: -a (its letter stays refused: the reference aligns before fusion appends its records, so its\n"
        "CIGARs and overlaps disagree, while --cigar aligns the final records; align_overlaps still aligns any PAF),\n"
        "-d other than 1, -m, -S -B, gzipped input.\n",
        f);
}

[[noreturn]] void refuse(const std::string& what)
{
    std::cerr << "cudamapper: " << what << std::endl;
    std::exit(1);
}

bool is_gzip(const std::string& path)
{
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f)
        return false;
    const int a = std::fgetc(f), b = std::fgetc(f);
    std::fclose(f);
    return a == 0x1f && b == 0x8b;
}

struct packed_reads
{
    std::string bases;
    std::vector<int64_t> offsets{0};
    explicit packed_reads(const std::vector<FastaSequence>& reads)
    {
        for (const FastaSequence& r : reads)
        {
            bases += r.seq;
            offsets.push_back(static_cast<int64_t>(bases.size()));
        }
    }
};

} // namespace

int main(int argc, char** argv)
{
    int32_t k = 15, w = 10, min_residues = 3, min_overlap_len = 250, min_bases_per_residue = 1000;
    double index_size = 30, target_index_size = 30, filtering_parameter = 1e-5;
    float min_overlap_fraction = 0.8f;
    bool rescue = false, drop = false, custom_filter = false;
    int cigar = 0, chain = 0;
    int32_t chain_max_gap = 5000, chain_bandwidth = 500, chain_min_score = 40, chain_max_chains = 4;
    const char* chain_option_given = nullptr; // the first --chain-* option seen
    int32_t query_host = 10, query_device = 5, target_host = 10, target_device = 5;
    bool query_host_set = false, query_device_set = false, target_host_set = false, target_device_set = false;
    const struct option options[] = {
        {"kmer-size", required_argument, 0, 'k'},
        {"window-size", required_argument, 0, 'w'},
        {"num-devices", required_argument, 0, 'd'},
        {"max-cached-memory", required_argument, 0, 'm'},
        {"index-size", required_argument, 0, 'i'},
        {"target-index-size", required_argument, 0, 't'},
        {"filtering-parameter", required_argument, 0, 'F'},
        {"alignment-engines", required_argument, 0, 'a'},
        {"min-residues", required_argument, 0, 'r'},
        {"min-overlap-length", required_argument, 0, 'l'},
        {"min-bases-per-residue", required_argument, 0, 'b'},
        {"min-overlap-fraction", required_argument, 0, 'z'},
        {"rescue-overlap-ends", no_argument, 0, 'R'},
        {"drop-fused-overlaps", no_argument, 0, 'D'},
        {"cigar", no_argument, &cigar, 1},
        {"chain", no_argument, &chain, 1},
        {"chain-max-gap", required_argument, 0, 1001},
        {"chain-bandwidth", required_argument, 0, 1002},
        {"chain-min-score", required_argument, 0, 1003},
        {"chain-max-chains", required_argument, 0, 1004},
        {"query-indices-in-host-memory", required_argument, 0, 'Q'},
        {"query-indices-in-device-memory", required_argument, 0, 'q'},
        {"target-indices-in-host-memory", required_argument, 0, 'C'},
        {"target-indices-in-device-memory", required_argument, 0, 'c'},
        {"version", no_argument, 0, 'v'},
        {"help", no_argument, 0, 'h'},
        {0, 0, 0, 0},
    };
    try
    {
        int c = 0;
        while ((c = getopt_long(argc, argv, "k:w:d:m:i:t:F:a:r:l:b:z:RDQ:q:C:c:BSvh", options, nullptr)) != -1)
        {
            switch (c)
            {
            case 'k': k = std::stoi(optarg); break;
            case 'w': w = std::stoi(optarg); break;
            case 'i': index_size = std::stod(optarg); break;
            case 't': target_index_size = std::stod(optarg); break;
            case 'F':
                filtering_parameter = std::stod(optarg);
                custom_filter       = true;
                break;
            case 'r': min_residues = std::stoi(optarg); break;
            case 'l': min_overlap_len = std::stoi(optarg); break;
            case 'b': min_bases_per_residue = std::stoi(optarg); break;
            case 'z': min_overlap_fraction = std::stof(optarg); break;
            case 'R': rescue = true; break;
            case 'D': drop = true; break;
            case 0: break; // --cigar, --chain: the flag is set by getopt_long
            case 1001:
                chain_max_gap      = std::stoi(optarg);
                chain_option_given = "--chain-max-gap";
                break;
            case 1002:
                chain_bandwidth    = std::stoi(optarg);
                chain_option_given = "--chain-bandwidth";
                break;
            case 1003:
                chain_min_score    = std::stoi(optarg);
                chain_option_given = "--chain-min-score";
                break;
            case 1004:
                chain_max_chains   = std::stoi(optarg);
                chain_option_given = "--chain-max-chains";
                break;
            case 'd':
                if (std::stoi(optarg) != 1)
                    refuse("-d: this tool runs on one device");
                break;
            case 'a':
                refuse("-a is not part of this tool: fused records are appended after alignment in the reference, so "
                       "its CIGARs and overlaps disagree; run align_overlaps on this tool's PAF instead");
            case 'm': refuse("-m is not supported: there is no caching allocator to size");
            case 'Q':
                query_host     = std::stoi(optarg);
                query_host_set = true;
                break;
            case 'q':
                query_device     = std::stoi(optarg);
                query_device_set = true;
                break;
            case 'C':
                target_host     = std::stoi(optarg);
                target_host_set = true;
                break;
            case 'c':
                target_device     = std::stoi(optarg);
                target_device_set = true;
                break;
            case 'S':
            case 'B': refuse("-S / -B are not supported: the output is PAF");
            case 'v': std::cout << "cudamapper (genomeworks_amd, gfx950)" << std::endl; return 1;
            case 'h': help(stdout); return 1;
            default: return 1;
            }
        }
        if (k < 1 || k > 32)
            refuse("kmer of size " + std::to_string(k) + " is not allowed, maximum k = 32");
        if (w < 1)
            refuse("-w / --window-size must be at least 1");
        if (filtering_parameter > 1.0 || filtering_parameter < 0.0)
            refuse("-F / --filtering-parameter must be in range [0.0, 1.0]");
        if (index_size <= 0 || target_index_size <= 0)
            refuse("-i / -t must be positive");
        if (chain_option_given && !chain)
            refuse(std::string(chain_option_given) + " needs --chain");
        if (chain_max_gap < 1)
            refuse("--chain-max-gap must be at least 1");
        if (chain_bandwidth < 0)
            refuse("--chain-bandwidth must not be negative");
        if (chain_min_score < 0)
            refuse("--chain-min-score must not be negative");
        if (chain_max_chains < 1 || chain_max_chains > 64)
            refuse("--chain-max-chains must be in range [1, 64]");
        if (argc - optind < 2)
        {
            std::cerr << "Invalid inputs. Please refer to the help function." << std::endl;
            help(stderr);
            return 1;
        }
        if (query_host_set || query_device_set || target_host_set || target_device_set)
        {
            if (!target_host_set)
            {
                std::cerr << "-C / --target-indices-in-host-memory not set, using -Q / --query-indices-in-host-memory "
                             "value: "
                          << query_host << std::endl;
                target_host = query_host;
            }
            if (!target_device_set)
            {
                std::cerr << "-c / --target-indices-in-device-memory not set, using -q / "
                             "--query-indices-in-device-memory value: "
                          << query_device << std::endl;
                target_device = query_device;
            }
            if (query_host < 1 || query_device < 1 || target_host < 1 || target_device < 1)
                refuse("-Q / -q / -C / -c must be at least 1");
            if (target_host < target_device)
                refuse("-C / --target-indices-in-host-memory  has to be larger or equal than -c / "
                       "--target-indices-in-device-memory");
            if (query_host < query_device)
                refuse("-Q / --query-indices-in-host-memory  has to be larger or equal than -q / "
                       "--query-indices-in-device-memory");
        }
        else
            query_host = query_device = target_host = target_device = 1;
        const std::string query_path = argv[optind], target_path = argv[optind + 1];
        const bool all_to_all = query_path == target_path;
        if (is_gzip(query_path) || is_gzip(target_path))
            refuse("gzipped input is not supported");
        if (all_to_all && (query_host != target_host || query_device != target_device))
            refuse("the same file as query and target needs -C equal to -Q and -c equal to -q");
        if (all_to_all)
        {
            target_index_size = index_size;
            std::cerr << "NOTE - Since query and target files are same, activating all_to_all mode. Query index size "
                         "used for both files."
                      << std::endl;
        }
        const std::vector<FastaSequence> queries = read_fasta(query_path);
        const std::vector<FastaSequence> own_targets = all_to_all ? std::vector<FastaSequence>() : read_fasta(target_path);
        const std::vector<FastaSequence>& targets = all_to_all ? queries : own_targets;

        // the frequency filter is off for less than 0.5 Mbp of input unless -F was given
        int64_t total = 0, short_reads = 0;
        for (const std::vector<FastaSequence>* set : {&queries, &own_targets})
            for (const FastaSequence& r : *set)
            {
                total += static_cast<int64_t>(r.seq.size());
                short_reads += static_cast<int64_t>(r.seq.size()) < static_cast<int64_t>(k) + w - 1 ? 1 : 0;
            }
        if (total < 500000 && !custom_filter)
            filtering_parameter = 1.0;
        if (short_reads > 0 && !cigar) // with --cigar the library refuses them, and says why
            std::cerr << "WARNING: " << short_reads << " reads are shorter than k + w - 1 = " << (k + w - 1)
                      << " bases; they are skipped and the read ids behind them in their index shift" << std::endl;

        const packed_reads q(queries);
        const packed_reads t(own_targets);
        const char* target_bases      = all_to_all ? nullptr : t.bases.data();
        const int64_t* target_offsets = all_to_all ? nullptr : t.offsets.data();
        const int64_t query_limit     = static_cast<int64_t>(index_size * 1000000.0);
        const int64_t target_limit    = static_cast<int64_t>(target_index_size * 1000000.0);
        gw_mapper_overlaps* result =
            chain ? gw_mapper_map_batched_chained(
                        q.bases.data(), q.offsets.data(), static_cast<int32_t>(queries.size()), target_bases,
                        target_offsets, static_cast<int32_t>(own_targets.size()), k, w, filtering_parameter,
                        min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction, query_limit,
                        target_limit, 1, drop ? 1 : 0, rescue ? 1 : 0, cigar, 0, query_host, query_device, target_host,
                        target_device, chain_max_gap, chain_bandwidth, chain_min_score, chain_max_chains, nullptr)
                  : gw_mapper_map_batched_cached(
                        q.bases.data(), q.offsets.data(), static_cast<int32_t>(queries.size()), target_bases,
                        target_offsets, static_cast<int32_t>(own_targets.size()), k, w, filtering_parameter,
                        min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction, query_limit,
                        target_limit, 1, drop ? 1 : 0, rescue ? 1 : 0, cigar, 0, query_host, query_device, target_host,
                        target_device, nullptr);
        if (!result)
            refuse(gw_mapper_last_error());
        std::vector<overlap_record> records(static_cast<size_t>(gw_mapper_overlaps_count(result)));
        gw_mapper_overlaps_copy(result, records.data(), static_cast<int64_t>(records.size()), nullptr, nullptr);
        std::vector<std::string> cigars;
        if (cigar)
        {
            std::string text(static_cast<size_t>(gw_mapper_overlaps_cigar_text_bytes(result)), '\0');
            std::vector<int64_t> offsets(records.size() + 1, 0);
            gw_mapper_overlaps_copy_cigars(result, &text[0], offsets.data(), nullptr, nullptr);
            for (size_t i = 0; i < records.size(); ++i)
                cigars.push_back(text.substr(static_cast<size_t>(offsets[i]), static_cast<size_t>(offsets[i + 1] - offsets[i])));
        }
        gw_mapper_overlaps_destroy(result);

        std::vector<Overlap> overlaps(records.size());
        for (size_t i = 0; i < records.size(); ++i)
        {
            const overlap_record& r = records[i];
            if (r.query_read_id >= queries.size() || r.target_read_id >= targets.size())
                refuse("an overlap names a read outside the input");
            Overlap& o                       = overlaps[i];
            o.query_read_id_                 = r.query_read_id;
            o.target_read_id_                = r.target_read_id;
            o.query_start_position_in_read_  = r.query_start_position_in_read;
            o.target_start_position_in_read_ = r.target_start_position_in_read;
            o.query_end_position_in_read_    = r.query_end_position_in_read;
            o.target_end_position_in_read_   = r.target_end_position_in_read;
            o.relative_strand                = static_cast<RelativeStrand>(r.relative_strand);
            o.num_residues_                  = r.num_residues;
            o.overlap_complete               = r.overlap_complete != 0;
        }
        print_paf(overlaps, cigars, queries, targets, k, stdout);
        return 0;
    }
    catch (const std::exception& e)
    {
        std::cerr << "cudamapper: " << e.what() << std::endl;
        return 1;
    }
}
