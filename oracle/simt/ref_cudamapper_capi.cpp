// ref_cudamapper_capi.cpp -- TEST INFRASTRUCTURE (oracle/simt): a flat C interface over the REFERENCE's cudamapper classes -- its own
// minimizer.cu, index_gpu.cu / index_gpu.cuh, matcher_gpu.cu and overlapper_triggered.cu compiled by g++ from the reference checkout (REF of oracle/Makefile.ref) where
// they lie and run on the CPU by the SIMT emulator of simt.hpp (oracle/Makefile.ref, target ref_cudamapper_simt ->
// oracle/_ref/libref_cudamapper_simt.so). This file only calls the reference's classes: IndexGPU<Minimizer> over an in-memory
// io::FastaParser, MatcherGPU over two Index objects, OverlapperTriggered::get_overlaps over a device_buffer<Anchor>.
// Used by tests/ref_cudamapper.py to check tests/oracle_mapper.c and to write tests/golden/cudamapper_reference_simt.npz.
#include <claraparabricks/genomeworks/cudamapper/index.hpp>
#include <claraparabricks/genomeworks/cudamapper/types.hpp>
#include <claraparabricks/genomeworks/io/fasta_parser.hpp>
#include <claraparabricks/genomeworks/utils/allocator.hpp>
#include <claraparabricks/genomeworks/utils/device_buffer.hpp>

#include "index_gpu.cuh"
#include "matcher_gpu.cuh"
#include "minimizer.hpp"
#include "overlapper_triggered.hpp"

#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudamapper;

namespace
{
/// reads held in memory; read id `first_read_id + i` is the i-th of them
class MemoryParser : public io::FastaParser
{
public:
    MemoryParser(const char* bases, const int64_t* offsets, int n_reads, read_id_t first_read_id)
        : first_(first_read_id)
    {
        for (int i = 0; i < n_reads; ++i)
            reads_.push_back(io::FastaSequence{"read_" + std::to_string(first_read_id + i), std::string(bases + offsets[i], bases + offsets[i + 1])});
    }
    number_of_reads_t get_num_seqences() const override { return static_cast<number_of_reads_t>(first_ + reads_.size()); }
    const io::FastaSequence& get_sequence_by_id(read_id_t id) const override { return reads_.at(id - first_); }

private:
    read_id_t first_;
    std::vector<io::FastaSequence> reads_;
};

/// an Index over arrays handed in (what a test stored of an earlier rcm_index_create, or built by hand)
class ArrayIndex : public Index
{
public:
    ArrayIndex(DefaultDeviceAllocator allocator, int64_t n, const uint64_t* rep, const uint32_t* rid, const uint32_t* pos, const uint8_t* dir,
               int64_t n_unique, const uint64_t* unique, const uint32_t* first, int64_t n_first, read_id_t number_of_reads,
               read_id_t smallest, read_id_t largest, position_in_read_t longest)
        : rep_(n, allocator), rid_(n, allocator), pos_(n, allocator), dir_(n, allocator), unique_(n_unique, allocator), first_(n_first, allocator)
        , number_of_reads_(number_of_reads), smallest_(smallest), largest_(largest), longest_(longest)
    {
        std::memcpy(rep_.data(), rep, sizeof(uint64_t) * n);
        std::memcpy(rid_.data(), rid, sizeof(uint32_t) * n);
        std::memcpy(pos_.data(), pos, sizeof(uint32_t) * n);
        for (int64_t i = 0; i < n; ++i) dir_.data()[i] = static_cast<SketchElement::DirectionOfRepresentation>(dir[i]);
        std::memcpy(unique_.data(), unique, sizeof(uint64_t) * n_unique);
        std::memcpy(first_.data(), first, sizeof(uint32_t) * n_first);
    }
    const device_buffer<representation_t>& representations() const override { return rep_; }
    const device_buffer<read_id_t>& read_ids() const override { return rid_; }
    const device_buffer<position_in_read_t>& positions_in_reads() const override { return pos_; }
    const device_buffer<SketchElement::DirectionOfRepresentation>& directions_of_reads() const override { return dir_; }
    const device_buffer<representation_t>& unique_representations() const override { return unique_; }
    const device_buffer<std::uint32_t>& first_occurrence_of_representations() const override { return first_; }
    read_id_t number_of_reads() const override { return number_of_reads_; }
    read_id_t smallest_read_id() const override { return smallest_; }
    read_id_t largest_read_id() const override { return largest_; }
    position_in_read_t number_of_basepairs_in_longest_read() const override { return longest_; }
    bool is_ready() const override { return true; }
    void wait_to_be_ready() override {}

private:
    device_buffer<representation_t> rep_;
    device_buffer<read_id_t> rid_;
    device_buffer<position_in_read_t> pos_;
    device_buffer<SketchElement::DirectionOfRepresentation> dir_;
    device_buffer<representation_t> unique_;
    device_buffer<std::uint32_t> first_;
    read_id_t number_of_reads_, smallest_, largest_;
    position_in_read_t longest_;
};

struct RefIndex
{
    std::unique_ptr<Index> index;
};
struct RefAnchors
{
    std::vector<Anchor> anchors;
};
} // namespace

static_assert(sizeof(Anchor) == 16, "tests/oracle_mapper.py ANCHOR");
static_assert(sizeof(Overlap) == 36 && offsetof(Overlap, relative_strand) == 24 && offsetof(Overlap, num_residues_) == 28 &&
                  offsetof(Overlap, overlap_complete) == 32,
              "tests/oracle_mapper.py OVERLAP");

#pragma GCC visibility push(default)
extern "C" {

// IndexGPU<Minimizer>(allocator, parser, IndexDescriptor(first_read_id, n_reads), k, w, hash, filtering_parameter) over the n_reads reads
// bases[offsets[i] .. offsets[i + 1]); null when the reference threw
void* rcm_index_create(const char* bases, const int64_t* offsets, int n_reads, unsigned first_read_id, int k, int w, int hash_representations,
                       double filtering_parameter)
{
    try
    {
        MemoryParser parser(bases, offsets, n_reads, first_read_id);
        DefaultDeviceAllocator allocator = create_default_device_allocator(int64_t(256) << 20);
        auto h                           = std::make_unique<RefIndex>();
        h->index = std::make_unique<IndexGPU<Minimizer>>(allocator, parser, IndexDescriptor(first_read_id, n_reads), k, w, hash_representations != 0,
                                                         filtering_parameter);
        h->index->wait_to_be_ready();
        return h.release();
    }
    catch (...)
    {
        return nullptr;
    }
}

void* rcm_index_from_arrays(long long n, const uint64_t* rep, const uint32_t* rid, const uint32_t* pos, const uint8_t* dir, long long n_unique,
                            const uint64_t* unique, const uint32_t* first, long long n_first, unsigned number_of_reads, unsigned smallest,
                            unsigned largest, unsigned longest)
{
    try
    {
        DefaultDeviceAllocator allocator = create_default_device_allocator(int64_t(256) << 20);
        auto h                           = std::make_unique<RefIndex>();
        h->index = std::make_unique<ArrayIndex>(allocator, n, rep, rid, pos, dir, n_unique, unique, first, n_first, number_of_reads, smallest, largest, longest);
        return h.release();
    }
    catch (...)
    {
        return nullptr;
    }
}

void rcm_index_destroy(void* h) { delete static_cast<RefIndex*>(h); }

// sizes[0..2] = elements, unique representations, entries of first_occurrence_of_representations;
// scalars[0..3] = number_of_reads, smallest_read_id, largest_read_id, number_of_basepairs_in_longest_read
void rcm_index_sizes(void* h, long long* sizes, unsigned* scalars)
{
    const Index& ix = *static_cast<RefIndex*>(h)->index;
    sizes[0]        = ix.representations().size();
    sizes[1]        = ix.unique_representations().size();
    sizes[2]        = ix.first_occurrence_of_representations().size();
    scalars[0]      = ix.number_of_reads();
    scalars[1]      = ix.smallest_read_id();
    scalars[2]      = ix.largest_read_id();
    scalars[3]      = ix.number_of_basepairs_in_longest_read();
}

void rcm_index_arrays(void* h, uint64_t* rep, uint32_t* rid, uint32_t* pos, uint8_t* dir, uint64_t* unique, uint32_t* first)
{
    const Index& ix = *static_cast<RefIndex*>(h)->index;
    const auto n    = ix.representations().size();
    std::memcpy(rep, ix.representations().data(), sizeof(uint64_t) * n);
    std::memcpy(rid, ix.read_ids().data(), sizeof(uint32_t) * n);
    std::memcpy(pos, ix.positions_in_reads().data(), sizeof(uint32_t) * n);
    for (std::ptrdiff_t i = 0; i < n; ++i) dir[i] = static_cast<uint8_t>(ix.directions_of_reads().data()[i]);
    std::memcpy(unique, ix.unique_representations().data(), sizeof(uint64_t) * ix.unique_representations().size());
    std::memcpy(first, ix.first_occurrence_of_representations().data(), sizeof(uint32_t) * ix.first_occurrence_of_representations().size());
}

// MatcherGPU(allocator, query, target).anchors(); null when the reference threw
void* rcm_anchors_create(void* query, void* target)
{
    try
    {
        DefaultDeviceAllocator allocator = create_default_device_allocator(int64_t(256) << 20);
        MatcherGPU matcher(allocator, *static_cast<RefIndex*>(query)->index, *static_cast<RefIndex*>(target)->index);
        auto h = std::make_unique<RefAnchors>();
        h->anchors.assign(matcher.anchors().data(), matcher.anchors().data() + matcher.anchors().size());
        return h.release();
    }
    catch (...)
    {
        return nullptr;
    }
}
long long rcm_anchors_size(void* h) { return static_cast<long long>(static_cast<RefAnchors*>(h)->anchors.size()); }
void rcm_anchors_copy(void* h, void* out)
{
    const auto& a = static_cast<RefAnchors*>(h)->anchors;
    if (!a.empty()) std::memcpy(out, a.data(), sizeof(Anchor) * a.size());
}
void rcm_anchors_destroy(void* h) { delete static_cast<RefAnchors*>(h); }

// OverlapperTriggered(allocator).get_overlaps(...) on `n` sorted anchors; `out` holds n records; -1 when the reference threw
long long rcm_overlaps(const void* anchors, long long n, int all_to_all, long long min_residues, long long min_overlap_len,
                       long long min_bases_per_residue, float min_overlap_fraction, void* out)
{
    try
    {
        DefaultDeviceAllocator allocator = create_default_device_allocator(int64_t(256) << 20);
        device_buffer<Anchor> anchors_d(n, allocator);
        if (n > 0) std::memcpy(anchors_d.data(), anchors, sizeof(Anchor) * n);
        OverlapperTriggered overlapper(allocator);
        std::vector<Overlap> overlaps;
        overlapper.get_overlaps(overlaps, anchors_d, all_to_all != 0, min_residues, min_overlap_len, min_bases_per_residue, min_overlap_fraction);
        if (!overlaps.empty()) std::memcpy(out, overlaps.data(), sizeof(Overlap) * overlaps.size());
        return static_cast<long long>(overlaps.size());
    }
    catch (...)
    {
        return -1;
    }
}
}
#pragma GCC visibility pop
