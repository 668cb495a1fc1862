// The public surface of the infix / prefix alignment types, as a caller's translation unit sees it: the enumerators,
// the factories that take them, the Alignment accessors and the C entry points. Compiled and linked by
// tests/test_semiglobal_interface.py; run without a GPU, it only checks what needs none.
#include <claraparabricks/genomeworks/cudaaligner/aligner.hpp>
#include <claraparabricks/genomeworks/cudaaligner/alignment.hpp>
#include <claraparabricks/genomeworks/cudaaligner/cudaaligner.hpp>

#include <gw_capi.h>
#include <gwhip_semiglobal.h>

#include <cstdio>
#include <memory>

using namespace claraparabricks::genomeworks;
using namespace claraparabricks::genomeworks::cudaaligner;

static_assert(AlignmentType::global_alignment == 0 && AlignmentType::unset == 1, "the reference's values stay");
static_assert(AlignmentType::infix_alignment == 2 && AlignmentType::prefix_alignment == 3, "the new types follow unset");

// a caller's own Alignment keeps compiling: the new accessors are not pure
struct WholeTarget : Alignment
{
    std::string q = "ACGT", t = "ACGGT";
    std::vector<AlignmentState> s;
    std::vector<int8_t> a;
    std::vector<int32_t> r;
    const std::string& get_query_sequence() const override { return q; }
    const std::string& get_target_sequence() const override { return t; }
    std::string convert_to_cigar(CigarFormat) const override { return ""; }
    AlignmentType get_alignment_type() const override { return AlignmentType::global_alignment; }
    bool is_optimal() const override { return true; }
    StatusType get_status() const override { return StatusType::success; }
    const std::vector<AlignmentState>& get_alignment() const override { return s; }
    const std::vector<int8_t>& get_actions() const override { return a; }
    const std::vector<int32_t>& get_runlengths() const override { return r; }
    int32_t get_edit_distance() const override { return 0; }
    FormattedAlignment format_alignment(int32_t) const override { return {}; }
};

int main(int argc, char** argv)
{
    WholeTarget w;
    if (w.get_target_begin() != 0 || w.get_target_end() != 5) return 1;
    // the addresses only: the linker must find every new entry point
    auto typed   = &gw_aligner_create_typed;
    auto range   = &gw_alignment_target_range;
    auto scan    = &gwhip_semiglobal_ends;
    auto gather  = &gwhip_semiglobal_gather;
    auto factory = static_cast<std::unique_ptr<Aligner> (*)(int32_t, int32_t, int32_t, AlignmentType, cudaStream_t, int32_t, int64_t)>(&create_aligner);
    if (!typed || !range || !scan || !gather || !factory) return 2;
    if (gwhip_semiglobal_workspace_bytes(4, 2048) != 256) return 3;                       // registers: no per-pair state
    if (gwhip_semiglobal_workspace_bytes(4, GWHIP_SEMIGLOBAL_REGISTER_QUERY + 1) <= 256) return 4;
    if (argc > 1 && argv[1][0] == 'g') // with a GPU: the factories themselves
    {
        auto infix = create_aligner(100, 300, 4, AlignmentType::infix_alignment, nullptr, 0, int64_t(1) << 30);
        if (infix->add_alignment("GAC", 3, "TTAC", 4) != StatusType::success) return 5;
        infix->align_all();
        infix->sync_alignments();
        const Alignment& al = *infix->get_alignments().at(0);
        if (al.get_alignment_type() != AlignmentType::infix_alignment || al.get_target_begin() != 2 || al.get_target_end() != 4) return 6;
        if (al.convert_to_cigar(CigarFormat::extended) != "1D2=" || al.format_alignment().target != "-AC") return 7;
        bool thrown = false;
        try
        {
            create_aligner(AlignmentType::prefix_alignment, 64, nullptr, 0, int64_t(1) << 30); // the FixedBandAligner overload
        }
        catch (const std::runtime_error&)
        {
            thrown = true;
        }
        if (!thrown) return 8;
    }
    std::puts("ok");
    return 0;
}
