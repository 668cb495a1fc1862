// gwm_pileup.hip -- cudamapper on gfx950: pileups, the per-base counts of aligned overlaps (include/gwhip_mapper.h,
// gwm_overlap_pileup and gwm_pair_pileup). A third consumer of the chunk loop of
// gwm_align_chunks.hpp: where gwm_align_overlaps turns the per-column states into text and gwm_window_segments into
// records, this adds them into six counters per base of the read that owns the position -- A, C, G, T, deletion,
// insertion -- and leaves the states where they are. Only the counters cross to the host.
//
// One wave64 per alignment over tiles of 64 columns in forward column order, by the walk of gwm_column_walk.hpp that
// the segment kernel shares, which gives every lane the query and target position of its column; the last column's
// state is carried between tiles in a wave-uniform register. A column that consumes a base of the owner issues one
// returnless atomic add on its cell; the first column of a run that consumes none issues one on the insertion cell of
// the owner base before the run. The supplier's base is read from the resident read set. No LDS, no scratch. Integer
// sums: the result depends neither on the order of the atomics nor on the chunking. The kernel and its launch are in
// gwm_pileup_kernel.hpp, which the variant caller (gwm_variants.hip) runs in its own chunk callback.
#include "gwm_pileup_kernel.hpp"

extern "C" {

void gwm_pileup_free(gwm_pileup* pileup)
{
    if (!pileup)
        return;
    (void)hipFree(pileup->counts);
    *pileup = gwm_pileup{};
}

int gwm_overlap_pileup(const gwm_overlap* overlaps, int64_t n, const char* query_bases, const int64_t* query_offsets,
                       int32_t n_queries, uint32_t first_query_read_id, const char* target_bases,
                       const int64_t* target_offsets, int32_t n_targets, uint32_t first_target_read_id,
                       int64_t max_device_bytes, void* stream, gwm_pileup* out)
{
    *out = gwm_pileup{};
    try
    {
        check_chunk_arguments("gwm_overlap_pileup", n_queries, n_targets, max_device_bytes, n);
        hipStream_t s = static_cast<hipStream_t>(stream);
        dbuf<uint32_t> counts;
        const int64_t n_bases = zeroed_counts(target_offsets, n_targets, s, counts);
        const ReadSet q = read_set(query_bases, query_offsets, n_queries, first_query_read_id);
        const ReadSet t = read_set(target_bases, target_offsets, n_targets, first_target_read_id);
        if (n > 0)
            gwm::align_chunks("gwm_overlap_pileup", overlaps, n, q, t, max_device_bytes, gwm::Scoring{}, s, out->stage_ms,
                              [&](const AlignedChunk& c) { add_role<false>(c, q, t, n_bases, counts.p, s); });
        GWM_CHECK(hipStreamSynchronize(s));
        out->n_bases = n_bases;
        out->counts  = counts.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        *out = gwm_pileup{};
        return -1;
    }
}

int gwm_pair_pileup(const gwm_overlap* pairs, int64_t n, const char* bases, const int64_t* offsets, int32_t n_reads,
                    uint32_t first_read_id, int64_t max_device_bytes, void* stream, gwm_pileup* out)
{
    *out = gwm_pileup{};
    try
    {
        check_chunk_arguments("gwm_pair_pileup", n_reads, n_reads, max_device_bytes, n);
        hipStream_t s = static_cast<hipStream_t>(stream);
        dbuf<uint32_t> counts;
        const int64_t n_bases = zeroed_counts(offsets, n_reads, s, counts);
        const ReadSet r = read_set(bases, offsets, n_reads, first_read_id);
        if (n > 0)
            gwm::align_chunks("gwm_pair_pileup", pairs, n, r, r, max_device_bytes, gwm::Scoring{}, s, out->stage_ms,
                              [&](const AlignedChunk& c) {
                                  add_role<false>(c, r, r, n_bases, counts.p, s);
                                  add_role<true>(c, r, r, n_bases, counts.p, s);
                              });
        GWM_CHECK(hipStreamSynchronize(s));
        out->n_bases = n_bases;
        out->counts  = counts.release();
        return 0;
    }
    catch (const std::exception& e)
    {
        gwm_set_error(e.what());
        *out = gwm_pileup{};
        return -1;
    }
}

} // extern "C"
