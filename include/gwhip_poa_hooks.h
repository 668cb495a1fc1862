/* gwhip_poa_hooks.h -- C ABI of libgwhip_poa_hooks.so: TEST-ONLY entry points next to the gwhip_poa_test_* hooks of gwhip.h,
 * built as a library of its own (genomeworks_amd/poa_hooks/) so that the stamped kernel source set of libgwhip.so
 * (genomeworks_amd.build.kernel_source_digest) does not change with a test hook. Same conventions as the unit hooks of
 * gwhip.h: device pointers, the reference's array layout with SizeT = int32, 50 slots per node. */
#ifndef GWHIP_POA_HOOKS_H
#define GWHIP_POA_HOOKS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The merge every window kernel runs (add_alignment_parallel, csrc/poa_graph_device.h) on one wavefront, on the arrays
   gwhip_poa_test_add_alignment (the serial addAlignmentToGraph) takes. The alignment is laid out as the
   traceback writes it: entry alignment_length - 1 holds read position 0 and entry 0 the last read position, so that the serial
   routine's walk from the last entry down meets the read front to back.
   scratch16 != 0: 16-bit scratch entries (the type of the LDS-table kernels; max_nodes_per_graph <= 32767), else 32-bit entries
   (the instantiation of the graphs beyond the LDS tables). scratch: gwhip_poa_test_add_alignment_parallel_scratch_bytes()
   device bytes, 16-byte aligned. *rc (device int32) gets the merge's return value as it is: 0 (and *node_count is updated), a
   StatusType, or -1 = "nothing was modified, the serial routine has to take this read".
   Returns 0, or the hipError_t of the launch (hipErrorInvalidValue for ids that do not fit 16-bit scratch). */
size_t gwhip_poa_test_add_alignment_parallel_scratch_bytes(int32_t read_length, int32_t max_nodes_per_graph, int32_t scratch16);
int gwhip_poa_test_add_alignment_parallel(uint8_t* nodes, int32_t* node_count, int32_t* node_alignments,
                                          uint16_t* node_alignment_count, int32_t* incoming_edges,
                                          uint16_t* incoming_edge_count, int32_t* outgoing_edges,
                                          uint16_t* outgoing_edge_count, uint16_t* incoming_edge_w, int32_t alignment_length,
                                          const int32_t* alignment_graph, const uint8_t* read, const int32_t* alignment_read,
                                          uint16_t* node_coverage_counts, const int8_t* base_weights, int32_t read_length,
                                          int32_t max_nodes_per_graph, int32_t scratch16, void* scratch, int32_t* rc,
                                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
