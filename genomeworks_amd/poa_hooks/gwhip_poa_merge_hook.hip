// gwhip_poa_merge_hook.hip -- TEST-ONLY: the merge every production window runs (add_alignment_parallel,
// csrc/poa_graph_device.h) on caller-provided arrays, next to gwhip_poa_test_add_alignment (libgwhip.so), which runs the
// serial add_alignment_to_graph. The reference's known-answer vectors of addAlignment (cudapoa_add_alignment.cuh:335) reach
// the shipped merge through it. A library of its own (libgwhip_poa_hooks.so), see include/gwhip_poa_hooks.h.
#include <hip/hip_runtime.h>

#include "gwhip_poa_hooks.h"

#include "../csrc/poa_device.h"
#include "../csrc/poa_graph_device.h"

namespace gwhip
{

// One wavefront. NodeT = int32_t is the instantiation of the graphs beyond the LDS tables, whose scratch lies in the score
// matrix; NodeT = int16_t is the scratch type of the LDS-table kernels. Here the scratch (gnode and curr, read_length entries
// each rounded up to 64, then one bit per node) is the caller's buffer either way.
template <typename NodeT>
__global__ __launch_bounds__(kWave) void add_alignment_parallel_hook_kernel(GraphView<int32_t> g, int32_t* node_count, int32_t alignment_length,
                                                                            const int32_t* alignment_graph, const uint8_t* read,
                                                                            const int32_t* alignment_read, const int8_t* base_weights,
                                                                            int32_t read_length, int32_t max_nodes_per_graph, void* scratch,
                                                                            int32_t* rc)
{
    const int lane       = threadIdx.x;
    const int32_t count  = *node_count;
    const int32_t lpad   = (read_length + 63) & ~63;
    NodeT* gnode         = reinterpret_cast<NodeT*>(scratch);
    NodeT* curr          = gnode + lpad;
    uint32_t* onpath     = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(scratch) + gw_align_up(2 * (size_t)lpad * sizeof(NodeT), 16));
    int32_t new_count    = 0;
    const int32_t par_rc = add_alignment_parallel<int32_t, false, NodeT>(new_count, g, count, alignment_length, alignment_graph, alignment_read,
                                                                         read, base_weights, read_length, nullptr, 0, 0, max_nodes_per_graph,
                                                                         gnode, curr, onpath, lane);
    wave_sync();
    if (lane == 0)
    {
        *rc = par_rc;
        if (par_rc == 0) *node_count = new_count;
    }
}

} // namespace gwhip

using namespace gwhip;

extern "C" {

size_t gwhip_poa_test_add_alignment_parallel_scratch_bytes(int32_t read_length, int32_t max_nodes_per_graph, int32_t scratch16)
{
    const size_t lpad = ((size_t)read_length + 63) & ~size_t(63);
    return gw_align_up(2 * lpad * (scratch16 ? sizeof(int16_t) : sizeof(int32_t)), 16) + (((size_t)max_nodes_per_graph + 31) / 32) * 4;
}

int gwhip_poa_test_add_alignment_parallel(uint8_t* nodes, int32_t* node_count, int32_t* node_alignments,
                                          uint16_t* node_alignment_count, int32_t* incoming_edges,
                                          uint16_t* incoming_edge_count, int32_t* outgoing_edges,
                                          uint16_t* outgoing_edge_count, uint16_t* incoming_edge_w, int32_t alignment_length,
                                          const int32_t* alignment_graph, const uint8_t* read, const int32_t* alignment_read,
                                          uint16_t* node_coverage_counts, const int8_t* base_weights, int32_t read_length,
                                          int32_t max_nodes_per_graph, int32_t scratch16, void* scratch, int32_t* rc,
                                          void* stream)
{
    if (read_length < 1 || alignment_length < 1 || max_nodes_per_graph < 1 || (scratch16 && max_nodes_per_graph > 32767))
        return (int)hipErrorInvalidValue;
    GraphView<int32_t> g{};
    g.nodes                = nodes;
    g.node_alignments      = node_alignments;
    g.node_alignment_count = node_alignment_count;
    g.incoming_edges       = incoming_edges;
    g.incoming_edge_count  = incoming_edge_count;
    g.outgoing_edges       = outgoing_edges;
    g.outgoing_edge_count  = outgoing_edge_count;
    g.incoming_edge_w      = incoming_edge_w;
    g.coverage             = node_coverage_counts;
    if (scratch16)
        hipLaunchKernelGGL(add_alignment_parallel_hook_kernel<int16_t>, dim3(1), dim3(kWave), 0, (hipStream_t)stream, g, node_count,
                           alignment_length, alignment_graph, read, alignment_read, base_weights, read_length, max_nodes_per_graph, scratch, rc);
    else
        hipLaunchKernelGGL(add_alignment_parallel_hook_kernel<int32_t>, dim3(1), dim3(kWave), 0, (hipStream_t)stream, g, node_count,
                           alignment_length, alignment_graph, read, alignment_read, base_weights, read_length, max_nodes_per_graph, scratch, rc);
    return (int)hipGetLastError();
}

} // extern "C"
