// What the kernels over a PatchGraph's edge array share (graph_apply.hip, graph_attend.hip): the edges are cut into segments of GA_SEG,
// a block each, and the row of an edge comes out of a bounded search over the offsets.
#pragma once
#include <cstdint>

namespace dagl {

constexpr int GA_SEG = 128;                   // edges per block: dagl_graph_apply_segment()

// the row that holds edge p: the largest r in [0, n_rows) with row_off[r] <= p (empty rows share an offset with their successor)
__device__ __forceinline__ int ga_row_of(const int64_t* __restrict__ row_off, int n_rows, long long p) {
    int lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (row_off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace dagl
