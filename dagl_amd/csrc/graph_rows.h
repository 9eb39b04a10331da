// What the kernels over a PatchGraph's edge array share (graph_apply.hip, graph_attend.hip, graph_forward.hip): the edges are cut into
// segments of GA_SEG, a block each, and the row of an edge comes out of a bounded search over the offsets; the source row of an edge in
// the value map and the gather of a run of edges (the apply side); the logit of an edge and the dot product's pieces (the attend side).
#pragma once
#include <cstdint>
#include "dagl_common.h"

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

// ---- the apply side ---------------------------------------------------------------------------------------------------------------
constexpr int GA_BATCH = 8;                   // gathers in flight per thread
constexpr int GA_C4 = P / 4;                  // 196 float4 per patch row

struct GaArgs {
    const int64_t* row_off; int n_rows;       // CSR (or transposed CSR) offsets [n_rows + 1]
    const int32_t* key; const float* weight; const int32_t* perm /* NULL: weight[e] */;
    long long E;
    const float* src; int n_src;              // MAP: the padded map, n_src = N;  !MAP: [n_src, 784]
    int L, W, Wp; long long img4;             // MAP: rows per image, map geometry, float4 per image
    float* out;                               // [n_rows, 784]
    float* part;                              // [chunks, 784]
};

// float4 offset of an edge's source row, -1 = the edge contributes nothing
template <bool MAP>
__device__ __forceinline__ long long ga_source(const GaArgs& a, int row, int key) {
    if ((unsigned)key >= (unsigned)a.n_src) return -1;
    if (!MAP) return (long long)key * GA_C4;
    const int b = row / a.L;
    const int jy = key / a.W, jx = key - jy * a.W;
    return (long long)b * a.img4 + ((long long)jy * a.Wp + jx) * (CH / 4);
}

// the weighted sum of a run of edges [e, end) of the staged segment (sh_of: float4 offset of the source row or -1, sh_w: weight), the
// calling thread's float4 column of it: `src` points at that column of source row 0.  GA_BATCH gathers in flight, edge order.
// (graph_apply_segment_kernel keeps this loop in its own body: called from here the compiler allocates its registers in another order,
// and that kernel's device code is pinned.)
__device__ __forceinline__ float4 ga_gather_run(const float4* src, const long long* sh_of, const float* sh_w, int e, int end) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = e; j < end; j += GA_BATCH) {
        float w[GA_BATCH]; float4 v[GA_BATCH]; bool live[GA_BATCH];
#pragma unroll
        for (int u = 0; u < GA_BATCH; ++u) {
            const int i = min(j + u, end - 1);
            const long long of = sh_of[i];
            live[u] = j + u < end && of >= 0;
            v[u] = src[of >= 0 ? of : 0];
            w[u] = sh_w[i];
        }
#pragma unroll
        for (int u = 0; u < GA_BATCH; ++u) {
            acc.x = live[u] ? fmaf(w[u], v[u].x, acc.x) : acc.x; acc.y = live[u] ? fmaf(w[u], v[u].y, acc.y) : acc.y;
            acc.z = live[u] ? fmaf(w[u], v[u].z, acc.z) : acc.z; acc.w = live[u] ? fmaf(w[u], v[u].w, acc.w) : acc.w;
        }
    }
    return acc;
}

// ---- the attend side --------------------------------------------------------------------------------------------------------------
constexpr int GT_C4 = D / 4;                  // 49 float4 per feature row

struct GtArgs {
    const int64_t* row_off; int n_rows;       // CSR offsets [B L + 1]
    const int32_t* key; long long E;
    const float* wq; const float* x;          // [B L, 196], [B N, 196]
    const float* tau;                         // [B L] or NULL (no margin)
    int L, N; float scale; int edges_only;
};

// logit of a score; m = the margin (1 without tau): the edge is "on" iff m != 0.  The products are rounded one by one (no contraction
// into the caller's z - M): every kernel must see the bits the row maximum was taken from, or the heaviest edge of a one-hot row weighs
// e^(rounding residue) instead of 1 and the backward's g_e - c_r no longer cancels
__device__ __forceinline__ float gt_logit(const GtArgs& a, int row, float s, float& m) {
#pragma clang fp contract(off)
    m = 1.f;
    if (a.tau != nullptr) {
        const float d = s - a.tau[row];
        m = d > 0.f ? d : 0.f;
    }
    return a.scale * s * m;
}

__device__ __forceinline__ float gt_dot4(const float4 p, const float4 q) { return p.x * q.x + p.y * q.y + p.z * q.z + p.w * q.w; }

// <q, k> of two 196-float rows by the 16 lanes of an edge's group: lane l reads float4 l, l + 16, l + 32 and (lane 0) 48 of both rows,
// then a fixed 4-step reduction; every lane of the group returns the sum
__device__ __forceinline__ float gt_edge_dot(const float4* __restrict__ q, const float4* __restrict__ k, int l) {
    const bool tail = l + 48 < GT_C4;
    const int c3 = tail ? l + 48 : GT_C4 - 1;
    const float4 q0 = q[l], q1 = q[l + 16], q2 = q[l + 32], q3 = q[c3];
    const float4 k0 = k[l], k1 = k[l + 16], k2 = k[l + 32], k3 = k[c3];
    float acc = gt_dot4(q0, k0);
    acc += gt_dot4(q1, k1);
    acc += gt_dot4(q2, k2);
    acc += tail ? gt_dot4(q3, k3) : 0.f;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
    return acc;
}

__device__ __forceinline__ long long gt_clamp(long long v, long long E) { return v < 0 ? 0 : (v > E ? E : v); }

}  // namespace dagl
