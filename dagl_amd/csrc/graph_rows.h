// What the routes over a PatchGraph's edge array share (graph_apply.hip, graph_attend.hip, graph_forward.hip, graph_refresh.hip,
// graph_lists.hip; each keeps its kernels, its launches and its C entries in its own file).
//   device  the edges are cut into segments of GA_SEG, a block each, and the row of an edge comes out of a bounded search over the
//           offsets; the source row of an edge in the value map and the gather of a run of edges (the apply side); the logit of an
//           edge, the dot product's pieces, the feature row of a key and the statistics of a run (the attend side).
//   host    the checks every entry makes of its shape and operands, the call and argument structs and how they are filled.
// Kernels that keep a shared loop in their own body, because called from here the compiler allocates registers in another order and their
// device code is pinned (tools/same_device_code.sh): graph_apply_segment_kernel its gather loop (ga_gather_run),
// graph_apply_combine_kernel its two clamps (gt_clamp).  Everything else calls the helpers below.
// Left written out on purpose: rf_max / rf_sum / rf_scan of graph_refresh.hip (templated on the block size, and they add the waves'
// partials one after the other where block_sum_f64 adds (w0 + w1) + (w2 + w3): other bits); rf_ord (a total order for the rank cut,
// no other route ranks); graph_attend_rows_kernel next to graph_forward_combine_kernel (the second fuses the sum into its scaling loop);
// graph_forward.hip's training kernels next to their models -- graph_forward_row_stats_kernel (the combine kernel's (M, D) into arrays
// of their own), graph_forward_bwd_rows_kernel (graph_attend_bwd_rows_kernel), graph_forward_bwd_combine_kernel
// (graph_attend_combine_kernel at either width): a __global__ lives in one translation unit, and graph_attend.hip's are pinned.
#pragma once
#include <cstdint>
#include "dagl_common.h"

namespace dagl {

constexpr int GA_SEG = 128;                   // edges per block: dagl_graph_apply_segment()

// the segment of the calling block: its first edge and how many it holds (GA_SEG but for the last block)
struct GaSegment { long long p0; int m; };
__device__ __forceinline__ GaSegment ga_segment(long long E) {
    const long long p0 = (long long)blockIdx.x * GA_SEG;
    return {p0, (int)((E - p0 < GA_SEG) ? E - p0 : GA_SEG)};
}

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
// (graph_forward_segment_kernel and graph_attend_product_kernel call it; graph_apply_segment_kernel keeps the loop in its own body: above.)
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

// float4 offset of key's feature row in [B N, 196] as query row `row` of [B L] sees it, -1 = key outside [0, N)
__device__ __forceinline__ long long gt_feature_row(int L, int N, int row, int key) {
    return (unsigned)key < (unsigned)N ? ((long long)(row / L) * N + key) * GT_C4 : -1;
}

// the statistics of a segment's runs: a slot per row and per segment (the run that came in from an earlier segment leaves the segment's)
struct GfStats { float* row_max; double* row_sum; float* chunk_max; double* chunk_sum; };

// one (max, sum e^(z - max)) per run of equal row of the staged segment (m edges from p0: sh_row, sh_z), by the thread of the run's
// first edge, in edge order.  KEEP: e^(z - max) of every edge stays in sh_w
template <bool KEEP>
__device__ __forceinline__ void gt_run_stats(const GtArgs& a, long long p0, int m, const int* sh_row, const float* sh_z, float* sh_w,
                                             const GfStats& st) {
    const int t = threadIdx.x;
    if (t < m && (t == 0 || sh_row[t - 1] != sh_row[t])) {
        const int row = sh_row[t];
        int end = t + 1;
        while (end < m && sh_row[end] == row) ++end;
        float mx = sh_z[t];
        for (int j = t + 1; j < end; ++j) mx = fmaxf(mx, sh_z[j]);
        double sum = 0.0;
        for (int j = t; j < end; ++j) {
            const float p = expf(sh_z[j] - mx);
            sum += (double)p;
            if (KEEP) sh_w[j] = p;
        }
        if (a.row_off[row] < p0) { st.chunk_max[blockIdx.x] = mx; st.chunk_sum[blockIdx.x] = sum; }
        else { st.row_max[row] = mx; st.row_sum[row] = sum; }
    }
}

// ---- host: what the entries share --------------------------------------------------------------------------------------------------
static inline size_t ga_chunks(int64_t E) { return (size_t)((E + GA_SEG - 1) / GA_SEG); }

static inline GfStats carve_stats(Carver& cv, size_t rows, size_t chunks) {
    GfStats st;
    st.row_max = cv.take<float>(rows);
    st.row_sum = cv.take<double>(rows);
    st.chunk_max = cv.take<float>(chunks);
    st.chunk_sum = cv.take<double>(chunks);
    return st;
}

// the checks of a graph call, in the order every entry makes them; 0 = passed (dagl_last_error says why not)
static inline int graph_dims_ok(const char* who, int B, int H, int W) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    DAGL_REQUIRE((int64_t)B * H * W < (1ll << 30), "%s: batch too large for 32-bit row ids", who);
    return DAGL_OK;
}
static inline int graph_edges_ok(const char* who, int64_t total_edges) {
    DAGL_REQUIRE(total_edges >= 0 && total_edges < (1ll << 31), "%s: total_edges=%lld outside [0, 2^31)", who, (long long)total_edges);
    return DAGL_OK;
}
static inline int graph_shape_ok(const char* who, int B, int H, int W, int64_t total_edges) {
    const int rc = graph_dims_ok(who, B, H, W);
    return rc ? rc : graph_edges_ok(who, total_edges);
}

// what the attend side asks of its operands.  more_ok: the pointers an entry adds to the null test; more_flags: the flags it adds
static inline int graph_operands_ok(const char* who, const float* wq_rows, const float* x_rows, const int64_t* row_off, const int32_t* key,
                                    int64_t total_edges, float scale, int flags, bool more_ok = true, int more_flags = 0) {
    DAGL_REQUIRE(wq_rows && x_rows && row_off && (total_edges == 0 || key) && more_ok, "%s: null tensor pointer", who);
    DAGL_REQUIRE(((uintptr_t)wq_rows % 16) == 0 && ((uintptr_t)x_rows % 16) == 0, "%s: feature rows must be 16-byte aligned", who);
    DAGL_REQUIRE((flags & ~(DAGL_GRAPH_ATTEND_EDGES_ONLY | more_flags)) == 0, "%s: unknown flags 0x%x", who, flags);
    DAGL_REQUIRE(scale > 0.f && scale < INFINITY, "%s: scale=%g must be positive and finite", who, (double)scale);
    return DAGL_OK;
}

// what the attend, forward and refresh calls share
struct GraphAttendCall {
    const float* wq_rows; const float* x_rows;             // [B L, 196], [B N, 196]
    const int64_t* row_off; const int32_t* key; int64_t E;
    const float* tau;                                      // [B L] or null: no margin
    float scale; bool edges_only;
};
static inline GraphAttendCall graph_attend_call(const float* wq_rows, const float* x_rows, const int64_t* row_off, const int32_t* key,
                                                int64_t total_edges, const float* tau, float scale, int flags) {
    return GraphAttendCall{wq_rows, x_rows, row_off, key, total_edges, tau, scale, (flags & DAGL_GRAPH_ATTEND_EDGES_ONLY) != 0};
}

static inline GtArgs gt_args(int B, const Grid& g, const GraphAttendCall& c) {
    GtArgs a{};
    a.row_off = c.row_off; a.n_rows = B * g.L; a.key = c.key; a.E = c.E;
    a.wq = c.wq_rows; a.x = c.x_rows; a.tau = c.tau; a.L = g.L; a.N = g.N; a.scale = c.scale; a.edges_only = c.edges_only ? 1 : 0;
    return a;
}

// the CSR rows over the padded value map (out / part are the caller's)
static inline GaArgs ga_map_args(int B, const Grid& g, const float* b2p, const int64_t* row_off, const int32_t* key, const float* weight,
                                 int64_t E) {
    GaArgs a{};
    a.row_off = row_off; a.n_rows = B * g.L; a.key = key; a.weight = weight; a.perm = nullptr; a.E = E;
    a.src = b2p; a.n_src = g.N; a.L = g.L; a.W = g.W; a.Wp = g.Wp; a.img4 = (long long)g.Hp * g.Wp * (CH / 4);
    return a;
}

}  // namespace dagl
