// A CE block run on a GIVEN patch graph (ABI 409): out[b] = fold(A_G[b] . V(b2[b])) / cnt with A_G the CSR rows b L .. b L + L - 1 of a
// PatchGraph (graph.hip exports one; callers edit it) -- dagl.py:263-272 with `yi` supplied by the caller -- and its gradients with
// respect to the value map and the edge weights.
//
// Degrees are whatever the caller made them: top-k rows of 8 next to edited rows of N keys, empty rows, rows longer than N (keys may
// repeat and come in any order).  So the work is cut by EDGES, not rows (the idiom of backward.hip's edge_segreduce_kernel /
// row_fixup_kernel): block c takes the edges [c SEG, (c + 1) SEG) of the whole array and walks the runs of equal row inside them.
// A run that STARTS in the chunk goes to its row of the output, a run that came in from an earlier chunk to the chunk's one partial
// row; graph_apply_combine_kernel then adds, per row, the partials of the chunks it crosses in chunk order.  The longest row costs no
// more than its share of chunks, a chunk holds up to SEG short rows, every sum has a fixed order (no float atomics): the same bits on
// every call.  The grids come from E and the row count alone; nothing is read on the host.
//
// One kernel serves both products (template MAP):
//   MAP   rows = the B L queries, key = patch index 0 .. N-1 of the row's image; the 784 floats of a key are read from the padded
//         NHWC value map as aggregate_direct.h reads them ([N, 784] value rows never exist);
//   !MAP  (the backward's A^T . dAgg over the transposed CSR) rows = the B N keys, key = global query row, the 784 floats come from
//         a materialised [B L, 784] array and the weight of transposed edge e is weight[perm[e]].
// A key (or perm entry) outside its range contributes nothing and is tested BEFORE an address is formed; row indices come out of a
// bounded search: no array content can make a kernel read or write outside its buffers.
#include "dagl_common.h"
#include "graph_rows.h"

namespace dagl {

int launch_fold_patches(hipStream_t s, int B, int Hp, int Wp, int C, int k, int stride, int oy, int ox, int oh, int ow, const float* drows,
                        float* dmap);

template <bool MAP>
__global__ __launch_bounds__(256) void graph_apply_segment_kernel(GaArgs a) {
    __shared__ long long sh_of[GA_SEG];
    __shared__ float sh_w[GA_SEG];
    __shared__ int sh_row[GA_SEG];
    const int t = threadIdx.x;
    const auto [p0, m] = ga_segment(a.E);
    if (t < m) {
        const long long p = p0 + t;
        const int row = ga_row_of(a.row_off, a.n_rows, p);
        long long of = ga_source<MAP>(a, row, a.key[p]);
        long long wi = p;
        if (a.perm != nullptr) {
            wi = a.perm[p];
            if (wi < 0 || wi >= a.E) of = -1;
        }
        sh_of[t] = of;
        sh_w[t] = of >= 0 ? a.weight[wi] : 0.f;
        sh_row[t] = row;
    }
    __syncthreads();
    const int r = t < GA_C4 ? t : GA_C4 - 1;                   // (threads 196..255 stage edges, then idle along)
    const float4* src = reinterpret_cast<const float4*>(a.src) + (MAP ? (r / 28) * a.Wp * (CH / 4) + r % 28 : r);
    int e = 0;
    while (e < m) {
        const int cur = sh_row[e];
        int end = e + 1;
        while (end < m && sh_row[end] == cur) ++end;
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
        // a run that came in from an earlier chunk (only the first can) leaves this chunk's partial row, any other starts its row
        const bool head = a.row_off[cur] < p0;
        float4* dst = reinterpret_cast<float4*>(head ? a.part + (size_t)blockIdx.x * P : a.out + (size_t)cur * P);
        if (t < GA_C4) dst[t] = acc;
        e = end;
    }
}

// per row: nothing (the row lies inside one chunk), zeros (an empty row), or its start + the partials of the chunks it crosses, in
// chunk order: wave w adds the partials c0 + 1 + w, c0 + 5 + w, .. , the four sums join the row's start in wave order
__global__ __launch_bounds__(256) void graph_apply_combine_kernel(const int64_t* __restrict__ row_off, long long E,
                                                                   const float* __restrict__ part, float* __restrict__ out) {
    __shared__ float4 sh[4][GA_C4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    long long lo = row_off[blockIdx.x], hi = row_off[blockIdx.x + 1];
    lo = lo < 0 ? 0 : (lo > E ? E : lo);                       // (gt_clamp, written out: called from graph_rows.h this kernel's device code changes)
    hi = hi < 0 ? 0 : (hi > E ? E : hi);
    float4* o = reinterpret_cast<float4*>(out + (size_t)blockIdx.x * P);
    if (hi <= lo) {
        if (t < GA_C4) o[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const long long c0 = lo / GA_SEG, c1 = (hi - 1) / GA_SEG;
    if (c0 == c1) return;
    const float4* pp = reinterpret_cast<const float4*>(part);
    float4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long c = c0 + 1 + w; c <= c1; c += 8) {
        const bool two = c + 4 <= c1;
        float4 h0[4], h1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = lane + 64 * u < GA_C4 ? lane + 64 * u : GA_C4 - 1;
            h0[u] = pp[(size_t)c * GA_C4 + col];
            h1[u] = pp[(size_t)(two ? c + 4 : c) * GA_C4 + col];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[u].x += h0[u].x; acc[u].y += h0[u].y; acc[u].z += h0[u].z; acc[u].w += h0[u].w;
            if (two) { acc[u].x += h1[u].x; acc[u].y += h1[u].y; acc[u].z += h1[u].z; acc[u].w += h1[u].w; }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (lane + 64 * u < GA_C4) sh[w][lane + 64 * u] = acc[u];
    __syncthreads();
    if (t < GA_C4) {
        float4 s = o[t];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float4 h = sh[k][t]; s.x += h.x; s.y += h.y; s.z += h.z; s.w += h.w; }
        o[t] = s;
    }
}

// d weight[e] = <dAgg[row(e)], V[key(e)]>: the same chunks of SEG edges, a wave per edge (lane = float4 columns lane + 64 u)
__global__ __launch_bounds__(256) void graph_apply_dweight_kernel(GaArgs a, const float* __restrict__ dagg, float* __restrict__ dweight) {
    __shared__ long long sh_of[GA_SEG];
    __shared__ int sh_row[GA_SEG];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const auto [p0, m] = ga_segment(a.E);
    if (t < m) {
        const int row = ga_row_of(a.row_off, a.n_rows, p0 + t);
        sh_of[t] = ga_source<true>(a, row, a.key[p0 + t]);
        sh_row[t] = row;
    }
    __syncthreads();
    int voff[4], col[4]; bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        ok[u] = lane + 64 * u < GA_C4;
        col[u] = ok[u] ? lane + 64 * u : GA_C4 - 1;
        voff[u] = (col[u] / 28) * a.Wp * (CH / 4) + col[u] % 28;
    }
    const float4* vm = reinterpret_cast<const float4*>(a.src);
    const float4* dg = reinterpret_cast<const float4*>(dagg);
    for (int e0 = w; e0 < m; e0 += 8) {                        // two edges per step: sixteen loads in flight per lane
        float4 v[2][4], d[2][4]; long long of[2]; int e[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            e[i] = e0 + 4 * i < m ? e0 + 4 * i : e0;
            of[i] = sh_of[e[i]];
            const float4* vj = vm + (of[i] >= 0 ? of[i] : 0);
            const float4* dr = dg + (size_t)sh_row[e[i]] * GA_C4;
#pragma unroll
            for (int u = 0; u < 4; ++u) { v[i][u] = vj[voff[u]]; d[i][u] = dr[col[u]]; }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float s = d[i][u].x * v[i][u].x + d[i][u].y * v[i][u].y + d[i][u].z * v[i][u].z + d[i][u].w * v[i][u].w;
                acc += ok[u] ? s : 0.f;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0 && (i == 0 || e0 + 4 < m)) dweight[p0 + e[i]] = of[i] >= 0 ? acc : 0.f;
        }
    }
}

// forward: agg [B L, 784] + the chunks' partial rows;  backward: dAgg [B L, 784] + d V rows [B N, 784] + partial rows.  The one
// walk behind the size (null base) and both launches
struct GaWs { float* agg; float* dv; float* part; size_t bytes; };
static GaWs ga_carve(void* ws, int B, const Grid& g, int64_t E, bool backward) {
    Carver cv(ws);
    GaWs w;
    w.agg = cv.take<float>((size_t)B * g.L * P);
    w.dv = backward ? cv.take<float>((size_t)B * g.N * P) : nullptr;
    w.part = cv.take<float>((ga_chunks(E) + 1) * P);
    w.bytes = cv.bytes();
    return w;
}
static size_t graph_apply_workspace_bytes(int B, const Grid& g, int64_t E, bool backward) { return ga_carve(nullptr, B, g, E, backward).bytes; }

template <bool MAP>
static int ga_product(hipStream_t s, GaArgs a) {
    if (a.E > 0) {
        hipLaunchKernelGGL(graph_apply_segment_kernel<MAP>, dim3((unsigned)ga_chunks(a.E)), dim3(256), 0, s, a);
        DAGL_LAUNCH_CHECK("graph_apply_segment_kernel");
    }
    hipLaunchKernelGGL(graph_apply_combine_kernel, dim3((unsigned)a.n_rows), dim3(256), 0, s, a.row_off, a.E, a.part, a.out);
    DAGL_LAUNCH_CHECK("graph_apply_combine_kernel");
    return DAGL_OK;
}

static int launch_graph_apply(hipStream_t s, int B, const Grid& g, const float* b2p, const int64_t* row_off, const int32_t* key,
                              const float* weight, int64_t E, float* out, void* workspace) {
    const GaWs w = ga_carve(workspace, B, g, E, false);
    GaArgs a = ga_map_args(B, g, b2p, row_off, key, weight, E);
    a.out = w.agg; a.part = w.part;
    const int rc = ga_product<true>(s, a);
    if (rc) return rc;
    return launch_fold(s, B, g, a.out, out);
}

static int launch_graph_apply_backward(hipStream_t s, int B, const Grid& g, const float* b2p, const int64_t* row_off, const int32_t* key,
                                       const float* weight, int64_t E, const float* d_out, const int64_t* col_off, const int32_t* src_row,
                                       const int32_t* perm, float* d_b2p /* or null */, float* d_weight /* or null */, void* workspace) {
    const GaWs w = ga_carve(workspace, B, g, E, true);
    float *dagg = w.agg, *dv = w.dv, *part = w.part;
    int rc = launch_unfold_dout(s, B, g, d_out, dagg);
    if (rc) return rc;
    if (d_weight != nullptr && E > 0) {
        const GaArgs a = ga_map_args(B, g, b2p, row_off, key, weight, E);
        hipLaunchKernelGGL(graph_apply_dweight_kernel, dim3((unsigned)ga_chunks(E)), dim3(256), 0, s, a, dagg, d_weight);
        DAGL_LAUNCH_CHECK("graph_apply_dweight_kernel");
    }
    if (d_b2p != nullptr) {
        // d V rows = A^T dAgg: the same product over the transposed CSR, rows read from dAgg
        GaArgs a{};
        a.row_off = col_off; a.n_rows = B * g.N; a.key = src_row; a.weight = weight; a.perm = perm; a.E = E;
        a.src = dagg; a.n_src = B * g.L; a.L = 1; a.W = 1; a.Wp = 1; a.img4 = 0;
        a.out = dv; a.part = part;
        if ((rc = ga_product<false>(s, a))) return rc;
        // d b2p = the stride-1 adjoint of unfold: every pixel of the padded map is written
        return launch_fold_patches(s, B, g.Hp, g.Wp, CH, KS, 1, 0, 0, g.H, g.W, dv, d_b2p);
    }
    return DAGL_OK;
}

static size_t graph_apply_bytes(const char* who, int B, int H, int W, int64_t total_edges, bool backward) {
    if (graph_shape_ok(who, B, H, W, total_edges)) return 0;
    return graph_apply_workspace_bytes(B, make_grid(H, W), total_edges, backward);
}

}  // namespace dagl

using namespace dagl;

extern "C" {

// (ABI 409) a block run on a given patch graph; workspace = whole bytes of the forward / backward call
int dagl_graph_apply_segment(void) { return GA_SEG; }

size_t dagl_graph_apply_workspace_bytes(int B, int H, int W, int64_t total_edges) {
    return graph_apply_bytes("dagl_graph_apply_workspace_bytes", B, H, W, total_edges, false);
}

size_t dagl_graph_apply_backward_workspace_bytes(int B, int H, int W, int64_t total_edges) {
    return graph_apply_bytes("dagl_graph_apply_backward_workspace_bytes", B, H, W, total_edges, true);
}

int dagl_graph_apply(void* stream, int B, int H, int W, const float* b2p, const int64_t* row_off, const int32_t* key, const float* weight,
                     int64_t total_edges, float* out, void* workspace, size_t ws_bytes) {
    int rc = graph_shape_ok("dagl_graph_apply", B, H, W, total_edges);
    if (rc) return rc;
    DAGL_REQUIRE(b2p && row_off && out && (total_edges == 0 || (key && weight)), "dagl_graph_apply: null tensor pointer");
    DAGL_REQUIRE(((uintptr_t)b2p % 16) == 0, "dagl_graph_apply: b2p must be 16-byte aligned");
    const Grid g = make_grid(H, W);
    if ((rc = check_workspace("dagl_graph_apply", workspace, ws_bytes, graph_apply_workspace_bytes(B, g, total_edges, false)))) return rc;
    return launch_graph_apply((hipStream_t)stream, B, g, b2p, row_off, key, weight, total_edges, out, workspace);
}

int dagl_graph_apply_backward(void* stream, int B, int H, int W, const float* b2p, const int64_t* row_off, const int32_t* key,
                              const float* weight, int64_t total_edges, const float* d_out, const int64_t* col_off,
                              const int32_t* src_row, const int32_t* perm, float* d_b2p, float* d_weight, void* workspace,
                              size_t ws_bytes) {
    int rc = graph_shape_ok("dagl_graph_apply_backward", B, H, W, total_edges);
    if (rc) return rc;
    DAGL_REQUIRE(b2p && row_off && d_out && (total_edges == 0 || (key && weight)), "dagl_graph_apply_backward: null tensor pointer");
    DAGL_REQUIRE(d_b2p == nullptr || (col_off && (total_edges == 0 || (src_row && perm))),
                 "dagl_graph_apply_backward: null transposed CSR (col_off, src_row, perm are required with d_b2p)");
    DAGL_REQUIRE(((uintptr_t)b2p % 16) == 0 && ((uintptr_t)d_b2p % 16) == 0, "dagl_graph_apply_backward: maps must be 16-byte aligned");
    const Grid g = make_grid(H, W);
    if ((rc = check_workspace("dagl_graph_apply_backward", workspace, ws_bytes, graph_apply_workspace_bytes(B, g, total_edges, true)))) return rc;
    return launch_graph_apply_backward((hipStream_t)stream, B, g, b2p, row_off, key, weight, total_edges, d_out, col_off, src_row, perm,
                                       d_b2p, d_weight, workspace);
}

}  // extern "C"
