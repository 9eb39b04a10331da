// The forward on a GIVEN patch graph in one crossing of the edge array: out = dagl_graph_apply(weight = dagl_graph_attend(...)) without
// the `score` and `weight` arrays -- the semantics are those two entries', include/dagl_ce.h.  With Wq [B L, 196] / X [B N, 196] the
// fc1 / fc2 features and V the 7x7 patches of the value map, per edge e of row r:
//   S_e = <Wq[r], X[b N + key_e]>, z_e and on_e by gt_logit (graph_rows.h), w_e = on_e e^(z_e - M) / D,  agg[r] = sum_e w_e V[key_e]
// with (M, D) the row's statistics in the reference's or the edges-only normalisation; out = fold(agg) / cnt.
//
// Work is cut by edges as in graph_apply.hip / graph_attend.hip: block c takes the edges [c SEG, (c + 1) SEG) whatever rows they belong to.
//   segment kernel  the scores of the segment (an edge per 16 lanes, gt_edge_dot), then per run of equal row its fp32 maximum m, the
//                   fp64 sum of e^(z - m) in edge order and the partial row sum_on e^(z - m) V[key] gathered from the map
//                   (ga_gather_run).  A run that starts in the segment leaves its row's slots, the run that came in from an earlier
//                   segment the segment's.
//   combine kernel  per row: M over its start and the segments it crosses (0 joins in when keys are off the graph), D in segment
//                   order, and the row = sum of the partial rows scaled by e^(m_c - M), in segment order, / D.  Empty rows become zeros.
//   fold            launch_fold, as dagl_graph_apply.
// The maximum is fp32, the statistics' sums fp64 in a fixed order, no float atomics: the same arrays give the same bits on every call.
// Grids come from E and B L alone; nothing is read on the host.  Every row index comes out of the bounded search, every key is
// range-tested before an address is formed: no array content makes a kernel leave its buffers.
//
// What bounds it: the segment kernel reads 2 x 784 B of features and 3136 B of value patch per edge, nearly all of it out of L2 at the
// degrees the selection produces; at k = 8 it is a launch of E / 128 short blocks and the call is bounded by its three launches and the
// fold's pass over the aggregated rows.
#include "dagl_common.h"
#include "graph_rows.h"

namespace dagl {

__global__ __launch_bounds__(256) void graph_forward_segment_kernel(GtArgs a, GaArgs v, GfStats st) {
    __shared__ long long sh_x[GA_SEG];        // float4 offset of the key's feature row, -1 = key out of range
    __shared__ long long sh_of[GA_SEG];       // float4 offset of the key's patch in the map, -1 = the edge carries no value row
    __shared__ int sh_row[GA_SEG];
    __shared__ float sh_z[GA_SEG];
    __shared__ float sh_w[GA_SEG];            // e^(z - the run's maximum)
    const int t = threadIdx.x;
    const auto [p0, m] = ga_segment(a.E);
    if (t < m) {
        const int row = ga_row_of(a.row_off, a.n_rows, p0 + t);
        const int key = a.key[p0 + t];
        sh_row[t] = row;
        sh_x[t] = gt_feature_row(a.L, a.N, row, key);
        sh_of[t] = ga_source<true>(v, row, key);
    }
    __syncthreads();
    const int l = t & 15, grp = t >> 4;
    const float4* wq = reinterpret_cast<const float4*>(a.wq);
    const float4* xk = reinterpret_cast<const float4*>(a.x);
    for (int e = grp; e < m; e += 16) {
        const long long of = sh_x[e];
        const int row = sh_row[e];
        const float acc = gt_edge_dot(wq + (size_t)row * GT_C4, xk + (of >= 0 ? of : 0), l);
        if (l == 0) {
            float mg;
            sh_z[e] = gt_logit(a, row, of >= 0 ? acc : 0.f, mg);
            if (mg == 0.f) sh_of[e] = -1;                      // off: it takes part in D and weighs 0
        }
    }
    __syncthreads();
    gt_run_stats<true>(a, p0, m, sh_row, sh_z, sh_w, st);
    __syncthreads();
    const int r = t < GA_C4 ? t : GA_C4 - 1;                   // (threads 196..255 stage and score edges, then idle along)
    const float4* src = reinterpret_cast<const float4*>(v.src) + (r / 28) * v.Wp * (CH / 4) + r % 28;
    // only the segment's first run can have come in from an earlier segment: one look at the offsets, outside the chain of the runs
    const bool first_came_in = m > 0 && a.row_off[sh_row[0]] < p0;
    int e = 0;
    while (e < m) {
        const int cur = sh_row[e];
        int end = e + 1;
        while (end < m && sh_row[end] == cur) ++end;
        const float4 acc = ga_gather_run(src, sh_of, sh_w, e, end);
        const bool head = e == 0 && first_came_in;
        float4* dst = reinterpret_cast<float4*>(head ? v.part + (size_t)blockIdx.x * P : v.out + (size_t)cur * P);
        if (t < GA_C4) dst[t] = acc;
        e = end;
    }
}

// per row: zeros (an empty row), or its start and the partial rows of the segments it crosses brought onto the row's maximum, in
// segment order, over D.  Every thread forms M and D itself from the same slots in the same order: no broadcast, the same bits
__global__ __launch_bounds__(256) void graph_forward_combine_kernel(GtArgs a, GfStats st, const float* __restrict__ part,
                                                                     float* __restrict__ agg) {
    __shared__ double sh_sc[256];             // e^(m_c - M) of a batch of segments
    const int t = threadIdx.x, row = blockIdx.x;
    const long long lo = gt_clamp(a.row_off[row], a.E), hi = gt_clamp(a.row_off[row + 1], a.E);
    float4* o = reinterpret_cast<float4*>(agg + (size_t)row * P);
    if (hi <= lo) {
        if (t < GA_C4) o[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const long long deg = hi - lo, c0 = lo / GA_SEG, c1 = (hi - 1) / GA_SEG;
    const bool off_graph = !a.edges_only && deg < a.N;
    const float m0 = st.row_max[row];
    float M = off_graph ? fmaxf(m0, 0.f) : m0;
    for (long long c = c0 + 1; c <= c1; ++c) M = fmaxf(M, st.chunk_max[c]);
    const double sc0 = exp((double)m0 - (double)M);
    double sum = st.row_sum[row] * sc0;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < GA_C4) {
        const float f = (float)sc0;
        const float4 h = o[t];
        s = make_float4(f * h.x, f * h.y, f * h.z, f * h.w);
    }
    const float4* pp = reinterpret_cast<const float4*>(part);
    for (long long cb = c0 + 1; cb <= c1; cb += 256) {         // (block-uniform bounds)
        const int nb = (int)((c1 - cb + 1 < 256) ? c1 - cb + 1 : 256);
        __syncthreads();
        if (t < nb) sh_sc[t] = exp((double)st.chunk_max[cb + t] - (double)M);
        __syncthreads();
        for (int i = 0; i < nb; ++i) {
            const double sc = sh_sc[i];
            sum += st.chunk_sum[cb + i] * sc;
            if (t < GA_C4) {
                const float f = (float)sc;
                const float4 h = pp[(size_t)(cb + i) * GA_C4 + t];
                s.x = fmaf(f, h.x, s.x); s.y = fmaf(f, h.y, s.y); s.z = fmaf(f, h.z, s.z); s.w = fmaf(f, h.w, s.w);
            }
        }
    }
    if (off_graph) sum += (double)(a.N - deg) * exp(-(double)M);
    if (t < GA_C4) {
        const float inv = (float)(1.0 / sum);
        o[t] = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// agg [B L, 784], one partial row and one (max, sum) slot per segment, one slot per row.  The one walk behind the size (null base)
// and the launches
struct GfWs { float* agg; float* part; GfStats st; size_t bytes; };
static GfWs gf_carve(void* ws, int B, const Grid& g, int64_t E) {
    Carver cv(ws);
    GfWs w{};
    const size_t rows = (size_t)B * g.L, chunks = ga_chunks(E) + 1;
    w.agg = cv.take<float>(rows * P);
    w.part = cv.take<float>(chunks * P);
    w.st = carve_stats(cv, rows, chunks);
    w.bytes = cv.bytes();
    return w;
}
static size_t graph_forward_workspace_bytes(int B, const Grid& g, int64_t E) { return gf_carve(nullptr, B, g, E).bytes; }

static int launch_graph_forward(hipStream_t s, int B, const Grid& g, const GraphAttendCall& c, const float* b2p, float* out, void* workspace) {
    const GfWs w = gf_carve(workspace, B, g, c.E);
    const GtArgs a = gt_args(B, g, c);
    GaArgs v = ga_map_args(B, g, b2p, c.row_off, c.key, nullptr, c.E);
    v.out = w.agg; v.part = w.part;
    if (c.E > 0) {
        hipLaunchKernelGGL(graph_forward_segment_kernel, dim3((unsigned)ga_chunks(c.E)), dim3(256), 0, s, a, v, w.st);
        DAGL_LAUNCH_CHECK("graph_forward_segment_kernel");
    }
    hipLaunchKernelGGL(graph_forward_combine_kernel, dim3((unsigned)a.n_rows), dim3(256), 0, s, a, w.st, w.part, w.agg);
    DAGL_LAUNCH_CHECK("graph_forward_combine_kernel");
    return launch_fold(s, B, g, w.agg, out);
}

}  // namespace dagl

using namespace dagl;

extern "C" {

// the fused forward on a given patch graph (no ABI bump: found by symbol)
size_t dagl_graph_forward_workspace_bytes(int B, int H, int W, int64_t total_edges) {
    if (graph_shape_ok("dagl_graph_forward_workspace_bytes", B, H, W, total_edges)) return 0;
    return graph_forward_workspace_bytes(B, make_grid(H, W), total_edges);
}

int dagl_graph_forward(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                       const int64_t* row_off, const int32_t* key, int64_t total_edges, const float* tau, float scale, int flags,
                       float* out, void* workspace, size_t ws_bytes) {
    const char* who = "dagl_graph_forward";
    int rc = graph_shape_ok(who, B, H, W, total_edges);
    if (rc || (rc = graph_operands_ok(who, wq_rows, x_rows, row_off, key, total_edges, scale, flags))) return rc;
    DAGL_REQUIRE(b2p && out, "dagl_graph_forward: null tensor pointer");
    DAGL_REQUIRE(((uintptr_t)b2p % 16) == 0, "dagl_graph_forward: b2p must be 16-byte aligned");
    const Grid g = make_grid(H, W);
    if ((rc = check_workspace(who, workspace, ws_bytes, graph_forward_workspace_bytes(B, g, total_edges)))) return rc;
    const GraphAttendCall c = graph_attend_call(wq_rows, x_rows, row_off, key, total_edges, tau, scale, flags);
    return launch_graph_forward((hipStream_t)stream, B, g, c, b2p, out, workspace);
}

}  // extern "C"
