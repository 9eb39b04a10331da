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

struct GfStats { float* row_max; double* row_sum; float* chunk_max; double* chunk_sum; };

__global__ __launch_bounds__(256) void graph_forward_segment_kernel(GtArgs a, GaArgs v, GfStats st) {
    __shared__ long long sh_x[GA_SEG];        // float4 offset of the key's feature row, -1 = key out of range
    __shared__ long long sh_of[GA_SEG];       // float4 offset of the key's patch in the map, -1 = the edge carries no value row
    __shared__ int sh_row[GA_SEG];
    __shared__ float sh_z[GA_SEG];
    __shared__ float sh_w[GA_SEG];            // e^(z - the run's maximum)
    const int t = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * GA_SEG;
    const int m = (int)((a.E - p0 < GA_SEG) ? a.E - p0 : GA_SEG);
    if (t < m) {
        const int row = ga_row_of(a.row_off, a.n_rows, p0 + t);
        const int key = a.key[p0 + t];
        sh_row[t] = row;
        sh_x[t] = (unsigned)key < (unsigned)a.N ? ((long long)(row / a.L) * a.N + key) * GT_C4 : -1;
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
    // one (max, sum) per run of equal row, by the thread of the run's first edge, in edge order
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
            sh_w[j] = p;
        }
        if (a.row_off[row] < p0) { st.chunk_max[blockIdx.x] = mx; st.chunk_sum[blockIdx.x] = sum; }
        else { st.row_max[row] = mx; st.row_sum[row] = sum; }
    }
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
    const size_t rows = (size_t)B * g.L, chunks = (size_t)((E + GA_SEG - 1) / GA_SEG) + 1;
    w.agg = cv.take<float>(rows * P);
    w.part = cv.take<float>(chunks * P);
    w.st.row_max = cv.take<float>(rows);
    w.st.row_sum = cv.take<double>(rows);
    w.st.chunk_max = cv.take<float>(chunks);
    w.st.chunk_sum = cv.take<double>(chunks);
    w.bytes = cv.bytes();
    return w;
}
size_t graph_forward_workspace_bytes(int B, const Grid& g, int64_t E) { return gf_carve(nullptr, B, g, E).bytes; }

int launch_graph_forward(hipStream_t s, int B, const Grid& g, const GraphAttendCall& c, const float* b2p, float* out, void* workspace) {
    const GfWs w = gf_carve(workspace, B, g, c.E);
    GtArgs a{};
    a.row_off = c.row_off; a.n_rows = B * g.L; a.key = c.key; a.E = c.E;
    a.wq = c.wq_rows; a.x = c.x_rows; a.tau = c.tau; a.L = g.L; a.N = g.N; a.scale = c.scale; a.edges_only = c.edges_only ? 1 : 0;
    GaArgs v{};
    v.row_off = c.row_off; v.n_rows = a.n_rows; v.key = c.key; v.weight = nullptr; v.perm = nullptr; v.E = c.E;
    v.src = b2p; v.n_src = g.N; v.L = g.L; v.W = g.W; v.Wp = g.Wp; v.img4 = (long long)g.Hp * g.Wp * (CH / 4);
    v.out = w.agg; v.part = w.part;
    if (c.E > 0) {
        hipLaunchKernelGGL(graph_forward_segment_kernel, dim3((unsigned)((c.E + GA_SEG - 1) / GA_SEG)), dim3(256), 0, s, a, v, w.st);
        DAGL_LAUNCH_CHECK("graph_forward_segment_kernel");
    }
    hipLaunchKernelGGL(graph_forward_combine_kernel, dim3((unsigned)a.n_rows), dim3(256), 0, s, a, w.st, w.part, w.agg);
    DAGL_LAUNCH_CHECK("graph_forward_combine_kernel");
    return launch_fold(s, B, g, w.agg, out);
}

}  // namespace dagl
