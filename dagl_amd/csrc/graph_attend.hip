// Attention on a GIVEN patch graph (ABI 412): the block's own edge weights on a structure the caller supplies -- dagl.py:250-261 restricted
// to the edges of a PatchGraph -- and their gradients.  With Wq [B L, 196] / X [B N, 196] the fc1 / fc2 features, per edge e of row r
// (image b = r / L, key_e in [0, N)):
//   S_e = <Wq[r], X[b N + key_e]>
//   tau given:  m_e = relu(S_e - tau_r), z_e = scale S_e m_e, on_e = (m_e != 0)       (the adaptive rule, dagl.py:256-261)
//   tau NULL:   z_e = scale S_e, on_e = 1                                             (the fixed-k variant)
//   reference normalisation:  M = max(max_e z_e, 0 if deg_r < N),  D = sum_e e^(z_e - M) + max(N - deg_r, 0) e^(-M)  -- every key off the
//   graph is one of the reference's e^0 --;  edges-only: M = max_e z_e, D = sum_e e^(z_e - M);  w_e = on_e e^(z_e - M) / D.
// deg_r counts EDGES: a repeated key is an entry of its own.  A key outside [0, N) is tested before an address is formed; it scores 0,
// weighs 0 and takes part in D with that score.
//
// Work is cut by edges as in graph_apply.hip: block c takes the edges [c SEG, (c + 1) SEG) whatever rows they belong to.
//   forward   score kernel: an edge per 16 lanes (49 float4 of both 784-byte rows, a fixed 4-step reduction), then per run of equal
//             row inside the chunk one (max, sum e^(z - max)) -- the run that came in from an earlier chunk leaves the chunk's slot, any
//             other its row's; rows kernel: per row the slots of the chunks it crosses, in chunk order, rescaled by e^(m_c - M);
//             weight kernel: per edge.
//   backward  c_r = sum w_e g_e and d tau_r = -scale sum_on S_e w_e (g_e - c_r) through the same chunk / row slots (three sums),
//             d S_e per edge, then  d Wq = CSR x X rows  and  d X = transposed CSR x Wq rows  as the segment + combine product of
//             graph_apply.hip with 49 float4 per row.
// The maximum is fp32, every sum of the statistics fp64 in a fixed order, no float atomics: the same input gives the same bits on every
// call.  Grids come from E and the row counts alone; nothing is read on the host.  Every row index comes out of the bounded search or
// of the workspace this call wrote, every key and perm entry is range-tested: no array content makes a kernel leave its buffers.
#include "dagl_common.h"
#include "graph_rows.h"

namespace dagl {

// ---- forward ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void graph_attend_score_kernel(GtArgs a, float* __restrict__ score, int32_t* __restrict__ row_of,
                                                                  float* __restrict__ row_max, double* __restrict__ row_sum,
                                                                  float* __restrict__ chunk_max, double* __restrict__ chunk_sum) {
    __shared__ long long sh_x[GA_SEG];        // float4 offset of the key's feature row, -1 = key out of range
    __shared__ int sh_row[GA_SEG];
    __shared__ float sh_z[GA_SEG];
    const int t = threadIdx.x;
    const auto [p0, m] = ga_segment(a.E);
    if (t < m) {
        const int row = ga_row_of(a.row_off, a.n_rows, p0 + t);
        const int key = a.key[p0 + t];
        sh_row[t] = row;
        sh_x[t] = gt_feature_row(a.L, a.N, row, key);
        row_of[p0 + t] = row;
    }
    __syncthreads();
    // an edge per 16 lanes (gt_edge_dot)
    const int l = t & 15, grp = t >> 4;
    const float4* wq = reinterpret_cast<const float4*>(a.wq);
    const float4* xk = reinterpret_cast<const float4*>(a.x);
    for (int e = grp; e < m; e += 16) {
        const long long of = sh_x[e];
        const int row = sh_row[e];
        const float acc = gt_edge_dot(wq + (size_t)row * GT_C4, xk + (of >= 0 ? of : 0), l);
        if (l == 0) {
            const float s = of >= 0 ? acc : 0.f;
            float mg;
            score[p0 + e] = s;
            sh_z[e] = gt_logit(a, row, s, mg);
        }
    }
    __syncthreads();
    gt_run_stats<false>(a, p0, m, sh_row, sh_z, nullptr, GfStats{row_max, row_sum, chunk_max, chunk_sum});
}

// per non-empty row: (M, D) over its start and the chunks it crosses, in chunk order, written over the row's slots
// (graph_forward_combine_kernel forms the same (M, D) but fuses the sum into its loop over the partial rows: the two stay apart)
__global__ __launch_bounds__(256) void graph_attend_rows_kernel(GtArgs a, float* __restrict__ row_max, double* __restrict__ row_sum,
                                                                 const float* __restrict__ chunk_max, const double* __restrict__ chunk_sum) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_rows) return;
    const long long lo = gt_clamp(a.row_off[r], a.E), hi = gt_clamp(a.row_off[r + 1], a.E);
    if (hi <= lo) return;
    const long long deg = hi - lo, c0 = lo / GA_SEG, c1 = (hi - 1) / GA_SEG;
    const bool off_graph = !a.edges_only && deg < a.N;
    const float m0 = row_max[r];
    float M = off_graph ? fmaxf(m0, 0.f) : m0;
    for (long long c = c0 + 1; c <= c1; ++c) M = fmaxf(M, chunk_max[c]);
    double sum = row_sum[r] * exp((double)m0 - (double)M);
    for (long long c = c0 + 1; c <= c1; ++c) sum += chunk_sum[c] * exp((double)chunk_max[c] - (double)M);
    if (off_graph) sum += (double)(a.N - deg) * exp(-(double)M);
    row_max[r] = M;
    row_sum[r] = sum;
}

__global__ __launch_bounds__(256) void graph_attend_weight_kernel(GtArgs a, const float* __restrict__ score, const int32_t* __restrict__ row_of,
                                                                   const float* __restrict__ row_max, const double* __restrict__ row_sum,
                                                                   float* __restrict__ weight) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.E) return;
    const int row = row_of[e];
    float mg;
    const float z = gt_logit(a, row, score[e], mg);
    const bool on = mg != 0.f && (unsigned)a.key[e] < (unsigned)a.N;
    weight[e] = on ? (float)((double)expf(z - row_max[row]) / row_sum[row]) : 0.f;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// per run of equal row inside a chunk: sum w g, sum_on S w g, sum_on S w (fp64, edge order)
__global__ __launch_bounds__(GA_SEG) void graph_attend_bwd_partial_kernel(GtArgs a, const float* __restrict__ score,
                                                                           const float* __restrict__ weight, const float* __restrict__ dweight,
                                                                           int32_t* __restrict__ row_of, double* __restrict__ row_part,
                                                                           double* __restrict__ chunk_part) {
    __shared__ double sh_p[3][GA_SEG];
    __shared__ int sh_row[GA_SEG];
    const int t = threadIdx.x;
    const auto [p0, m] = ga_segment(a.E);
    if (t < m) {
        const int row = ga_row_of(a.row_off, a.n_rows, p0 + t);
        const float s = score[p0 + t];
        const double w = weight[p0 + t], g = dweight[p0 + t];
        float mg;
        gt_logit(a, row, s, mg);
        const bool on = a.tau != nullptr && mg != 0.f;
        sh_row[t] = row;
        row_of[p0 + t] = row;
        sh_p[0][t] = w * g;
        sh_p[1][t] = on ? (double)s * w * g : 0.0;
        sh_p[2][t] = on ? (double)s * w : 0.0;
    }
    __syncthreads();
    if (t < m && (t == 0 || sh_row[t - 1] != sh_row[t])) {
        const int row = sh_row[t];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int j = t; j < m && sh_row[j] == row; ++j) { s0 += sh_p[0][j]; s1 += sh_p[1][j]; s2 += sh_p[2][j]; }
        double* dst = a.row_off[row] < p0 ? chunk_part + (size_t)blockIdx.x * 3 : row_part + (size_t)row * 3;
        dst[0] = s0; dst[1] = s1; dst[2] = s2;
    }
}

// per row: c_r (left in the row's first slot) and d tau_r; an empty row has c = 0, d tau = 0
__global__ __launch_bounds__(256) void graph_attend_bwd_rows_kernel(GtArgs a, double* __restrict__ row_part, const double* __restrict__ chunk_part,
                                                                     float* __restrict__ d_tau) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_rows) return;
    const long long lo = gt_clamp(a.row_off[r], a.E), hi = gt_clamp(a.row_off[r + 1], a.E);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (hi > lo) {
        s0 = row_part[(size_t)r * 3]; s1 = row_part[(size_t)r * 3 + 1]; s2 = row_part[(size_t)r * 3 + 2];
        for (long long c = lo / GA_SEG + 1; c <= (hi - 1) / GA_SEG; ++c) {
            s0 += chunk_part[c * 3]; s1 += chunk_part[c * 3 + 1]; s2 += chunk_part[c * 3 + 2];
        }
    }
    row_part[(size_t)r * 3] = s0;
    if (d_tau != nullptr) d_tau[r] = (float)(-(double)a.scale * (s1 - s0 * s2));
}

__global__ __launch_bounds__(256) void graph_attend_dscore_kernel(GtArgs a, const float* __restrict__ score, const float* __restrict__ weight,
                                                                   const float* __restrict__ dweight, const int32_t* __restrict__ row_of,
                                                                   const double* __restrict__ row_part, float* __restrict__ dscore) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.E) return;
    const int row = row_of[e];
    const float s = score[e];
    float mg;
    gt_logit(a, row, s, mg);
    const bool on = mg != 0.f && (unsigned)a.key[e] < (unsigned)a.N;
    const float slope = a.tau != nullptr ? mg + s : 1.f;
    const float dev = (float)((double)dweight[e] - row_part[(size_t)row * 3]);
    dscore[e] = on ? a.scale * slope * weight[e] * dev : 0.f;
}

// out[row] = sum over the row's edges of weight[e] src[source row of e]: graph_apply_segment_kernel<false> with 49 float4 per row, a
// wave per chunk.  L > 0: rows are queries, source row = (row / L) N + key with key in [0, N);  L = 0: source row = key in [0, n_key)
struct GtProduct {
    const int64_t* row_off; int n_rows;
    const int32_t* key; const float* weight; const int32_t* perm /* NULL: weight[e] */;
    long long E;
    const float* src; int n_key; int L, N;
    float* out;                               // [n_rows, 196]
    float* part;                              // [chunks, 196]
};

__global__ __launch_bounds__(64) void graph_attend_product_kernel(GtProduct a) {
    __shared__ long long sh_of[GA_SEG];
    __shared__ float sh_w[GA_SEG];
    __shared__ int sh_row[GA_SEG];
    const int t = threadIdx.x;
    const auto [p0, m] = ga_segment(a.E);
    for (int i = t; i < m; i += 64) {
        const long long p = p0 + i;
        const int row = ga_row_of(a.row_off, a.n_rows, p);
        const int key = a.key[p];
        long long of = -1;
        if (a.L > 0) of = gt_feature_row(a.L, a.N, row, key);
        else if ((unsigned)key < (unsigned)a.n_key) of = (long long)key * GT_C4;
        long long wi = p;
        if (a.perm != nullptr) {
            wi = a.perm[p];
            if (wi < 0 || wi >= a.E) of = -1;
        }
        sh_of[i] = of;
        sh_w[i] = of >= 0 ? a.weight[wi] : 0.f;
        sh_row[i] = row;
    }
    __syncthreads();
    const float4* src = reinterpret_cast<const float4*>(a.src) + (t < GT_C4 ? t : GT_C4 - 1);
    int e = 0;
    while (e < m) {
        const int cur = sh_row[e];
        int end = e + 1;
        while (end < m && sh_row[end] == cur) ++end;
        const float4 acc = ga_gather_run(src, sh_of, sh_w, e, end);
        // a run that came in from an earlier chunk (only the first can) leaves this chunk's partial row, any other starts its row
        const bool head = a.row_off[cur] < p0;
        float4* dst = reinterpret_cast<float4*>(head ? a.part + (size_t)blockIdx.x * D : a.out + (size_t)cur * D);
        if (t < GT_C4) dst[t] = acc;
        e = end;
    }
}

// per row: nothing (the row lies inside one chunk), zeros (an empty row), or its start + the partials of the chunks it crosses, in
// chunk order
__global__ __launch_bounds__(64) void graph_attend_combine_kernel(const int64_t* __restrict__ row_off, long long E,
                                                                   const float* __restrict__ part, float* __restrict__ out) {
    const int t = threadIdx.x;
    if (t >= GT_C4) return;
    const long long lo = gt_clamp(row_off[blockIdx.x], E), hi = gt_clamp(row_off[blockIdx.x + 1], E);
    float4* o = reinterpret_cast<float4*>(out + (size_t)blockIdx.x * D);
    if (hi <= lo) {
        o[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const long long c0 = lo / GA_SEG, c1 = (hi - 1) / GA_SEG;
    if (c0 == c1) return;
    const float4* pp = reinterpret_cast<const float4*>(part);
    float4 s = o[t];
#pragma unroll 4
    for (long long c = c0 + 1; c <= c1; ++c) {
        const float4 h = pp[(size_t)c * GT_C4 + t];
        s.x += h.x; s.y += h.y; s.z += h.z; s.w += h.w;
    }
    o[t] = s;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// forward: the row of every edge, a (max, sum) slot per row and per chunk;  backward: the rows, d S, three sums per row and per chunk,
// the products' partial rows.  The one walk behind the sizes (null base) and both launches
struct GtWs { int32_t* row_of; GfStats st; float* dscore; double* row_part; double* chunk_part; float* part; size_t bytes; };
static GtWs gt_carve(void* ws, int B, const Grid& g, int64_t E, bool backward) {
    Carver cv(ws);
    GtWs w{};
    const size_t rows = (size_t)B * g.L, chunks = ga_chunks(E) + 1;
    w.row_of = cv.take<int32_t>((size_t)E + 1);
    if (!backward) {
        w.st = carve_stats(cv, rows, chunks);
    } else {
        w.dscore = cv.take<float>((size_t)E + 1);
        w.row_part = cv.take<double>(rows * 3);
        w.chunk_part = cv.take<double>(chunks * 3);
        w.part = cv.take<float>(chunks * D);
    }
    w.bytes = cv.bytes();
    return w;
}
static size_t graph_attend_workspace_bytes(int B, const Grid& g, int64_t E, bool backward) { return gt_carve(nullptr, B, g, E, backward).bytes; }

static int launch_graph_attend(hipStream_t s, int B, const Grid& g, const GraphAttendCall& c, float* score, float* weight, void* workspace) {
    if (c.E == 0) return DAGL_OK;
    const GtWs w = gt_carve(workspace, B, g, c.E, false);
    const GtArgs a = gt_args(B, g, c);
    hipLaunchKernelGGL(graph_attend_score_kernel, dim3((unsigned)ga_chunks(c.E)), dim3(256), 0, s, a, score, w.row_of, w.st.row_max, w.st.row_sum,
                       w.st.chunk_max, w.st.chunk_sum);
    DAGL_LAUNCH_CHECK("graph_attend_score_kernel");
    hipLaunchKernelGGL(graph_attend_rows_kernel, dim3((unsigned)((a.n_rows + 255) / 256)), dim3(256), 0, s, a, w.st.row_max, w.st.row_sum,
                       w.st.chunk_max, w.st.chunk_sum);
    DAGL_LAUNCH_CHECK("graph_attend_rows_kernel");
    hipLaunchKernelGGL(graph_attend_weight_kernel, dim3((unsigned)((c.E + 255) / 256)), dim3(256), 0, s, a, score, w.row_of, w.st.row_max,
                       w.st.row_sum, weight);
    DAGL_LAUNCH_CHECK("graph_attend_weight_kernel");
    return DAGL_OK;
}

static int gt_product(hipStream_t s, const GtProduct& p) {
    if (p.E > 0) {
        hipLaunchKernelGGL(graph_attend_product_kernel, dim3((unsigned)ga_chunks(p.E)), dim3(64), 0, s, p);
        DAGL_LAUNCH_CHECK("graph_attend_product_kernel");
    }
    hipLaunchKernelGGL(graph_attend_combine_kernel, dim3((unsigned)p.n_rows), dim3(64), 0, s, p.row_off, p.E, p.part, p.out);
    DAGL_LAUNCH_CHECK("graph_attend_combine_kernel");
    return DAGL_OK;
}

static int launch_graph_attend_backward(hipStream_t s, int B, const Grid& g, const GraphAttendCall& c, const float* score,
                                        const float* weight, const float* d_weight, const int64_t* col_off, const int32_t* src_row,
                                        const int32_t* perm, float* d_wq_rows /* or null */, float* d_x_rows /* or null */,
                                        float* d_tau /* or null */, void* workspace) {
    const GtWs w = gt_carve(workspace, B, g, c.E, true);
    const GtArgs a = gt_args(B, g, c);
    if (c.E > 0) {
        hipLaunchKernelGGL(graph_attend_bwd_partial_kernel, dim3((unsigned)ga_chunks(c.E)), dim3(GA_SEG), 0, s, a, score, weight, d_weight,
                           w.row_of, w.row_part, w.chunk_part);
        DAGL_LAUNCH_CHECK("graph_attend_bwd_partial_kernel");
    }
    if (c.E > 0 || d_tau != nullptr) {
        hipLaunchKernelGGL(graph_attend_bwd_rows_kernel, dim3((unsigned)((a.n_rows + 255) / 256)), dim3(256), 0, s, a, w.row_part,
                           w.chunk_part, d_tau);
        DAGL_LAUNCH_CHECK("graph_attend_bwd_rows_kernel");
    }
    if (c.E > 0 && (d_wq_rows != nullptr || d_x_rows != nullptr)) {
        hipLaunchKernelGGL(graph_attend_dscore_kernel, dim3((unsigned)((c.E + 255) / 256)), dim3(256), 0, s, a, score, weight, d_weight,
                           w.row_of, w.row_part, w.dscore);
        DAGL_LAUNCH_CHECK("graph_attend_dscore_kernel");
    }
    int rc;
    if (d_wq_rows != nullptr) {
        // d Wq[r] = sum over the row's edges of d S_e X[b N + key_e]
        GtProduct p{};
        p.row_off = c.row_off; p.n_rows = B * g.L; p.key = c.key; p.weight = w.dscore; p.perm = nullptr; p.E = c.E;
        p.src = c.x_rows; p.n_key = g.N; p.L = g.L; p.N = g.N; p.out = d_wq_rows; p.part = w.part;
        if ((rc = gt_product(s, p))) return rc;
    }
    if (d_x_rows != nullptr) {
        // d X[b N + j] = sum over the column's edges of d S_e Wq[row(e)]: the same product over the transposed CSR
        GtProduct p{};
        p.row_off = col_off; p.n_rows = B * g.N; p.key = src_row; p.weight = w.dscore; p.perm = perm; p.E = c.E;
        p.src = c.wq_rows; p.n_key = B * g.L; p.L = 0; p.N = 0; p.out = d_x_rows; p.part = w.part;
        if ((rc = gt_product(s, p))) return rc;
    }
    return DAGL_OK;
}

static size_t graph_attend_bytes(const char* who, int B, int H, int W, int64_t total_edges, bool backward) {
    if (graph_shape_ok(who, B, H, W, total_edges)) return 0;
    return graph_attend_workspace_bytes(B, make_grid(H, W), total_edges, backward);
}

}  // namespace dagl

using namespace dagl;

extern "C" {

// (ABI 412) attention on a given patch graph
size_t dagl_graph_attend_workspace_bytes(int B, int H, int W, int64_t total_edges) {
    return graph_attend_bytes("dagl_graph_attend_workspace_bytes", B, H, W, total_edges, false);
}

size_t dagl_graph_attend_backward_workspace_bytes(int B, int H, int W, int64_t total_edges) {
    return graph_attend_bytes("dagl_graph_attend_backward_workspace_bytes", B, H, W, total_edges, true);
}

int dagl_graph_attend(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const int64_t* row_off,
                      const int32_t* key, int64_t total_edges, const float* tau, float scale, int flags, float* score, float* weight,
                      void* workspace, size_t ws_bytes) {
    const char* who = "dagl_graph_attend";
    int rc = graph_shape_ok(who, B, H, W, total_edges);
    if (rc || (rc = graph_operands_ok(who, wq_rows, x_rows, row_off, key, total_edges, scale, flags))) return rc;
    DAGL_REQUIRE(total_edges == 0 || (score && weight), "dagl_graph_attend: null tensor pointer");
    const Grid g = make_grid(H, W);
    if ((rc = check_workspace(who, workspace, ws_bytes, graph_attend_workspace_bytes(B, g, total_edges, false)))) return rc;
    const GraphAttendCall c = graph_attend_call(wq_rows, x_rows, row_off, key, total_edges, tau, scale, flags);
    return launch_graph_attend((hipStream_t)stream, B, g, c, score, weight, workspace);
}

int dagl_graph_attend_backward(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const int64_t* row_off,
                               const int32_t* key, int64_t total_edges, const float* tau, float scale, int flags, const float* score,
                               const float* weight, const float* d_weight, const int64_t* col_off, const int32_t* src_row,
                               const int32_t* perm, float* d_wq_rows, float* d_x_rows, float* d_tau, void* workspace, size_t ws_bytes) {
    const char* who = "dagl_graph_attend_backward";
    int rc = graph_shape_ok(who, B, H, W, total_edges);
    if (rc || (rc = graph_operands_ok(who, wq_rows, x_rows, row_off, key, total_edges, scale, flags))) return rc;
    DAGL_REQUIRE(total_edges == 0 || (score && weight && d_weight), "dagl_graph_attend_backward: null tensor pointer");
    DAGL_REQUIRE(d_x_rows == nullptr || (col_off && (total_edges == 0 || (src_row && perm))),
                 "dagl_graph_attend_backward: null transposed CSR (col_off, src_row, perm are required with d_x_rows)");
    DAGL_REQUIRE(d_tau == nullptr || tau != nullptr, "dagl_graph_attend_backward: d_tau asked for without tau");
    DAGL_REQUIRE(((uintptr_t)d_wq_rows % 16) == 0 && ((uintptr_t)d_x_rows % 16) == 0,
                 "dagl_graph_attend_backward: gradient rows must be 16-byte aligned");
    const Grid g = make_grid(H, W);
    if ((rc = check_workspace(who, workspace, ws_bytes, graph_attend_workspace_bytes(B, g, total_edges, true)))) return rc;
    const GraphAttendCall c = graph_attend_call(wq_rows, x_rows, row_off, key, total_edges, tau, scale, flags);
    return launch_graph_attend_backward((hipStream_t)stream, B, g, c, score, weight, d_weight, col_off, src_row, perm, d_wq_rows, d_x_rows,
                                        d_tau, workspace);
}

}  // extern "C"
