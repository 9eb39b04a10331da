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
//
// Training (dagl_graph_forward_train / dagl_graph_forward_backward): the forward above, unchanged, plus one launch that leaves (M, D) per
// row -- twelve bytes a row are all that is kept between forward and backward --, and a backward that recomputes S_e, w_e and
// g_e = <dAgg[r], V[key_e]> in one crossing of the edges: the kernels and their order are written out in front of the backward below.
//
// A whole CES stage (dagl_graph_stage_forward): the kernels take the image of a row as row / L and the image of a key's features as
// (row / L) N + key, and a stage's graph is one CSR over 4 B head-major images -- with B' = 4 B and the four heads' operands stacked
// head-major they serve the stage unchanged; the entry stops at the aggregated rows and ends in launch_stage_fold_mix (aggregate.hip).
// Its backward starts in stage_mix_grad.hip and continues in dagl_graph_forward_backward with B' = 4 B.
#include "dagl_common.h"
#include "graph_rows.h"

namespace dagl {

int launch_fold_patches(hipStream_t s, int B, int Hp, int Wp, int C, int k, int stride, int oy, int ox, int oh, int ow, const float* drows,
                        float* dmap);

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

// ---- training: the row statistics the backward starts from --------------------------------------------------------------------------
// per row: the (M, D) graph_forward_combine_kernel forms out of the same slots, in its order and with its expressions, left in arrays of
// their own (the combine kernel and its launch stay as they are).  Empty rows: 0 and 1, never read
__global__ __launch_bounds__(256) void graph_forward_row_stats_kernel(GtArgs a, GfStats st, float* __restrict__ row_max_out,
                                                                       double* __restrict__ row_sum_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n_rows) return;
    const long long lo = gt_clamp(a.row_off[r], a.E), hi = gt_clamp(a.row_off[r + 1], a.E);
    if (hi <= lo) {
        row_max_out[r] = 0.f;
        row_sum_out[r] = 1.0;
        return;
    }
    const long long deg = hi - lo, c0 = lo / GA_SEG, c1 = (hi - 1) / GA_SEG;
    const bool off_graph = !a.edges_only && deg < a.N;
    const float m0 = st.row_max[r];
    float M = off_graph ? fmaxf(m0, 0.f) : m0;
    for (long long c = c0 + 1; c <= c1; ++c) M = fmaxf(M, st.chunk_max[c]);
    const double sc0 = exp((double)m0 - (double)M);
    double sum = st.row_sum[r] * sc0;
    for (long long c = c0 + 1; c <= c1; ++c) {
        const double sc = exp((double)st.chunk_max[c] - (double)M);
        sum += st.chunk_sum[c] * sc;
    }
    if (off_graph) sum += (double)(a.N - deg) * exp(-(double)M);
    row_max_out[r] = M;
    row_sum_out[r] = sum;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// The gradients of the route from (M, D) per row alone -- no per-edge array outlives the forward.  With dAgg = unfold(d_out / cnt):
//   g_e = <dAgg[r], V[key_e]>,  c_r = sum_e w_e g_e,  d S_e = on_e scale slope_e w_e (g_e - c_r)  (slope_e = m_e + S_e with tau, else 1)
//   d tau_r = -scale sum_on S_e w_e (g_e - c_r),  d Wq = CSR x X rows,  d X = transposed CSR x Wq rows,  d V = transposed CSR x dAgg rows
//   edge kernel     the ONE crossing of the edges that gathers: per segment the scores again (gt_edge_dot and gt_logit as the forward
//                   ran them: the same bits of z under the forward's M), w_e from the saved (M, D), g_e from the map and dAgg (a wave
//                   per edge), S / w / g of every edge into the call's scratch and per run of equal row the fp64 sums
//                   sum w g, sum_on S w g, sum_on S w in edge order (row and segment slots as the statistics')
//   rows kernel     c_r and d tau_r over the slots of the segments a row crosses, in segment order
//   products        segment + combine as graph_attend_product_kernel: d S_e is formed where a segment is staged, out of the scratch
//                   and c_r; d V rows are folded into the map as dagl_graph_apply_backward folds them
// Any subset of the outputs carries the bits of the full call: every product has its own launches and reads the same scratch.
struct GfEdge { float* s; float* w; float* g; };              // [E] each: S_e, w_e (0 on edges that are off or off the map), g_e

__global__ __launch_bounds__(256) void graph_forward_bwd_edge_kernel(GtArgs a, GaArgs v, const float* __restrict__ row_max,
                                                                      const double* __restrict__ row_sum, const float* __restrict__ dagg,
                                                                      GfEdge ed, double* __restrict__ row_part, double* __restrict__ chunk_part) {
    __shared__ long long sh_x[GA_SEG];        // float4 offset of the key's feature row, -1 = key out of range
    __shared__ long long sh_of[GA_SEG];       // float4 offset of the key's patch in the map, -1 = no value row
    __shared__ int sh_row[GA_SEG];
    __shared__ float sh_s[GA_SEG];
    __shared__ float sh_g[GA_SEG];
    __shared__ double sh_p[3][GA_SEG];
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
    {   // the scores: an edge per 16 lanes, as graph_forward_segment_kernel
        const int l = t & 15, grp = t >> 4;
        const float4* wq = reinterpret_cast<const float4*>(a.wq);
        const float4* xk = reinterpret_cast<const float4*>(a.x);
        for (int e = grp; e < m; e += 16) {
            const long long of = sh_x[e];
            const float acc = gt_edge_dot(wq + (size_t)sh_row[e] * GT_C4, xk + (of >= 0 ? of : 0), l);
            if (l == 0) sh_s[e] = of >= 0 ? acc : 0.f;
        }
    }
    {   // g_e: a wave per edge, lane = float4 columns lane + 64 u of the patch and of the row of dAgg (graph_apply_dweight_kernel)
        const int lane = t & 63, w = t >> 6;
        int voff[4], col[4]; bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ok[u] = lane + 64 * u < GA_C4;
            col[u] = ok[u] ? lane + 64 * u : GA_C4 - 1;
            voff[u] = (col[u] / 28) * v.Wp * (CH / 4) + col[u] % 28;
        }
        const float4* vm = reinterpret_cast<const float4*>(v.src);
        const float4* dg = reinterpret_cast<const float4*>(dagg);
        // (one edge per step: two per step, as graph_apply_dweight_kernel takes them, cost 18 registers here and moved no timing, §7)
        for (int e = w; e < m; e += 4) {
            const long long of = sh_of[e];
            const float4* vj = vm + (of >= 0 ? of : 0);
            const float4* dr = dg + (size_t)sh_row[e] * GA_C4;
            float4 pv[4], pd[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { pv[u] = vj[voff[u]]; pd[u] = dr[col[u]]; }
            float acc = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float s = pd[u].x * pv[u].x + pd[u].y * pv[u].y + pd[u].z * pv[u].z + pd[u].w * pv[u].w;
                acc += ok[u] ? s : 0.f;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) sh_g[e] = of >= 0 ? acc : 0.f;
        }
    }
    __syncthreads();
    if (t < m) {
        const int row = sh_row[t];
        const float s = sh_s[t], g = sh_g[t];
        float mg;
        const float z = gt_logit(a, row, s, mg);
        const bool live = mg != 0.f && sh_x[t] >= 0;
        const float w = live ? (float)((double)expf(z - row_max[row]) / row_sum[row]) : 0.f;
        ed.s[p0 + t] = s; ed.w[p0 + t] = w; ed.g[p0 + t] = g;
        const bool on = a.tau != nullptr && mg != 0.f;
        const double wd = w, gd = g;
        sh_p[0][t] = wd * gd;
        sh_p[1][t] = on ? (double)s * wd * gd : 0.0;
        sh_p[2][t] = on ? (double)s * wd : 0.0;
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
__global__ __launch_bounds__(256) void graph_forward_bwd_rows_kernel(GtArgs a, double* __restrict__ row_part, const double* __restrict__ chunk_part,
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

// d S of edge e of query row `row` (both in range), out of the scratch and the row's c
__device__ __forceinline__ float gf_dscore(const GtArgs& a, const GfEdge& ed, const double* __restrict__ row_part, int row, long long e) {
    const float w = ed.w[e];
    if (w == 0.f) return 0.f;                                  // off, off the map, or a weight that underflowed: nothing either way
    const float s = ed.s[e];
    float mg;
    gt_logit(a, row, s, mg);
    const float slope = a.tau != nullptr ? mg + s : 1.f;
    const float dev = (float)((double)ed.g[e] - row_part[(size_t)row * 3]);
    return a.scale * slope * w * dev;
}

// the three products.  out[row] = sum over the row's edges of weight_e src[source row of e], C4 float4 per row:
//   GF_DWQ  rows = the CSR's queries, source = x_rows[b N + key], weight = d S_e
//   GF_DX   rows = the transposed CSR's keys, source = wq_rows[src_row], weight = d S of edge perm[p]
//   GF_DV   rows = the transposed CSR's keys, source = dAgg[src_row] (784 floats), weight = w of edge perm[p]
// A key, source row or perm entry outside its range is tested before an address is formed and contributes nothing.
enum { GF_DWQ = 0, GF_DX = 1, GF_DV = 2 };
struct GfProduct {
    const int64_t* row_off; int n_rows;       // CSR or transposed CSR offsets [n_rows + 1]
    const int32_t* key; const int32_t* perm;  // key / src_row [E]; perm [E] (transposed)
    const float* src;
    int n_query;                              // B L: the range of a transposed edge's source row
    float* out;                               // [n_rows, 4 C4]
    float* part;                              // [chunks, 4 C4]
};

template <int MODE>
__global__ __launch_bounds__(MODE == GF_DV ? 256 : 64) void graph_forward_bwd_product_kernel(GtArgs a, GfProduct p, GfEdge ed,
                                                                                            const double* __restrict__ row_part) {
    constexpr int C4 = MODE == GF_DV ? GA_C4 : GT_C4, BLOCK = MODE == GF_DV ? 256 : 64;
    __shared__ long long sh_of[GA_SEG];
    __shared__ float sh_w[GA_SEG];
    __shared__ int sh_row[GA_SEG];
    const int t = threadIdx.x;
    const auto [p0, m] = ga_segment(a.E);
    for (int i = t; i < m; i += BLOCK) {
        const long long q = p0 + i;
        const int row = ga_row_of(p.row_off, p.n_rows, q);
        const int key = p.key[q];
        long long of = -1;
        float w = 0.f;
        if (MODE == GF_DWQ) {
            of = gt_feature_row(a.L, a.N, row, key);
            if (of >= 0) w = gf_dscore(a, ed, row_part, row, q);
        } else {
            const long long e = p.perm[q];
            if ((unsigned)key < (unsigned)p.n_query && e >= 0 && e < a.E) {
                of = (long long)key * C4;
                w = MODE == GF_DX ? gf_dscore(a, ed, row_part, key, e) : ed.w[e];
            }
        }
        sh_of[i] = of;
        sh_w[i] = w;
        sh_row[i] = row;
    }
    __syncthreads();
    const float4* src = reinterpret_cast<const float4*>(p.src) + (t < C4 ? t : C4 - 1);
    int e = 0;
    while (e < m) {
        const int cur = sh_row[e];
        int end = e + 1;
        while (end < m && sh_row[end] == cur) ++end;
        const float4 acc = ga_gather_run(src, sh_of, sh_w, e, end);
        // a run that came in from an earlier segment (only the first can) leaves this segment's partial row, any other starts its row
        const bool head = p.row_off[cur] < p0;
        float4* dst = reinterpret_cast<float4*>(head ? p.part + (size_t)blockIdx.x * (4 * C4) : p.out + (size_t)cur * (4 * C4));
        if (t < C4) dst[t] = acc;
        e = end;
    }
}

// per row: nothing (the row lies inside one segment), zeros (an empty row), or its start + the partials of the segments it crosses, in
// segment order (graph_attend_combine_kernel at either width)
template <int C4>
__global__ __launch_bounds__(C4 > 64 ? 256 : 64) void graph_forward_bwd_combine_kernel(const int64_t* __restrict__ row_off, long long E,
                                                                                    const float* __restrict__ part, float* __restrict__ out) {
    const int t = threadIdx.x;
    if (t >= C4) return;
    const long long lo = gt_clamp(row_off[blockIdx.x], E), hi = gt_clamp(row_off[blockIdx.x + 1], E);
    float4* o = reinterpret_cast<float4*>(out + (size_t)blockIdx.x * (4 * C4));
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
        const float4 h = pp[(size_t)c * C4 + t];
        s.x += h.x; s.y += h.y; s.z += h.z; s.w += h.w;
    }
    o[t] = s;
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

// the forward up to its fold: the aggregated rows agg [B L, 784] are left in the workspace (gf_carve(...).agg).
// row_max_out / row_sum_out: the training forward's row statistics (both or neither); the forward's own launches are the same either way
static int launch_graph_forward_rows(hipStream_t s, int B, const Grid& g, const GraphAttendCall& c, const float* b2p, const GfWs& w,
                                     float* row_max_out = nullptr, double* row_sum_out = nullptr) {
    const GtArgs a = gt_args(B, g, c);
    GaArgs v = ga_map_args(B, g, b2p, c.row_off, c.key, nullptr, c.E);
    v.out = w.agg; v.part = w.part;
    if (c.E > 0) {
        hipLaunchKernelGGL(graph_forward_segment_kernel, dim3((unsigned)ga_chunks(c.E)), dim3(256), 0, s, a, v, w.st);
        DAGL_LAUNCH_CHECK("graph_forward_segment_kernel");
    }
    hipLaunchKernelGGL(graph_forward_combine_kernel, dim3((unsigned)a.n_rows), dim3(256), 0, s, a, w.st, w.part, w.agg);
    DAGL_LAUNCH_CHECK("graph_forward_combine_kernel");
    if (row_max_out != nullptr) {
        hipLaunchKernelGGL(graph_forward_row_stats_kernel, dim3((unsigned)((a.n_rows + 255) / 256)), dim3(256), 0, s, a, w.st, row_max_out,
                           row_sum_out);
        DAGL_LAUNCH_CHECK("graph_forward_row_stats_kernel");
    }
    return DAGL_OK;
}

static int launch_graph_forward(hipStream_t s, int B, const Grid& g, const GraphAttendCall& c, const float* b2p, float* out, void* workspace,
                                float* row_max_out = nullptr, double* row_sum_out = nullptr) {
    const GfWs w = gf_carve(workspace, B, g, c.E);
    const int rc = launch_graph_forward_rows(s, B, g, c, b2p, w, row_max_out, row_sum_out);
    return rc ? rc : launch_fold(s, B, g, w.agg, out);
}

// a whole CES stage on its frozen graph: the rows of the four heads as 4 B images (the kernels take the image of a row as row / L: the
// head-major operands [4, B, ...] ARE those of 4 B images), then the stage's fold + mix + residual on the rows.  cat_out (training, with
// the row statistics): the pre-mix concat map [4, B, 16, H, W] head-major, fold_kernel's bits -- what the fused kernel forms per pixel
static int launch_graph_stage_forward(hipStream_t s, int B, const Grid& g, const GraphAttendCall& c, const float* b2p4, const float* x,
                                      const float* mix_w, const float* mix_b, float* out, float* row_max_out, double* row_sum_out,
                                      float* cat_out, void* workspace) {
    const GfWs w = gf_carve(workspace, 4 * B, g, c.E);
    int rc = launch_graph_forward_rows(s, 4 * B, g, c, b2p4, w, row_max_out, row_sum_out);
    if (rc) return rc;
    if (cat_out != nullptr && (rc = launch_fold(s, 4 * B, g, w.agg, cat_out))) return rc;
    return launch_stage_fold_mix(s, B, g, w.agg, x, mix_w, mix_b, out);
}

// backward: dAgg [B L, 784], d V rows [B N, 784], the products' partial rows, S / w / g per edge, three sums per row and per segment
struct GfBwdWs { float* dagg; float* dv; float* part; GfEdge ed; double* row_part; double* chunk_part; size_t bytes; };
static GfBwdWs gf_bwd_carve(void* ws, int B, const Grid& g, int64_t E) {
    Carver cv(ws);
    GfBwdWs w{};
    const size_t rows = (size_t)B * g.L, chunks = ga_chunks(E) + 1;
    w.dagg = cv.take<float>(rows * P);
    w.dv = cv.take<float>((size_t)B * g.N * P);
    w.part = cv.take<float>(chunks * P);
    w.ed.s = cv.take<float>((size_t)E + 1);
    w.ed.w = cv.take<float>((size_t)E + 1);
    w.ed.g = cv.take<float>((size_t)E + 1);
    w.row_part = cv.take<double>(rows * 3);
    w.chunk_part = cv.take<double>(chunks * 3);
    w.bytes = cv.bytes();
    return w;
}
static size_t graph_forward_backward_workspace_bytes(int B, const Grid& g, int64_t E) { return gf_bwd_carve(nullptr, B, g, E).bytes; }

struct GfGrads { float* d_wq_rows; float* d_x_rows; float* d_tau; float* d_b2p; };     // each may be null: not computed

template <int MODE>
static int gf_product(hipStream_t s, const GtArgs& a, const GfProduct& p, const GfEdge& ed, const double* row_part) {
    constexpr int C4 = MODE == GF_DV ? GA_C4 : GT_C4, BLOCK = MODE == GF_DV ? 256 : 64;
    if (a.E > 0) {
        hipLaunchKernelGGL(graph_forward_bwd_product_kernel<MODE>, dim3((unsigned)ga_chunks(a.E)), dim3(BLOCK), 0, s, a, p, ed, row_part);
        DAGL_LAUNCH_CHECK("graph_forward_bwd_product_kernel");
    }
    hipLaunchKernelGGL(graph_forward_bwd_combine_kernel<C4>, dim3((unsigned)p.n_rows), dim3(BLOCK), 0, s, p.row_off, (long long)a.E, p.part,
                       p.out);
    DAGL_LAUNCH_CHECK("graph_forward_bwd_combine_kernel");
    return DAGL_OK;
}

static int launch_graph_forward_backward(hipStream_t s, int B, const Grid& g, const GraphAttendCall& c, const float* b2p, const float* row_max,
                                         const double* row_sum, const float* d_out, const int64_t* col_off, const int32_t* src_row,
                                         const int32_t* perm, const GfGrads& d, void* workspace) {
    const GfBwdWs w = gf_bwd_carve(workspace, B, g, c.E);
    const GtArgs a = gt_args(B, g, c);
    int rc;
    if (c.E > 0) {
        if ((rc = launch_unfold_dout(s, B, g, d_out, w.dagg))) return rc;
        const GaArgs v = ga_map_args(B, g, b2p, c.row_off, c.key, nullptr, c.E);
        hipLaunchKernelGGL(graph_forward_bwd_edge_kernel, dim3((unsigned)ga_chunks(c.E)), dim3(256), 0, s, a, v, row_max, row_sum, w.dagg, w.ed,
                           w.row_part, w.chunk_part);
        DAGL_LAUNCH_CHECK("graph_forward_bwd_edge_kernel");
    }
    if (c.E > 0 || d.d_tau != nullptr) {
        hipLaunchKernelGGL(graph_forward_bwd_rows_kernel, dim3((unsigned)((a.n_rows + 255) / 256)), dim3(256), 0, s, a, w.row_part, w.chunk_part,
                           d.d_tau);
        DAGL_LAUNCH_CHECK("graph_forward_bwd_rows_kernel");
    }
    if (d.d_wq_rows != nullptr) {
        GfProduct p{};
        p.row_off = c.row_off; p.n_rows = a.n_rows; p.key = c.key; p.perm = nullptr; p.src = c.x_rows; p.n_query = a.n_rows;
        p.out = d.d_wq_rows; p.part = w.part;
        if ((rc = gf_product<GF_DWQ>(s, a, p, w.ed, w.row_part))) return rc;
    }
    if (d.d_x_rows != nullptr) {
        GfProduct p{};
        p.row_off = col_off; p.n_rows = B * g.N; p.key = src_row; p.perm = perm; p.src = c.wq_rows; p.n_query = a.n_rows;
        p.out = d.d_x_rows; p.part = w.part;
        if ((rc = gf_product<GF_DX>(s, a, p, w.ed, w.row_part))) return rc;
    }
    if (d.d_b2p != nullptr) {
        GfProduct p{};
        p.row_off = col_off; p.n_rows = B * g.N; p.key = src_row; p.perm = perm; p.src = w.dagg; p.n_query = a.n_rows;
        p.out = w.dv; p.part = w.part;
        if ((rc = gf_product<GF_DV>(s, a, p, w.ed, w.row_part))) return rc;
        // d b2p = the stride-1 adjoint of unfold: every pixel of the padded map is written
        return launch_fold_patches(s, B, g.Hp, g.Wp, CH, KS, 1, 0, 0, g.H, g.W, w.dv, d.d_b2p);
    }
    return DAGL_OK;
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

// the same forward for training: `out` carries dagl_graph_forward's bits, (M, D) per row are left for dagl_graph_forward_backward
int dagl_graph_forward_train(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                             const int64_t* row_off, const int32_t* key, int64_t total_edges, const float* tau, float scale, int flags,
                             float* out, float* row_max_out, double* row_sum_out, void* workspace, size_t ws_bytes) {
    const char* who = "dagl_graph_forward_train";
    int rc = graph_shape_ok(who, B, H, W, total_edges);
    if (rc || (rc = graph_operands_ok(who, wq_rows, x_rows, row_off, key, total_edges, scale, flags, b2p && out && row_max_out && row_sum_out)))
        return rc;
    DAGL_REQUIRE(((uintptr_t)b2p % 16) == 0, "dagl_graph_forward_train: b2p must be 16-byte aligned");
    const Grid g = make_grid(H, W);
    if ((rc = check_workspace(who, workspace, ws_bytes, graph_forward_workspace_bytes(B, g, total_edges)))) return rc;
    const GraphAttendCall c = graph_attend_call(wq_rows, x_rows, row_off, key, total_edges, tau, scale, flags);
    return launch_graph_forward((hipStream_t)stream, B, g, c, b2p, out, workspace, row_max_out, row_sum_out);
}

size_t dagl_graph_forward_backward_workspace_bytes(int B, int H, int W, int64_t total_edges) {
    if (graph_shape_ok("dagl_graph_forward_backward_workspace_bytes", B, H, W, total_edges)) return 0;
    return graph_forward_backward_workspace_bytes(B, make_grid(H, W), total_edges);
}

int dagl_graph_forward_backward(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                                const int64_t* row_off, const int32_t* key, int64_t total_edges, const float* tau, float scale, int flags,
                                const float* row_max, const double* row_sum, const float* d_out, const int64_t* col_off,
                                const int32_t* src_row, const int32_t* perm, float* d_wq_rows, float* d_x_rows, float* d_tau, float* d_b2p,
                                void* workspace, size_t ws_bytes) {
    const char* who = "dagl_graph_forward_backward";
    int rc = graph_shape_ok(who, B, H, W, total_edges);
    if (rc || (rc = graph_operands_ok(who, wq_rows, x_rows, row_off, key, total_edges, scale, flags, b2p && row_max && row_sum && d_out)))
        return rc;
    DAGL_REQUIRE((d_x_rows == nullptr && d_b2p == nullptr) || (col_off && (total_edges == 0 || (src_row && perm))),
                 "dagl_graph_forward_backward: null transposed CSR (col_off, src_row, perm are required with d_x_rows and d_b2p)");
    DAGL_REQUIRE(d_tau == nullptr || tau != nullptr, "dagl_graph_forward_backward: d_tau asked for without tau");
    DAGL_REQUIRE(((uintptr_t)b2p % 16) == 0 && ((uintptr_t)d_b2p % 16) == 0, "dagl_graph_forward_backward: maps must be 16-byte aligned");
    DAGL_REQUIRE(((uintptr_t)d_wq_rows % 16) == 0 && ((uintptr_t)d_x_rows % 16) == 0,
                 "dagl_graph_forward_backward: gradient rows must be 16-byte aligned");
    const Grid g = make_grid(H, W);
    if ((rc = check_workspace(who, workspace, ws_bytes, graph_forward_backward_workspace_bytes(B, g, total_edges)))) return rc;
    const GraphAttendCall c = graph_attend_call(wq_rows, x_rows, row_off, key, total_edges, tau, scale, flags);
    return launch_graph_forward_backward((hipStream_t)stream, B, g, c, b2p, row_max, row_sum, d_out, col_off, src_row, perm,
                                         GfGrads{d_wq_rows, d_x_rows, d_tau, d_b2p}, workspace);
}

// a CES stage on its frozen graph, four heads in one launch set, ending in the fused fold + mix (no ABI bump: found by symbol)
static int graph_stage_shape_ok(const char* who, int B, int H, int W, int64_t total_edges) {
    int rc = graph_dims_ok(who, B, H, W);
    if (rc) return rc;
    DAGL_REQUIRE((int64_t)4 * B * H * W < (1ll << 30), "%s: batch too large for 32-bit row ids", who);
    return graph_shape_ok(who, 4 * B, H, W, total_edges);
}

size_t dagl_graph_stage_forward_workspace_bytes(int B, int H, int W, int64_t total_edges) {
    if (graph_stage_shape_ok("dagl_graph_stage_forward_workspace_bytes", B, H, W, total_edges)) return 0;
    return graph_forward_workspace_bytes(4 * B, make_grid(H, W), total_edges);
}

int dagl_graph_stage_forward(void* stream, int B, int H, int W, const float* wq_rows4, const float* x_rows4, const float* b2p4,
                             const int64_t* row_off, const int32_t* key, int64_t total_edges, const float* tau4, float scale, int flags,
                             const float* x, const float* mix_w, const float* mix_b, float* out, float* row_max_out, double* row_sum_out,
                             float* cat_out, void* workspace, size_t ws_bytes) {
    const char* who = "dagl_graph_stage_forward";
    int rc = graph_stage_shape_ok(who, B, H, W, total_edges);
    if (rc || (rc = graph_operands_ok(who, wq_rows4, x_rows4, row_off, key, total_edges, scale, flags, b2p4 != nullptr))) return rc;
    DAGL_REQUIRE(((uintptr_t)b2p4 % 16) == 0, "%s: b2p must be 16-byte aligned", who);
    DAGL_REQUIRE(x && mix_w && mix_b && out, "%s: null tensor pointer", who);
    const int training = (row_max_out != nullptr) + (row_sum_out != nullptr) + (cat_out != nullptr);
    DAGL_REQUIRE(training == 0 || training == 3, "%s: the training outputs come together (row_max_out, row_sum_out, cat_out: %d of 3 given)",
                 who, training);
    const Grid g = make_grid(H, W);
    if ((rc = check_workspace(who, workspace, ws_bytes, graph_forward_workspace_bytes(4 * B, g, total_edges)))) return rc;
    const GraphAttendCall c = graph_attend_call(wq_rows4, x_rows4, row_off, key, total_edges, tau4, scale, flags);
    return launch_graph_stage_forward((hipStream_t)stream, B, g, c, b2p4, x, mix_w, mix_b, out, row_max_out, row_sum_out, cat_out,
                                      workspace);
}

}  // extern "C"
