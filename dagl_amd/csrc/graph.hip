// Export of the learned patch graph as CSR (dagl_ce_graph_count / dagl_ce_graph_fill): for every query patch the keys with
// mask_b[i, j] != 0 and their weights A[i, j] = softmax(10 S m)[i, j] mask_b[i, j] -- the non-zeros of `yi`, dagl.py:256-261 (fixed-k
// variant: GReccR2b_3mh_1-checkpoint.py:242-250) -- which the forward paths never materialise.  A diagnostic path on the all-fp32 route
// (scan = "exact" / topk_wide.hip): fp32 map -> project.hip features -> row thresholds -> per chunk of query rows S = Wq X^T on
// gemm32_kernel, then per row
//   count  adaptive test with the row's mean * thr / bias; fixed-k modes: the k-th largest score by wide_radix_select (only passing keys
//          rank in the intersection mode); the degree, the largest logit, the softmax denominator over ALL keys (masked keys count
//          e^(0 - M)) as an fp64 sum in a fixed order
//   scan   exclusive scan of the B L degrees into int64 row offsets (row_scan_kernel, select.hip)
//   fill   ordered compaction of the passing keys (wave / block prefix scans, no atomics: the same arrays on every call), ties at the
//          k-th place to the lower key index as in wide_attend_kernel; key, weight and optionally score in key order.
// Count and fill see the same scores because fill RECOMPUTES each chunk with the same product: an element of gemm32_kernel is one fmaf
// chain over k whatever tile it sits in, so the scores do not depend on the chunk height either.  Keeping them would need
// L x N floats (1 GiB per image at 256^2) between two calls the host sits between.
#include <string.h>

#include "dagl_common.h"
#include "wide_select.h"

namespace dagl {

constexpr int GR_THREADS = 256;
constexpr int GR_UB = 4;                             // float4 loads in flight per thread (one in flight cost dense_train's row kernels a third)
constexpr int GR_TILE = GR_THREADS * 4;              // keys per block step
constexpr unsigned GR_ALL_TIES = 0x7fffffffu;

struct GraphArgs {
    int N, L, mode, k;
    int b, r0, R;                                    // image, first query and number of queries of the chunk
    const float* scores; long long ldn;              // [R, ldn]
    const float* mt; const float* bs;                // [B, L] mean * thr, bias (adaptive modes)
    int32_t* deg; uint2* sel; double* row_m; double* row_z;     // [B L]: degree, {threshold key, ties taken}, largest logit, denominator
    const int64_t* row_off; long long n_rows;        // [B L + 1]
    int32_t* key; float* weight; float* score;       // [E]; score may be null
    long long capacity;
};

// logit of a kept key: 10 S m with m = relu(S - mean thr + bias) as the mask saw it (fp32), m = 1 in the fixed-k mode -- in fp64, unlike the
// fp32 forms of wide_select.h
__device__ __forceinline__ double graph_logit(float s, bool adaptive, float mtq, float bsq) {
    const double m = adaptive ? (double)((s - mtq) + bsq) : 1.0;
    return (double)SOFTMAX_SCALE * (double)s * m;
}

// every thread: f(j, S[j]) for its keys j, ascending; GR_UB float4 loads in flight (rows are padded to 32 floats)
template <class F>
__device__ __forceinline__ void graph_row_walk(const float* __restrict__ row, int N, F&& f) {
    const int tid = threadIdx.x;
    for (int c0 = 0; c0 < N; c0 += GR_TILE * GR_UB) {
        float4 v[GR_UB];
#pragma unroll
        for (int u = 0; u < GR_UB; ++u) {
            const int j = c0 + u * GR_TILE + 4 * tid;
            v[u] = *reinterpret_cast<const float4*>(row + (j < N ? j : 0));
        }
#pragma unroll
        for (int u = 0; u < GR_UB; ++u) {
            const int j = c0 + u * GR_TILE + 4 * tid;
            const float sc[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) if (j + q < N) f(j + q, sc[q]);
        }
    }
}

struct GraphCountShared {
    WideSelShared sel;
    double dred[GR_THREADS];
    int ired[2][GR_THREADS / 64];
};

// (an LDS tree over all the threads: another association, so other bits, than block_sum_f64 / block_max_f32 of dagl_common.h)
__device__ __forceinline__ double graph_block_sum(double v, double* dred) {      // fixed tree: the same sum on every run
    const int tid = threadIdx.x;
    dred[tid] = v;
    __syncthreads();
    for (int st = GR_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) dred[tid] += dred[tid + st];
        __syncthreads();
    }
    const double r = dred[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double graph_block_max(double v, double* dred) {
    const int tid = threadIdx.x;
    dred[tid] = v;
    __syncthreads();
    for (int st = GR_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) dred[tid] = fmax(dred[tid], dred[tid + st]);
        __syncthreads();
    }
    const double r = dred[0];
    __syncthreads();
    return r;
}

// block = one score row
__global__ __launch_bounds__(GR_THREADS) void graph_row_count_kernel(GraphArgs a) {
    __shared__ GraphCountShared sh;
    const int slot = blockIdx.x, tid = threadIdx.x, w = tid >> 6;
    const size_t ql = (size_t)a.b * a.L + a.r0 + slot;
    const float* __restrict__ row = a.scores + (size_t)slot * a.ldn;
    const bool adaptive = a.mode != DAGL_MODE_TOPK;
    const float mtq = adaptive ? a.mt[ql] : 0.f, bsq = adaptive ? a.bs[ql] : 0.f;
    const int N = a.N;
    // a key passes when its sort key (0 = fails the adaptive test) lies above T, or AT T among the first `need` such keys;
    // without a k (or k >= N) T = 0: every candidate
    unsigned T = 0u, need = 0u;
    if (a.mode != DAGL_MODE_ADAPTIVE && a.k < N) {
        unsigned bin_count;
        wide_radix_select(row, N, a.k, adaptive, mtq, bsq, sh.sel, T, need, bin_count);
        if (need >= bin_count) need = GR_ALL_TIES;
    }
    int n_gt = 0, n_eq = 0;
    double m_gt = -1.0;                              // (logits of kept keys are >= 0)
    graph_row_walk(row, N, [&](int, float s) {
        const unsigned key = wide_key(s, adaptive, mtq, bsq);
        if (key > T) { ++n_gt; m_gt = fmax(m_gt, graph_logit(s, adaptive, mtq, bsq)); }
        else if (key == T && key != 0u) ++n_eq;
    });
    n_gt = wave_sum_i32(n_gt); n_eq = wave_sum_i32(n_eq);
    if ((tid & 63) == 0) { sh.ired[0][w] = n_gt; sh.ired[1][w] = n_eq; }
    __syncthreads();
    n_gt = sh.ired[0][0] + sh.ired[0][1] + sh.ired[0][2] + sh.ired[0][3];
    n_eq = sh.ired[1][0] + sh.ired[1][1] + sh.ired[1][2] + sh.ired[1][3];
    const int ties = (int)min((unsigned)n_eq, need);
    const int deg = n_gt + ties;
    // the tied keys share one score, hence one logit
    const double l_tie = ties > 0 ? graph_logit(__uint_as_float(T - 1u), adaptive, mtq, bsq) : -1.0;
    double M = fmax(graph_block_max(m_gt, sh.dred), l_tie);
    if (deg < N) M = fmax(M, 0.0);                   // masked keys: logit 0
    double z = 0.0;
    graph_row_walk(row, N, [&](int, float s) {
        if (wide_key(s, adaptive, mtq, bsq) > T) z += exp(graph_logit(s, adaptive, mtq, bsq) - M);
    });
    z = graph_block_sum(z, sh.dred);
    if (tid == 0) {
        if (ties > 0) z += (double)ties * exp(l_tie - M);
        z += (double)(N - deg) * exp(-M);
        a.deg[ql] = deg; a.sel[ql] = make_uint2(T, need); a.row_m[ql] = M; a.row_z[ql] = z;
    }
}

// block = one score row: the passing keys in key order at the row's offset
__global__ __launch_bounds__(GR_THREADS) void graph_row_fill_kernel(GraphArgs a) {
    __shared__ int sh_pass[2][GR_THREADS / 64], sh_eq[2][GR_THREADS / 64];
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t ql = (size_t)a.b * a.L + a.r0 + slot;
    if (a.row_off[a.n_rows] > a.capacity) return;    // (block-uniform) never a partial write
    const int deg = a.deg[ql];
    if (deg == 0) return;
    const float* __restrict__ row = a.scores + (size_t)slot * a.ldn;
    const bool adaptive = a.mode != DAGL_MODE_TOPK;
    const float mtq = adaptive ? a.mt[ql] : 0.f, bsq = adaptive ? a.bs[ql] : 0.f;
    const int N = a.N;
    const uint2 sel = a.sel[ql];
    const unsigned T = sel.x, need = sel.y;
    const bool ranked = need != GR_ALL_TIES && need != 0u;          // a tie at the k-th place: the `need` lowest key indices win
    const double M = a.row_m[ql], inv_z = 1.0 / a.row_z[ql];
    const int64_t base = a.row_off[ql];
    int run = 0, eq_run = 0, par = 0;
    for (int c0 = 0; c0 < N; c0 += GR_TILE * GR_UB) {
        float4 v[GR_UB];
#pragma unroll
        for (int u = 0; u < GR_UB; ++u) {
            const int j = c0 + u * GR_TILE + 4 * tid;
            v[u] = *reinterpret_cast<const float4*>(row + (j < N ? j : 0));
        }
#pragma unroll
        for (int u = 0; u < GR_UB; ++u) {
            const int j = c0 + u * GR_TILE + 4 * tid;
            if (c0 + u * GR_TILE >= N) break;                       // (block-uniform)
            const float sc[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            unsigned key[4]; bool eq[4], ps[4];
            int n_eq = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                key[q] = j + q < N ? wide_key(sc[q], adaptive, mtq, bsq) : 0u;
                eq[q] = key[q] == T && key[q] != 0u;
                n_eq += eq[q] ? 1 : 0;
            }
            int rank = 0;
            if (ranked) {                                           // (block-uniform) rank of the tied keys in key order
                const int incl = wave_scan_incl_i32(n_eq);
                if (lane == 63) sh_eq[par][w] = incl;
                __syncthreads();
                rank = eq_run + incl - n_eq;
#pragma unroll
                for (int ww = 0; ww < GR_THREADS / 64; ++ww) { const int t = sh_eq[par][ww]; if (ww < w) rank += t; eq_run += t; }
            }
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ps[q] = key[q] > T || (eq[q] && (need == GR_ALL_TIES || (unsigned)rank < need));
                if (eq[q]) ++rank;
                cnt += ps[q] ? 1 : 0;
            }
            const int incl = wave_scan_incl_i32(cnt);
            if (lane == 63) sh_pass[par][w] = incl;
            __syncthreads();
            int pos = run + incl - cnt;
#pragma unroll
            for (int ww = 0; ww < GR_THREADS / 64; ++ww) { const int t = sh_pass[par][ww]; if (ww < w) pos += t; run += t; }
            par ^= 1;            // (two sets of words: a wave may be a step ahead of the others' reads, never two)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!ps[q] || pos >= deg) continue;           // (pos < deg always: the count pass saw the same scores; a guard, not a path)
                const int64_t e = base + pos++;
                a.key[e] = j + q;
                a.weight[e] = (float)(exp(graph_logit(sc[q], adaptive, mtq, bsq) - M) * inv_z);
                if (a.score) a.score[e] = sc[q];
            }
        }
    }
}

// ---- plan: chunk height, workspace carve -------------------------------------------------------------------------------------------
int graph_plan(int B, int H, int W, int mode, int k, int rows_per_chunk, GraphPlan& p) {
    p = GraphPlan{};
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1, "dagl_ce_graph: bad shape B=%d H=%d W=%d", B, H, W);
    DAGL_REQUIRE(mode == DAGL_MODE_ADAPTIVE || mode == DAGL_MODE_TOPK || mode == DAGL_MODE_ADAPTIVE_TOPK,
                 "dagl_ce_graph: unknown mode 0x%x", mode);
    if (mode != DAGL_MODE_ADAPTIVE) DAGL_REQUIRE(k >= 1, "dagl_ce_graph: k=%d < 1", k);
    DAGL_REQUIRE(rows_per_chunk >= 0, "dagl_ce_graph: rows_per_chunk=%d < 0", rows_per_chunk);
    DAGL_REQUIRE((int64_t)H * W < (1ll << 30), "dagl_ce_graph: image too large");
    p.g = make_grid(H, W);
    const Grid& g = p.g;
    DAGL_REQUIRE((int64_t)B * g.L < (1ll << 31), "dagl_ce_graph: batch too large");
    p.B = B; p.mode = mode;
    p.k = mode == DAGL_MODE_ADAPTIVE ? 0 : (k > g.N ? g.N : k);      // top_k = min(num_edge, N)
    p.ldn = (long long)(g.N + 31) / 32 * 32;
    // rows per chunk: the wide top-k path's (2048, 512 MiB of scores at most, whole 128-row tiles of the product) unless forced
    long long c = rows_per_chunk;
    if (c == 0) {
        c = ((long long)512 << 20) / (p.ldn * 4) / 128 * 128;
        if (c < 128) c = 128;
        if (c > 2048) c = 2048;
    }
    p.rows = (int)(c < g.L ? c : g.L);
    const size_t BL = (size_t)B * g.L;
    Carver cv;
    p.o_b1p = cv.reserve((size_t)B * g.Hp * g.Wp * CH * sizeof(float));
    p.o_wp1 = cv.reserve((size_t)DPAD * P * sizeof(float));
    p.o_wp2 = cv.reserve((size_t)DPAD * P * sizeof(float));
    p.o_x = cv.reserve((size_t)B * feat_rows(g.N) * DS * sizeof(float));
    p.o_wq = cv.reserve((size_t)B * feat_rows(g.L) * DS * sizeof(float));
    p.o_colsum = cv.reserve((size_t)B * DS * sizeof(double));
    p.o_mt = cv.reserve(BL * sizeof(float));
    p.o_bias = cv.reserve(BL * sizeof(float));
    p.o_deg = cv.reserve(BL * sizeof(int32_t));
    p.o_sel = cv.reserve(BL * sizeof(uint2));
    p.o_rowm = cv.reserve(BL * sizeof(double));
    p.o_rowz = cv.reserve(BL * sizeof(double));
    p.o_scores = cv.reserve((size_t)p.rows * p.ldn * sizeof(float));
    p.o_end = cv.bytes();
    return DAGL_OK;
}

static GraphArgs graph_args(const GraphPlan& p, void* ws) {
    GraphArgs a;
    memset(&a, 0, sizeof(a));
    a.N = p.g.N; a.L = p.g.L; a.mode = p.mode; a.k = p.k;
    a.scores = at<float>(ws, p.o_scores); a.ldn = p.ldn;
    a.mt = at<float>(ws, p.o_mt); a.bs = at<float>(ws, p.o_bias);
    a.deg = at<int32_t>(ws, p.o_deg); a.sel = at<uint2>(ws, p.o_sel);
    a.row_m = at<double>(ws, p.o_rowm); a.row_z = at<double>(ws, p.o_rowz);
    a.n_rows = (long long)p.B * p.g.L;
    return a;
}

// the scores of every chunk of query rows in turn (one product [R, 196] x [196, N] on the fp32 matrix cores, chains of 48 products as
// in topk_wide.hip), `kernel` over its rows
template <class K>
static int graph_chunks(hipStream_t s, const GraphPlan& p, void* ws, GraphArgs a, K kernel, const char* name) {
    const Grid& g = p.g;
    const int rows_q = feat_rows(g.L), rows_x = feat_rows(g.N);
    const float* wq = at<float>(ws, p.o_wq);
    const float* x = at<float>(ws, p.o_x);
    for (int b = 0; b < p.B; ++b)
        for (int r0 = 0; r0 < g.L; r0 += p.rows) {
            a.b = b; a.r0 = r0; a.R = (g.L - r0 < p.rows) ? g.L - r0 : p.rows;
            Gemm32 gm;
            gm.M = a.R; gm.N = g.N; gm.K = D; gm.batch = 1;
            gm.A = wq + ((size_t)b * rows_q + r0) * DS; gm.lda = DS; gm.sA = 0; gm.a_kc = 1;
            gm.B = x + (size_t)b * rows_x * DS; gm.ldb = DS; gm.sB = 0; gm.b_kc = 1;
            gm.C = at<float>(ws, p.o_scores); gm.ldc = p.ldn; gm.sC = 0;
            gm.alpha = 1.f; gm.beta = 0.f; gm.bias = nullptr; gm.relu = 0; gm.chunk_tiles = 3;
            const int rc = launch_gemm32(s, gm);
            if (rc) return rc;
            hipLaunchKernelGGL(kernel, dim3(a.R), dim3(GR_THREADS), 0, s, a);
            DAGL_LAUNCH_CHECK(name);
        }
    return DAGL_OK;
}

int launch_graph_count(hipStream_t s, const GraphPlan& p, const float* b1, const float* thr, const float* bias, const float* fc1_w,
                       const float* fc1_b, const float* fc2_w, const float* fc2_b, int64_t* row_off, void* ws) {
    const Grid& g = p.g;
    const size_t BL = (size_t)p.B * g.L;
    float* b1p = at<float>(ws, p.o_b1p);
    float* X = at<float>(ws, p.o_x);
    float* Wq = at<float>(ws, p.o_wq);
    double* colsum = at<double>(ws, p.o_colsum);
    int rc;
    // fp32 map, packed weights, features, row thresholds: the launches of the scan = "exact" forward (capi.hip stage_layout .. stage_thresholds)
    if ((rc = launch_pad_nhwc(s, p.B, g.H, g.W, b1, b1p))) return rc;
    if ((rc = launch_pack_fc_weight(s, fc1_w, at<float>(ws, p.o_wp1)))) return rc;
    if ((rc = launch_pack_fc_weight(s, fc2_w, at<float>(ws, p.o_wp2)))) return rc;
    ZeroList zl;
    const int rx = feat_rows(g.N), rq = feat_rows(g.L);
    zl.add(X + (size_t)g.N * DS, (size_t)(rx - g.N) * DS * sizeof(float), p.B, (size_t)rx * DS * sizeof(float));
    zl.add(Wq + (size_t)g.L * DS, (size_t)(rq - g.L) * DS * sizeof(float), p.B, (size_t)rq * DS * sizeof(float));
    zl.add(colsum, align_up((size_t)p.B * DS * sizeof(double), 16));
    if ((rc = launch_zero_regions(s, zl))) return rc;
    ProjectLaunch pj;
    pj.B = p.B; pj.g = g; pj.which = 3; pj.map = b1p; pj.colsum = colsum;
    pj.keys.wp = at<float>(ws, p.o_wp2); pj.keys.bias = fc2_b; pj.keys.feat = X;
    pj.queries.wp = at<float>(ws, p.o_wp1); pj.queries.bias = fc1_b; pj.queries.feat = Wq;
    if ((rc = launch_project(s, pj))) return rc;
    if (p.mode != DAGL_MODE_TOPK) {
        if ((rc = launch_query_thresholds(s, p.B, g.L, g.N, Wq, colsum, thr, at<float>(ws, p.o_mt)))) return rc;
        DAGL_HIP_TRY(hipMemcpyAsync(at<float>(ws, p.o_bias), bias, BL * sizeof(float), hipMemcpyDeviceToDevice, s));   // (fill is not handed the inputs again)
    }
    if ((rc = graph_chunks(s, p, ws, graph_args(p, ws), graph_row_count_kernel, "graph_row_count_kernel"))) return rc;
    return launch_row_scan(s, (int)BL, at<int32_t>(ws, p.o_deg), row_off);
}

int launch_graph_fill(hipStream_t s, const GraphPlan& p, const int64_t* row_off, int32_t* key, float* weight, float* score,
                      long long capacity, void* ws) {
    GraphArgs a = graph_args(p, ws);
    a.row_off = row_off; a.key = key; a.weight = weight; a.score = score; a.capacity = capacity;
    return graph_chunks(s, p, ws, a, graph_row_fill_kernel, "graph_row_fill_kernel");
}

}  // namespace dagl
