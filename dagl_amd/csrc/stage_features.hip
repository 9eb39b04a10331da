// The features of a whole CES stage for the patch-graph routes (dagl_graph_stage_features16): the inference forward's heads-as-batch
// prologue and projection -- ONE conv_pair16_kernel launch for the g / theta maps of up to four heads, ONE project16_kernel launch for
// their keys and queries (prologue.hip, project16.hip; capi.hip prologue_fused / stage_project are the same sequence inside a forward) --
// and ONE launch of the kernel below, which turns the projection's padded rows into the operands the row kernels of graph_refresh.hip
// read: dense [heads, B, n, 196] rows, the margin's tau, the range verdict.
#include "dagl_common.h"
#include "thr_bias4.h"

namespace dagl {

// ---- stage_features_out_kernel ---------------------------------------------------------------------------------------------------------
// One wavefront per feature row, keys first ([heads B N] rows), then queries ([heads B L]); a block of four waves walks the rows with
// the grid's stride.  A row is 51 float4 (DS = 204 floats, 816 B) of which the first 49 (196 floats, 784 B) are kept: lane i < 49
// moves float4 i, both sides 16-byte aligned and contiguous over the wave, nothing staged.  A query row that wants the margin keeps its
// float4 for the fp64 dot with its image's column sums: lane i sums its four products in column order, the lanes meet in the xor
// butterfly of query_thresholds_kernel (project.hip: 32, 16, .., 1), and lane 0 finishes thr / bias from the four channel-group
// partials exactly as that kernel does.
struct StageFeatOut {
    int hb, N, L, rows_k, rows_q;            // heads x images; keys / queries per image; rows allocated per image (feat_rows)
    const float* xf; const float* wqf;       // [hb, rows_k, DS], [hb, rows_q, DS]: what project16_kernel wrote
    float* x_rows; float* wq_rows;           // [hb, N, 196], [hb, L, 196]
    float* tau;                              // [hb, L] or null: no margin
    const double* colsum;                    // [hb, DS]
    const float* part;                       // [heads][4][imgs][L][2] partial sums of the thr / bias heads
    const float* thr_b[4]; const float* bias_b[4];
    int imgs;
    float* b2p; size_t b2p_floats;           // the value maps of all heads: NaN-filled when the call left the range (b2p[0] of every head with it)
    RangeTag range;
};

constexpr int SF_WAVES = 4;                  // waves (rows in flight) per block

__global__ __launch_bounds__(64 * SF_WAVES) void stage_features_out_kernel(StageFeatOut a) {
    const int lane = threadIdx.x & 63;
    // (rows are counted in 32 bits: the entry refuses heads B H W >= 2^30, and L <= N)
    const unsigned wave0 = blockIdx.x * SF_WAVES + (threadIdx.x >> 6), n_waves = gridDim.x * SF_WAVES;
    const bool poisoned = a.range.word != nullptr && *a.range.word == a.range.tag;
    if (a.range.done != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *a.range.done = a.range.tag;
    const float qnan = __builtin_nanf("");
    const unsigned n_keys = (unsigned)a.hb * (unsigned)a.N, n_rows = n_keys + (unsigned)a.hb * (unsigned)a.L;
    for (unsigned r = wave0; r < n_rows; r += n_waves) {
        const bool query = r >= n_keys;
        const unsigned rr = query ? r - n_keys : r;
        const unsigned n = (unsigned)(query ? a.L : a.N);
        const unsigned b = rr / n, i = rr - b * n;
        const float* src = (query ? a.wqf : a.xf) + ((size_t)b * (size_t)(query ? a.rows_q : a.rows_k) + i) * DS;
        float* dst = (query ? a.wq_rows : a.x_rows) + (size_t)rr * D;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < D / 4) {
            v = *reinterpret_cast<const float4*>(src + 4 * lane);
            *reinterpret_cast<float4*>(dst + 4 * lane) =
                make_float4(poisoned ? qnan : v.x, poisoned ? qnan : v.y, poisoned ? qnan : v.z, poisoned ? qnan : v.w);
        }
        if (query && a.tau != nullptr) {                       // (wave-uniform)
            double acc = 0.0;
            if (lane < D / 4) {
                const double* cs = a.colsum + (size_t)b * DS + 4 * lane;
                acc = (double)v.x * cs[0];
                acc += (double)v.y * cs[1];
                acc += (double)v.z * cs[2];
                acc += (double)v.w * cs[3];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (lane == 0) {
                const float mean = (float)(acc / (double)a.N);
                const int head = (int)(b / (unsigned)a.imgs), img = (int)b - head * a.imgs;
                const size_t np = (size_t)a.imgs * a.L;
                const float2* pp = reinterpret_cast<const float2*>(a.part) + (size_t)head * 4 * np + (size_t)img * a.L + i;
                const float2 p0 = pp[0], p1 = pp[np], p2 = pp[2 * np], p3 = pp[3 * np];
                // (selects, not a[head]: a runtime index into the by-value argument would put the tables into scratch)
                const float* tb = head == 0 ? a.thr_b[0] : head == 1 ? a.thr_b[1] : head == 2 ? a.thr_b[2] : a.thr_b[3];
                const float* bb = head == 0 ? a.bias_b[0] : head == 1 ? a.bias_b[1] : head == 2 ? a.bias_b[2] : a.bias_b[3];
                const float tv = ((p0.x + p1.x) + (p2.x + p3.x)) + tb[0];
                const float bv = ((p0.y + p1.y) + (p2.y + p3.y)) + bb[0];
                a.tau[rr] = poisoned ? qnan : mean * tv - bv;
            }
        }
    }
    if (poisoned) {                                            // one word per call: the whole stage's value maps go with it
        const float4 nan4 = make_float4(qnan, qnan, qnan, qnan);
        const size_t n4 = a.b2p_floats / 4;                    // (16 channels per pixel: a multiple of 4)
        for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += (size_t)gridDim.x * blockDim.x)
            reinterpret_cast<float4*>(a.b2p)[t] = nan4;
    }
}

static int launch_stage_features_out(hipStream_t s, const StageFeatOut& a) {
    // a streaming copy: at most 8 blocks of 256 threads per CU of the 256, the rest by the grid's stride
    const size_t n_rows = (size_t)a.hb * ((size_t)a.N + a.L);
    const size_t blocks = (n_rows + SF_WAVES - 1) / SF_WAVES;
    const unsigned grid = (unsigned)(blocks < 2048 ? blocks : 2048);
    hipLaunchKernelGGL(stage_features_out_kernel, dim3(grid), dim3(64 * SF_WAVES), 0, s, a);
    DAGL_LAUNCH_CHECK("stage_features_out_kernel");
    return DAGL_OK;
}

// ---- the workspace: written once, walked by the size function and by the entry -----------------------------------------------------------
struct StageFeatWs {
    int64_t* words;                          // range word, completion word (RangeTag)
    double* colsum;                          // [hb, DS]
    unsigned char* convw;                    // [heads] packed g / theta weights
    uint16_t *wp1h, *wp2h;                   // [heads] packed fc1 / fc2 weights
    uint16_t *map_hi, *map_lo, *map_hi2, *map_lo2;     // the key / query map's two tiers, [hb, Hp, Wp, 16] each
    float* amax; int slots;                  // [heads][slots] |b1| of the conv blocks' waves
    float *X, *Wq;                           // [hb, feat_rows(N), DS], [hb, feat_rows(L), DS]
    float *thr_part, *colpart;               // margin only
    size_t bytes;
};

static StageFeatWs stage_feat_carve(void* ws, int heads, int B, const Grid& g, bool margin) {
    Carver cv(ws);
    const size_t hb = (size_t)heads * B, map_h = hb * g.Hp * g.Wp * CH;
    StageFeatWs w;
    w.words = cv.take<int64_t>(2);
    w.colsum = cv.take<double>(hb * DS);
    w.convw = cv.take<unsigned char>((size_t)heads * CONV_W16_BYTES);
    w.wp1h = cv.take<uint16_t>((size_t)heads * P16_PACKED_HALFS);
    w.wp2h = cv.take<uint16_t>((size_t)heads * P16_PACKED_HALFS);
    w.map_hi = cv.take<uint16_t>(map_h); w.map_lo = cv.take<uint16_t>(map_h);
    w.map_hi2 = cv.take<uint16_t>(map_h); w.map_lo2 = cv.take<uint16_t>(map_h);
    w.slots = conv16_blocks_per_head(g, heads, B);
    w.amax = cv.take<float>((size_t)heads * w.slots);
    w.X = cv.take<float>(hb * feat_rows(g.N) * DS);
    w.Wq = cv.take<float>(hb * feat_rows(g.L) * DS);
    w.thr_part = margin ? cv.take<float>(8 * hb * g.L) : nullptr;
    w.colpart = margin ? cv.take<float>(hb * project16_key_blocks(g) * 224) : nullptr;
    w.bytes = cv.bytes();
    return w;
}

static int stage_feat_dims_ok(const char* who, int heads, int B, int H, int W) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    DAGL_REQUIRE(heads >= 1 && heads <= 4, "%s: heads=%d, 1..4 expected", who, heads);
    DAGL_REQUIRE((int64_t)heads * B * H * W < (1ll << 30), "%s: batch too large for 32-bit row ids", who);
    return DAGL_OK;
}

}  // namespace dagl

using namespace dagl;

extern "C" {

size_t dagl_graph_stage_features16_workspace_bytes(int heads, int B, int H, int W, int margin) {
    if (stage_feat_dims_ok("dagl_graph_stage_features16_workspace_bytes", heads, B, H, W)) return 0;
    return stage_feat_carve(nullptr, heads, B, make_grid(H, W), margin != 0).bytes;
}

int dagl_graph_stage_features16(void* stream, int heads, int B, int H, int W, const float* x, const dagl_ce_weights* heads_w, int margin,
                                float* wq_rows, float* x_rows, float* b2p, float* tau, void* workspace, size_t workspace_bytes) {
    const char* who = "dagl_graph_stage_features16";
    int rc;
    if ((rc = stage_feat_dims_ok(who, heads, B, H, W))) return rc;
    DAGL_REQUIRE(x && heads_w && wq_rows && x_rows && b2p, "%s: null tensor pointer", who);
    for (int h = 0; h < heads; ++h) {
        const dagl_ce_weights& w = heads_w[h];
        DAGL_REQUIRE(w.g_w && w.g_b && w.theta_w && w.theta_b && w.fc1_w && w.fc1_b && w.fc2_w && w.fc2_b,
                     "%s: head %d has a null weight pointer", who, h);
        if (margin) DAGL_REQUIRE(w.thr_w && w.thr_b && w.bias_w && w.bias_b, "%s: head %d has a null thr / bias pointer (margin set)", who, h);
    }
    DAGL_REQUIRE((tau != nullptr) == (margin != 0), "%s: tau and margin come together (tau %s, margin=%d)", who, tau ? "given" : "NULL", margin);
    auto al16 = [](const void* p) { return ((uintptr_t)p % 16) == 0; };
    DAGL_REQUIRE(al16(x) && al16(wq_rows) && al16(x_rows) && al16(b2p) && al16(tau),
                 "%s: x, wq_rows, x_rows, b2p and tau must be 16-byte aligned", who);
    const Grid g = make_grid(H, W);
    const bool mg = margin != 0;
    if ((rc = check_workspace(who, workspace, workspace_bytes, stage_feat_carve(nullptr, heads, B, g, mg).bytes))) return rc;
    const StageFeatWs w = stage_feat_carve(workspace, heads, B, g, mg);
    hipStream_t s = (hipStream_t)stream;
    const int hb = heads * B;

    // 1. the call's words and column sums
    RangeTag rt;
    DAGL_HIP_TRY(hipMemsetAsync(w.words, 0, 2 * sizeof(int64_t), s));
    DAGL_HIP_TRY(hipMemsetAsync(w.colsum, 0, (size_t)hb * DS * sizeof(double), s));
    rt.word = reinterpret_cast<int32_t*>(w.words); rt.done = reinterpret_cast<int32_t*>(w.words + 1); rt.tag = next_call_tag();
    // 2. the weight packs
    ConvHeadSet hs = {};
    ThrHeadSet ths = {};
    const float* b1s[4]; const float* b2s[4];
    for (int h = 0; h < heads; ++h) {
        const dagl_ce_weights& hw = heads_w[h];
        unsigned char* convw = w.convw + (size_t)h * CONV_W16_BYTES;
        if ((rc = launch_pack_conv_weight16(s, hw.g_w, hw.theta_w, convw))) return rc;
        if ((rc = launch_pack_fc_weight16(s, hw.fc1_w, w.wp1h + (size_t)h * P16_PACKED_HALFS))) return rc;
        if ((rc = launch_pack_fc_weight16(s, hw.fc2_w, w.wp2h + (size_t)h * P16_PACKED_HALFS))) return rc;
        hs.x[h] = x; hs.w[h] = convw; hs.gb[h] = hw.g_b; hs.tb[h] = hw.theta_b;
        ths.x[h] = x; ths.thr_w[h] = hw.thr_w; ths.bias_w[h] = hw.bias_w;
    }
    for (int h = 0; h < 4; ++h) { b1s[h] = heads_w[h < heads ? h : 0].fc1_b; b2s[h] = heads_w[h < heads ? h : 0].fc2_b; }
    hs.imgs = B; ths.imgs = B;
    hs.tiers.hi2 = w.map_hi2; hs.tiers.lo2 = w.map_lo2; hs.tiers.amax = w.amax; hs.tiers.slots = w.slots;
    // 3. the maps' zero borders, the feature matrices' guard rows
    if ((rc = launch_zero_borders(s, hb, H, W, b2p, b2p))) return rc;
    if ((rc = launch_zero_borders16(s, hb, H, W, w.map_hi, w.map_lo))) return rc;
    if ((rc = launch_zero_borders16(s, hb, H, W, w.map_hi2, w.map_lo2))) return rc;
    ZeroList zl;
    const int rx = feat_rows(g.N), rq = feat_rows(g.L);
    zl.add(w.X + (size_t)g.N * DS, (size_t)(rx - g.N) * DS * sizeof(float), hb, (size_t)rx * DS * sizeof(float));
    zl.add(w.Wq + (size_t)g.L * DS, (size_t)(rq - g.L) * DS * sizeof(float), hb, (size_t)rq * DS * sizeof(float));
    if ((rc = launch_zero_regions(s, zl))) return rc;
    // 4. g / theta of every head: b2p, the fp16 planes of b1 (both tiers), the |b1| slots
    if ((rc = launch_conv_pair16_heads(s, heads, B, g, hs, b2p, nullptr, w.map_hi, w.map_lo, nullptr, 0, nullptr, 0, rt))) return rc;
    // 5. the thr / bias heads as a launch of their own only where they cannot ride in the projection's
    const bool ride = mg && thr_bias4_ok(g, ths, heads);
    if (mg && !ride && (rc = launch_thr_bias_heads(s, heads, B, g, ths, w.thr_part))) return rc;
    // 6. keys and queries of every head
    Project16Launch pj;
    pj.B = hb; pj.g = g; pj.which = 3; pj.heads = heads; pj.range = rt;
    pj.map_hi = w.map_hi; pj.map_lo = w.map_lo; pj.tiers = hs.tiers;
    pj.keys.wp = w.wp2h; pj.keys.bias = b2s; pj.keys.feat = w.X;
    pj.queries.wp = w.wp1h; pj.queries.bias = b1s; pj.queries.feat = w.Wq;
    if (mg) { pj.colsum = w.colsum; pj.colpart = w.colpart; }
    if (ride) { pj.thr_hs = &ths; pj.thr_head_imgs = hb; pj.thr_part = w.thr_part; }
    if ((rc = launch_project16(s, pj))) return rc;
    // 7. dense rows, tau, the range verdict
    StageFeatOut o = {};
    o.hb = hb; o.N = g.N; o.L = g.L; o.rows_k = rx; o.rows_q = rq;
    o.xf = w.X; o.wqf = w.Wq; o.x_rows = x_rows; o.wq_rows = wq_rows;
    o.tau = tau; o.colsum = w.colsum; o.part = w.thr_part; o.imgs = B;
    for (int h = 0; h < 4; ++h) { o.thr_b[h] = heads_w[h < heads ? h : 0].thr_b; o.bias_b[h] = heads_w[h < heads ? h : 0].bias_b; }
    o.b2p = b2p; o.b2p_floats = (size_t)hb * g.Hp * g.Wp * CH;
    o.range = rt;
    return launch_stage_features_out(s, o);
}

}  // extern "C"
