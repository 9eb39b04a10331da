// The backward of a CES stage's last launch, out = conv1x1(cat) + mix_b + x (stage_mix_kernel / stage_fold_mix_kernel, aggregate.hip),
// for the stage-fused forward on a frozen graph (dagl_graph_stage_forward, graph_forward.hip).  With d_out [B,64,H,W] the gradient of the
// stage's output, mix_w [64,64] (o, c) and cat the pre-mix concat map, kept HEAD-MAJOR as cat4 [4,B,16,H,W] (concat channel 16 h + c of
// image b = cat4[h, b, c]):
//   d_cat4[h, b, c, p] = sum_o mix_w[o][16 h + c] d_out[b, o, p]          stage_mix_dcat_kernel
//   d_mix_w[o][c]      = sum_{b, p} d_out[b, o, p] cat[b, c, p]           stage_mix_wgrad_kernel + stage_mix_wgrad_combine_kernel
//   d_mix_b[o]         = sum_{b, p} d_out[b, o, p]                        (the same two launches)
// d_cat4 is written head-major so that dagl_graph_forward_backward, run with B' = 4 B on d_cat4 viewed as [4 B,16,H,W], picks it up as
// its d_out: the division by the overlap count is unfold_dout_kernel's there, none is made here.  The gradient of the residual input is
// d_out itself.
//
// All three products run on the fp32 matrix cores (MFMA 16x16x4: A lane (i, g) = A[row i][k g], B lane (i, g) = B[k g][col i],
// D lane (i, g) = D[rows 4 g .. 4 g + 3][col i]; i = lane & 15, g = lane >> 4).
//   dcat   rows = 16 pixels, k = the 64 outputs, cols = the 16 channels of a head: the A operand is read with the pixels along the
//          lanes (64-byte runs of a channel plane), the transposed weight fragment stays in registers for the wave's tiles, and a lane
//          ends with four consecutive pixels of one channel: one float4 store (scalar stores where H W is no multiple of 4).
//   wgrad  rows = outputs, cols = concat channels, k = pixels.  A block takes a contiguous range of 64-pixel chunks, each of its waves
//          every fourth chunk of it and the whole 64 x 64 tile; a lane reads four consecutive pixels of a plane at a time (float4; the
//          k index of an MFMA step is a fixed permutation of the chunk's pixels, the same for both operands).  Every wave leaves its
//          tile and its 64 bias sums in a slot of its own; the combine launch adds the slots in slot order in fp64.
// No LDS, no float atomics, fixed summation order: the same operands give the same bits on every call.  The number of blocks of the
// wgrad launch depends on B H W alone.  Pixels beyond the map read as zeros and are never stored.
#include "dagl_common.h"
#include "graph_rows.h"

namespace dagl {

constexpr int DCAT_TILES = 4;                              // 16-pixel tiles per wave: the 64 weight loads of a lane serve 64 pixels

__global__ __launch_bounds__(256) void stage_mix_dcat_kernel(int B, int HW, int blocks_per_img, const float* __restrict__ d_out,
                                                             const float* __restrict__ mix_w, float* __restrict__ d_cat4) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / blocks_per_img;
    const int pw = ((blockIdx.x - b * blocks_per_img) * 4 + wave) * (16 * DCAT_TILES);
    if (pw >= HW) return;
    float wt[4][16];                                           // B fragment (h, T): mix_w[o = 4T + g][c = 16 h + i]
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int T = 0; T < 16; ++T) wt[h][T] = mix_w[(4 * T + g) * 64 + h * 16 + i];
    const bool vec = (HW & 3) == 0;                            // every plane and every 4-pixel group is 16-byte aligned
    const float* ob = d_out + (size_t)b * 64 * HW;
#pragma unroll 1
    for (int t = 0; t < DCAT_TILES; ++t) {
        const int p0 = pw + 16 * t;
        if (p0 >= HW) break;
        int px = p0 + i; if (px >= HW) px = HW - 1;
        float av[16];                                          // A fragment T: d_out[b, o = 4T + g, pixel p0 + i]
#pragma unroll
        for (int T = 0; T < 16; ++T) av[T] = ob[(size_t)(4 * T + g) * HW + px];
        f32x4 acc[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) acc[h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int T = 0; T < 16; ++T)
#pragma unroll
            for (int h = 0; h < 4; ++h) acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[T], wt[h][T], acc[h], 0, 0, 0);
        // D[row = pixel p0 + 4g + r][col = channel i] of head h
        const int pp = p0 + 4 * g;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            float* dst = d_cat4 + (((size_t)h * B + b) * CH + i) * HW + pp;
            if (vec) {
                if (pp < HW) *reinterpret_cast<float4*>(dst) = make_float4(acc[h][0], acc[h][1], acc[h][2], acc[h][3]);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (pp + r < HW) dst[r] = acc[h][r];
            }
        }
    }
}

constexpr int WGRAD_CHUNK = 64;                            // pixels of a wave's step: 16 MFMA k-steps of 4
constexpr int WGRAD_BLOCK_PIXELS = 4096;                   // pixels a block takes at least (its four waves: 16 chunks each)
constexpr int WGRAD_MAX_BLOCKS = 128;                      // the cap: 512 slots of 16.25 KiB for the combine launch to add
constexpr int WGRAD_SLOT = 64 * 64 + 64;                   // floats of a slot: the tile (o, c), then the 64 bias sums

static inline int wgrad_blocks(int B, int HW) {
    const long long nb = ((long long)B * HW + WGRAD_BLOCK_PIXELS - 1) / WGRAD_BLOCK_PIXELS;
    return (int)(nb < 1 ? 1 : nb > WGRAD_MAX_BLOCKS ? WGRAD_MAX_BLOCKS : nb);
}

// four consecutive pixels p .. p + 3 of a plane, zeros beyond the map.  vec: H W is a multiple of 4 (p is one always)
__device__ __forceinline__ float4 wgrad_load4(const float* __restrict__ plane, int p, int HW, bool vec) {
    if (vec) return p < HW ? *reinterpret_cast<const float4*>(plane + p) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v;
    v.x = p < HW ? plane[p] : 0.f;
    v.y = p + 1 < HW ? plane[p + 1] : 0.f;
    v.z = p + 2 < HW ? plane[p + 2] : 0.f;
    v.w = p + 3 < HW ? plane[p + 3] : 0.f;
    return v;
}

__global__ __launch_bounds__(256) void stage_mix_wgrad_kernel(int B, int HW, const float* __restrict__ d_out, const float* __restrict__ cat4,
                                                              float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int per_img = (HW + WGRAD_CHUNK - 1) / WGRAD_CHUNK;
    const long long total = (long long)B * per_img;
    const long long per_block = (total + gridDim.x - 1) / gridDim.x;
    const long long lo = per_block * blockIdx.x;
    long long hi = lo + per_block; if (hi > total) hi = total;
    const bool vec = (HW & 3) == 0;
    f32x4 acc[4][4];                                           // (m, n): d_w[o = 16 m + 4 g + r][c = 16 n + i]
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};                      // lane's share of d_b[o = 16 m + i]
#pragma unroll 1
    for (long long chunk = lo + wave; chunk < hi; chunk += 4) {
        const int b = (int)(chunk / per_img);
        const int p0 = (int)(chunk - (long long)b * per_img) * WGRAD_CHUNK;
        const float* ob = d_out + ((size_t)b * 64 + i) * HW;                    // plane o = 16 m + i: + 16 m planes
        const float* cb = cat4 + ((size_t)b * CH + i) * HW;                     // plane (head n, channel i): + n B 16 planes
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = p0 + 16 * j + 4 * g;                 // k-steps 4 j + e: lane group g carries pixel p + e
            float4 av[4], bv[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) av[m] = wgrad_load4(ob + (size_t)m * 16 * HW, p, HW, vec);
#pragma unroll
            for (int n = 0; n < 4; ++n) bv[n] = wgrad_load4(cb + (size_t)n * B * CH * HW, p, HW, vec);
#pragma unroll
            for (int m = 0; m < 4; ++m) bsum[m] += (av[m].x + av[m].y) + (av[m].z + av[m].w);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].x, bv[n].x, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].y, bv[n].y, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].z, bv[n].z, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].w, bv[n].w, acc[m][n], 0, 0, 0);
                }
        }
    }
    float* slot = part + (size_t)(blockIdx.x * 4 + wave) * WGRAD_SLOT;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) slot[(16 * m + 4 * g + r) * 64 + 16 * n + i] = acc[m][n][r];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float v = bsum[m];                                     // the four lane groups of a row: (g, g ^ 1) pairs, then the pairs
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (g == 0) slot[64 * 64 + 16 * m + i] = v;
    }
}

__global__ __launch_bounds__(256) void stage_mix_wgrad_combine_kernel(int n_slots, const float* __restrict__ part, float* __restrict__ d_mix_w,
                                                                      float* __restrict__ d_mix_b) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= WGRAD_SLOT) return;
    double s = 0.0;
    for (int k = 0; k < n_slots; ++k) s += (double)part[(size_t)k * WGRAD_SLOT + idx];
    if (idx < 64 * 64) {
        if (d_mix_w != nullptr) d_mix_w[idx] = (float)s;
    } else if (d_mix_b != nullptr) {
        d_mix_b[idx - 64 * 64] = (float)s;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static size_t stage_mix_backward_workspace_bytes(int B, int HW) {
    Carver cv(nullptr);
    cv.take<float>((size_t)wgrad_blocks(B, HW) * 4 * WGRAD_SLOT);
    return cv.bytes();
}

static int launch_stage_mix_backward(hipStream_t s, int B, int HW, const float* d_out, const float* cat4, const float* mix_w, float* d_cat4,
                                     float* d_mix_w, float* d_mix_b, void* workspace) {
    const int per_img = (HW + 64 * DCAT_TILES - 1) / (64 * DCAT_TILES);
    hipLaunchKernelGGL(stage_mix_dcat_kernel, dim3((unsigned)per_img * (unsigned)B), dim3(256), 0, s, B, HW, per_img, d_out, mix_w, d_cat4);
    DAGL_LAUNCH_CHECK("stage_mix_dcat_kernel");
    if (d_mix_w == nullptr && d_mix_b == nullptr) return DAGL_OK;
    Carver cv(workspace);
    const int blocks = wgrad_blocks(B, HW);
    float* part = cv.take<float>((size_t)blocks * 4 * WGRAD_SLOT);
    hipLaunchKernelGGL(stage_mix_wgrad_kernel, dim3((unsigned)blocks), dim3(256), 0, s, B, HW, d_out, cat4, part);
    DAGL_LAUNCH_CHECK("stage_mix_wgrad_kernel");
    hipLaunchKernelGGL(stage_mix_wgrad_combine_kernel, dim3((WGRAD_SLOT + 255) / 256), dim3(256), 0, s, blocks * 4, part, d_mix_w, d_mix_b);
    DAGL_LAUNCH_CHECK("stage_mix_wgrad_combine_kernel");
    return DAGL_OK;
}

static int stage_mix_backward_shape_ok(const char* who, int B, int H, int W) {
    const int rc = graph_dims_ok(who, B, H, W);
    if (rc) return rc;
    DAGL_REQUIRE((int64_t)4 * B * H * W < (1ll << 30), "%s: batch too large for 32-bit row ids", who);
    return DAGL_OK;
}

}  // namespace dagl

using namespace dagl;

extern "C" {

// the backward of a stage's mix on the head-major concat map (no ABI bump: found by symbol)
size_t dagl_ces_stage_mix_backward_workspace_bytes(int B, int H, int W) {
    if (stage_mix_backward_shape_ok("dagl_ces_stage_mix_backward_workspace_bytes", B, H, W)) return 0;
    return stage_mix_backward_workspace_bytes(B, H * W);
}

int dagl_ces_stage_mix_backward(void* stream, int B, int H, int W, const float* d_out, const float* cat4, const float* mix_w, float* d_cat4,
                                float* d_mix_w, float* d_mix_b, void* workspace, size_t ws_bytes) {
    const char* who = "dagl_ces_stage_mix_backward";
    int rc = stage_mix_backward_shape_ok(who, B, H, W);
    if (rc) return rc;
    DAGL_REQUIRE(d_out && mix_w && d_cat4 && (cat4 || (!d_mix_w && !d_mix_b)), "%s: null tensor pointer", who);
    DAGL_REQUIRE(((uintptr_t)d_out % 16) == 0 && ((uintptr_t)cat4 % 16) == 0 && ((uintptr_t)d_cat4 % 16) == 0,
                 "%s: d_out, cat4 and d_cat4 must be 16-byte aligned", who);
    if ((rc = check_workspace(who, workspace, ws_bytes, stage_mix_backward_workspace_bytes(B, H * W)))) return rc;
    return launch_stage_mix_backward((hipStream_t)stream, B, H * W, d_out, cat4, mix_w, d_cat4, d_mix_w, d_mix_b, workspace);
}

}  // extern "C"
