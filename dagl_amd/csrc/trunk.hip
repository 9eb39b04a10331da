// The residual trunk's convolutions (RR / CES around the block: DN_Gray/model/dagl.py:11-54, common.py:59-79) on the fp32 matrix
// cores: 2-D convolution, stride 1, padding ksize / 2, ksize 1 or 3, 1..64 input and output channels, fp32 NCHW at any B, H, W.
// Exact fp32 products with fp32 accumulation (v_mfma_f32_16x16x4_f32), the stock layer's arithmetic: no range limits.
//
//   forward / input gradient  out[o][pix] = sum_{c, tap} w[o][c][tap] x[c][pix + tap]: an implicit GEMM D[m = pixel][n = o],
//        K = channels x taps.  One block = (image, strip of rows, column tile of <= 128 pixels); its four waves (one per SIMD) split the 16-wide
//        output-channel groups and the 16-pixel tiles of a row.  A wave keeps the B fragments of its 16 output channels (all taps
//        and input channels: <= 144 registers) for its lifetime; input rows (with a one-pixel halo) live in an LDS ring of four
//        rows, the next row is fetched into registers under the multiplies.  The input gradient is the same kernel over the
//        weights flipped and transposed (dagl_trunk_pack_weights, transposed = 1).  The D fragment holds four consecutive pixels
//        of one channel per lane: 16-byte stores.  Epilogues: forward + bias, single-slope PReLU (optionally storing the
//        pre-activation), * res_scale + residual; input gradient * alpha, the PReLU backward from the saved pre-activation (with
//        per-block partial sums of the slope gradient), + skip gradient.
//   weight gradient  dW[o][c][tap] = sum_pix x[c][pix + tap] dy[o][pix]: D[m = c][n = o], K = pixels; a wave owns one (16 input
//        channels, 16 output channels) pair and keeps one accumulator per tap; blocks write partial sums, a second kernel adds
//        them in a fixed order (no atomics: the same bits on every call) together with the bias gradient (column sums of dy,
//        collected on the way) and the slope partials of the input gradient.
#include "dagl_common.h"

#include <type_traits>

namespace dagl {

typedef float f32x4t __attribute__((ext_vector_type(4)));

constexpr int TK_WAVES = 8;                    // weight gradient
constexpr int TK_THREADS = TK_WAVES * 64;
constexpr int TK_FWAVES = 4;                   // forward / input gradient: one wave per SIMD (the B fragments take <= 144 registers)
constexpr int TK_FTHREADS = TK_FWAVES * 64;
constexpr int TK_MAX_C = 64;
constexpr int TK_FWD_TW = 128;                 // widest column tile of the forward (LDS: 4 rows x 64 channels x 144 floats)
constexpr int TK_WG_TW = 64;                   // widest column tile of the weight gradient
constexpr int TK_WG_S = 66;                    // its staged floats per channel row (= 2 mod 32: 16 channels x 2 pixels hit 32 banks)

__host__ __device__ inline int tk_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }
__host__ __device__ inline int tk_nc(int cin) { return tk_pow2((cin + 3) / 4); }        // 4-channel k-steps, padded: 1, 2, 4, 8, 16
__host__ __device__ inline int tk_ngroups(int c) { return tk_pow2((c + 15) / 16); }      // 16-channel groups, padded: 1, 2, 4
__host__ __device__ inline int tk_fwd_stride(int tw) { return ((tw + 2 - 16 + 31) / 32) * 32 + 16; }   // >= tw + 2, = 16 mod 32

struct TkTiling { int n_ct, tw, rows_per_block, n_strips; };

static TkTiling tk_tiling(int B, int H, int W, int max_tw, int gran, int grid_y) {
    TkTiling t;
    t.n_ct = (W + max_tw - 1) / max_tw;
    t.tw = gran * (((W + gran - 1) / gran + t.n_ct - 1) / t.n_ct);
    long long rows = (long long)B * H * t.n_ct * grid_y;
    int r = (int)((rows + 255) / 256);                  // about one block per CU over the launch
    if (r < 1) r = 1;
    if (r > 64) r = 64;
    t.rows_per_block = r;
    t.n_strips = (H + r - 1) / r;
    return t;
}

struct TkConvArgs {
    int Cin, Cout, H, W, n_og, n_ct, tw, stride, rows_per_block, vec, dgrad;
    const float* x;            // [B, Cin, H, W]
    const float* wp;           // packed B fragments [n_og][ks * ks][nc][64]
    const float* bias;         // [Cout] or null (forward)
    const float* slope;        // PReLU slope (one float) or null
    const float* pre;          // input gradient: saved pre-activation [B, Cout, H, W]
    const float* res;          // forward: residual; input gradient: skip gradient ([B, Cout, H, W] or null)
    float res_scale, alpha;
    float* out;                // [B, Cout, H, W]
    float* pre_out;            // forward: pre-activation [B, Cout, H, W] or null
    double* slope_part;        // input gradient with slope: one fp64 partial per block
};

template <int KS, int NC>
__global__ __launch_bounds__(TK_FTHREADS, 1) void trunk_conv_kernel(TkConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tk_smem[];
    constexpr int KC = NC * 4, T = KS * KS, HALO = KS / 2;
    constexpr int CPW = (KC + TK_FWAVES - 1) / TK_FWAVES;         // staged channels per wave
    const int H = a.H, W = a.W, S = a.stride, CW = a.tw + 2, Cin = a.Cin, Cout = a.Cout;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ct = blockIdx.x % a.n_ct, strip = blockIdx.x / a.n_ct, b = blockIdx.z;
    const int x0 = ct * a.tw;
    const int y0 = strip * a.rows_per_block;
    const int y1 = (y0 + a.rows_per_block < H) ? y0 + a.rows_per_block : H;
    const int og = wave & (a.n_og - 1), tw = wave / a.n_og, n_tw = TK_FWAVES / a.n_og;
    const int m = lane & 15, q = lane >> 4;
    const float* xb = a.x + (size_t)b * Cin * H * W;

    // B fragments: B[k = channel 4 ch + q][n = output channel og * 16 + m] of every tap
    float wr[T][NC];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) wr[t][ch] = a.wp[((size_t)(og * T + t) * NC + ch) * 64 + lane];

    // staged column j of a row holds pixel x0 + j - 1; channels >= Cin and pixels outside the image are zeros
    float rx[CPW][3];
    auto fetch = [&](int y) {
        const bool row_ok = y >= 0 && y < H;
#pragma unroll
        for (int r = 0; r < CPW; ++r) {
            const int c = wave + TK_FWAVES * r;
            const bool ok = row_ok && c < Cin;
            const float* src = xb + ((size_t)(ok ? c : 0) * H + (ok ? y : 0)) * W;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int col = lane + 64 * k, gx = x0 + col - 1;
                rx[r][k] = (ok && col < CW && gx >= 0 && gx < W) ? src[gx] : 0.f;
            }
        }
    };
    auto store = [&](int y) {
        float* s = tk_smem + ((y + 1) & 3) * KC * S;
#pragma unroll
        for (int r = 0; r < CPW; ++r) {
            const int c = wave + TK_FWAVES * r;
            if (c < KC) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int col = lane + 64 * k;
                    if (col < CW) s[c * S + col] = rx[r][k];
                }
            }
        }
    };

    for (int y = y0 - HALO; y <= y0 + HALO; ++y) { fetch(y); store(y); }
    __syncthreads();

    const float sl = a.slope ? a.slope[0] : 0.f;
    double sp = 0.0;                                               // slope-gradient partial of this lane (input gradient), fp64
    const int o = og * 16 + m;
    const float bo = (a.bias && o < Cout) ? a.bias[o] : 0.f;

    // D[row = pixel 4 q + e][col = output channel m]: four consecutive pixels of channel o
    auto epilogue = [&](f32x4t v, int y, int t) {
        const int px0 = x0 + 16 * t + 4 * q;
        if (o >= Cout || px0 >= W) return;
        const int nv = (W - px0 < 4) ? W - px0 : 4;
        const size_t base = (((size_t)b * Cout + o) * H + y) * W + px0;
        const bool v4 = a.vec && nv == 4;
        float r[4] = {0.f, 0.f, 0.f, 0.f}, p[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.res) {
            if (v4) { const float4 t4 = *reinterpret_cast<const float4*>(a.res + base); r[0] = t4.x; r[1] = t4.y; r[2] = t4.z; r[3] = t4.w; }
            else for (int e = 0; e < nv; ++e) r[e] = a.res[base + e];
        }
        if (a.dgrad && a.slope) {
            if (v4) { const float4 t4 = *reinterpret_cast<const float4*>(a.pre + base); p[0] = t4.x; p[1] = t4.y; p[2] = t4.z; p[3] = t4.w; }
            else for (int e = 0; e < nv; ++e) p[e] = a.pre[base + e];
        }
        float val[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float z = v[e];
            if (!a.dgrad) {
                z += bo;
                p[e] = z;
                if (a.slope) z = z > 0.f ? z : sl * z;
                if (a.res) z = z * a.res_scale + r[e];
            } else {
                z *= a.alpha;
                if (a.slope) {
                    if (e < nv) sp += p[e] > 0.f ? 0.0 : (double)z * (double)p[e];
                    z = p[e] > 0.f ? z : sl * z;
                }
                if (a.res) z += r[e];
            }
            val[e] = z;
        }
        if (v4) {
            *reinterpret_cast<float4*>(a.out + base) = make_float4(val[0], val[1], val[2], val[3]);
            if (a.pre_out) *reinterpret_cast<float4*>(a.pre_out + base) = make_float4(p[0], p[1], p[2], p[3]);
        } else {
            for (int e = 0; e < nv; ++e) {
                a.out[base + e] = val[e];
                if (a.pre_out) a.pre_out[base + e] = p[e];
            }
        }
    };

    // one or two 16-pixel tiles of row y, each over four independent accumulation chains (K = channels x taps split by k-step mod 4,
    // added pairwise at the end: a quarter of the stock chain length, and no multiply waits for its predecessor)
    auto mac = [&](auto nt, int y, int ta, int tb) {
        constexpr int NT = decltype(nt)::value;
        f32x4t acc[NT][4];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4t){0.f, 0.f, 0.f, 0.f};
        const int pa = 16 * ta + m, pb = 16 * tb + m;
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
            const float* rrow = tk_smem + ((y + ky - HALO + 1) & 3) * KC * S + q * S + (1 - HALO);
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
#pragma unroll
                for (int ch = 0; ch < NC; ++ch) {
                    const float* rc = rrow + 4 * ch * S + kx;
                    const float bw = wr[ky * KS + kx][ch];
                    const int j = ((ky * KS + kx) * NC + ch) & 3;
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(rc[pa], bw, acc[0][j], 0, 0, 0);
                    if constexpr (NT == 2) acc[NT - 1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(rc[pb], bw, acc[NT - 1][j], 0, 0, 0);
                }
            }
        }
        epilogue((acc[0][0] + acc[0][1]) + (acc[0][2] + acc[0][3]), y, ta);
        if constexpr (NT == 2) epilogue((acc[NT - 1][0] + acc[NT - 1][1]) + (acc[NT - 1][2] + acc[NT - 1][3]), y, tb);
    };

    const int cols = (W - x0 < a.tw) ? W - x0 : a.tw;
    const int n_tiles = (cols + 15) / 16;
    for (int y = y0; y < y1; ++y) {
        const bool more = y + 1 < y1;
        if (more) fetch(y + HALO + 1);
        for (int t = tw; t < n_tiles; t += 2 * n_tw) {
            if (t + n_tw < n_tiles) mac(std::integral_constant<int, 2>(), y, t, t + n_tw);
            else mac(std::integral_constant<int, 1>(), y, t, t);
        }
        if (more) store(y + HALO + 1);                   // the slot of row y - HALO - 1: nobody reads it in this step
        __syncthreads();
    }

    if (a.dgrad && a.slope) {
        // fixed-order sums: lanes (butterfly), then the four waves in order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sp += __shfl_xor(sp, off);
        double* red = reinterpret_cast<double*>(tk_smem);
        if (lane == 0) red[wave] = sp;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < TK_FWAVES; ++w) s += red[w];
            a.slope_part[(size_t)blockIdx.z * gridDim.x + blockIdx.x] = s;
        }
    }
}

// weights [Cout][Cin][ks][ks] -> the B fragments of the effective convolution: [n_og][tap][nc][lane], lane = (k = c % 4) * 16 + o % 16.
// transposed: the convolution that computes the input gradient (outputs = the layer's inputs, taps mirrored)
__global__ __launch_bounds__(256) void trunk_pack_kernel(int Cin, int Cout, int T, int transposed, int n_og, int nc,
                                                         const float* __restrict__ w, float* __restrict__ wp) {
    const int n = n_og * T * nc * 64;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int lane = i & 63, ch = (i >> 6) % nc, t = (i / (64 * nc)) % T, og = i / (64 * nc * T);
    const int o = og * 16 + (lane & 15), c = 4 * ch + (lane >> 4);
    float v = 0.f;
    if (!transposed) {
        if (o < Cout && c < Cin) v = w[((size_t)o * Cin + c) * T + t];
    } else {
        if (o < Cin && c < Cout) v = w[((size_t)c * Cin + o) * T + (T - 1 - t)];
    }
    wp[i] = v;
}

struct TkWgradArgs {
    int Cin, Cout, H, W, n_cg, n_og, n_pairs, pb, ksplit, n_ct, tw, rows_per_block, n_strips;
    const float* x;            // [B, Cin, H, W]
    const float* dy;           // [B, Cout, H, W]
    float* part;               // [n_part][n_pairs][ks * ks * 256 + 16]
};

template <int KS>
__global__ __launch_bounds__(TK_THREADS, 1) void trunk_wgrad_kernel(TkWgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tk_smem[];
    constexpr int T = KS * KS, HALO = KS / 2, PS = T * 256 + 16;
    const int H = a.H, W = a.W, CW = a.tw + 2, Cin = a.Cin, Cout = a.Cout;
    const int KCx = a.n_cg * 16, KCo = a.n_og * 16;
    float* const xs = tk_smem;                                    // [4][KCx][66]
    float* const ds = xs + 4 * KCx * TK_WG_S;                     // [2][KCo][66]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ct = blockIdx.x % a.n_ct, strip = blockIdx.x / a.n_ct, b = blockIdx.z;
    const int x0 = ct * a.tw;
    const int y0 = strip * a.rows_per_block;
    const int y1 = (y0 + a.rows_per_block < H) ? y0 + a.rows_per_block : H;
    const int pl = wave % a.pb, ks = wave / a.pb;
    const int pair = blockIdx.y * a.pb + pl, cg = pair % a.n_cg, og = pair / a.n_cg;
    const int m = lane & 15, q = lane >> 4;
    const float* xb = a.x + (size_t)b * Cin * H * W;
    const float* db = a.dy + (size_t)b * Cout * H * W;

    float rx[8][2], rd[8];
    auto fetch_x = [&](int y) {
        const bool row_ok = y >= 0 && y < H;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int c = wave + TK_WAVES * r;
            const bool ok = row_ok && c < Cin;
            const float* src = xb + ((size_t)(ok ? c : 0) * H + (ok ? y : 0)) * W;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int col = lane + 64 * k, gx = x0 + col - 1;
                rx[r][k] = (ok && col < CW && gx >= 0 && gx < W) ? src[gx] : 0.f;
            }
        }
    };
    auto store_x = [&](int y) {
        float* s = xs + ((y + 1) & 3) * KCx * TK_WG_S;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int c = wave + TK_WAVES * r;
            if (c < KCx) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int col = lane + 64 * k;
                    if (col < CW) s[c * TK_WG_S + col] = rx[r][k];
                }
            }
        }
    };
    auto fetch_d = [&](int y) {                                   // staged column j holds pixel x0 + j
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int c = wave + TK_WAVES * r;
            const bool ok = y < H && c < Cout && lane < a.tw && x0 + lane < W;
            rd[r] = ok ? db[((size_t)c * H + y) * W + x0 + lane] : 0.f;
        }
    };
    auto store_d = [&](int y) {
        float* s = ds + (y & 1) * KCo * TK_WG_S;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int c = wave + TK_WAVES * r;
            if (c < KCo) s[c * TK_WG_S + lane] = rd[r];
        }
    };

    for (int y = y0 - HALO; y <= y0 + HALO; ++y) { fetch_x(y); store_x(y); }
    fetch_d(y0); store_d(y0);
    __syncthreads();

    f32x4t acc[T], acc2[T];                                       // two chains per tap: even / odd k-steps of the wave
#pragma unroll
    for (int t = 0; t < T; ++t) { acc[t] = (f32x4t){0.f, 0.f, 0.f, 0.f}; acc2[t] = acc[t]; }
    float bsum = 0.f;
    const int cols = (W - x0 < a.tw) ? W - x0 : a.tw;
    // a tile whose width is not a multiple of 4 ends in a partial step: its k lanes past the last real column hold zeros in dy, and
    // x must be zero there too -- xs holds the tile's last real pixels at those places (tap kx = 0), and inf * 0 is NaN.  The step
    // is peeled off the loops (their bound is the full steps) and run by the wave and into the chain that had it before: same bits
    const int n_steps = cols / 4;
    const int ks_u = __builtin_amdgcn_readfirstlane(ks);          // wave-uniform: the two branches below are scalar
    const bool part_mine = (cols & 3) && n_steps % a.ksplit == ks_u;
    const bool part_odd = ((n_steps - ks_u) / a.ksplit) & 1;
    const bool k_real = q < (cols & 3);
    for (int y = y0; y < y1; ++y) {
        const bool more = y + 1 < y1;
        if (more) { fetch_x(y + HALO + 1); fetch_d(y + 1); }
        // A[m = channel cg * 16 + m][k = pixel 4 s + q] (+ tap), B[k = pixel][n = output channel og * 16 + m]
        const float* dp = ds + (y & 1) * KCo * TK_WG_S + (og * 16 + m) * TK_WG_S + q;
        const float* xp[KS];
#pragma unroll
        for (int ky = 0; ky < KS; ++ky)
            xp[ky] = xs + ((y + ky - HALO + 1) & 3) * KCx * TK_WG_S + (cg * 16 + m) * TK_WG_S + q + (1 - HALO);
        int s = ks;
        for (; s + a.ksplit < n_steps; s += 2 * a.ksplit) {
            const int p0 = 4 * s, p1 = 4 * (s + a.ksplit);
            const float bv = dp[p0], bv1 = dp[p1];
            bsum += bv;
            bsum += bv1;
#pragma unroll
            for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    acc[ky * KS + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(xp[ky][p0 + kx], bv, acc[ky * KS + kx], 0, 0, 0);
                    acc2[ky * KS + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(xp[ky][p1 + kx], bv1, acc2[ky * KS + kx], 0, 0, 0);
                }
        }
        if (s < n_steps) {
            const int p0 = 4 * s;
            const float bv = dp[p0];
            bsum += bv;
#pragma unroll
            for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                for (int kx = 0; kx < KS; ++kx)
                    acc[ky * KS + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(xp[ky][p0 + kx], bv, acc[ky * KS + kx], 0, 0, 0);
        }
        if (part_mine) {
            const int p0 = 4 * n_steps;
            const float bv = dp[p0];
            bsum += bv;
#pragma unroll
            for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    const float av = k_real ? xp[ky][p0 + kx] : 0.f;
                    if (part_odd) acc2[ky * KS + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc2[ky * KS + kx], 0, 0, 0);
                    else acc[ky * KS + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[ky * KS + kx], 0, 0, 0);
                }
        }
        if (more) { store_x(y + HALO + 1); store_d(y + 1); }
        __syncthreads();
    }

#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] += acc2[t];
    // the k-split waves of a pair: fixed-order tree over LDS (the rings are dead, the buffer overlays them)
    constexpr int RED = (T * 4 + 1) * 64;
    for (int half = a.ksplit / 2; half >= 1; half >>= 1) {
        if (ks >= half && ks < 2 * half) {
            float* r = tk_smem + ((ks - half) * a.pb + pl) * RED;
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) r[(t * 4 + e) * 64 + lane] = acc[t][e];
            r[T * 4 * 64 + lane] = bsum;
        }
        __syncthreads();
        if (ks < half) {
            const float* r = tk_smem + (ks * a.pb + pl) * RED;
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t][e] += r[(t * 4 + e) * 64 + lane];
            bsum += r[T * 4 * 64 + lane];
        }
        __syncthreads();
    }
    if (ks == 0) {
        // D[row = channel 4 q + e][col = output channel m] -> [tap][o][c]: four consecutive channels per lane
        const size_t pblock = ((size_t)b * a.n_strips + strip) * a.n_ct + ct;
        float* out = a.part + (pblock * a.n_pairs + pair) * PS;
#pragma unroll
        for (int t = 0; t < T; ++t)
            *reinterpret_cast<float4*>(out + (t * 16 + m) * 16 + 4 * q) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
        bsum += __shfl_xor(bsum, 16);
        bsum += __shfl_xor(bsum, 32);
        if (lane < 16) out[T * 256 + lane] = bsum;
    }
}

struct TkReduceArgs {
    int Cin, Cout, T, n_cg, n_pairs, n_part, n_slope;
    float alpha;
    const float* part;
    const double* slope_part;
    float* d_w; float* d_b; float* d_slope;
};

// Block = 64 consecutive sums x 4 interleaved quarters of the blocks' partials, the quarters added in order: the same bits on every call
__global__ __launch_bounds__(256) void trunk_wgrad_reduce_kernel(TkReduceArgs a) {
    __shared__ float sq[4][64];
    __shared__ double sdq[4];
    const int PS = a.T * 256 + 16, NW = a.n_pairs * PS;
    const int j = threadIdx.x & 63, qq = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + j;
    float s = 0.f;
    double sd = 0.0;
    if (i < NW) {
        for (int p = qq; p < a.n_part; p += 4) s += a.part[(size_t)p * NW + i];
    } else if (i == NW && a.slope_part) {
        for (int p = qq; p < a.n_slope; p += 4) sd += a.slope_part[p];
    }
    sq[qq][j] = s;
    if (i == NW) sdq[qq] = sd;
    __syncthreads();
    if (qq != 0) return;
    s = ((sq[0][j] + sq[1][j]) + sq[2][j]) + sq[3][j];
    if (i < NW) {
        const int pair = i / PS, r = i - pair * PS, cg = pair % a.n_cg, og = pair / a.n_cg;
        if (r < a.T * 256) {
            const int t = r >> 8, o = og * 16 + ((r >> 4) & 15), c = cg * 16 + (r & 15);
            if (o < a.Cout && c < a.Cin) a.d_w[((size_t)o * a.Cin + c) * a.T + t] = s * a.alpha;
        } else {
            const int o = og * 16 + (r - a.T * 256);
            if (cg == 0 && o < a.Cout && a.d_b) a.d_b[o] = s * a.alpha;
        }
    } else if (i == NW && a.d_slope) {
        a.d_slope[0] = (float)(((sdq[0] + sdq[1]) + sdq[2]) + sdq[3]);
    }
}

static bool tk_shape_ok(int B, int Cin, int Cout, int H, int W, int ks) {
    return B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cin <= TK_MAX_C && Cout >= 1 && Cout <= TK_MAX_C && (ks == 1 || ks == 3);
}

static bool tk_a16(const void* p) { return p == nullptr || ((uintptr_t)p % 16) == 0; }

typedef void (*TkConvKernel)(TkConvArgs);

template <int KS>
static TkConvKernel tk_conv_kernel(int nc) {
    switch (nc) {
        case 1: return trunk_conv_kernel<KS, 1>;
        case 2: return trunk_conv_kernel<KS, 2>;
        case 4: return trunk_conv_kernel<KS, 4>;
        case 8: return trunk_conv_kernel<KS, 8>;
        default: return trunk_conv_kernel<KS, 16>;
    }
}

// one launch of the conv kernel: (Cin, Cout) are the EFFECTIVE convolution's (the input gradient swaps them)
static int tk_launch_conv(hipStream_t s, int B, int H, int W, int ks, TkConvArgs& a, const char* what) {
    const int nc = tk_nc(a.Cin);
    a.n_og = tk_ngroups(a.Cout);
    const TkTiling t = tk_tiling(B, H, W, TK_FWD_TW, 16, 1);
    a.n_ct = t.n_ct; a.tw = t.tw; a.rows_per_block = t.rows_per_block;
    a.stride = tk_fwd_stride(t.tw);
    a.vec = (W % 4) == 0 && tk_a16(a.out) && tk_a16(a.pre_out) && tk_a16(a.res) && tk_a16(a.pre);
    const size_t lds = (size_t)4 * nc * 4 * a.stride * sizeof(float);
    TkConvKernel k = (ks == 3) ? tk_conv_kernel<3>(nc) : tk_conv_kernel<1>(nc);
    DAGL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(t.n_strips * t.n_ct, 1, B), dim3(TK_FTHREADS), lds, s, a);
    DAGL_LAUNCH_CHECK(what);
    return DAGL_OK;
}

static int tk_wgrad_pb(int n_pairs) { return n_pairs < TK_WAVES ? n_pairs : TK_WAVES; }

}  // namespace dagl

using namespace dagl;

extern "C" {

size_t dagl_trunk_packed_floats(int Cin, int Cout, int ksize, int transposed) {
    if (!tk_shape_ok(1, Cin, Cout, 1, 1, ksize)) return 0;
    const int ci = transposed ? Cout : Cin, co = transposed ? Cin : Cout;
    return (size_t)tk_ngroups(co) * ksize * ksize * tk_nc(ci) * 64;
}

int dagl_trunk_pack_weights(void* stream, int Cin, int Cout, int ksize, int transposed, const float* w, float* packed) {
    DAGL_REQUIRE(tk_shape_ok(1, Cin, Cout, 1, 1, ksize), "dagl_trunk_pack_weights: 1 <= Cin, Cout <= 64 and ksize 1 or 3 required");
    DAGL_REQUIRE(w && packed, "dagl_trunk_pack_weights: null pointer");
    const int ci = transposed ? Cout : Cin, co = transposed ? Cin : Cout;
    const int n = (int)dagl_trunk_packed_floats(Cin, Cout, ksize, transposed);
    hipLaunchKernelGGL(trunk_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, Cin, Cout, ksize * ksize,
                       transposed ? 1 : 0, tk_ngroups(co), tk_nc(ci), w, packed);
    DAGL_LAUNCH_CHECK("trunk_pack_kernel");
    return DAGL_OK;
}

int dagl_trunk_conv_forward(void* stream, int B, int Cin, int Cout, int H, int W, int ksize, const float* x, const float* packed,
                            const float* bias, const float* slope, float* pre_out, float res_scale, const float* residual, float* out) {
    DAGL_REQUIRE(tk_shape_ok(B, Cin, Cout, H, W, ksize), "dagl_trunk_conv_forward: B, H, W >= 1, 1 <= Cin, Cout <= 64, ksize 1 or 3 required");
    DAGL_REQUIRE(x && packed && out, "dagl_trunk_conv_forward: null pointer");
    DAGL_REQUIRE(!pre_out || slope, "dagl_trunk_conv_forward: the pre-activation output needs the PReLU slope");
    TkConvArgs a = {};
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.dgrad = 0;
    a.x = x; a.wp = packed; a.bias = bias; a.slope = slope; a.res = residual; a.res_scale = res_scale; a.alpha = 1.f;
    a.out = out; a.pre_out = pre_out;
    return tk_launch_conv((hipStream_t)stream, B, H, W, ksize, a, "trunk_conv_kernel (forward)");
}

int dagl_trunk_input_grad_blocks(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    const TkTiling t = tk_tiling(B, H, W, TK_FWD_TW, 16, 1);
    return B * t.n_strips * t.n_ct;
}

int dagl_trunk_conv_input_grad(void* stream, int B, int Cin, int Cout, int H, int W, int ksize, const float* d_out,
                               const float* packed_t, float alpha, const float* slope, const float* pre, double* slope_part,
                               const float* skip_grad, float* d_in) {
    DAGL_REQUIRE(tk_shape_ok(B, Cin, Cout, H, W, ksize), "dagl_trunk_conv_input_grad: B, H, W >= 1, 1 <= Cin, Cout <= 64, ksize 1 or 3 required");
    DAGL_REQUIRE(d_out && packed_t && d_in, "dagl_trunk_conv_input_grad: null pointer");
    DAGL_REQUIRE(!slope || (pre && slope_part), "dagl_trunk_conv_input_grad: the PReLU backward needs the pre-activation and the slope partials");
    TkConvArgs a = {};
    a.Cin = Cout; a.Cout = Cin; a.H = H; a.W = W; a.dgrad = 1;
    a.x = d_out; a.wp = packed_t; a.slope = slope; a.pre = pre; a.res = skip_grad; a.res_scale = 1.f; a.alpha = alpha;
    a.out = d_in; a.slope_part = slope_part;
    return tk_launch_conv((hipStream_t)stream, B, H, W, ksize, a, "trunk_conv_kernel (input gradient)");
}

size_t dagl_trunk_weight_grad_scratch_bytes(int B, int Cin, int Cout, int H, int W, int ksize) {
    if (!tk_shape_ok(B, Cin, Cout, H, W, ksize)) return 0;
    const int n_pairs = tk_ngroups(Cin) * tk_ngroups(Cout);
    const TkTiling t = tk_tiling(B, H, W, TK_WG_TW, 4, n_pairs / tk_wgrad_pb(n_pairs));
    const size_t n_part = (size_t)B * t.n_strips * t.n_ct;
    return n_part * n_pairs * (ksize * ksize * 256 + 16) * sizeof(float);
}

int dagl_trunk_conv_weight_grad(void* stream, int B, int Cin, int Cout, int H, int W, int ksize, const float* x, const float* d_out,
                                float alpha, float* d_w, float* d_b, const double* slope_part, int n_slope_part, float* d_slope,
                                void* scratch, size_t scratch_bytes) {
    DAGL_REQUIRE(tk_shape_ok(B, Cin, Cout, H, W, ksize), "dagl_trunk_conv_weight_grad: B, H, W >= 1, 1 <= Cin, Cout <= 64, ksize 1 or 3 required");
    DAGL_REQUIRE(x && d_out && d_w, "dagl_trunk_conv_weight_grad: null pointer");
    DAGL_REQUIRE(!d_slope || (slope_part && n_slope_part >= 1), "dagl_trunk_conv_weight_grad: the slope gradient needs its partials");
    const size_t need = dagl_trunk_weight_grad_scratch_bytes(B, Cin, Cout, H, W, ksize);
    DAGL_REQUIRE(scratch && tk_a16(scratch) && scratch_bytes >= need,
                 "dagl_trunk_conv_weight_grad: scratch must be 16-byte aligned and hold %zu bytes", need);
    hipStream_t s = (hipStream_t)stream;
    TkWgradArgs a = {};
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
    a.n_cg = tk_ngroups(Cin); a.n_og = tk_ngroups(Cout); a.n_pairs = a.n_cg * a.n_og;
    a.pb = tk_wgrad_pb(a.n_pairs); a.ksplit = TK_WAVES / a.pb;
    const int gy = a.n_pairs / a.pb;
    const TkTiling t = tk_tiling(B, H, W, TK_WG_TW, 4, gy);
    a.n_ct = t.n_ct; a.tw = t.tw; a.rows_per_block = t.rows_per_block; a.n_strips = t.n_strips;
    a.x = x; a.dy = d_out; a.part = static_cast<float*>(scratch);
    const int T = ksize * ksize;
    const size_t ring = (size_t)(4 * a.n_cg * 16 + 2 * a.n_og * 16) * TK_WG_S * sizeof(float);
    const size_t red = (size_t)(a.ksplit / 2) * a.pb * (T * 4 + 1) * 64 * sizeof(float);
    const size_t lds = ring > red ? ring : red;
    auto k = (ksize == 3) ? trunk_wgrad_kernel<3> : trunk_wgrad_kernel<1>;
    DAGL_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(t.n_strips * t.n_ct, gy, B), dim3(TK_THREADS), lds, s, a);
    DAGL_LAUNCH_CHECK("trunk_wgrad_kernel");
    TkReduceArgs r = {};
    r.Cin = Cin; r.Cout = Cout; r.T = T; r.n_cg = a.n_cg; r.n_pairs = a.n_pairs;
    r.n_part = B * t.n_strips * t.n_ct; r.n_slope = d_slope ? n_slope_part : 0; r.alpha = alpha;
    r.part = a.part; r.slope_part = d_slope ? slope_part : nullptr; r.d_w = d_w; r.d_b = d_b; r.d_slope = d_slope;
    const int n_out = a.n_pairs * (T * 256 + 16) + 1;
    hipLaunchKernelGGL(trunk_wgrad_reduce_kernel, dim3((n_out + 63) / 64), dim3(256), 0, s, r);
    DAGL_LAUNCH_CHECK("trunk_wgrad_reduce_kernel");
    return DAGL_OK;
}

}  // extern "C"
