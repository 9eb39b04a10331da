// Dense neighbourhoods under autograd: forward + backward of the graph core (DN_Gray/model/dagl.py:250-272) when a
// query keeps more keys than a fixed-width list holds (default-initialised thr/bias heads keep ~95 % of the keys: the
// regime a training run starts in).  This is the reference's dense formulation -- S = Wq X^T, mask, softmax over ALL
// keys, A V -- and exactly what autograd derives from it, chunked over the queries so that the [L,N] matrices exist only
// one chunk at a time:
//
//   forward, per chunk of queries          S = Wq X^T                               gemm32  (dagl.py:250)
//                                          A = softmax(10 S m) mask_b, m = relu(..)  dense_softmax_fwd_kernel (:256-261)
//                                          agg = A V                                gemm32  (:263-264),  then fold (:265-272)
//   backward, per chunk                    d A = d agg V^T                          gemm32
//                                          S recomputed; c = sum_j A d A; d l = A (d A - c);
//                                          d S = 10 (m + S) d l, d m = 10 S d l       dense_softmax_bwd_kernel
//                                          d Wq = d S X,  d X += d S^T Wq,  d V += A^T d agg        gemm32 x 3
//   plus the dense mean term of dagl.py:256: mu_l = Wq_l . Xbar  ->  d Wq_l += d mu_l Xbar, d X_j += (sum_l d mu_l Wq_l)/N.
// V = the unfolded value patches [N,784] of one image (materialised here, as the reference does at :224-231; the
// inference paths never do); d V is folded back onto the 16-channel map by a gather (49 taps per pixel, no atomics).
// All sums run in a fixed order: bit-reproducible gradients.
#include "dagl_common.h"
#include "wide_select.h"
#include <atomic>

namespace dagl {

constexpr size_t DT_CHUNK_FLOATS = (size_t)128 << 20;      // floats per [chunk, N] matrix (512 MiB): the built-in budget
// the budget in force (dagl_ce_core_dense_chunk_floats: a testing and tuning hook); dt_plan reads it once per call
static std::atomic<long long> dt_chunk_floats{(long long)DT_CHUNK_FLOATS};

struct DtPlan {
    int Lc, n_chunks, Bc;            // queries per chunk, chunks per image, images per group
    long long ldn;                   // leading dimension of the [L,N] chunk matrices (N rounded up to 32)
    bool h16;                        // split-fp16 backward (one chunk per image group only)
    int Lp, kslices;                 // L rounded up to 32; split-K of d Wq
    int nk;                          // N rounded up to 32 kslices: the K extent of the copies whose rows run over the keys
    long long ldl, ldk;              // leading dimensions (halfs) of the copies whose rows run over the queries / the keys: extent + 64 -- a
                                     // power-of-two row stride (L = 1024: 2 KiB, N = 16384: 32 KiB) sends the 16 rows of every LDS-DMA piece
                                     // to the same memory channel (the products ran at a third of the fp32 ones' rate)
};

constexpr int DT_PK = 800;           // value-patch length 784 rounded up to the K step (50 taps of 16)
constexpr int DT_DK = 224;           // feature length 196 rounded up to the K step

static DtPlan dt_plan(int B, const Grid& g, bool backward) {
    DtPlan p;
    const size_t budget = (size_t)dt_chunk_floats.load(std::memory_order_relaxed);
    p.ldn = (g.N + 31) / 32 * 32;
    // (measured: skewing rows that are a multiple of 2 KiB long by 128 bytes does nothing for the row-per-block softmax kernels)
    long long lc = (long long)(budget / (size_t)p.ldn) / 128 * 128;
    if (lc < 128) lc = 128;
    p.Lc = (int)(lc < g.L ? lc : g.L);
    p.n_chunks = (g.L + p.Lc - 1) / p.Lc;
    p.Bc = 1;
    if (p.n_chunks == 1) {
        long long bc = (long long)(budget / ((size_t)p.Lc * p.ldn));
        p.Bc = (int)(bc < 1 ? 1 : (bc > B ? B : bc));
    }
    p.h16 = backward && p.n_chunks == 1;
    p.Lp = (g.L + 31) / 32 * 32;
    p.kslices = 1;
    {
        // d Wq = d S X: (L / 128) x 2 output tiles per image -- split K (the keys) until the launch fills the chip
        const long long tiles = (long long)((g.L + 127) / 128) * 2 * p.Bc;
        while (p.kslices < 8 && tiles * p.kslices < 512 && g.N >= 512 * p.kslices) p.kslices *= 2;
    }
    p.nk = (g.N + 32 * p.kslices - 1) / (32 * p.kslices) * (32 * p.kslices);
    p.ldl = p.Lp + 64; p.ldk = p.nk + 64;
    return p;
}

// The operands of the products, each described ONCE (dt_carve) for the launch that writes it and the products that read it.
// fp32: one matrix per image of the group, `stride` floats apart, rows `ld` floats apart; kc: the product's contraction index runs
// along the rows (Gemm32::a_kc / b_kc), down(): the same matrix contracted over its row index
template <class T>
struct MatT {
    T* p = nullptr; long long ld = 0, stride = 0; int kc = 1;
    MatT() = default;
    MatT(T* p_, long long ld_, long long stride_, int kc_ = 1) : p(p_), ld(ld_), stride(stride_), kc(kc_) {}
    template <class U> MatT(const MatT<U>& o) : p(o.p), ld(o.ld), stride(o.stride), kc(o.kc) {}      // a written matrix, read
    MatT down() const { return MatT(p, ld, stride, 0); }
};
using Mat32 = MatT<const float>;
using Out32 = MatT<float>;
// split fp16 (gemm16s.hip), K-contiguous rows of `ld` halfs: s x = hi + lo, lo `lo` halfs behind hi; s from *word (the tensor's largest
// magnitude, fcg_scale_of) or `fixed` where there is no word
struct Split16 { unsigned short* hi = nullptr; size_t lo = 0; long long ld = 0, stride = 0; const unsigned* word = nullptr; float fixed = 1.f; };

// the workspace of one call: the one walk that sizes it (null base) and hands its regions to the launches
struct DtWs {
    Out32 S, A, V, dV;               // [Bc][Lc][ldn] scores -> weights / d S, d A -> weights (backward); [Bc][N][P] value patches and their gradient
    float *dagg, *agg, *b2p;         // [B,L,P] d agg (backward) / agg (forward); b2 padded NHWC
    double* colsum; float *mt, *dmu, *dxbar; int32_t* deg; float* rowsum;
    int32_t* sel;                    // wide top-k modes: (sort key of the k-th best score, last key index taken at it)
    float *lse, *mu;                 // (their entry points keep the softmax statistics and the row means here)
    unsigned* words;                 // h16: the scale words -- 0 d agg, 1 values, 2 X, 3 Wq, 4 d S
    Split16 dgk, vk, xk, wqk, dsk;   // h16: d agg, V, X, Wq, d S by rows ...
    Split16 dgt, xt, wqt, dst, at;   // ... and d agg, X, Wq, d S, A transposed (A <= 1: 2^13, no word)
    float* part;                     // h16: split-K partial sums of d Wq
    size_t bytes;
};
static DtWs dt_carve(void* ws, int B, const Grid& g, const DtPlan& p, bool backward) {
    Carver cv(ws);
    DtWs w{};
    const size_t chunk = (size_t)p.Bc * p.Lc * p.ldn, BL = (size_t)B * g.L;
    const long long sS = (long long)p.Lc * p.ldn, sV = (long long)g.N * P;
    w.S = Out32(cv.take<float>(chunk), p.ldn, sS);
    if (backward) w.A = Out32(cv.take<float>(chunk), p.ldn, sS);
    w.V = Out32(cv.take<float>((size_t)p.Bc * sV), P, sV);
    if (backward) w.dV = Out32(cv.take<float>((size_t)p.Bc * sV), P, sV);
    (backward ? w.dagg : w.agg) = cv.take<float>(BL * P);
    w.b2p = cv.take<float>((size_t)B * g.Hp * g.Wp * CH);
    w.colsum = cv.take<double>((size_t)B * DS);
    w.mt = cv.take<float>(BL);
    w.dmu = cv.take<float>(BL);
    w.dxbar = cv.take<float>((size_t)B * D);
    w.deg = cv.take<int32_t>(BL);
    w.rowsum = cv.take<float>(BL);
    w.sel = cv.take<int32_t>(BL * 2);
    w.lse = cv.take<float>(BL * 2);
    w.mu = cv.take<float>(BL);
    if (p.h16) {
        w.words = cv.take<unsigned>(64);
        const auto split = [&](int rows, long long ld, int word) {       // [Bc][rows][ld] halfs, hi then lo
            const size_t halfs = (size_t)p.Bc * rows * ld;
            Split16 o;
            o.hi = cv.take<unsigned short>(2 * halfs); o.lo = halfs; o.ld = ld; o.stride = (long long)rows * ld;
            if (word < 0) o.fixed = 8192.f; else if (w.words) o.word = w.words + word;
            return o;
        };
        w.dgk = split(g.L, DT_PK, 0); w.dgt = split(P, p.ldl, 0); w.vk = split(g.N, DT_PK, 1);
        w.xk = split(g.N, DT_DK, 2); w.xt = split(D, p.ldk, 2); w.wqk = split(g.L, DT_DK, 3); w.wqt = split(D, p.ldl, 3);
        w.dsk = split(p.Lc, p.ldk, 4); w.dst = split(g.N, p.ldl, 4); w.at = split(g.N, p.ldl, -1);
        w.part = cv.take<float>((size_t)p.kslices * p.Bc * g.L * D);
    }
    w.bytes = cv.bytes();
    return w;
}

size_t dense_train_workspace_bytes(int B, const Grid& g, bool backward) { return dt_carve(nullptr, B, g, dt_plan(B, g, backward), backward).bytes; }

long long dense_train_chunk_floats(long long floats) {
    return dt_chunk_floats.exchange(floats > 0 ? floats : (long long)DT_CHUNK_FLOATS, std::memory_order_relaxed);
}

void dense_train_plan(int B, const Grid& g, bool backward, int32_t out[6]) {
    const DtPlan p = dt_plan(B, g, backward);
    out[0] = p.Lc; out[1] = p.n_chunks; out[2] = p.Bc; out[3] = p.kslices; out[4] = p.nk; out[5] = p.h16 ? 1 : 0;
}


// mu[b,l] = Wq_l . colsum / N (fp64 dot, as query_thresholds_kernel), mt = mu * thr: one wave per query, dense rows
__global__ __launch_bounds__(256) void dt_thresholds_kernel(int L, int N, const float* __restrict__ wq_rows,
                                                            const double* __restrict__ colsum, const float* __restrict__ thr,
                                                            float* __restrict__ mt, float* __restrict__ mu) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= L) return;
    const float* q = wq_rows + ((size_t)b * L + l) * D;
    const double* cs = colsum + (size_t)b * DS;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) acc += (double)q[d] * cs[d];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        const float mean = (float)(acc / (double)N);
        mu[(size_t)b * L + l] = mean;
        mt[(size_t)b * L + l] = mean * thr[(size_t)b * L + l];
    }
}

// wide top-k modes: one block per query row of the chunk -> sel[ql] = (T, jt)
template <bool ADAPTIVE>
__global__ __launch_bounds__(256) void dt_select_kernel(int N, long long ldn, int L, int l0, int Lc, int k, const float* __restrict__ sbuf,
                                                        const float* __restrict__ mt, const float* __restrict__ bs,
                                                        int32_t* __restrict__ sel, int b0) {
    __shared__ WideSelShared shs;
    __shared__ WideTieShared sht;
    const int lr = blockIdx.x, bi = blockIdx.y, tid = threadIdx.x;
    const size_t ql = (size_t)(b0 + bi) * L + l0 + lr;
    const float* row = sbuf + ((size_t)bi * Lc + lr) * ldn;
    const float mtq = ADAPTIVE ? mt[ql] : 0.f, bsq = ADAPTIVE ? bs[ql] : 0.f;
    unsigned T, need, bin_count;
    wide_radix_select(row, N, k, ADAPTIVE, mtq, bsq, shs, T, need, bin_count);
    const int jt = wide_tie_index(row, N, ADAPTIVE, mtq, bsq, T, need, bin_count, sht);
    if (tid == 0) { sel[2 * ql] = (int32_t)T; sel[2 * ql + 1] = jt; }
}

// one block per query row: S row -> A row in place (dagl.py:256-261); saves the softmax shift and denominator
template <int MODE>
__global__ __launch_bounds__(256) void dense_softmax_fwd_kernel(int N, long long ldn, int L, int l0, int Lc,
                                                                float* __restrict__ sbuf, const float* __restrict__ mt,
                                                                const float* __restrict__ bs, float* __restrict__ lse,
                                                                int32_t* __restrict__ deg, float* __restrict__ rowsum, int b0,
                                                                const int32_t* __restrict__ sel) {
    __shared__ double shd[4];
    __shared__ float shf[4];
    const int lr = blockIdx.x, bi = blockIdx.y;
    const size_t ql = (size_t)(b0 + bi) * L + l0 + lr;
    float* row = sbuf + ((size_t)bi * Lc + lr) * ldn;
    const float mtq = MODE == 1 ? 0.f : mt[ql], bsq = MODE == 1 ? 0.f : bs[ql];
    const unsigned T = MODE == 0 ? 0u : (unsigned)sel[2 * ql];
    const int jt = MODE == 0 ? 0 : sel[2 * ql + 1];
    float mx = 0.f;                                    // masked keys have logit 0 (N > deg) -- and if all pass, max >= ... handled below
    int cnt = 0;
    for (int j = threadIdx.x; j < N; j += 256) {
        bool pass; float m;
        const float l = row_logit<MODE>(row[j], j, mtq, bsq, SOFTMAX_SCALE, T, jt, pass, m);
        cnt += pass ? 1 : 0;
        mx = pass ? fmaxf(mx, l) : mx;
    }
    // (logits of passing keys are positive: S > 0 and m > 0, or zero when S = 0; so max over all keys = max(0, ...) either way)
    const float M = block_max_f32(mx, shf);
    double z = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) {
        bool pass; float m;
        const float l = row_logit<MODE>(row[j], j, mtq, bsq, SOFTMAX_SCALE, T, jt, pass, m);
        z += (double)expf(l - M);
    }
    const double Z = block_sum_f64(z, shd);
    const float invz = (float)(1.0 / Z);
    double rs = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) {
        bool pass; float m;
        const float l = row_logit<MODE>(row[j], j, mtq, bsq, SOFTMAX_SCALE, T, jt, pass, m);
        const float a = pass ? expf(l - M) * invz : 0.f;
        row[j] = a;
        rs += (double)a;
    }
    for (int j = N + threadIdx.x; j < ldn; j += 256) row[j] = 0.f;           // pad columns: zero weights
    const double RS = block_sum_f64(rs, shd);
    const double C = block_sum_f64((double)cnt, shd);
    if (threadIdx.x == 0) {
        lse[2 * ql] = M; lse[2 * ql + 1] = (float)Z;
        deg[ql] = (int32_t)C; rowsum[ql] = (float)RS;
    }
}

// one block per query row: sbuf = recomputed S row, abuf = d A row  ->  sbuf = d S row, abuf = A row
template <int MODE>
__global__ __launch_bounds__(256) void dense_softmax_bwd_kernel(int N, long long ldn, int L, int l0, int Lc,
                                                                float* __restrict__ sbuf, float* __restrict__ abuf,
                                                                const float* __restrict__ mt, const float* __restrict__ bs,
                                                                const float* __restrict__ lse, const float* __restrict__ mu,
                                                                const float* __restrict__ thr, float* __restrict__ dthr,
                                                                float* __restrict__ dbias, float* __restrict__ dmu, int b0,
                                                                unsigned* __restrict__ ds_word, const int32_t* __restrict__ sel) {
    __shared__ double shd[4];
    const int lr = blockIdx.x, bi = blockIdx.y;
    const size_t ql = (size_t)(b0 + bi) * L + l0 + lr;
    float* srow = sbuf + ((size_t)bi * Lc + lr) * ldn;
    float* arow = abuf + ((size_t)bi * Lc + lr) * ldn;
    float ds_max = 0.f;
    const float mtq = MODE == 1 ? 0.f : mt[ql], bsq = MODE == 1 ? 0.f : bs[ql];
    const unsigned T = MODE == 0 ? 0u : (unsigned)sel[2 * ql];
    const int jt = MODE == 0 ? 0 : sel[2 * ql + 1];
    // The softmax's shift and denominator are formed HERE, from the recomputed scores -- not taken from the forward: the
    // forward may have run on the streamed split-fp16 kernel, whose scores differ from these in the last bits; logits of
    // several hundred turn that into ~1e-3 of every weight of the row, and the head biases' gradients (sums over all
    // queries that cancel to 1e-4 of their terms) are only right when the weights are normalised by their own sum.
    (void)lse;
    __shared__ float shf[4];
    float mx = 0.f;
#pragma unroll 16
    for (int j = threadIdx.x; j < N; j += 256) {
        bool pass; float m;
        const float l = row_logit<MODE>(srow[j], j, mtq, bsq, SOFTMAX_SCALE, T, jt, pass, m);
        mx = pass ? fmaxf(mx, l) : mx;
    }
    const float M = block_max_f32(mx, shf);
    double zz = 0.0;
#pragma unroll 16
    for (int j = threadIdx.x; j < N; j += 256) {
        bool pass; float m;
        const float l = row_logit<MODE>(srow[j], j, mtq, bsq, SOFTMAX_SCALE, T, jt, pass, m);
        zz += (double)expf(l - M);
    }
    const float invz = (float)(1.0 / block_sum_f64(zz, shd));
    double c = 0.0;
#pragma unroll 16
    for (int j = threadIdx.x; j < N; j += 256) {
        bool pass; float m;
        const float l = row_logit<MODE>(srow[j], j, mtq, bsq, SOFTMAX_SCALE, T, jt, pass, m);
        const float a = pass ? expf(l - M) * invz : 0.f;
        c += (double)a * (double)arow[j];
    }
    const float cf = (float)block_sum_f64(c, shd);
    double sdm = 0.0;
#pragma unroll 16
    for (int j = threadIdx.x; j < N; j += 256) {
        bool pass; float m;
        const float s = srow[j];
        const float l = row_logit<MODE>(s, j, mtq, bsq, SOFTMAX_SCALE, T, jt, pass, m);
        const float a = pass ? expf(l - M) * invz : 0.f;
        const float dl = a * (arow[j] - cf);           // non-neighbours: A = 0 and their logit is the constant 0
        const float ds = MODE == 1 ? SOFTMAX_SCALE * dl          // the 0/1 mask is a constant: d (10 S) / d S
                                   : SOFTMAX_SCALE * (m + s) * dl; // d S  (a = 0 -> 0)
        srow[j] = ds;
        ds_max = fmaxf(ds_max, fabsf(ds));
        arow[j] = a;
        sdm += (double)(SOFTMAX_SCALE * s * dl);       // d m
    }
    for (int j = N + threadIdx.x; j < ldn; j += 256) { srow[j] = 0.f; arow[j] = 0.f; }
    const float S = (float)block_sum_f64(sdm, shd);
    if (ds_word != nullptr) {                          // the split-fp16 products' scale for d S (order-independent integer maximum)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ds_max = fmaxf(ds_max, __shfl_xor(ds_max, o));
        if ((threadIdx.x & 63) == 0 && ds_max > 0.f && ds_max < __builtin_inff()) atomicMax(ds_word, __float_as_uint(ds_max));
    }
    if (threadIdx.x == 0 && MODE != 1) {
        dbias[ql] = S;
        dthr[ql] = -mu[ql] * S;
        dmu[ql] = -thr[ql] * S;
    }
}

// (Measured and dropped: the row in registers -- S and d A read once, one expf per weight, 16-byte accesses; 512 threads x 32
// elements, 1 or 2 blocks per CU: 832 us against this kernel's 867 at [8, 1024 x 16384], whatever the variant.  2.1 GB in 0.83 ms;
// this kernel without its stores: 666 us -- one load in flight per thread and pass; the register form has all of a row's loads in
// flight but one block per CU, whose load / reduce / store phases do not overlap with anything: ~26 us per row and CU either way.)

// a chunk of queries of an image group: the coordinates the row-per-block kernels index with (grid = lc rows x nb images)
struct DtChunk { int b0, nb, l0, lc; int N; long long ldn; int L, Lc; };
static DtChunk dt_chunk(const Grid& g, const DtPlan& p, int b0, int nb, int l0) {
    return {b0, nb, l0, (g.L - l0 < p.Lc) ? g.L - l0 : p.Lc, g.N, p.ldn, g.L, p.Lc};
}
// the chunk's rows of a [B, L, cols] tensor (one row per query) / its images' rows of a [B, N, cols] one (one row per key)
template <class T> static MatT<T> dt_query_rows(const DtChunk& c, T* t, int cols) { return {t + ((size_t)c.b0 * c.L + c.l0) * cols, cols, (long long)c.L * cols}; }
template <class T> static MatT<T> dt_key_rows(const DtChunk& c, T* t, int cols) { return {t + (size_t)c.b0 * c.N * cols, cols, (long long)c.N * cols}; }

// wide top-k modes: the rows' (T, jt) from the chunk's scores
static int launch_dt_select(hipStream_t s, const DtChunk& c, int mode, int k, const DtWs& w, const float* bs) {
    const auto kern = mode == DAGL_MODE_ADAPTIVE_TOPK ? dt_select_kernel<true> : dt_select_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(c.lc, c.nb), dim3(256), 0, s, c.N, c.ldn, c.L, c.l0, c.Lc, k, w.S.p, w.mt, bs, w.sel, c.b0);
    DAGL_LAUNCH_CHECK("dt_select_kernel");
    return DAGL_OK;
}

// S, d A -> d S, A over the chunk's rows; ds_word: the split-fp16 products' scale word of d S, or null
static int launch_dense_softmax_bwd(hipStream_t s, const DtChunk& c, const DenseTrainBackward& a, const DtWs& w, const float* mu,
                                    unsigned* ds_word) {
    const auto kern = a.mode == DAGL_MODE_TOPK ? dense_softmax_bwd_kernel<1>
                    : a.mode == DAGL_MODE_ADAPTIVE_TOPK ? dense_softmax_bwd_kernel<2> : dense_softmax_bwd_kernel<0>;
    hipLaunchKernelGGL(kern, dim3(c.lc, c.nb), dim3(256), 0, s, c.N, c.ldn, c.L, c.l0, c.Lc, w.S.p, w.A.p, w.mt, a.bias, a.lse, mu, a.thr,
                       a.dthr, a.dbias, w.dmu, c.b0, ds_word, w.sel);
    DAGL_LAUNCH_CHECK("dense_softmax_bwd_kernel");
    return DAGL_OK;
}

// out[r, c] += rs[r] * v[c] * scale   (the rank-one terms of the dense row mean)
__global__ void dt_rank1_add_kernel(size_t rows, int rows_per_batch, const float* __restrict__ rs, const float* __restrict__ vf,
                                    const double* __restrict__ vd, int vstride, float scale, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * D) return;
    const size_t r = t / D; const int c = (int)(t - r * D);
    const size_t b = r / rows_per_batch;
    const float v = vf ? vf[b * vstride + c] : (float)(vd[b * vstride + c] * (double)scale);
    out[t] += (rs ? rs[r] : 1.0f) * (vf ? v * scale : v);
}

// d b2[b,c,y,x] = sum over the 49 keys whose window covers (y,x) of d V[key][(kh,kw,c)]; thread = pixel, fixed order
__global__ __launch_bounds__(256) void dt_fold_dv_kernel(Grid g, int nb, const float* __restrict__ dv, float* __restrict__ db2) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)nb * g.N) return;
    const size_t b = t / g.N; const size_t r = t - b * g.N;
    const int y = (int)(r / g.W), x = (int)(r - (size_t)y * g.W);
    float4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kh = 0; kh < KS; ++kh) {
        const int jy = y + 3 - kh;
        if (jy < 0 || jy >= g.H) continue;
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
            const int jx = x + 3 - kw;
            if (jx < 0 || jx >= g.W) continue;
            const float4* row = reinterpret_cast<const float4*>(dv + ((b * g.N + (size_t)jy * g.W + jx) * P + (kh * KS + kw) * CH));
#pragma unroll
            for (int q = 0; q < 4; ++q) { const float4 v = row[q]; acc[q].x += v.x; acc[q].y += v.y; acc[q].z += v.z; acc[q].w += v.w; }
        }
    }
    float* o = db2 + (b * CH * g.H + y) * g.W + x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o[(size_t)(4 * q + 0) * g.N] = acc[q].x; o[(size_t)(4 * q + 1) * g.N] = acc[q].y;
        o[(size_t)(4 * q + 2) * g.N] = acc[q].z; o[(size_t)(4 * q + 3) * g.N] = acc[q].w;
    }
}

static Gemm32 dt_gemm(int M, int N, int K, int batch, const Mat32& A, const Mat32& Bm, const Out32& C, float beta, bool grad = false) {
    Gemm32 g;
    g.M = M; g.N = N; g.K = K; g.batch = batch; g.A = A.p; g.lda = A.ld; g.sA = A.stride; g.a_kc = A.kc;
    g.B = Bm.p; g.ldb = Bm.ld; g.sB = Bm.stride; g.b_kc = Bm.kc; g.C = C.p; g.ldc = C.ld; g.sC = C.stride;
    g.alpha = 1.0f; g.beta = beta; g.bias = nullptr; g.relu = 0;
    // S: chains of 48 products; the long forward contraction A V: 128.  Gradient products (1e-3 bar, contractions of at
    // most a few thousand terms per chunk of queries / 16 384 keys) run unchunked: 140 instead of 236 registers, a third
    // block per CU.
    g.chunk_tiles = grad ? 0 : ((K == D) ? 3 : 8);
    return g;
}

// padded b2, and with threshold heads the keys' column sums and mt = mu thr
static int dt_prepare(hipStream_t s, const DenseTrainArgs& a, const DtWs& w, float* mu) {
    int rc;
    if ((rc = launch_pad_nhwc(s, a.B, a.g.H, a.g.W, a.b2, w.b2p))) return rc;
    if (a.thr == nullptr) return DAGL_OK;                // (the fixed-k mode has no threshold heads)
    if ((rc = launch_colsum_rows(s, a.B, a.g.N, a.x_rows, w.colsum))) return rc;
    hipLaunchKernelGGL(dt_thresholds_kernel, dim3((a.g.L + 3) / 4, a.B), dim3(256), 0, s, a.g.L, a.g.N, a.wq_rows, w.colsum, a.thr, w.mt, mu);
    DAGL_LAUNCH_CHECK("dt_thresholds_kernel");
    return DAGL_OK;
}

int launch_dense_train_forward(hipStream_t s, const DenseTrainForward& args) {
    DenseTrainForward a = args;
    if (!a.heads()) a.thr = a.bias = nullptr;
    const int B = a.B; const Grid& g = a.g;
    const DtPlan p = dt_plan(B, g, false);
    const DtWs w = dt_carve(a.ws, B, g, p, false);
    if (a.ws_bytes < w.bytes) { set_error("dense forward: workspace %zu B < required %zu B", a.ws_bytes, w.bytes); return DAGL_ERR_WORKSPACE; }
    float* lse = a.lse ? a.lse : w.lse;
    float* mu = a.mu ? a.mu : w.mu;
    int rc;
    if ((rc = dt_prepare(s, a, w, mu))) return rc;
    const auto softmax = a.mode == DAGL_MODE_TOPK ? dense_softmax_fwd_kernel<1>
                       : a.mode == DAGL_MODE_ADAPTIVE_TOPK ? dense_softmax_fwd_kernel<2> : dense_softmax_fwd_kernel<0>;
    for (int b0 = 0; b0 < B; b0 += p.Bc) {
        const int nb = (B - b0 < p.Bc) ? B - b0 : p.Bc;
        if ((rc = launch_unfold_values(s, nb, g, w.b2p + (size_t)b0 * g.Hp * g.Wp * CH, w.V.p))) return rc;
        for (int l0 = 0; l0 < g.L; l0 += p.Lc) {
            const DtChunk c = dt_chunk(g, p, b0, nb, l0);
            // S = Wq X^T
            if ((rc = launch_gemm32(s, dt_gemm(c.lc, g.N, D, c.nb, dt_query_rows(c, a.wq_rows, D), dt_key_rows(c, a.x_rows, D), w.S, 0.f)))) return rc;
            if (a.mode != DAGL_MODE_ADAPTIVE)
                if ((rc = launch_dt_select(s, c, a.mode, a.k, w, a.bias))) return rc;
            hipLaunchKernelGGL(softmax, dim3(c.lc, c.nb), dim3(256), 0, s, c.N, c.ldn, c.L, c.l0, c.Lc, w.S.p, w.mt, a.bias, lse, w.deg, w.rowsum,
                               c.b0, w.sel);
            DAGL_LAUNCH_CHECK("dense_softmax_fwd_kernel");
            // agg = A V
            if ((rc = launch_gemm32(s, dt_gemm(c.lc, P, g.N, c.nb, w.S, w.V.down(), dt_query_rows(c, w.agg, P), 0.f)))) return rc;
        }
    }
    if ((rc = launch_fold(s, B, g, w.agg, a.out))) return rc;
    if (a.stats) if ((rc = launch_degree_stats(s, (size_t)B * g.L, w.deg, a.stats))) return rc;
    return DAGL_OK;
}


// ---- split-fp16 operands of the backward's five products (gemm16s.hip) --------------------------------------------------------
// src fp32 [R][C] (leading dimension ld) -> hi / lo [R][Cp] halfs (row stride ldo), s x = hi + lo, pad columns zero; s from *word (largest magnitude
// of the tensor, fcg_scale_of) or `fixed` when word is null.  Thread = (row, octet of columns).
__global__ __launch_bounds__(256) void dt_split_rows_kernel(size_t R, int C, long long ld, int Cp, long long ldo, const float* __restrict__ src,
                                                            const unsigned* __restrict__ word, float fixed,
                                                            unsigned short* __restrict__ hi, unsigned short* __restrict__ lo) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int o8 = Cp / 8;
    if (t >= R * o8) return;
    const size_t r = t / o8; const int c0 = 8 * (int)(t - r * o8);
    const float sc = word ? fcg_scale_of(*word) : fixed;
    const float* p = src + r * ld + c0;
    unsigned short vh[8], vl[8];
    if (c0 + 8 <= C) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        g16_split(a.x * sc, vh[0], vl[0]); g16_split(a.y * sc, vh[1], vl[1]); g16_split(a.z * sc, vh[2], vl[2]); g16_split(a.w * sc, vh[3], vl[3]);
        g16_split(b.x * sc, vh[4], vl[4]); g16_split(b.y * sc, vh[5], vl[5]); g16_split(b.z * sc, vh[6], vl[6]); g16_split(b.w * sc, vh[7], vl[7]);
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) g16_split((c0 + u < C) ? p[u] * sc : 0.f, vh[u], vl[u]);
    }
    *reinterpret_cast<uint4*>(hi + r * ldo + c0) = *reinterpret_cast<const uint4*>(vh);
    *reinterpret_cast<uint4*>(lo + r * ldo + c0) = *reinterpret_cast<const uint4*>(vl);
}

// src fp32 [batch][R][C] (ld, batch stride ss) -> transposed hi / lo [batch][C][Rp] halfs (row stride ldo; Rp >= R a multiple of 32, pad zero).
// Block = 64 rows x 64 columns: 256-byte row reads, transposed in LDS, 128-byte runs written.
__global__ __launch_bounds__(256) void dt_split_transpose_kernel(int R, int C, long long ld, long long ss, int Rp, long long ldo, long long sd,
                                                                 const float* __restrict__ src, const unsigned* __restrict__ word,
                                                                 float fixed, unsigned short* __restrict__ hi,
                                                                 unsigned short* __restrict__ lo) {
    __shared__ __attribute__((aligned(16))) unsigned short th[64][64 + 8];
    __shared__ __attribute__((aligned(16))) unsigned short tl[64][64 + 8];
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const float sc = word ? fcg_scale_of(*word) : fixed;
    const float* sb = src + (long long)b * ss;
    float v[16];                                                             // all of a thread's 16 loads in flight, then the splits
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = threadIdx.x + 256 * u, r = e >> 6, c = e & 63;
        v[u] = (r0 + r < R && c0 + c < C) ? sb[(long long)(r0 + r) * ld + c0 + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int e = threadIdx.x + 256 * u, r = e >> 6, c = e & 63;
        g16_split(v[u] * sc, th[c][r], tl[c][r]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 8; e += 256) {                        // (column, octet of rows)
        const int c = e >> 3, r8 = e & 7;
        if (c0 + c >= C || r0 + 8 * r8 >= Rp) continue;
        const long long o = (long long)b * sd + (long long)(c0 + c) * ldo + r0 + 8 * r8;
        *reinterpret_cast<uint4*>(hi + o) = *reinterpret_cast<const uint4*>(&th[c][8 * r8]);
        *reinterpret_cast<uint4*>(lo + o) = *reinterpret_cast<const uint4*>(&tl[c][8 * r8]);
    }
}

// value patches of the zero-bordered map, split: out[b][n][(kh,kw,c)] (50 taps of 16 halfs: tap 49 = zero pad); thread = (key, tap)
__global__ __launch_bounds__(256) void dt_unfold_values_split_kernel(int H, int W, size_t total, const float* __restrict__ mp,
                                                                     const unsigned* __restrict__ word,
                                                                     unsigned short* __restrict__ hi, unsigned short* __restrict__ lo) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;                                                  // total = nb * N * 50
    const int Wp = W + 2 * PADPIX, Hp = H + 2 * PADPIX;
    const size_t key = t / 50; const int tap = (int)(t - key * 50);
    const size_t b = key / ((size_t)H * W); const int n = (int)(key - b * (size_t)H * W);
    const int y = n / W, x = n - y * W;
    const float sc = fcg_scale_of(*word);
    unsigned short vh[16], vl[16];
    if (tap < KS * KS) {
        const int kh = tap / KS, kw = tap - kh * KS;
        const float4* src = reinterpret_cast<const float4*>(mp + ((b * Hp + y + kh) * (size_t)Wp + x + kw) * CH);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = src[q];
            g16_split(v.x * sc, vh[4 * q], vl[4 * q]); g16_split(v.y * sc, vh[4 * q + 1], vl[4 * q + 1]);
            g16_split(v.z * sc, vh[4 * q + 2], vl[4 * q + 2]); g16_split(v.w * sc, vh[4 * q + 3], vl[4 * q + 3]);
        }
    } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) { vh[u] = 0; vl[u] = 0; }
    }
    uint4* oh = reinterpret_cast<uint4*>(hi + t * 16); uint4* ol = reinterpret_cast<uint4*>(lo + t * 16);
    oh[0] = reinterpret_cast<const uint4*>(vh)[0]; oh[1] = reinterpret_cast<const uint4*>(vh)[1];
    ol[0] = reinterpret_cast<const uint4*>(vl)[0]; ol[1] = reinterpret_cast<const uint4*>(vl)[1];
}

// the rows of `src` (R of them over the whole group, C columns) -> `o`, Cp >= C columns per row
static int dt_split_rows(hipStream_t s, size_t R, int C, const Mat32& src, int Cp, const Split16& o) {
    const size_t items = R * (size_t)(Cp / 8);
    hipLaunchKernelGGL(dt_split_rows_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, R, C, src.ld, Cp, o.ld, src.p, o.word, o.fixed,
                       o.hi, o.hi + o.lo);
    DAGL_LAUNCH_CHECK("dt_split_rows_kernel");
    return DAGL_OK;
}

// `src` [nb][R][C] -> `o` [nb][C][Rp], Rp >= R
static int dt_split_transpose(hipStream_t s, int nb, int R, int C, const Mat32& src, int Rp, const Split16& o) {
    hipLaunchKernelGGL(dt_split_transpose_kernel, dim3((Rp + 63) / 64, (C + 63) / 64, nb), dim3(256), 0, s, R, C, src.ld, src.stride, Rp, o.ld,
                       o.stride, src.p, o.word, o.fixed, o.hi, o.hi + o.lo);
    DAGL_LAUNCH_CHECK("dt_split_transpose_kernel");
    return DAGL_OK;
}

// slices > 1: K = the contraction length of one slice, the slices' raw sums in `part`
static Gemm16s dt_gemm16(int M, int N, int K, int nb, const Split16& A, const Split16& Bm, const Out32& C, int slices = 1, float* part = nullptr) {
    Gemm16s g;
    g.M = M; g.N = N; g.K = K; g.a_hi = A.hi; g.a_lo = A.hi + A.lo; g.b_hi = Bm.hi; g.b_lo = Bm.hi + Bm.lo; g.lda = A.ld; g.ldb = Bm.ld;
    g.a_rows = M; g.b_rows = N; g.C = C.p; g.ldc = C.ld; g.part = part; g.slices = slices; g.scale_word = A.word; g.scale_word_b = Bm.word;
    g.alpha0 = 1.f / (A.fixed * Bm.fixed); g.batch = nb; g.sA = A.stride; g.sB = Bm.stride; g.sC = C.stride;
    return g;
}

// The backward of one image group (all queries in one chunk) with its five products on the fp16 matrix cores, split operands:
// 580 GFLOP per head at [8, 128 x 128] ran at 85 TFLOP/s on the fp32 matrix cores (54 % of their peak) -- 6.8 ms per head and
// step, half of the adaptive-mode training step.  Operand copies: K-contiguous rows for both sides of every product, i.e.
// d agg, V, Wq, X by rows, and d agg, X, Wq, d S, A transposed; every tensor scaled by a power of two taken from its largest
// magnitude (A <= 1: 2^13).  The softmax backward between the products stays in fp32 on fp32 S and d A.
static int dt_backward_group16(hipStream_t s, const DenseTrainBackward& a, const DtPlan& p, const DtWs& w, int b0, int nb, const float* mu) {
    int rc;
    const Grid& g = a.g;
    const int L = g.L, N = g.N, Lp = p.Lp;
    const DtChunk c = dt_chunk(g, p, b0, nb, 0);
    const Mat32 dagg = dt_query_rows<const float>(c, w.dagg, P), wq = dt_query_rows(c, a.wq_rows, D), x = dt_key_rows(c, a.x_rows, D);
    const float* b2p = w.b2p + (size_t)b0 * g.Hp * g.Wp * CH;
    DAGL_HIP_TRY(hipMemsetAsync(w.words, 0, 256, s));
    if ((rc = launch_absmax(s, (size_t)nb * L * P, dagg.p, w.words + 0))) return rc;
    if ((rc = launch_absmax(s, (size_t)nb * g.Hp * g.Wp * CH, b2p, w.words + 1))) return rc;
    if ((rc = launch_absmax(s, (size_t)nb * N * D, x.p, w.words + 2))) return rc;
    if ((rc = launch_absmax(s, (size_t)nb * L * D, wq.p, w.words + 3))) return rc;
    // operand copies that do not depend on the softmax
    if ((rc = dt_split_rows(s, (size_t)nb * L, P, dagg, DT_PK, w.dgk))) return rc;
    if ((rc = dt_split_transpose(s, nb, L, P, dagg, Lp, w.dgt))) return rc;
    {
        const size_t total = (size_t)nb * N * 50;
        hipLaunchKernelGGL(dt_unfold_values_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g.H, g.W, total, b2p,
                           w.vk.word, w.vk.hi, w.vk.hi + w.vk.lo);
        DAGL_LAUNCH_CHECK("dt_unfold_values_split_kernel");
    }
    if ((rc = dt_split_rows(s, (size_t)nb * N, D, x, DT_DK, w.xk))) return rc;
    if ((rc = dt_split_transpose(s, nb, N, D, x, p.nk, w.xt))) return rc;
    if ((rc = dt_split_rows(s, (size_t)nb * L, D, wq, DT_DK, w.wqk))) return rc;
    if ((rc = dt_split_transpose(s, nb, L, D, wq, Lp, w.wqt))) return rc;
    // d A = d agg V^T ; S = Wq X^T
    if ((rc = launch_gemm16s(s, dt_gemm16(L, N, DT_PK, nb, w.dgk, w.vk, w.A)))) return rc;
    if ((rc = launch_gemm16s(s, dt_gemm16(L, N, DT_DK, nb, w.wqk, w.xk, w.S)))) return rc;
    if ((rc = launch_dense_softmax_bwd(s, c, a, w, mu, w.words + 4))) return rc;
    // d S by rows and transposed, A transposed
    if ((rc = dt_split_rows(s, (size_t)nb * p.Lc, (int)p.ldn, w.S, p.nk, w.dsk))) return rc;
    if ((rc = dt_split_transpose(s, nb, L, N, w.S, Lp, w.dst))) return rc;
    if ((rc = dt_split_transpose(s, nb, L, N, w.A, Lp, w.at))) return rc;
    // d Wq = d S X (split over the keys)
    if ((rc = launch_gemm16s(s, dt_gemm16(L, D, p.nk / p.kslices, nb, w.dsk, w.xt, dt_query_rows(c, a.dwq_rows, D), p.kslices, w.part)))) return rc;
    // d X = d S^T Wq ; d V = A^T d agg
    if ((rc = launch_gemm16s(s, dt_gemm16(N, D, Lp, nb, w.dst, w.wqt, dt_key_rows(c, a.dx_rows, D))))) return rc;
    if ((rc = launch_gemm16s(s, dt_gemm16(N, P, Lp, nb, w.at, w.dgt, w.dV)))) return rc;
    return DAGL_OK;
}

// ... and with the products in fp32, chunk by chunk: d X and d V add up over the chunks
static int dt_backward_group32(hipStream_t s, const DenseTrainBackward& a, const DtPlan& p, const DtWs& w, int b0, int nb, const float* mu) {
    int rc;
    const Grid& g = a.g;
    if ((rc = launch_unfold_values(s, nb, g, w.b2p + (size_t)b0 * g.Hp * g.Wp * CH, w.V.p))) return rc;
    for (int l0 = 0; l0 < g.L; l0 += p.Lc) {
        const DtChunk c = dt_chunk(g, p, b0, nb, l0);
        const Mat32 dagg = dt_query_rows<const float>(c, w.dagg, P), wq = dt_query_rows(c, a.wq_rows, D), x = dt_key_rows(c, a.x_rows, D);
        const float beta = (l0 == 0) ? 0.f : 1.f;
        // d A = d agg V^T ; S = Wq X^T
        if ((rc = launch_gemm32(s, dt_gemm(c.lc, g.N, P, nb, dagg, w.V, w.A, 0.f, true)))) return rc;
        if ((rc = launch_gemm32(s, dt_gemm(c.lc, g.N, D, nb, wq, x, w.S, 0.f)))) return rc;
        if (a.mode != DAGL_MODE_ADAPTIVE)
            if ((rc = launch_dt_select(s, c, a.mode, a.k, w, a.bias))) return rc;
        if ((rc = launch_dense_softmax_bwd(s, c, a, w, mu, nullptr))) return rc;
        // d Wq = d S X
        if ((rc = launch_gemm32(s, dt_gemm(c.lc, D, g.N, nb, w.S, x.down(), dt_query_rows(c, a.dwq_rows, D), 0.f, true)))) return rc;
        // d X (+)= d S^T Wq
        if ((rc = launch_gemm32(s, dt_gemm(g.N, D, c.lc, nb, w.S.down(), wq.down(), dt_key_rows(c, a.dx_rows, D), beta, true)))) return rc;
        // d V (+)= A^T d agg
        if ((rc = launch_gemm32(s, dt_gemm(g.N, P, c.lc, nb, w.A.down(), dagg.down(), w.dV, beta, true)))) return rc;
    }
    return DAGL_OK;
}

int launch_dense_train_backward(hipStream_t s, const DenseTrainBackward& args) {
    DenseTrainBackward a = args;
    if (!a.heads()) { a.thr = a.bias = nullptr; a.dthr = a.dbias = nullptr; }
    const int B = a.B; const Grid& g = a.g;
    const DtPlan p = dt_plan(B, g, true);
    const DtWs w = dt_carve(a.ws, B, g, p, true);
    if (a.ws_bytes < w.bytes) { set_error("dense backward: workspace %zu B < required %zu B", a.ws_bytes, w.bytes); return DAGL_ERR_WORKSPACE; }
    // the wide top-k modes re-select from the recomputed scores: the fp32 product of the forward, bit for bit (a split-fp16 S could
    // order two near-equal scores the other way round)
    const bool h16 = p.h16 && !a.fp32_products && a.mode == DAGL_MODE_ADAPTIVE;
    float* mu = w.rowsum;                                     // recomputed with the thresholds (same values as the forward's)
    int rc;
    if ((rc = dt_prepare(s, a, w, mu))) return rc;
    if ((rc = launch_unfold_dout(s, B, g, a.dout, w.dagg))) return rc;
    for (int b0 = 0; b0 < B; b0 += p.Bc) {
        const int nb = (B - b0 < p.Bc) ? B - b0 : p.Bc;
        if ((rc = h16 ? dt_backward_group16(s, a, p, w, b0, nb, mu) : dt_backward_group32(s, a, p, w, b0, nb, mu))) return rc;
        const size_t n = (size_t)nb * g.N;
        hipLaunchKernelGGL(dt_fold_dv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, nb, w.dV.p, a.db2 + (size_t)b0 * CH * g.N);
        DAGL_LAUNCH_CHECK("dt_fold_dv_kernel");
    }
    // dense mean term: d Wq_l += d mu_l Xbar ;  d X_j += (sum_l d mu_l Wq_l) / N   (the fixed-k mode has no threshold)
    if (a.heads()) {
        const size_t nq = (size_t)B * g.L * D, nk = (size_t)B * g.N * D;
        hipLaunchKernelGGL(dt_rank1_add_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (size_t)B * g.L, g.L, w.dmu, nullptr,
                           w.colsum, DS, 1.0f / (float)g.N, a.dwq_rows);
        DAGL_LAUNCH_CHECK("dt_rank1_add_kernel");
        if ((rc = launch_dxbar(s, B, g.L, a.wq_rows, w.dmu, w.dxbar))) return rc;
        hipLaunchKernelGGL(dt_rank1_add_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, (size_t)B * g.N, g.N, nullptr, w.dxbar,
                           nullptr, D, 1.0f / (float)g.N, a.dx_rows);
        DAGL_LAUNCH_CHECK("dt_rank1_add_kernel");
    }
    return DAGL_OK;
}

}  // namespace dagl
