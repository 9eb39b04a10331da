// What every route's mask and softmax share: the logit of a key (three forms, below), and the row-wise selection of the k best scores
// by radix selection over the scores' bit patterns with its rule for a tie at the k-th place (the inference form of the wide top-k
// modes, topk_wide.hip; their differentiable form, dense_train.hip; the generic-geometry route, generic.hip; the graph export,
// graph.hip).  Reference: top_k = min(num_edge, N) best scores of every query, GReccR2b_3mh_1-checkpoint.py:242-250
// (CA_model-checkpoint.py:134-143 uses 500).
#pragma once
#include "dagl_common.h"

namespace dagl {

// ------------------------------------------------------------------------------------------------------
// The logit of a key.  m = (S - mean thr) + bias, pass = m > 0, l = (S m) scale: DN_Gray/model/dagl.py:256-260 in fp32, in the
// reference's expression order, the products rounded one by one (__fmul_rn: no contraction into an FMA, whatever surrounds the call)
// -- this is what ties every route to the reference bit for bit.  The fixed-k variant's mask is 0/1, so m = 1 on a kept key:
// l = S scale (GReccR2b_3mh_1-checkpoint.py:242-250).  mtq = mean thr and bsq = bias of the query.
// Separate by design: gt_logit (graph_rows.h) forms scale S m with m = relu(S - tau), a rounding order its backward depends on;
// graph_logit (graph.hip) forms the products in fp64; dense_attend_kernel (dense.hip) has the same expression packed two keys wide (dnf2) in its
// fenced block at the register cap.
// ------------------------------------------------------------------------------------------------------
// a key that is kept (a list entry): no mask test
__device__ __forceinline__ float edge_logit(float s, float mtq, float bsq, bool adaptive) {
    float m = 1.0f;
    if (adaptive) m = (s - mtq) + bsq;
    return __fmul_rn(__fmul_rn(s, m), SOFTMAX_SCALE);
}
// the adaptive mask: a masked key's logit is 0 (the softmax runs over ALL keys, dagl.py:259: yi * mask)
__device__ __forceinline__ float masked_logit(float s, float mtq, float bsq, bool& pass) {
    const float m = (s - mtq) + bsq;
    pass = m > 0.f;
    return pass ? __fmul_rn(__fmul_rn(s, m), SOFTMAX_SCALE) : 0.f;
}

// sort key of a score: 0 = "not a candidate" (fails the adaptive test of the intersection mode), else bits + 1
// (scores are >= 0 -- sums of products of post-ReLU features --, so their bit patterns sort like the values)
__device__ __forceinline__ unsigned wide_key(float s, bool adaptive, float mtq, float bsq) {
    if (adaptive && !(((s - mtq) + bsq) > 0.f)) return 0u;
    return __float_as_uint(fmaxf(s, 0.f)) + 1u;
}
// whether key j is one of the k best: (T, jt) = sort key of the k-th best score (wide_radix_select) and the last key index taken
// AT that key (wide_tie_index: ties go to the lower index)
__device__ __forceinline__ bool wide_taken(unsigned key, int j, unsigned T, int jt) {
    return key != 0u && (key > T || (key == T && j <= jt));
}

// a key of a whole score row.  MODE 0: the adaptive mask.  MODE 1: the k best scores of the row, a 0/1 mask (m = 1).  MODE 2: both
// tests, m = relu(S - mean thr + bias) on the k best of the keys that pass.  m is what the backward needs (d S = scale (m + S) d l).
template <int MODE>
__device__ __forceinline__ float row_logit(float s, int j, float mtq, float bsq, float scale, unsigned T, int jt, bool& pass, float& m) {
    m = 1.f;
    if (MODE != 1) { m = (s - mtq) + bsq; pass = m > 0.f; }
    if (MODE != 0) pass = wide_taken(wide_key(s, MODE == 2, mtq, bsq), j, T, jt);
    return pass ? __fmul_rn(__fmul_rn(s, m), scale) : 0.f;
}

struct WideSelShared {
    unsigned hist[256];
    unsigned prefix, remaining, bin_count;
};

// One block of 256 threads, one score row: T = sort key of the k-th best score (4 x 8-bit digits, most significant first), `need` =
// how many of the `bin_count` keys equal to T belong to the k best (all of them when need >= bin_count).  Block-uniform results.
__device__ __forceinline__ void wide_radix_select(const float* __restrict__ row, int N, int k, bool adaptive, float mtq, float bsq,
                                                  WideSelShared& sh, unsigned& T, unsigned& need, unsigned& bin_count) {
    const int tid = threadIdx.x;
    if (tid == 0) { sh.prefix = 0u; sh.remaining = (unsigned)k; }
    bin_count = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        sh.hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = sh.prefix;
        // (the high digit -- sign and seven exponent bits -- is the same for nearly every score of a row: 64 lanes adding to one LDS
        // word serialise, 65 536 times.  There the wave counts its lanes per distinct digit first: one add per digit.  For the second
        // digit, with ~100 distinct values per wave, that loop was 3.6x SLOWER than the plain adds.)
        for (int j0 = 0; j0 < N; j0 += 256) {
            const int j = j0 + tid;
            unsigned key = 0u; bool act = false;
            if (j < N) { key = wide_key(row[j], adaptive, mtq, bsq); act = pass == 0 || (key >> (shift + 8)) == prefix; }
            const unsigned bin = (key >> shift) & 255u;
            if (pass == 0) {
                unsigned long long todo = __ballot(act);
                while (todo) {                                                  // wave-uniform loop: one round per distinct digit
                    const int first = __ffsll((long long)todo) - 1;
                    const unsigned b0 = (unsigned)__builtin_amdgcn_readlane((int)bin, first);
                    const unsigned long long same = __ballot(act && bin == b0);
                    if ((tid & 63) == first) atomicAdd(&sh.hist[b0], (unsigned)__popcll(same));
                    todo &= ~same;
                }
            } else if (act) atomicAdd(&sh.hist[bin], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned rem = sh.remaining, cum = 0; int bin = 0;
            for (int bq = 255; bq >= 0; --bq) {
                if (cum + sh.hist[bq] >= rem) { bin = bq; break; }
                cum += sh.hist[bq];
            }
            // (fewer than k keys in all: bin 0 is reached with cum + hist[0] = N >= rem, k <= N by construction)
            sh.remaining = rem - cum; sh.prefix = (prefix << 8) | (unsigned)bin; sh.bin_count = sh.hist[bin];
        }
        __syncthreads();
        bin_count = sh.bin_count;
    }
    T = sh.prefix; need = sh.remaining;
}

// A tie at the k-th place, after wide_radix_select (same block, same row): the `need` lowest key indices of the `bin_count` keys equal
// to T win.  Returns the last key index taken at T -- 0x7fffffff when all of them are (need >= bin_count).  Block-uniform.
struct WideTieShared { int cnt[4]; int jt; };
__device__ __forceinline__ int wide_tie_index(const float* __restrict__ row, int N, bool adaptive, float mtq, float bsq, unsigned T,
                                              unsigned need, unsigned bin_count, WideTieShared& sh) {
    if (need >= bin_count) return 0x7fffffff;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int run = 0;
    for (int j0 = 0; j0 < N; j0 += 256) {
        const int j = j0 + tid;
        const bool eq = j < N && wide_key(row[j], adaptive, mtq, bsq) == T;
        const unsigned long long eqb = __ballot(eq);
        if (lane == 0) sh.cnt[w] = __popcll(eqb);
        __syncthreads();
        int before = run;
        for (int u = 0; u < w; ++u) before += sh.cnt[u];
        const int rank = before + __popcll(eqb & ((1ull << lane) - 1ull));
        if (eq && rank == (int)need - 1) sh.jt = j;
        run += sh.cnt[0] + sh.cnt[1] + sh.cnt[2] + sh.cnt[3];
        __syncthreads();
        if (run >= (int)need) break;
    }
    return sh.jt;
}

}  // namespace dagl
