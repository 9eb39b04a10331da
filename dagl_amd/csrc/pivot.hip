// Pivot keys: the subset of keys the top-k screen takes its candidate threshold from (screen.hip).
//
// theta = "at least k DISTINCT keys score >= theta" holds for the k-th largest score over ANY set of distinct keys, so the sampling
// pass may score whichever keys it likes; what the choice changes is how many keys it scores and how many candidates survive the
// filter.  Both feature sets are post-ReLU (>= 0), so S = Wq . X is dominated by the key's own magnitude: the keys with the largest
// feature row sums are near the top of most queries' lists.  The two heaviest keys of every 64 consecutive ones (N / 32 keys instead
// of the N / 8 of "every 8th key tile") give a threshold as good as the one from every second tile.
//
// project16_kernel leaves per key PIVOT_SLOTS partial row sums (slot = first output tile of the block that wrote it: 0 and 4 for the
// two tile groups of a unit, 0..6 for the single-tile overhang blocks; unwritten slots of a written key are zero).  Here one wave per
// 64-key block adds them in slot order, picks the two largest sums (a tie goes to the lower key, a NaN counts as -inf, keys past N
// do not exist) and copies those keys' bf16 rows into the dense matrix Xp the screen kernels stream in place of Xh.
// Block v's rows go to step v % steps, rows 2 (v / steps) + {0, 1}: neighbouring blocks (similar patches) land in different steps, so a
// query's best pivots do not share one (chunk, half) segment, of which only the GKEEP largest group maxima reach the threshold kernel.
// A block with fewer than two keys leaves zero rows (score 0: below every real threshold; theta = 0 means "pass everything").
#include "dagl_common.h"

namespace dagl {

__device__ __forceinline__ float pivot_rowsum(const float* __restrict__ slots) {
    const float4 a = *reinterpret_cast<const float4*>(slots), b = *reinterpret_cast<const float4*>(slots + 4);
    return (((((a.x + a.y) + a.z) + a.w) + b.x) + b.y) + b.z;
}

// lowest lane among `in` holding the largest s (-1: no lane in)
__device__ __forceinline__ int pivot_pick(float s, bool in) {
    const float m = wave_max_f32(in ? s : -__builtin_inff());
    const unsigned long long bal = __ballot(in && s == m);
    return bal ? __ffsll((long long)bal) - 1 : -1;
}

__global__ __launch_bounds__(256) void pivot_keys_kernel(PivotArgs a) {
    if (a.policy != nullptr && *a.policy != 0) return;          // the workspace is on the tight threshold: nobody reads the pivots
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);           // 64-key block (wave-uniform)
    const int b = blockIdx.y;
    if (v >= 32 * a.steps) return;
    const int key = v * 64 + lane;
    const bool valid = v < a.n_blk && key < a.N;
    float s = -__builtin_inff();
    if (valid) s = pivot_rowsum(a.rowsum + ((size_t)b * a.N + key) * PIVOT_SLOTS);
    if (!(s == s)) s = -__builtin_inff();
    const int p0 = pivot_pick(s, valid);
    const int p1 = pivot_pick(s, valid && lane != p0);           // never the same key twice
    const int j = lane >> 5, c = lane & 31;
    const int pk = j ? p1 : p0;
    if (c < DSH / 8) {
        uint4 row = make_uint4(0u, 0u, 0u, 0u);
        if (pk >= 0) row = reinterpret_cast<const uint4*>(a.xh + ((size_t)b * a.rows_xh + (size_t)v * 64 + pk) * DSH)[c];
        const size_t dst = (size_t)(v % a.steps) * 64 + 2 * (v / a.steps) + j;
        reinterpret_cast<uint4*>(a.xp + ((size_t)b * a.rows_xp + dst) * DSH)[c] = row;
    }
    if (c == 0 && v < a.n_blk) a.pidx[((size_t)b * a.n_blk + v) * 2 + j] = pk >= 0 ? v * 64 + pk : -1;
}

int launch_pivot_keys(hipStream_t s, const PivotArgs& a) {
    hipLaunchKernelGGL(pivot_keys_kernel, dim3((32 * a.steps + 3) / 4, a.B), dim3(256), 0, s, a);
    DAGL_LAUNCH_CHECK("pivot_keys_kernel");
    return DAGL_OK;
}

// debug entry point: the row sums as pivot_keys_kernel forms them
__global__ void pivot_rowsum_kernel(size_t n, const float* __restrict__ slots, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = pivot_rowsum(slots + i * PIVOT_SLOTS);
}

int launch_pivot_rowsum(hipStream_t s, size_t n_keys, const float* slots, float* out) {
    hipLaunchKernelGGL(pivot_rowsum_kernel, dim3((unsigned)((n_keys + 255) / 256)), dim3(256), 0, s, n_keys, slots, out);
    DAGL_LAUNCH_CHECK("pivot_rowsum_kernel");
    return DAGL_OK;
}

}  // namespace dagl
