// Pivot keys: the subset of keys the top-k screen takes its candidate threshold from (screen.hip).
//
// theta = "at least k DISTINCT keys score >= theta" holds for the k-th largest score over ANY set of distinct keys, so the sampling
// pass may score whichever keys it likes; what the choice changes is how many keys it scores and how many candidates survive the
// filter.  Both feature sets are post-ReLU (>= 0), so S = Wq . X is dominated by the key's own magnitude: the keys with the largest
// feature row sums are near the top of most queries' lists.  The two heaviest keys of every 64 consecutive ones (N / 32 keys instead
// of the N / 8 of "every 8th key tile") give a threshold as good as the one from every second tile.
//
// project16_kernel leaves per key PIVOT_SLOTS partial row sums (slot = first output tile of the block that wrote it: 0 and 4 for the
// two tile groups of a unit, 0..6 for the single-tile overhang blocks; unwritten slots of a written key are zero).  One wave per
// 64-key block adds them in slot order and picks the two largest sums (a tie goes to the lower key, a NaN counts as -inf, keys past N
// do not exist): the rule itself is in pivot_pick.h.
// Block v's rows form step v % steps, rows 2 (v / steps) + {0, 1}: neighbouring blocks (similar patches) land in different steps, so a
// query's best pivots do not share one (chunk, half) segment, of which only the GKEEP largest group maxima reach the threshold kernel.
// A block with fewer than two keys leaves zero rows (score 0: below every real threshold; theta = 0 means "pass everything").
//
// Who applies it.  Where every block of the sampling launch has one pivot step (pv_steps_per_split == 1: the benchmark's 256 x 256
// and everything smaller) pivot_sample_kernel (screen.hip) picks its step's keys itself and fetches their rows from Xh into its LDS
// tile: no launch here, Xp stays unwritten (round 8).  pivot_keys_kernel below is the form with the dense matrix Xp between two
// launches -- it copies the picked rows there and the screen kernels stream Xp in place of Xh --, kept for the maps whose sampling
// blocks loop over several steps (512 x 512: 16 per block, where the ring does overlap something), for 256-query blocks under a
// policy word, and behind DAGL_PIVOT_SAMPLE=0 for comparing the two.  Both leave the same pidx and the same group maxima.
#include "dagl_common.h"
#include "pivot_pick.h"

namespace dagl {

__global__ __launch_bounds__(256) void pivot_keys_kernel(PivotArgs a) {
    if (a.policy != nullptr && *a.policy != 0) return;          // the workspace is on the tight threshold: nobody reads the pivots
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);           // 64-key block (wave-uniform)
    const int b = blockIdx.y;
    if (v >= 32 * a.steps) return;
    bool valid;
    const float s = pivot_key_sum(a, b, v, lane, valid);
    int k0, k1;
    pivot_pick2(s, valid, v, lane, k0, k1);
    const int j = lane >> 5, c = lane & 31;
    const int pk = j ? k1 : k0;
    if (c < DSH / 8) {
        uint4 row = make_uint4(0u, 0u, 0u, 0u);
        if (pk >= 0) row = reinterpret_cast<const uint4*>(a.xh + ((size_t)b * a.rows_xh + pk) * DSH)[c];
        const size_t dst = (size_t)(v % a.steps) * 64 + 2 * (v / a.steps) + j;
        reinterpret_cast<uint4*>(a.xp + ((size_t)b * a.rows_xp + dst) * DSH)[c] = row;
    }
    if (c == 0 && v < a.n_blk) a.pidx[((size_t)b * a.n_blk + v) * 2 + j] = pk;
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
