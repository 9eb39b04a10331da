// The pivot rule of pivot.hip as device functions: shared by pivot_keys_kernel (pivot.hip) and pivot_sample_kernel (screen.hip), which
// must pick the same keys bit for bit.
#pragma once
#include "dagl_common.h"

namespace dagl {

// a key's feature row sum: its PIVOT_SLOTS partial sums (project16_kernel) added in slot order
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

// One wave, lane = key of the 64-key block v of image b.  The key's row sum (valid: the key exists -- keys past N and blocks past
// n_blk do not) ...
__device__ __forceinline__ float pivot_key_sum(const PivotArgs& a, int b, int v, int lane, bool& valid) {
    const int key = v * 64 + lane;
    valid = v < a.n_blk && key < a.N;
    float s = -__builtin_inff();
    if (valid) s = pivot_rowsum(a.rowsum + ((size_t)b * a.N + key) * PIVOT_SLOTS);
    return s;
}
// ... and the block's two pivots as key indices (-1: the block has no such key): a tie goes to the lower key, a NaN sum counts as -inf
__device__ __forceinline__ void pivot_pick2(float s, bool valid, int v, int lane, int& k0, int& k1) {
    if (!(s == s)) s = -__builtin_inff();
    const int p0 = pivot_pick(s, valid);
    const int p1 = pivot_pick(s, valid && lane != p0);           // never the same key twice
    k0 = p0 >= 0 ? v * 64 + p0 : -1;
    k1 = p1 >= 0 ? v * 64 + p1 : -1;
}

}  // namespace dagl
