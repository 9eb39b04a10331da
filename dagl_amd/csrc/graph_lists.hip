// The patch graph of a differentiable forward, from the neighbour lists that forward already holds: dagl_ce_core_forward's fixed-width
// lists [B, L, width] (selection order, a count per row) -> the CSR of dagl_ce_graph_fill (keys ascending inside a row, int64 offsets).
// The weights are the lists' own (exp(l_t) / Z_l with the unlisted keys' e^0 in Z_l = the export's A): nothing is computed here, data moves.
//
//   lists_rows_kernel<false>   a wavefront per query row, a slot per lane: ballot of the valid slots -> degree
//   row_scan_kernel            select.hip: int32 degrees -> int64 exclusive offsets, row_off[B L] = E
//   lists_rows_kernel<true>    the same wavefront per row: a slot's rank = valid slots with a smaller key, or an equal key in a lower
//                              slot (a stable order); the lane stores its entry at row_off[r] + rank
//
// Written for ARBITRARY lists: a count is clamped to [0, width], a key outside [0, N) is dropped before anything is stored, so every key
// of the result is valid whatever the lists hold.  E <= B L width <= capacity (checked on the host): no capacity test on the device.
// No atomics, no host read: the same lists give the same bits on every call, and the three launches can be captured.
#include "dagl_common.h"
#include "graph_rows.h"

namespace dagl {

constexpr int GL_ROWS = 4;                     // rows (wavefronts) per block

template <bool FILL>
__global__ __launch_bounds__(GL_ROWS * 64) void lists_rows_kernel(int n_rows, int width, int N, const int32_t* __restrict__ nb_idx,
                                                                  const float* __restrict__ nb_wgt, const float* __restrict__ nb_s,
                                                                  const int32_t* __restrict__ nb_cnt, int32_t* __restrict__ deg,
                                                                  const int64_t* __restrict__ row_off, int32_t* __restrict__ key,
                                                                  float* __restrict__ weight, float* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * GL_ROWS + (threadIdx.x >> 6);
    if (row >= n_rows) return;                                   // (the whole wavefront)
    const int cnt = min(max(nb_cnt[row], 0), width);             // the slots the row owns
    const size_t slot = (size_t)row * width + lane;              // read only where lane < cnt <= width
    const int k = (lane < cnt) ? nb_idx[slot] : -1;
    const bool valid = lane < cnt && k >= 0 && k < N;
    const unsigned long long mask = __ballot(valid);
    if (!FILL) {
        if (lane == 0) deg[row] = __popcll(mask);
        return;
    }
    int rank = 0;
    for (int t = 0; t < cnt; ++t) {                              // cnt is the same in every lane
        const int kt = __shfl(k, t);
        if (((mask >> t) & 1ull) && (kt < k || (kt == k && t < lane))) ++rank;
    }
    if (!valid) return;
    const int64_t e = row_off[row] + rank;                       // < row_off[row + 1] <= E
    key[e] = k;
    weight[e] = nb_wgt[slot];
    if (score) score[e] = nb_s[slot];
}

struct ListsWs { int32_t* deg; size_t bytes; };

static ListsWs lists_carve(void* ws, size_t n_rows) {
    Carver cv(ws);
    ListsWs w;
    w.deg = cv.take<int32_t>(n_rows);
    w.bytes = cv.bytes();
    return w;
}

static int launch_graph_from_lists(hipStream_t s, int n_rows, int width, int N, const int32_t* nb_idx, const float* nb_wgt, const float* nb_s,
                                   const int32_t* nb_cnt, int64_t* row_off, int32_t* key, float* weight, float* score, void* workspace) {
    const ListsWs w = lists_carve(workspace, (size_t)n_rows);
    const dim3 grid((n_rows + GL_ROWS - 1) / GL_ROWS), block(GL_ROWS * 64);
    hipLaunchKernelGGL(lists_rows_kernel<false>, grid, block, 0, s, n_rows, width, N, nb_idx, nb_wgt, nb_s, nb_cnt, w.deg, row_off, key,
                       weight, score);
    DAGL_LAUNCH_CHECK("lists_rows_kernel<degree>");
    const int rc = launch_row_scan(s, n_rows, w.deg, row_off);
    if (rc) return rc;
    hipLaunchKernelGGL(lists_rows_kernel<true>, grid, block, 0, s, n_rows, width, N, nb_idx, nb_wgt, nb_s, nb_cnt, w.deg, row_off, key,
                       weight, score);
    DAGL_LAUNCH_CHECK("lists_rows_kernel<fill>");
    return DAGL_OK;
}

}  // namespace dagl

using namespace dagl;

extern "C" {

// the patch graph from a forward's neighbour lists (no ABI bump: found by symbol)
size_t dagl_graph_from_lists_workspace_bytes(int B, int H, int W) {
    if (graph_dims_ok("dagl_graph_from_lists_workspace_bytes", B, H, W)) return 0;
    return lists_carve(nullptr, (size_t)B * make_grid(H, W).L).bytes;
}

int dagl_graph_from_lists(void* stream, int B, int H, int W, int width, const int32_t* nb_idx, const float* nb_wgt, const float* nb_s,
                          const int32_t* nb_cnt, int64_t* row_off_out, int32_t* key_out, float* weight_out, float* score_out,
                          int64_t capacity_edges, void* workspace, size_t ws_bytes) {
    int rc = graph_dims_ok("dagl_graph_from_lists", B, H, W);
    if (rc) return rc;
    DAGL_REQUIRE(width >= 1 && width <= DAGL_MAX_TOPK, "dagl_graph_from_lists: width=%d outside [1, %d]", width, DAGL_MAX_TOPK);
    const Grid g = make_grid(H, W);
    const int64_t n_rows = (int64_t)B * g.L, slots = n_rows * width;
    DAGL_REQUIRE(slots < (1ll << 31), "dagl_graph_from_lists: B L width = %lld slots, 2^31 or more", (long long)slots);
    DAGL_REQUIRE(nb_idx && nb_wgt && nb_cnt && row_off_out && key_out && weight_out, "dagl_graph_from_lists: null tensor pointer");
    DAGL_REQUIRE((nb_s == nullptr) == (score_out == nullptr), "dagl_graph_from_lists: nb_s and score_out go together (both or neither)");
    if (capacity_edges < slots) {
        set_error("dagl_graph_from_lists: capacity %lld edges < B L width = %lld", (long long)capacity_edges, (long long)slots);
        return DAGL_ERR_WORKSPACE;
    }
    if ((rc = check_workspace("dagl_graph_from_lists", workspace, ws_bytes, lists_carve(nullptr, (size_t)n_rows).bytes))) return rc;
    return launch_graph_from_lists((hipStream_t)stream, (int)n_rows, width, g.N, nb_idx, nb_wgt, nb_s, nb_cnt, row_off_out, key_out, weight_out,
                                   score_out, workspace);
}

}  // extern "C"
