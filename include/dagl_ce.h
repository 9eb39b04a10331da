/*
 * dagl_ce.h -- C ABI of the MI355X-native patch-graph attention head.
 *
 * One data-parallel hot path is implemented behind this boundary: the body of
 * the reference method CE.forward (DN_Gray/model/dagl.py:207-275, identical
 * forks in CAR/, Demosaic/, DN_Real/), i.e. everything after the four stock
 * prologue convolutions (dagl.py:208-215) up to and including the batch
 * concatenation (dagl.py:274).
 *
 * The reference has no FFI: its boundary is the Python call self.cX_Y(x) in
 * CES.forward (dagl.py:114,116,118).  The host-side mirror of that call is
 * dagl_amd.CE (an nn.Module with the reference's constructor, parameter names
 * and forward signature); it reaches the device code only through the entry
 * points declared here (ctypes), so that the same library can be bound from
 * any other host language.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 / int32 data unless stated;
 *   - buffers are caller-owned; nothing is allocated or freed in here;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     all work is enqueued on it; entry points that must read a device value
 *     back (noted below) wait for that copy (an event or a synchronise of that stream), nothing else ever does;
 *   - return value 0 = OK, negative = DAGL_ERR_*; dagl_last_error() gives a
 *     thread-local message; no entry point aborts the process;
 *   - the library holds no global mutable state and is re-entrant.
 *
 * Fixed hyper-parameters (constructor defaults the reference never overrides,
 * dagl.py:175-176, CES passes only in_channels, dagl.py:94-109):
 *   ksize 7, query stride 4, key/value stride 1, inter_channels 16,
 *   softmax_scale 10, patch length P = 16*7*7 = 784, feature length D = 196.
 */
#ifndef DAGL_CE_H
#define DAGL_CE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAGL_KSIZE      7
#define DAGL_QSTRIDE    4
#define DAGL_CH         16            /* inter_channels                         */
#define DAGL_P          784           /* patch row length  = 16*7*7             */
#define DAGL_D          196           /* similarity feature length = P/4        */
#define DAGL_DS         204           /* row stride (floats) of feature rows    */
#define DAGL_PADPIX     3             /* zero border of the padded NHWC maps    */

/* neighbour-selection modes */
#define DAGL_MODE_ADAPTIVE       0    /* shipped: relu(S - mean*thr + bias) != 0   (dagl.py:256-257) */
#define DAGL_MODE_TOPK           1    /* fixed-k variant (GReccR2b_3mh_1-checkpoint.py:242-250)      */
#define DAGL_MODE_ADAPTIVE_TOPK  2    /* adaptive mask intersected with the k best scores            */

/* OR-ed into `mode`: scan all L*N scores on the fp32 matrix cores instead of screening them in bf16 and
 * refining the survivors (both give the same neighbours)                             */
#define DAGL_FLAG_EXACT_SCAN     0x100
/* OR-ed into `mode`: this workspace last served an identical call -- same memory, same (B,H,W,mode,k), unchanged
 * fc1 / fc2 / g / theta weights -- and nothing else wrote to it since.  The call then reuses what that call left behind
 * (packed fc and convolution weights, the zero borders of the padded maps, the zero guard rows of the feature matrices)
 * instead of rebuilding it: four launches fewer per forward (inference loops)                                */
#define DAGL_FLAG_WEIGHTS_PACKED 0x200
/* OR-ed into `mode` (adaptive mode, >= 2048 keys): expect dense neighbourhoods -- go straight to the streamed dense
 * formulation (info->path 4) instead of trying per-query lists first.  A performance hint only: the result is the
 * same either way; info->total_edges tells the caller whether the hint still pays                              */
#define DAGL_FLAG_DENSE_HINT     0x400

/* OR-ed into `mode` (adaptive mode behind the bf16 screen): do not wait for the call's verdict on the host.  The few queries
 * whose neighbourhood overflows the lists are redone in-stream as always; whether that covered the call (it does not when
 * most queries overflow or the flagged rows are too heavy: the host would have sent the call to the dense formulation) is
 * decided on the device: an unserved call's output is NaN-filled -- never wrong numbers -- and dagl_ce_range_check reports
 * it (bit 1, sticky).  No host synchronisation at all: such a call can be captured into a HIP graph.  info is not filled
 * beyond required_bytes / path.  Callers use it once a workspace's calls have been served in-stream before (dagl_amd.CE).   */
#define DAGL_FLAG_NO_WAIT        0x800

/* OR-ed into `mode` (top-k modes behind the bf16 screen): take the candidate threshold from every SECOND key tile instead of the
 * sampled subset (every 8th tile; round 7: the two heaviest keys of every 64, where dagl_ce_pivot_debug applies) and give a query's candidate segments eight times the slots (every tile, where a gigabyte of records does not hold that many).  The sampled threshold is as good as the true k-th best on maps
 * whose scores are spread evenly (the synthetic benchmark features); on natural-image features the k-th best of an eighth of the
 * keys lies 4-25 % below the true one, hundreds to thousands of keys pass it, the slots overflow and most query groups land on
 * the fp32 redo pass (2.6 ms instead of 0.25 at 256^2, tools/time_real_image.py).  Costs half a pass more of the screen's
 * matrix work (+25 us at 256^2); the result is the same either way.
 * Round 4: WITHOUT either flag the choice is made ON THE DEVICE and kept in the workspace ("policy" word): a call whose sampled
 * threshold let ANY query overflow its candidate slots (its whole 128-query group takes the fp32 redo pass: 84 us per group at
 * 256^2) switches the workspace to the tight threshold for good (the word is sticky; kernels read it at their start: no host
 * poll, valid under HIP-graph replay).  On a cold workspace (no DAGL_FLAG_WEIGHTS_PACKED: the first call of a shape) a call with
 * more than a fiftieth of its query GROUPS flagged re-runs sampling, filter and refine with the tight threshold in-stream (four
 * gated launches that exit at once otherwise) instead of sending those groups to the fp32 redo pass: ~0.4 ms instead of 2.7 at
 * 256^2.  Maps of up to 16 384 keys start on the tight threshold (it costs nothing there).  A segment whose slots are full spills
 * into its query's shared area (256 records) before the query is flagged: the redo pass is left to maps flat enough for
 * thousands of candidates per query.  DAGL_FLAG_TIGHT_TOPK forces the tight threshold, DAGL_FLAG_SAMPLED_TOPK the
 * sampled one (tests, benchmarks of that path); dagl_ce_range_check's bit 2 still reports whether the last call's redo pass
 * had work.                                                                                                                    */
#define DAGL_FLAG_TIGHT_TOPK     0x1000
#define DAGL_FLAG_SAMPLED_TOPK   0x2000
/* OR-ed into `mode` (top-k modes behind the bf16 screen, dagl_ce_forward_fused): do NOT queue the fp32 redo pass behind the refine
 * kernel.  On a warm workspace that pass is one launch that finds nothing flagged and exits (4.7 us of a 0.23 ms call at 256^2:
 * the launch, not the grid).  Without it a call whose screen DID flag a query group (candidate slots and spill area full: maps flat
 * enough for thousands of candidates per query) cannot be served: its output is NaN-filled by the last kernel -- never wrong
 * numbers -- and dagl_ce_range_check reports it (bit 4, sticky) like a range violation.  For callers that poll: dagl_amd.CE sets it
 * once a poll has found the workspace's recent calls without redo work and drops it for good when a poll reports bit 4.       */
#define DAGL_FLAG_NO_REDO        0x4000

#define DAGL_MAX_TOPK            64   /* widest per-query neighbour LIST of the top-k modes (the fixed-k variant defaults to
                                         num_edge = 50, GReccR2b_3mh_1-checkpoint.py:155,243); k > N = H*W means every key:
                                         top_k = min(k, N) (:243), the lists are then min(k, N) wide.  min(k, N) beyond it
                                         (a stray sibling uses min(500, N), CA_model-checkpoint.py:134-143): the inference entry
                                         points take every query's score row in the dense form instead -- scores of 2048 queries
                                         at a time on the fp32 matrix cores, k-th largest per row by radix selection (ties to the
                                         lower key index, as in the lists), mask / softmax / weighted sum row-wise (info.path 6;
                                         ~5 ms per head at 256^2, k = 500); the training entry points (dagl_ce_core_forward,
                                         lists handed to the backward) and dagl_ces_stage_forward return an error for it      */
#define DAGL_FAST_CAP            64   /* per-query slots of the single-pass adaptive path (fp32 scan, training lists) */
#define DAGL_LIST_CAP           256   /* per-query slots of the screened adaptive path (inference): long-tailed degrees */

/* error codes */
#define DAGL_OK                   0
#define DAGL_ERR_INVALID         -1   /* bad argument (shape, mode, k, null pointer, alignment)      */
#define DAGL_ERR_WORKSPACE       -2   /* workspace too small; info->required_bytes says how much     */
#define DAGL_ERR_HIP             -3   /* a HIP call / launch failed (message has hipGetErrorString)  */
#define DAGL_ERR_NO_DEVICE       -4   /* no gfx950 device visible                                    */
#define DAGL_ERR_UNSUPPORTED     -5   /* training entry point: neighbourhood denser than DAGL_FAST_CAP */

typedef struct dagl_profile dagl_profile;     /* opaque stage profile, see dagl_profile_* below */

typedef struct dagl_ce_info {
    int64_t required_bytes;   /* workspace this call needed (valid on OK and on ERR_WORKSPACE)      */
    int64_t total_edges;      /* sum of degrees over all queries of the batch                       */
    int64_t redone_queries;   /* bf16 screen: queries whose candidate slots / list overflowed and were redone
                                 (-1 = not read back; the debug entry point and the adaptive mode read it);
                                 path 4: queries whose degree exceeds the neighbour lists' width (256)     */
    int32_t max_degree;       /* largest per-query degree                                           */
    int32_t path;             /* 0 = fp32 scan, single-pass lists, 1 = fp32 scan, two-pass CSR (some degree >
                                 FAST_CAP), 2 = fp32 scan, per-lane top-k lists, 3 = bf16 screen + refine,
                                 4 = dense neighbourhoods: streamed dense formulation (no lists),
                                 5 = dense formulation under autograd (dagl_ce_core_dense_forward),
                                 6 = top-k modes with min(k, N) > DAGL_MAX_TOPK: row-wise dense form (no lists),
                                 8 = graph export (dagl_ce_graph_count) */
    int32_t range_fallback;   /* 1 = an operand left the range of the split-fp16 kernels (|activation| >= 3750, see
                                 below: weights, dense-regime features, |b1| >= 1.5e7, non-finite input) and the call was re-run on the fp32 path */
    int32_t dense_rerun_blocks; /* path 4 / 5: blocks of 64 queries the streamed dense formulation ran a second time (rows whose
                                 exact maximum the top-1 screen could not serve: flat maps); 0 otherwise (ABI 404; was `reserved`) */
} dagl_ce_info;

/* Range of the default (split-fp16) path.
 * Activations (round 6): the fused entry points (dagl_ce_forward_fused, dagl_ces_stage_forward) have NO fixed limit on the input
 * and serve |b1| = |g(x)| < 1.5e7 with the same launches -- the prologue splits x with a power-of-two scale of each block's own
 * and writes the key / query map in two tiers (16 b1 and 2^-8 b1 as fp16 pairs), the projection multiplies the tier that holds the
 * head's values (csrc/dagl_common.h B1Tiers): finite in, finite out, on the first call, without a host round trip, under HIP-graph
 * replay.  (The reference's own fp32 logits 10 S m ~ b1^4 overflow at b1 ~ 2e8.)  dagl_ce_forward (maps computed by the caller)
 * and the training entry points keep the fine tier: |b1| < 3750.  Still fixed: |w_conv| < 234, |w_fc| < 58 (checked when the
 * weights are packed; dagl_amd.CE moves a module with larger weights to DAGL_FLAG_EXACT_SCAN before its first call) and
 * |features| < 937 in the dense regime.  A call that meets an operand beyond these (or a non-finite one) never returns numbers
 * computed from it: its output is NaN-filled by the last kernel, and
 *   - the adaptive modes, which read statistics back anyway, notice and re-run the call on the fp32 path at once
 *     (info->range_fallback = 1; the result is the exact scan's);
 *   - the top-k modes have no host round trip: dagl_ce_range_check(workspace) tells (one synchronisation) whether ANY
 *     call on that workspace left the range since the last check (the word is sticky and cleared by the check that
 *     reports it); re-run with DAGL_FLAG_EXACT_SCAN (no range limit).
 *   - the training entry points (dagl_project_patches16, dagl_ce_core_dense_forward) NaN-fill their outputs likewise; the
 *     dense forward re-runs itself in its fp32 form when it reads statistics back (info != NULL, range_fallback = 1).   */
int dagl_ce_range_check(void* stream, int B, int H, int W, int mode, int k, void* workspace, size_t ws_bytes,
                        int* violated /* bit 0: range, bit 1: an unserved DAGL_FLAG_NO_WAIT call, bit 2 (top-k modes, not sticky):
                                         the LAST call's redo pass had flagged query groups (see DAGL_FLAG_TIGHT_TOPK), bit 3 (top-k
                                         modes): the workspace's threshold policy word has switched to the tight threshold, bit 4 (sticky):
                                         a DAGL_FLAG_NO_REDO call had flagged query groups (its output is NaN-filled) */);

/* ---- library ------------------------------------------------------------------------------- */
/* ABI version of THIS header: bumped whenever a struct or a signature declared here changes (round 3: dagl_ce_info is 40
 * bytes, dagl_ce_prologue takes `scratch`, dagl_ce_core_dense_forward takes `flags`, k <= 64; round 4: DAGL_FLAG_SAMPLED_TOPK,
 * the workspace layout carries the top-k policy words; 403: dagl_ce_core_wide_forward / _backward; 404:
 * dagl_ce_info.dense_rerun_blocks in the place of `reserved`; 405: dagl_fc_grad16_dmap; 408: dagl_ce_graph_*; 409: dagl_graph_apply*;
 * 410: dagl_ce_core_dense_chunk_floats, dagl_ce_core_dense_plan; 411: dagl_ce_pivot_debug; 412: dagl_graph_attend*;
 * workspace sizes unchanged).  dagl_graph_forward* (the training pair dagl_graph_forward_train / _backward included), dagl_ce_wide_debug, dagl_graph_from_lists*, dagl_graph_refresh*, dagl_graph_step*, dagl_graph_stage_step*, dagl_graph_search*, dagl_graph_stage_search*,
 * dagl_ces_stage_fold_mix, dagl_ces_stage_mix, dagl_graph_stage_forward*, dagl_ces_stage_mix_backward*, dagl_fc_grad16_plan,
 * dagl_conv_pair_backward_plan, dagl_ce_prologue16_plan, dagl_ce_prologue16_debug*, dagl_project16_plan and dagl_ce_project16_debug* came in without a bump -- no declared signature or struct changed --: a caller that
 * wants them detects them by symbol (dlsym), as dagl_amd/_lib.py does for every entry of its table.  A caller compares
 * dagl_version() with the DAGL_ABI_VERSION it was built against and refuses a mismatch (dagl_amd/_lib.py does).           */
#define DAGL_ABI_VERSION 412
int         dagl_version(void);                 /* DAGL_ABI_VERSION of the library = 10000*major + 100*minor + patch */
const char* dagl_last_error(void);              /* thread-local, never NULL                         */
int         dagl_device_check(void);            /* OK iff the current HIP device is gfx950          */

/* Measurement aid (bench.py's roofline line; replaces nothing in the reference): what the matrix pipes SUSTAIN on this device
 * under the screen's multiply stream alone -- `blocks` blocks of 16 waves, `steps` x 26 v_mfma_f32_32x32x16_bf16 per wave,
 * operands in registers.  clocks[2*b] = shader clocks, clocks[2*b+1] = 100 MHz ticks of block b's loop (device memory,
 * 2*blocks uint64); sink = one float of device memory.  FLOP of a launch = blocks * 16 * steps * 26 * 32768; time it with
 * events on `stream`.                                                                                                      */
int dagl_probe_mfma_bf16(void* stream, int blocks, int steps, unsigned long long* clocks, float* sink);
/* Self-test (replaces nothing in the reference): the wave-wide reductions / scan the per-query kernels run on the DPP path
 * (dagl_amd/csrc/dagl_common.h) against a serial evaluation; *mismatches_dev (one int of device memory) = lanes that disagree. */
int dagl_selftest_wave_ops(void* stream, int* mismatches_dev);

/* ---- whole block: replaces dagl.py:216-274 (CE.forward after its prologue convs) -------------- */

/* Bytes of workspace dagl_ce_forward needs for the single-pass / top-k paths (a two-pass CSR
 * fallback may ask for more through DAGL_ERR_WORKSPACE + info->required_bytes).                  */
size_t dagl_ce_workspace_bytes(int B, int H, int W, int mode, int k);

/*
 * b1   [B,16,H,W]  g(b)      key/query feature map   (dagl.py:208)
 * b2   [B,16,H,W]  theta(b)  value feature map       (dagl.py:209)
 * thr  [B,L]       thr_conv(same_pad(b))             (dagl.py:213-214)   L = ceil(H/4)*ceil(W/4)
 * bias [B,L]       bias_conv(same_pad(b))            (dagl.py:215)
 *      (thr/bias may be NULL in DAGL_MODE_TOPK)
 * fc1_w [196,784] fc1_b [196]  query projection  (dagl.py:196-199), element order (c,kh,kw)
 * fc2_w [196,784] fc2_b [196]  key   projection  (dagl.py:200-203)
 * out  [B,16,H,W]  the block's return value          (dagl.py:274)
 * The adaptive mode waits on the host for its verdict (overflowed queries, degrees): a small copy + event queued
 * behind the neighbour refinement, in front of the gather / fold -- those are still running when the call returns;
 * calls that fall back to the dense formulation / CSR lists synchronise `stream` once more for their counters.
 */
int dagl_ce_forward(void* stream, int B, int H, int W,
                    const float* b1, const float* b2, const float* thr, const float* bias,
                    const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                    int mode, int k, float* out,
                    void* workspace, size_t ws_bytes, dagl_ce_info* info);

/* The whole of CE.forward (dagl.py:207-275) from the block's input: the four prologue convolutions are
 * computed in here too (prologue.hip), so no stock conv runs on the path.
 *   x [B,64,H,W];  g_w [16,64,3,3] g_b [16];  theta_w [16,64,1,1] theta_b [16];
 *   thr_w / bias_w [1,64,7,7], thr_b / bias_b [1]  (may be NULL in DAGL_MODE_TOPK)
 *   prof: optional stage profile (NULL = none)                                                    */
int dagl_ce_forward_fused(void* stream, int B, int H, int W, const float* x,
                          const float* g_w, const float* g_b, const float* theta_w, const float* theta_b,
                          const float* thr_w, const float* thr_b, const float* bias_w, const float* bias_b,
                          const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                          int mode, int k, float* out,
                          void* workspace, size_t ws_bytes, dagl_ce_info* info, dagl_profile* prof);

/* One CES stage (DN_Gray/model/dagl.py:114,116,118): the four heads that share the input x, the 1x1 mixing
 * convolution over their concatenation and the residual,
 *     out = conv1x1(cat(head_1(x), .., head_4(x))) + x,          x, out: [B,64,H,W]
 * as ONE launch set: the heads become a batch dimension (4x fewer launches, 4x more blocks per launch).
 * Dense adaptive neighbourhoods (degree > DAGL_FAST_CAP) are not served here: the call returns
 * DAGL_ERR_WORKSPACE with info->required_bytes = -1 and the caller falls back to four dagl_ce_forward_fused
 * calls + its own mix.  mix_w [64,64,1,1], mix_b [64].                                               */
typedef struct dagl_ce_weights {
    const float *g_w, *g_b, *theta_w, *theta_b, *thr_w, *thr_b, *bias_w, *bias_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} dagl_ce_weights;
size_t dagl_ces_stage_workspace_bytes(int B, int H, int W, int mode, int k);
int dagl_ces_stage_forward(void* stream, int B, int H, int W, const float* x, const dagl_ce_weights* heads4,
                           const float* mix_w, const float* mix_b, int mode, int k, float* out,
                           void* workspace, size_t ws_bytes, dagl_ce_info* info, dagl_profile* prof);

/* Same call with optional per-query read-outs for parity tests (any of them may be NULL):
 *   deg_out [B,L] int32  neighbours per query     (reference: (mask != 0).sum(1), dagl.py:257)
 *   rowsum_out [B,L]     sum_j A_ij               (reference: softmax mass left after masking, :261)
 *   agg_out [B,L,784]    aggregated query patches (reference: torch.mm(yi,pi), :263-264), element
 *                        order (kh,kw,c)                                                           */
int dagl_ce_forward_debug(void* stream, int B, int H, int W,
                          const float* b1, const float* b2, const float* thr, const float* bias,
                          const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                          int mode, int k, float* out,
                          void* workspace, size_t ws_bytes, dagl_ce_info* info,
                          int32_t* deg_out, float* rowsum_out, float* agg_out);

/* (ABI 411) Read-out for tests of the top-k screen's threshold source (csrc/pivot.hip): calls of a top-k mode behind the screen that
 * use the SAMPLED threshold (the policy word, or DAGL_FLAG_SAMPLED_TOPK) with k <= 16 on maps of N >= 1024 k keys take it from the
 * two keys with the largest feature row sum of every 64 consecutive keys.  What the LAST such call on `workspace` (same B, H, W,
 * mode, k) left there, copied to device memory (either pointer may be NULL):
 *   pivot_idx_out  [B, ceil(N/64), 2] int32  the picked keys of every 64-key block, larger row sum first (-1: the block holds no
 *                                            second key)
 *   key_rowsum_out [B, N] fp32               sum over the 196 features of relu(fc2(patch)), as the kernel adds it up
 * The row sums share their workspace region with the aggregated rows: after a call that materialised those (dagl_ce_forward_debug
 * with agg_out) only pivot_idx_out is meaningful.  Under the workspace's policy word (neither threshold flag) the pivots are used
 * only by calls that carry DAGL_FLAG_WEIGHTS_PACKED (a workspace that last served an identical call), and only where the tile
 * sampling would skip three of four tiles or more (long key streams): every other call under the policy word -- a caller that
 * never sets that flag included -- keeps the tile sampling, whose overflow on such a call decides the policy.
 * DAGL_ERR_UNSUPPORTED: calls of this shape / mode / k keep the tile sampling (nothing was written).                              */
int dagl_ce_pivot_debug(void* stream, int B, int H, int W, int mode, int k, void* workspace, size_t ws_bytes,
                        int32_t* pivot_idx_out, float* key_rowsum_out);

/* Read-out for tests of the wide top-k path (csrc/topk_wide.hip; found by symbol, no ABI bump): top-k modes with 64 < min(k, N)
 * <= 1024 hand every query row to a one-block list kernel, which declines the rows whose sample misleads it (too many candidates for
 * a wave's segment, or fewer than k in all); declined rows go through the three-kernel form behind it, as every row does when
 * min(k, N) > 1024.  What the LAST such call on `workspace` (same B, H, W, mode, k) left there for its LAST batch of query rows -- with
 * L <= 2048 that is every row of the last image --, copied to device memory:
 *   served_out [min(L, rows per batch)] int32   1 = the list kernel served the row, 0 = it declined it
 * DAGL_ERR_UNSUPPORTED: calls of this mode / k are not on the wide path, or run no list kernel (nothing was written).           */
int dagl_ce_wide_debug(void* stream, int B, int H, int W, int mode, int k, void* workspace, size_t ws_bytes, int32_t* served_out);

/* ---- (ABI 408) the learned patch graph as CSR: csrc/graph.hip --------------------------------------------------------------------
 * For every image and query patch i the keys j with mask_b[i,j] != 0 and their weights A[i,j] = softmax(10 S m)[i,j] mask_b[i,j]
 * -- the non-zeros of `yi`, dagl.py:256-261; not renormalised: the masked keys' e^0 stay in the denominator -- in all three modes
 * (DAGL_MODE_TOPK: the min(k, N) best scores, ties to the lower key index; DAGL_MODE_ADAPTIVE_TOPK: the k best of the keys that pass
 * the adaptive test).  No flags in `mode`.  CSR over the B L query rows:
 *   row_off [B L + 1] int64   row offsets (a dense graph at 256^2 holds 2.7e8 edges)
 *   key     [E] int32         key patch index 0 .. N-1, row-major over H x W, strictly ascending inside a row
 *   weight  [E] fp32          A[i,j]
 *   score   [E] fp32          S[i,j] (optional)
 * Everything runs on the all-fp32 route (DAGL_FLAG_EXACT_SCAN's projections and thresholds, score rows on the fp32 matrix cores a
 * chunk of `rows_per_chunk` query rows at a time; 0 = the library's choice, at most 2048): the reference semantics, which agree with
 * the neighbours a screened forward used except at pairs within fp32 rounding of the selection boundary.  Inputs as dagl_ce_forward's
 * (any input width) without the value map, which the graph does not depend on.  A diagnostic path: nothing here is tuned for speed.
 * Two phases around ONE host read:
 *   dagl_ce_graph_count   queues everything up to the exclusive scan of the degrees into row_off_out (device memory) and returns
 *                         without synchronising; row_off_out[r + 1] - row_off_out[r] are the exact degrees, row_off_out[B L] the
 *                         number of edges E -- the caller reads that word (its one synchronisation), allocates E entries and calls
 *   dagl_ce_graph_fill    with the SAME workspace, untouched in between (it holds the features and each row's selection threshold
 *                         and softmax statistics), the same B, H, W, mode, k, rows_per_chunk, the offsets and total_edges = the
 *                         word it read.  capacity_edges < total_edges is DAGL_ERR_WORKSPACE, never a partial write (the kernels
 *                         check the capacity against the device's own total once more and write nothing beyond it).
 * The arrays are the same on every call (ordered compaction, fixed-order fp64 sums, no atomics).  info: required_bytes, path 8.      */
size_t dagl_ce_graph_workspace_bytes(int B, int H, int W, int mode, int k, int rows_per_chunk);
int dagl_ce_graph_count(void* stream, int B, int H, int W, const float* b1, const float* thr, const float* bias,
                        const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b, int mode, int k,
                        int rows_per_chunk, int64_t* row_off_out, void* workspace, size_t ws_bytes, dagl_ce_info* info);
int dagl_ce_graph_fill(void* stream, int B, int H, int W, int mode, int k, int rows_per_chunk, const int64_t* row_off,
                       int32_t* key_out, float* weight_out, float* score_out /* may be NULL */, int64_t total_edges,
                       int64_t capacity_edges, void* workspace, size_t ws_bytes);

/* ---- (ABI 409) a block run on a GIVEN patch graph: csrc/graph_apply.hip ------------------------------------------------------------
 * The consumer of the export above:  out[b] = fold(A_G[b] . V(b2[b])) / cnt  -- dagl.py:263-272 with `yi` supplied by the caller: A_G[b]
 * the [L, N] matrix the CSR rows b L .. b L + L - 1 describe, V the 7x7 stride-1 patches of the value map theta(x) (dagl.py:209, 224),
 * fold and overlap count those of dagl_fold_normalize.  The graph need not come from dagl_ce_graph_fill: keys may be in any order inside
 * a row and may repeat (repeats add up), weights are arbitrary floats, a row may be empty or longer than N.  A key outside [0, N)
 * contributes nothing; it is tested before an address is formed, so no array content makes a kernel read outside the map.
 *   b2p     [B,H+6,W+6,16]  zero-bordered NHWC value map, as dagl_ce_prologue writes it (value rows are read from it on the fly)
 *   row_off [B L + 1] int64, key [E] int32, weight [E] fp32   (key / weight may be NULL when total_edges = 0);  total_edges < 2^31
 *   out     [B,16,H,W]
 * The edge array is cut into segments of dagl_graph_apply_segment() edges, a block each, whatever rows they belong to: the longest
 * row does not set the launch time and short rows share a block; the partial rows of a row that crosses segments are added in segment
 * order (no float atomics): two calls on the same arrays return the same bits.  Grids come from total_edges and B L: nothing is read
 * on the host, the call can be captured.  Workspace: dagl_graph_apply_workspace_bytes = [B L, 784] aggregated rows + one 784-float
 * partial row per segment (24.5 bytes per edge).
 *
 * dagl_graph_apply_backward: gradients of that call.  dAgg = unfold(d_out / cnt);
 *   d_weight [E]  (may be NULL)  d_weight[e] = <dAgg[row(e)], V[key(e)]>, the patch read from the map; 0 for a key outside [0, N)
 *   d_b2p [B,H+6,W+6,16] (may be NULL)  the stride-1 adjoint of unfold of the rows d V = A_G^T dAgg, every element written (the
 *           border too).  d V runs through the same segmented product over the TRANSPOSED CSR, which the caller supplies:
 *           col_off [B N + 1] int64 offsets over the columns b N + key, src_row [E] int32 the query row b L + i of each transposed edge,
 *           perm [E] int32 its position in key / weight (a stable sort of b N + key: dagl_amd.PatchGraph.transpose); entries outside
 *           their range contribute nothing.
 * Workspace: dagl_graph_apply_backward_workspace_bytes = dAgg [B L, 784] + the d V rows [B N, 784] (205 MB at 256^2: this route
 * materialises them, which is acceptable for a diagnostic / fine-tuning path) + the partial rows.  Fixed summation order throughout. */
int    dagl_graph_apply_segment(void);
size_t dagl_graph_apply_workspace_bytes(int B, int H, int W, int64_t total_edges);
size_t dagl_graph_apply_backward_workspace_bytes(int B, int H, int W, int64_t total_edges);
int dagl_graph_apply(void* stream, int B, int H, int W, const float* b2p, const int64_t* row_off, const int32_t* key,
                     const float* weight, int64_t total_edges, float* out, void* workspace, size_t ws_bytes);
int dagl_graph_apply_backward(void* stream, int B, int H, int W, const float* b2p, const int64_t* row_off, const int32_t* key,
                              const float* weight, int64_t total_edges, const float* d_out, const int64_t* col_off,
                              const int32_t* src_row, const int32_t* perm, float* d_b2p /* may be NULL */,
                              float* d_weight /* may be NULL */, void* workspace, size_t ws_bytes);

/* ---- (ABI 412) attention on a GIVEN patch graph: csrc/graph_attend.hip ---------------------------------------------------------------
 * The third leg next to the export and dagl_graph_apply: the block's own edge weights on a structure the caller supplies -- dagl.py:250-261
 * restricted to the edges of the CSR -- and their gradients.  Rows r = b L + i, key_e in [0, N) a key of image b = r / L:
 *   wq_rows [B,L,196], x_rows [B,N,196]  the fc1 / fc2 features (contiguous 784-byte rows, 16-byte aligned)
 *   S_e = <wq_rows[r], x_rows[b, key_e]>                                       -> score [E]
 *   tau [B L] given:  m_e = relu(S_e - tau_r), z_e = scale S_e m_e, on_e = (m_e != 0)   (the adaptive rule; tau_r = mean_j(S_rj) thr_r - bias_r)
 *   tau NULL:         z_e = scale S_e, on_e = 1                                         (the fixed-k variant)
 *   flags = 0:  M = max(max_e z_e, 0 if deg_r < N),  D = sum_e e^(z_e - M) + max(N - deg_r, 0) e^(-M): every key off the graph counts as
 *               the reference's e^0;  DAGL_GRAPH_ATTEND_EDGES_ONLY: a plain softmax over the row's edges, M = max_e z_e, D = sum_e e^(z_e - M)
 *   w_e = on_e e^(z_e - M) / D                                                 -> weight [E]
 * deg_r counts edges: a repeated key is an entry of its own (it is NOT merged with its twin).  Empty rows produce nothing.  A key outside
 * [0, N) is tested before an address is formed: it scores 0, weighs 0 and takes part in D with score 0.
 * Edges are cut into segments of dagl_graph_apply_segment() whatever rows they belong to; maxima are fp32, the sums of the statistics fp64,
 * every sum has a fixed order and there are no float atomics: the same arrays give the same bits on every call.  Grids come from
 * total_edges and the row counts: nothing is read on the host, the calls can be captured.  total_edges = 0: key, score, weight may be NULL.
 *
 * dagl_graph_attend_backward: with g_e = d_weight[e], c_r = sum_e w_e g_e:
 *   d S_e = scale (m_e + S_e) w_e (g_e - c_r) on edges with on_e (tau given), scale w_e (g_e - c_r) (tau NULL), else 0
 *   d_tau [B L]           = -scale sum_on S_e w_e (g_e - c_r)                    (may be NULL; needs tau)
 *   d_wq_rows [B,L,196]   = sum_{e in r} d S_e x_rows[b, key_e]                  (may be NULL)
 *   d_x_rows [B,N,196]    = sum_{key_e = j} d S_e wq_rows[r_e]                   (may be NULL; needs the transposed CSR of
 *                           dagl_graph_apply_backward: col_off [B N + 1], src_row [E], perm [E])
 * Every element of a requested output is written.  score / weight are the forward's outputs. */
#define DAGL_GRAPH_ATTEND_EDGES_ONLY 0x1
size_t dagl_graph_attend_workspace_bytes(int B, int H, int W, int64_t total_edges);
size_t dagl_graph_attend_backward_workspace_bytes(int B, int H, int W, int64_t total_edges);
int dagl_graph_attend(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const int64_t* row_off,
                      const int32_t* key, int64_t total_edges, const float* tau /* NULL: no margin */, float scale,
                      int flags /* bit 0: edges-only normalisation */, float* score, float* weight, void* workspace, size_t ws_bytes);
int dagl_graph_attend_backward(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const int64_t* row_off,
                               const int32_t* key, int64_t total_edges, const float* tau, float scale, int flags, const float* score,
                               const float* weight, const float* d_weight, const int64_t* col_off, const int32_t* src_row,
                               const int32_t* perm, float* d_wq_rows /* may be NULL */, float* d_x_rows /* may be NULL */,
                               float* d_tau /* may be NULL */, void* workspace, size_t ws_bytes);

/* ---- the forward on a GIVEN patch graph in one crossing of the edges: csrc/graph_forward.hip (ABI 412, detected by symbol) ----------
 * out = dagl_graph_apply(weight = dagl_graph_attend(...)) without materialising `score` or `weight`: the operands and the semantics are
 * exactly those written above for the two entries -- S_e, with tau the margin m_e, z_e, on_e; flags = 0 the reference's normalisation
 * (every key off the graph counts as e^0), DAGL_GRAPH_ATTEND_EDGES_ONLY the edges-only softmax; a repeated key is an entry of its own;
 * a key outside [0, N) is tested before an address is formed, scores 0, takes part in D and contributes no value row; empty rows give
 * zero aggregated rows; fold and overlap count are dagl_graph_apply's.
 *   wq_rows [B,L,196], x_rows [B,N,196] fp32 (16-byte aligned), b2p [B,H+6,W+6,16] the zero-bordered value map (16-byte aligned),
 *   row_off [B L + 1] int64, key [E] int32 (may be NULL when total_edges = 0: the output is all zeros), tau [B L] or NULL, out [B,16,H,W]
 * One launch per segment of dagl_graph_apply_segment() edges forms the scores and, per run of edges that share a row, the fp32 maximum,
 * the fp64 sum of e^(z - max) and the 784-float partial row sum on_e e^(z - max) V[key_e]; a launch per row brings those onto the row's
 * maximum in segment order, adds the (N - deg) e^(-M) term and divides; the fold follows: three launches for the six of the two calls.
 * No float atomics, fixed summation order: the same arrays give the same bits on every call (they differ from the two-call result by
 * fp32 roundings: the weights are applied as e^(z - max) and scaled afterwards).  Grids come from total_edges and B L: nothing is read
 * on the host, the call can be captured.  Workspace: dagl_graph_forward_workspace_bytes = [B L, 784] aggregated rows + per segment one
 * 784-float partial row and a (max, sum) slot + a slot per row.  Every argument is checked before the first launch. */
size_t dagl_graph_forward_workspace_bytes(int B, int H, int W, int64_t total_edges);
int dagl_graph_forward(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                       const int64_t* row_off, const int32_t* key, int64_t total_edges, const float* tau /* NULL: no margin */, float scale,
                       int flags /* bit 0: edges-only normalisation */, float* out, void* workspace, size_t ws_bytes);

/* ---- training on a GIVEN patch graph in one crossing of the edges: csrc/graph_forward.hip (ABI 412, detected by symbol) --------------
 * dagl_graph_forward_train: dagl_graph_forward -- the same operands, checks, launches and workspace (dagl_graph_forward_workspace_bytes),
 * `out` bit for bit -- plus one launch that leaves the row statistics the forward normalised with:
 *   row_max_out [B L] fp32 = M_r, row_sum_out [B L] fp64 = D_r (the (N - deg) e^(-M) term included); an empty row gets 0 and 1, which
 *   nothing reads.  These twelve bytes per row are all a caller keeps for the backward: no per-edge array.
 * dagl_graph_forward_backward: the gradients of that forward from d_out [B,16,H,W], the forward's operands and (row_max, row_sum).  With
 * dAgg = unfold(d_out / cnt) as dagl_graph_apply_backward forms it and w_e = on_e e^(z_e - M_r) / D_r recomputed from the saved statistics:
 *   g_e = <dAgg[r], V[key_e]> (0 on an edge without a value row),  c_r = sum_e w_e g_e
 *   d S_e = scale (m_e + S_e) w_e (g_e - c_r) on edges with on_e (tau given), scale w_e (g_e - c_r) (tau NULL), else 0
 *   d_tau [B L]           = -scale sum_on S_e w_e (g_e - c_r)                    (may be NULL; needs tau)
 *   d_wq_rows [B,L,196]   = sum_{e in r} d S_e x_rows[b, key_e]                  (may be NULL)
 *   d_x_rows [B,N,196]    = sum_{key_e = j} d S_e wq_rows[r_e]                   (may be NULL; needs the transposed CSR)
 *   d_b2p [B,H+6,W+6,16]  = the fold of d V[j] = sum_{key_e = j} w_e dAgg[r_e]   (may be NULL; needs the transposed CSR)
 * col_off [B N + 1] / src_row [E] / perm [E]: the transposed CSR of dagl_graph_apply_backward.  Every element of a requested output is
 * written, and any subset of the outputs carries the bits of the full call.  One launch per segment of dagl_graph_apply_segment() edges
 * recomputes S_e (the forward's own arithmetic: the heaviest edge of a one-hot row weighs exactly 1), w_e and g_e and leaves the fp64
 * partial sums of c_r and d tau_r; a launch per row finishes them; the three products are segment + combine launches over the CSR and
 * its transpose, d S_e formed where a segment is staged; d V rows are folded as dagl_graph_apply_backward folds them.  Maxima fp32,
 * sums of statistics fp64 in edge and segment order, no float atomics: the same arrays give the same bits on every call.  A key,
 * src_row or perm entry outside its range is tested before an address is formed and contributes nothing (the key still counted in D).
 * Grids come from total_edges and the row counts: nothing is read on the host.  Workspace: dagl_graph_forward_backward_workspace_bytes =
 * dAgg [B L, 784] + d V rows [B N, 784] + a partial row per segment + three floats per edge (S, w, g: scratch of this call) + three
 * fp64 sums per row and per segment.  Every argument is checked before the first launch: null pointers, 16-byte alignment of the
 * feature rows, the maps and the gradient rows, d_tau without tau, d_x_rows / d_b2p without the transposed CSR, the workspace size. */
int dagl_graph_forward_train(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                             const int64_t* row_off, const int32_t* key, int64_t total_edges, const float* tau /* NULL: no margin */,
                             float scale, int flags /* bit 0: edges-only normalisation */, float* out, float* row_max_out,
                             double* row_sum_out, void* workspace, size_t ws_bytes);
size_t dagl_graph_forward_backward_workspace_bytes(int B, int H, int W, int64_t total_edges);
int dagl_graph_forward_backward(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                                const int64_t* row_off, const int32_t* key, int64_t total_edges, const float* tau, float scale, int flags,
                                const float* row_max, const double* row_sum, const float* d_out, const int64_t* col_off,
                                const int32_t* src_row, const int32_t* perm, float* d_wq_rows /* may be NULL */,
                                float* d_x_rows /* may be NULL */, float* d_tau /* may be NULL */, float* d_b2p /* may be NULL */,
                                void* workspace, size_t ws_bytes);

/* ---- a whole CES stage on its FROZEN graph, forward and backward: csrc/graph_forward.hip, csrc/stage_mix_grad.hip (ABI 412, by symbol) --
 * dagl_graph_stage_forward: dagl_graph_forward for the four heads of a stage in ONE launch set, ending in dagl_ces_stage_fold_mix.  The
 * kernels of dagl_graph_forward take the image of a row as row / L, so the heads' operands stacked head-major are those of 4 B images:
 *   wq_rows4 [4,B,L,196], x_rows4 [4,B,N,196] (16-byte aligned), b2p4 [4,B,H+6,W+6,16] (16-byte aligned), tau4 [4,B,L] or NULL: contiguous,
 *   (row_off [4 B L + 1], key [E]) ONE CSR over the head-major rows, row (h B + b) L + i = query i of image b under head h, keys in [0, N);
 *   x [B,64,H,W] the stage's input, mix_w [64,64], mix_b [64], out [B,64,H,W] = conv1x1(cat_h(fold(agg_h) / cnt)) + mix_b + x.
 * Launches: the segment and combine launches of dagl_graph_forward with B' = 4 B, then the fused fold + mix on the aggregated rows; every
 * row is dagl_graph_forward's for its head bit for bit.  total_edges = 0 gives mix_b + x.  The three training outputs come together or not
 * at all (refused otherwise) and leave `out` bit for bit: row_max_out [4 B L] fp32 / row_sum_out [4 B L] fp64 (dagl_graph_forward_train's,
 * one more launch) and cat_out [4,B,16,H,W], the pre-mix concat map head-major (one fold launch with B' = 4 B: dagl_graph_forward's `out`
 * of the stacked operands, the values the fused kernel forms per pixel).  Workspace: dagl_graph_forward_workspace_bytes of 4 B images.
 * Checks: the shape (4 B H W < 2^30), dagl_graph_forward's on the stacked operands, the mix operands, the training outputs, the workspace.
 *
 * dagl_ces_stage_mix_backward: the backward of that last launch from d_out [B,64,H,W] and the saved cat4 [4,B,16,H,W]:
 *   d_cat4 [4,B,16,H,W][h,b,c,p] = sum_o mix_w[o][16 h + c] d_out[b,o,p] -- head-major and NOT divided by the overlap count: viewed as
 *     [4 B,16,H,W] it is the d_out of dagl_graph_forward_backward on the stacked operands, which divides;
 *   d_mix_w [64,64][o][c] = sum_{b,p} d_out[b,o,p] cat[b,c,p], d_mix_b [64][o] = sum_{b,p} d_out[b,o,p]   (each may be NULL; cat4 may be
 *     NULL when both are).  The gradient of the residual input x is d_out itself.
 * fp32 MFMA 16x16x4 throughout; the weight gradient is split over contiguous pixel ranges -- the number of blocks depends on B H W alone
 * and is capped --, every wave leaves its 64 x 64 tile and bias sums in a slot of its own and one more launch adds the slots in slot order
 * in fp64: no float atomics, the same operands give the same bits on every call.  d_out, cat4 and d_cat4 must be 16-byte aligned. */
size_t dagl_graph_stage_forward_workspace_bytes(int B, int H, int W, int64_t total_edges);
int dagl_graph_stage_forward(void* stream, int B, int H, int W, const float* wq_rows4, const float* x_rows4, const float* b2p4,
                             const int64_t* row_off, const int32_t* key, int64_t total_edges, const float* tau4 /* NULL: no margin */,
                             float scale, int flags /* bit 0: edges-only normalisation */, const float* x, const float* mix_w,
                             const float* mix_b, float* out, float* row_max_out /* may be NULL */, double* row_sum_out /* may be NULL */,
                             float* cat_out /* may be NULL */, void* workspace, size_t ws_bytes);
size_t dagl_ces_stage_mix_backward_workspace_bytes(int B, int H, int W);
int dagl_ces_stage_mix_backward(void* stream, int B, int H, int W, const float* d_out, const float* cat4, const float* mix_w, float* d_cat4,
                                float* d_mix_w /* may be NULL */, float* d_mix_b /* may be NULL */, void* workspace, size_t ws_bytes);

/* ---- the patch graph of a differentiable forward, from its own neighbour lists: csrc/graph_lists.hip (ABI 412, detected by symbol) ---
 * dagl_ce_core_forward leaves each query's neighbours as fixed-width lists in selection order; nb_wgt = exp(l_t) / Z_l with the unlisted
 * keys' e^0 in Z_l is exactly the export's A = softmax(10 S m) mask.  This call changes the container alone: lists -> the CSR of
 * dagl_ce_graph_fill.  It is written for ARBITRARY lists, not only for what the selection produces:
 *   nb_idx [B,L,width] int32, nb_wgt [B,L,width] fp32, nb_s [B,L,width] fp32 or NULL, nb_cnt [B,L] int32;  1 <= width <= 64
 *   row r = b L + i owns the slots t < min(max(nb_cnt[r], 0), width); a slot whose key is outside [0, H W) is dropped (every key written
 *   is valid, whatever a range-violating call left in the lists); the survivors are written in ascending key order, equal keys in slot
 *   order (stable), weight and score following their key.
 *   row_off_out [B L + 1] int64  exclusive scan of the surviving degrees, row_off_out[B L] = E
 *   key_out / weight_out / score_out [capacity_edges]  entries [0, E) written, nothing at E and beyond; score_out NULL iff nb_s NULL
 * capacity_edges < B L width is DAGL_ERR_WORKSPACE (E cannot exceed B L width, so the kernels carry no capacity test of their own);
 * B L width >= 2^31 is DAGL_ERR_INVALID.  One call queues three launches -- a wavefront per row counts its valid slots (ballot), the
 * exclusive scan, the same wavefront per row ranks and stores its slots -- with no host read and no atomics: the same lists give the
 * same bits on every call, and the call can be captured (the CALLER reads row_off_out[B L] to learn E).  Workspace:
 * dagl_graph_from_lists_workspace_bytes = the [B L] int32 degrees.  Every argument is checked before the first launch. */
size_t dagl_graph_from_lists_workspace_bytes(int B, int H, int W);
int dagl_graph_from_lists(void* stream, int B, int H, int W, int width, const int32_t* nb_idx, const float* nb_wgt,
                          const float* nb_s /* may be NULL */, const int32_t* nb_cnt, int64_t* row_off_out /* [B L + 1] */,
                          int32_t* key_out, float* weight_out, float* score_out /* NULL iff nb_s is NULL */, int64_t capacity_edges,
                          void* workspace, size_t ws_bytes);

/* ---- refresh of a patch graph on a new input: csrc/graph_refresh.hip (ABI 412, detected by symbol) -----------------------------------
 * The structure update that costs O(edges) instead of the L N scan of dagl_ce_graph_*: every query row looks only at the keys in a
 * (2 radius + 1)^2 window around each of its previous neighbours, scores them exactly, applies the selection rule to them and a new
 * CSR comes out -- what dagl_graph_attend / dagl_graph_forward / dagl_graph_apply take.  The input structure follows dagl_graph_attend's
 * rules: keys in any order, repeats, keys outside [0, N) and empty rows are all allowed.
 *   candidates of row r = b L + i: the SET of keys (y + dy) W + (x + dx), (y, x) = (key_e / W, key_e % W) over the row's edges with key_e in
 *     [0, N), |dy|, |dx| <= radius, 0 <= y + dy < H, 0 <= x + dx < W (clipped at the border, not wrapped; a key outside [0, N) contributes
 *     nothing; repeated and overlapping windows give each key once; radius = 0: the row's distinct valid keys), keys of image b
 *   score S_j = <wq_rows[r], x_rows[b, j]>, the bits dagl_graph_attend gives the same pair; it depends on nothing else of the call
 *   selection: tau given -> j passes iff S_j - tau_r > 0 (fp32, formed as dagl_graph_attend forms its margin), tau NULL -> all pass;
 *     k > 0 -> the min(k, passing) passing candidates with the largest S, a tie at the last place to the lower key; k = 0 -> no rank cut.
 *     (adaptive: tau, k = 0; topk: NULL, k; adaptive_topk: both.)  DAGL_GRAPH_REFRESH_KEEP_ALL: every candidate is kept -- the output
 *     structure is the dilated graph, k is not looked at, edges with margin 0 weigh 0.
 *   row_off_out [B L + 1] int64, row_off_out[B L] = E;  key_out / weight_out / score_out [capacity_edges]: entries [0, E), keys strictly
 *     ascending inside a row, score = the unscaled S, weight = what dagl_graph_attend defines on the OUTPUT structure with the same tau,
 *     scale and normalisation bit (flags bit 0 = DAGL_GRAPH_ATTEND_EDGES_ONLY; default: the reference's softmax, every key off the graph
 *     counting as e^0).  Maxima fp32, sums fp64 in a fixed order, no float atomics: the same arrays give the same bits on every call.
 *   status_out [2] int64 (device): rows longer than max_row_edges -- such a row comes out EMPTY, it is never truncated --, and the largest
 *     number of distinct candidates a row had.
 * Limits: 0 <= radius <= 8; max_row_edges (2 radius + 1)^2 <= dagl_graph_refresh_max_candidates() (a compile-time constant >= 2048: 64-key
 * lists at radius 2), else DAGL_ERR_UNSUPPORTED; total_edges (2 radius + 1)^2 < 2^31; capacity_edges >= what the call may produce --
 * total_edges (2 radius + 1)^2, or B L k when k > 0 (without KEEP_ALL) and that is smaller --, else DAGL_ERR_WORKSPACE.  Workspace:
 * dagl_graph_refresh_workspace_bytes = the [B L] degrees + three staging arrays of total_edges (2 radius + 1)^2 entries (row r stages at
 * row_off[r] (2 radius + 1)^2: no scan places it).  Three launches: a block per row (a wavefront per row when max_row_edges
 * (2 radius + 1)^2 <= 128; DAGL_GRAPH_REFRESH_BLOCK_ROWS forces the block form, for measurements), the offsets' scan, an ordered copy.
 * Every argument is checked before the first launch; nothing is read on the host and the call can be captured: the CALLER reads
 * row_off_out[B L] and status_out.  total_edges = 0 gives an empty graph (key may then be NULL). */
#define DAGL_GRAPH_REFRESH_KEEP_ALL   0x2
#define DAGL_GRAPH_REFRESH_BLOCK_ROWS 0x4
int    dagl_graph_refresh_max_candidates(void);
size_t dagl_graph_refresh_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius);
int    dagl_graph_refresh(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const int64_t* row_off,
                          const int32_t* key, int64_t total_edges, int max_row_edges, int radius, const float* tau /* NULL: no margin */,
                          int k /* 0: no rank cut */, float scale, int flags, int64_t* row_off_out /* [B L + 1] */, int32_t* key_out,
                          float* weight_out, float* score_out, int64_t capacity_edges,
                          int64_t* status_out /* [2]: rows longer than max_row_edges, largest candidate count met */, void* workspace,
                          size_t ws_bytes);

/* ---- a sequence step: the refresh and the block's output on its result in one call: csrc/graph_refresh.hip (detected by symbol) -------
 * dagl_graph_refresh's operands, limits, flags and outputs, plus the zero-bordered value map b2p [B,H+6,W+6,16] (16-byte aligned, as
 * dagl_graph_forward takes it) and out [B,16,H,W].  The graph outputs are, bit for bit, what dagl_graph_refresh writes for the same
 * arguments.  With weight' / key' the kept entries of row r of that result and V the 7x7 patches of the value map,
 *   agg[r] = sum_c weight'_c V[key'_c],   out = fold(agg) / cnt   (fold and overlap count are dagl_graph_apply's)
 * each element of agg[r] one fp32 fmaf chain over the kept entries in ascending key order, whichever form of the row kernel runs (a
 * wavefront or a block per row): no float atomics, the same arrays give the same bits on every call, with or without the graph outputs.
 * A row with nothing kept -- an empty input row, every candidate failing tau, only keys outside [0, N), a row longer than max_row_edges --
 * is a row of ZEROS of agg; a row longer than max_row_edges is counted in status_out[0] and never truncated.  total_edges = 0: out is
 * all zeros.
 *   row_off_out, key_out, weight_out, score_out ALL NULL: the output alone -- no degrees, no staging, no scan, no copy; capacity_edges is
 *     not looked at; the two status words are still written.  Some of them NULL (but for key_out / weight_out / score_out at
 *     total_edges = 0) is DAGL_ERR_INVALID.
 *   status_out [2] int64 (device), as dagl_graph_refresh.
 * Workspace: dagl_graph_step_workspace_bytes = the [B L, 784] aggregated rows + (want_graph) dagl_graph_refresh's regions.  Launches: the
 * row kernel with its aggregation epilogue, (graph outputs) the offsets' scan and the ordered copy, the fold.  Every argument is checked
 * before the first launch; nothing is read on the host and the call can be captured: the CALLER reads row_off_out[B L] and status_out. */
size_t dagl_graph_step_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius, int want_graph);
int    dagl_graph_step(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                       const int64_t* row_off, const int32_t* key, int64_t total_edges, int max_row_edges, int radius,
                       const float* tau /* NULL: no margin */, int k /* 0: no rank cut */, float scale, int flags, float* out,
                       int64_t* row_off_out /* [B L + 1] or NULL */, int32_t* key_out, float* weight_out, float* score_out,
                       int64_t capacity_edges, int64_t* status_out /* [2] */, void* workspace, size_t ws_bytes);

/* ---- the search step on a patch graph: csrc/graph_refresh.hip (detected by symbol) ----------------------------------------------------
 * dagl_graph_search / dagl_graph_search_step: dagl_graph_refresh / dagl_graph_step with two more candidate sources, so that a graph can
 * improve from call to call, recover neighbours that moved farther than radius, and be built from any start without an L N scan.  The
 * arguments of the plain entry, then propagate, explore, seed.  With Lh x Lw = ceil(H / 4) x ceil(W / 4) the query grid, wd = 2 radius + 1
 * and row r = b L + qy Lw + qx, the candidates of r are the SET union of
 *   (a) own:        as dagl_graph_refresh -- the wd^2 window, clipped at the map border, around every edge of r with key in [0, N);
 *   (b) propagate:  for (dqy, dqx) in {(0,-1), (0,+1), (-1,0), (+1,0)} with (qy + dqy, qx + dqx) inside the query grid of the SAME image
 *                   (never across a grid-row end or an image boundary) and every edge of that row with key (y, x) in [0, N): the wd^2
 *                   window around (y - 4 dqy, x - 4 dqx), clipped cell by cell (the centre may lie off the map).  The adjacent rows are
 *                   read from the INPUT graph (Jacobi): the result does not depend on scheduling;
 *   (c) explore=m:  m keys of image b, key_t = ((uint64) h_t N) >> 32, h_t = lowbias32(lowbias32((uint32) r ^ seed) + t), t = 0 .. m - 1,
 *                   lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 (uint32).  No window.
 * Scores, selection, weights, the aggregation and the output layout are the plain entries': a pair's score has the same bits.  A row is
 * processed when it has any raw candidate, also with no edge of its own.  It comes out EMPTY, never truncated, when its own degree or an
 * adjacent row's (propagate) exceeds max_row_edges -- counted once in status_out[0].  status_out[1]: the largest distinct count.
 * Limits, beyond the plain entries': propagate 0 or 1 and 0 <= explore <= 256, else DAGL_ERR_INVALID;
 * (1 + 4 propagate) max_row_edges wd^2 + explore <= dagl_graph_refresh_max_candidates(), else DAGL_ERR_UNSUPPORTED; capacity_edges >=
 * (1 + 4 propagate) total_edges wd^2 + explore B L, or B L k when k > 0 (without KEEP_ALL) and that is smaller, else DAGL_ERR_WORKSPACE.
 * With explore > 0 an input of total_edges = 0 is populated (key may be NULL, the outputs may not).  Workspace:
 * dagl_graph_search_workspace_bytes (k: 0 with KEEP_ALL; aggregate: the step; want_graph: the step's graph outputs) -- the staging
 * arrays hold B L k entries under a rank cut (row r at r k), else the bound above (row r at the prefix sum of its rows' bounds, formed
 * from row_off in the kernel: no scan, no host read).  A wavefront per row when the row bound is <= 128.  propagate = explore = 0: the
 * plain entry's launches, workspace and bits.  Nothing is read on the host; the same arrays and seed give the same bits on every call. */
size_t dagl_graph_search_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius, int propagate, int explore, int k,
                                         int want_graph, int aggregate);
int    dagl_graph_search(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const int64_t* row_off,
                         const int32_t* key, int64_t total_edges, int max_row_edges, int radius, const float* tau, int k, float scale,
                         int flags, int64_t* row_off_out, int32_t* key_out, float* weight_out, float* score_out, int64_t capacity_edges,
                         int64_t* status_out, void* workspace, size_t ws_bytes, int propagate, int explore, uint32_t seed);
int    dagl_graph_search_step(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                              const int64_t* row_off, const int32_t* key, int64_t total_edges, int max_row_edges, int radius,
                              const float* tau, int k, float scale, int flags, float* out, int64_t* row_off_out, int32_t* key_out,
                              float* weight_out, float* score_out, int64_t capacity_edges, int64_t* status_out, void* workspace,
                              size_t ws_bytes, int propagate, int explore, uint32_t seed);

/* ---- the step on a fixed-width patch graph: csrc/graph_refresh.hip (detected by symbol, no ABI bump) -----------------------------------
 * dagl_graph_step_fixed: dagl_graph_step (b2p / out given), dagl_graph_refresh (both NULL) and, with propagate / explore set, their
 * search forms, on a graph held as `width` slots per row instead of a CSR -- so that the graph output has a size known before the call,
 * nothing is read on the host and the call can be captured into a HIP graph WITH its graph output.
 *   input   key_in [B L, width_in] int32, deg_in [B L] int32: row r holds its edges in slots 0 .. deg_in[r] - 1 (deg_in is read clamped
 *           to [0, width_in]; slots behind the degree are never read; keys as in the CSR entries: any order, repeats count once, keys
 *           outside [0, N) contribute nothing).
 *   output  key_out / weight_out / score_out [B L, width_out], deg_out [B L]: the kept entries of row r in ascending key order in slots
 *           0 .. deg_out[r] - 1, then key -1, weight 0, score 0 up to width_out.  EVERY slot and degree is written by every call: the
 *           arrays need no clearing.  out [B,16,H,W] as dagl_graph_step's.
 * Candidates, scores, selection, weights and the aggregation are the CSR entries': for the same rows the kept (key, score, weight) and
 * out carry the same bits as dagl_graph_refresh / _step / _search / _search_step give with max_row_edges = width_in.  A row that keeps
 * more than width_out entries comes out EMPTY (degree 0, filler, zeros to out), never truncated, and is counted in status[0] -- possible
 * only without a rank cut (k = 0) or with DAGL_GRAPH_REFRESH_KEEP_ALL.  status[1]: the largest number of distinct candidates of a row.
 * One row launch (a wavefront per row when (1 + 4 propagate) width_in (2 radius + 1)^2 + explore <= 128, else a block per row), then
 * the fold when out is wanted: no staging, no scan, no copy.  flags: DAGL_GRAPH_ATTEND_EDGES_ONLY, DAGL_GRAPH_REFRESH_KEEP_ALL,
 * DAGL_GRAPH_REFRESH_BLOCK_ROWS.  Refused before any launch: the shape and operand checks of dagl_graph_step; width_in or width_out < 1;
 * B L width >= 2^31; propagate not 0 / 1, explore outside 0..256; exactly one of b2p and out NULL; k > 0 without KEEP_ALL and
 * width_out < min(k, N); an output array that overlaps an input array (DAGL_ERR_INVALID); that row bound above
 * dagl_graph_refresh_max_candidates() (DAGL_ERR_UNSUPPORTED); too small a workspace (DAGL_ERR_WORKSPACE).  Workspace:
 * dagl_graph_step_fixed_workspace_bytes -- the [B L, 784] aggregated rows when out is wanted, else 0 (workspace may then be NULL). */
size_t dagl_graph_step_fixed_workspace_bytes(int B, int H, int W, int want_out);
int    dagl_graph_step_fixed(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows,
                             const float* b2p /* NULL: the refresh alone */, const int32_t* key_in, const int32_t* deg_in, int width_in,
                             int radius, const float* tau, int k, float scale, int flags, int propagate, int explore, uint32_t seed,
                             float* out /* NULL iff b2p NULL */, int32_t* key_out, float* weight_out, float* score_out, int32_t* deg_out,
                             int width_out, int64_t* status /* [2] */, void* workspace, size_t workspace_bytes);

/* ---- the sequence step of a whole CES stage: csrc/graph_refresh.hip, csrc/aggregate.hip (detected by symbol) ---------------------------
 * dagl_ces_stage_fold_mix: the end of a stage from its four heads' aggregated rows, in one launch:
 *     out = conv1x1(cat_h(fold(agg_h) / cnt)) + mix_b + x
 *   agg [4, B, L, 784] head-major (head h, image b, query i at ((h B + b) L + i) 784), element order (kh, kw, c), 16-byte aligned;
 *   x, out [B,64,H,W];  mix_w [64,64] (output, concat channel: the stage's 1x1 convolution),  mix_b [64].
 *   Per pixel the <= 2 x 2 covering windows of each head are added in the order of dagl_fold_normalize and divided by the window count
 *   (the 64 concat values are dagl_fold_normalize's bits; the [B,64,H,W] concat map is never stored), then the 64 x 64 product on the
 *   fp32 matrix cores, the bias, the residual.  No float atomics: the same arrays give the same bits on every call.
 * dagl_graph_stage_step: dagl_graph_step for the four heads of a stage that share the input, and that end on its result.
 *   wq_rows4, x_rows4, b2p4, tau4: HOST tables of four device pointers, entry h = head h's wq_rows [B L, 196], x_rows [B N, 196],
 *     b2p [B,H+6,W+6,16] and tau [B L] as dagl_graph_step takes them for B images; tau4 NULL or four NULL entries: no margin; some entries
 *     NULL is DAGL_ERR_INVALID.  No feature is copied or stacked.
 *   row_off [4 B L + 1], key [total_edges]: ONE CSR over the head-major rows, row (h B + b) L + i = query i of image b under head h.
 *   max_row_edges, radius, k, scale, flags: as dagl_graph_step, the same for the four heads.
 *   out [B,64,H,W] = dagl_ces_stage_fold_mix of the four heads' aggregated rows, each row dagl_graph_step's bits for its head.
 *   row_off_out [4 B L + 1], key_out / weight_out / score_out [capacity_edges], or ALL NULL (the output alone): rows h B L .. (h + 1) B L
 *     hold, bit for bit, what dagl_graph_step writes for head h's operands and its slice of the input graph, the offsets continuing
 *     from head to head (row_off_out[r] - row_off_out[h B L] are that call's offsets).  capacity_edges >= total_edges (2 radius + 1)^2,
 *     or 4 B L k when k > 0 (without KEEP_ALL) and that is smaller.
 *   status_out [2] int64 (device): the rows longer than max_row_edges summed over the heads (each comes out empty, never truncated), the
 *     largest number of distinct candidates over all rows.
 * Limits, refusals and error codes are dagl_graph_step's with 4 B in the place of B.  total_edges = 0: out = mix_b + x.  Workspace:
 * dagl_graph_stage_step_workspace_bytes = the [4 B L, 784] aggregated rows + (want_graph) dagl_graph_refresh's regions over 4 B L rows.
 * Launches: the row kernel once per head on its slice of the offsets (a row stages at the absolute row_off[r] (2 radius + 1)^2), (graph
 * outputs) one scan and one ordered copy over all rows, the fold + mix.  Every argument is checked before the first launch; nothing is
 * read on the host and the call can be captured: the CALLER reads row_off_out[4 B L] and status_out. */
int    dagl_ces_stage_fold_mix(void* stream, int B, int H, int W, const float* agg, const float* x, const float* mix_w,
                               const float* mix_b, float* out);
/* The launch it saves, on its own (for measurements): out = conv1x1(cat) + mix_b + x on a STORED concat map cat [B,64,H,W] -- the end of
 * dagl_ces_stage_forward; dagl_fold_normalize on the [4 B] heads' rows writes such a map when B = 1.  B <= 65535. */
int    dagl_ces_stage_mix(void* stream, int B, int H, int W, const float* cat, const float* x, const float* mix_w, const float* mix_b,
                          float* out);
size_t dagl_graph_stage_step_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius, int want_graph);
int    dagl_graph_stage_step(void* stream, int B, int H, int W, const float* const* wq_rows4, const float* const* x_rows4,
                             const float* const* b2p4, const int64_t* row_off, const int32_t* key, int64_t total_edges, int max_row_edges,
                             int radius, const float* const* tau4 /* NULL: no margin */, int k /* 0: no rank cut */, float scale, int flags,
                             const float* x, const float* mix_w, const float* mix_b, float* out,
                             int64_t* row_off_out /* [4 B L + 1] or NULL */, int32_t* key_out, float* weight_out, float* score_out,
                             int64_t capacity_edges, int64_t* status_out /* [2] */, void* workspace, size_t ws_bytes);

/* ---- the fixed-width step of a whole CES stage: csrc/graph_refresh.hip (detected by symbol, no ABI bump) ---------------------------------
 * dagl_graph_stage_step_fixed: dagl_graph_step_fixed for the four heads of a stage in ONE row launch, ending in dagl_ces_stage_fold_mix --
 * the stage-fused step that hands back its graph at a size known before the call: nothing is read on the host and the call can be
 * captured into a HIP graph WITH its graph output.
 *   wq_rows4, x_rows4, b2p4, tau4: HOST tables of four device pointers as dagl_graph_stage_step takes them (tau4 NULL or four NULL
 *     entries: no margin; some entries NULL is DAGL_ERR_INVALID).
 *   key_in [4 B L, width_in], deg_in [4 B L]: the stage's graph over the head-major rows, row (h B + b) L + i = query i of image b under
 *     head h, slots and degrees as dagl_graph_step_fixed reads them (deg_in clamped to [0, width_in]).
 *   key_out / weight_out / score_out [4 B L, width_out], deg_out [4 B L]: rows h B L .. (h + 1) B L hold, bit for bit and filler included,
 *     what dagl_graph_step_fixed writes for head h's operands, its rows of the input and the same radius, k, scale, flags, propagate,
 *     explore and seed.  EVERY slot and degree is written by every call.  The random keys of a row come from the hash of the HEAD-LOCAL
 *     row; propagation reads rows r +- 1 and r +- Lw of the input inside the row's own image, so never another head's.
 *   b2p4, x, mix_w, mix_b, out [B,64,H,W]: all given -- out = dagl_ces_stage_fold_mix of the four heads' aggregated rows, each row
 *     dagl_graph_step_fixed's bits for its head -- or ALL NULL: the graph alone (the graph-only iterations of a search).
 *   status [2] int64 (device): the rows that came out empty for their length summed over the heads, the largest number of distinct
 *     candidates over all rows.
 * Launches: the status words' memset, ONE row kernel over the 4 B L rows (the heads' pointers travel by value in its arguments; a
 * wavefront per row when (1 + 4 propagate) width_in (2 radius + 1)^2 + explore <= 128 and DAGL_GRAPH_REFRESH_BLOCK_ROWS is not set, else
 * a block per row), then the fold + mix + residual when out is wanted: no staging, no scan, no copy.  Refused before any launch: what
 * dagl_graph_step_fixed refuses with 4 B L rows (4 B H W >= 2^30, 4 B L width >= 2^31), a NULL table, b2p4 / x / mix_w / mix_b / out
 * given in part, tau for some heads, a b2p4 entry that is not 16-byte aligned, an output array that overlaps an input array of any head
 * or a mix operand (DAGL_ERR_INVALID); the row bound above dagl_graph_refresh_max_candidates() (DAGL_ERR_UNSUPPORTED); too small a
 * workspace (DAGL_ERR_WORKSPACE).  Workspace: dagl_graph_stage_step_fixed_workspace_bytes -- the [4 B L, 784] aggregated rows when out
 * is wanted, else 0 (workspace may then be NULL). */
size_t dagl_graph_stage_step_fixed_workspace_bytes(int B, int H, int W, int want_out);
int    dagl_graph_stage_step_fixed(void* stream, int B, int H, int W, const float* const* wq_rows4, const float* const* x_rows4,
                                   const float* const* b2p4 /* NULL: the graph alone */, const int32_t* key_in, const int32_t* deg_in,
                                   int width_in, int radius, const float* const* tau4 /* NULL: no margin */, int k, float scale, int flags,
                                   int propagate, int explore, uint32_t seed, const float* x, const float* mix_w, const float* mix_b,
                                   float* out /* NULL iff b2p4 NULL */, int32_t* key_out, float* weight_out, float* score_out,
                                   int32_t* deg_out, int width_out, int64_t* status /* [2] */, void* workspace, size_t workspace_bytes);

/* ---- the features of a whole CES stage for the patch-graph routes: csrc/stage_features.hip (detected by symbol, no ABI bump) -------------
 * dagl_graph_stage_features16: what the stage entries above read -- dense feature rows, value maps, tau -- for `heads` (1..4) heads that
 * share the input x, by the inference forward's heads-as-batch kernels: the g / theta maps of all heads in ONE launch, their keys and
 * queries in ONE split-fp16 projection launch, ONE copy-out launch.
 *   x [B,64,H,W] fp32, shared by the heads; heads_w [heads]: HOST array of the heads' device pointers (thr_* / bias_* are looked at with
 *     margin != 0 only).
 *   wq_rows [heads,B,L,196], x_rows [heads,B,N,196]: fc1 / fc2 + ReLU of the 7x7x16 patches of g(x), rows post-ReLU; head h's slice is a
 *     contiguous [B,n,196] array, as dagl_graph_stage_step* take it.
 *   b2p [heads,B,H+6,W+6,16]: theta(x), NHWC, with a zero 3-pixel border (every element is written by every call).
 *   tau [heads,B,L] with margin != 0 (else NULL): mean_j S_ij * thr_i - bias_i, the mean as an fp64 dot of the query row with the fp64
 *     column sums of its image's keys, thr / bias from the four channel-group partial sums in the order of the forward's kernel.
 * Range: the planes carry both tiers of g(x) and the input its per-block scale, as in dagl_ces_stage_forward, so activations are served
 * up to |g(x)| < 1.5e7; weights beyond the split's range (|256 w_conv|, |1024 w_fc| < 65504) or a non-finite input set the call's range
 * word, and the copy-out then writes NaN into EVERY element of the four outputs (b2p[0] of every head with them): one word per call,
 * the whole stage, never numbers computed from inf halves.
 * Launches: two memsets (the call's words, the column sums), three weight packs per head, the border and guard-row zeroing, the conv
 * launch, the thr / bias heads (margin != 0 only; inside the projection's launch when W % 4 == 0 and x is 16-byte aligned), the
 * projection (+ its column-sum reduce with margin != 0), the copy-out.  Nothing is allocated and nothing is read on the host: the call
 * can be captured into a HIP graph.
 * Refused before any launch, in this order: B, H or W < 1, heads outside 1..4, heads B H W >= 2^30; a NULL array or a NULL weight of
 * head h; tau without margin or margin without tau; an array that is not 16-byte aligned (DAGL_ERR_INVALID); a workspace that is NULL or
 * not 256-byte aligned (DAGL_ERR_INVALID) or smaller than dagl_graph_stage_features16_workspace_bytes (DAGL_ERR_WORKSPACE, the size
 * named).  The size function returns 0 for a shape the entry refuses. */
size_t dagl_graph_stage_features16_workspace_bytes(int heads, int B, int H, int W, int margin);
int    dagl_graph_stage_features16(void* stream, int heads, int B, int H, int W, const float* x /* [B,64,H,W], shared by the heads */,
                                   const dagl_ce_weights* heads_w /* [heads] */, int margin, float* wq_rows /* [heads,B,L,196] */,
                                   float* x_rows /* [heads,B,N,196] */, float* b2p /* [heads,B,H+6,W+6,16] */,
                                   float* tau /* [heads,B,L] or NULL with margin = 0 */, void* workspace, size_t workspace_bytes);

/* ---- the search step of a whole CES stage: csrc/graph_refresh.hip (detected by symbol) ---------------------------------------------------
 * dagl_graph_stage_search / dagl_graph_stage_search_step: dagl_graph_search / dagl_graph_search_step for the four heads of a stage, on
 * the operands of dagl_graph_stage_step (HOST tables of four device pointers, ONE CSR over the 4 B L head-major rows, x, mix_w, mix_b,
 * out [B,64,H,W]) plus propagate, explore, seed.  Rows h B L .. (h + 1) B L of the graph outputs hold, bit for bit, what
 * dagl_graph_search / dagl_graph_search_step write when called with head h's operands, its slice of the input graph with rebased
 * offsets and the same propagate, explore and seed; the offsets continue from head to head.  out = dagl_ces_stage_fold_mix of the four
 * heads' aggregated rows, each row dagl_graph_search_step's bits -- the same with or without the graph outputs, in the wavefront and the
 * block form, and on every call.  Two consequences:
 *   - the random keys of row (h B + b) L + i come from the hash of the HEAD-LOCAL row r = b L + i of (c) above, not of the CSR row: the
 *     four heads explore the same keys, as they do head by head with one seed;
 *   - propagation never crosses an image, so it never crosses a head: the 4 B images of the CSR are images to rule (b).
 * status_out[0] is the sum over the heads, status_out[1] the maximum.  Limits, error codes and the capacity rule are
 * dagl_graph_search's with 4 B in the place of B (capacity_edges >= (1 + 4 propagate) total_edges wd^2 + 4 B L explore, or 4 B L k).
 * total_edges = 0 with explore > 0 populates the graph; with explore = 0 it gives an empty graph and out = mix_b + x.  propagate =
 * explore = 0 is allowed: the plain entries' bits per head.  tau4 as dagl_graph_stage_step (all or none).  The step's four graph outputs
 * may ALL be NULL (the output alone).  Workspace: dagl_graph_stage_search_workspace_bytes (k: 0 with KEEP_ALL) -- the staging arrays
 * hold 4 B L k entries under a rank cut (row r at r k), else (1 + 4 propagate) total_edges wd^2 + 4 B L explore, row r at the prefix sum
 * of the rows' bounds over the WHOLE CSR (a head's rows can need 5 E_h wd^2 entries: no per-head slice of the array holds them).
 * Launches: ONE row kernel over the 4 B L rows (the heads' pointers travel by value in its arguments; a wavefront per row when the row
 * bound is <= 128), (graph outputs) one scan and one ordered copy, (step) the fold + mix.  DAGL_GRAPH_STAGE_SEARCH_HEAD_LAUNCHES runs
 * that row kernel once per head instead, for measurements: the same bits.  Every argument is checked before the first launch; nothing is
 * read on the host, so a call without graph outputs can be captured: the CALLER reads row_off_out[4 B L] and status_out. */
#define DAGL_GRAPH_STAGE_SEARCH_HEAD_LAUNCHES 0x8
size_t dagl_graph_stage_search_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius, int propagate, int explore, int k,
                                               int want_graph, int aggregate);
int    dagl_graph_stage_search(void* stream, int B, int H, int W, const float* const* wq_rows4, const float* const* x_rows4,
                               const int64_t* row_off, const int32_t* key, int64_t total_edges, int max_row_edges, int radius,
                               const float* const* tau4 /* NULL: no margin */, int k /* 0: no rank cut */, float scale, int flags,
                               int64_t* row_off_out /* [4 B L + 1] */, int32_t* key_out, float* weight_out, float* score_out,
                               int64_t capacity_edges, int64_t* status_out /* [2] */, void* workspace, size_t ws_bytes, int propagate,
                               int explore, uint32_t seed);
int    dagl_graph_stage_search_step(void* stream, int B, int H, int W, const float* const* wq_rows4, const float* const* x_rows4,
                                    const float* const* b2p4, const int64_t* row_off, const int32_t* key, int64_t total_edges,
                                    int max_row_edges, int radius, const float* const* tau4 /* NULL: no margin */,
                                    int k /* 0: no rank cut */, float scale, int flags, const float* x, const float* mix_w,
                                    const float* mix_b, float* out, int64_t* row_off_out /* [4 B L + 1] or NULL */, int32_t* key_out,
                                    float* weight_out, float* score_out, int64_t capacity_edges, int64_t* status_out /* [2] */,
                                    void* workspace, size_t ws_bytes, int propagate, int explore, uint32_t seed);

/* ---- stage profile: hipEvents recorded at the stage boundaries on the caller's stream ---------
 * The benchmark times its steps with these (no synchronisation is added to the timed region;
 * dagl_profile_read waits for the recorded events afterwards).  Stage order:                     */
#define DAGL_N_STAGES        8
#define DAGL_STAGE_LAYOUT    0   /* pad/NHWC maps + fc weight pack                                  */
#define DAGL_STAGE_PROJECT   1   /* fc2 projection of the N key patches (+ column sums) and fc1
                                    projection of the L query patches: one launch                  */
#define DAGL_STAGE_THRESH    2   /* per-query adaptive thresholds                                   */
#define DAGL_STAGE_SAMPLE    3   /* top-k screen: sampled group maxima -> per-query threshold       */
#define DAGL_STAGE_SELECT    4   /* the full L*N scan: bf16 screen filter, or the fp32 select       */
#define DAGL_STAGE_EDGE      5   /* refine / candidate merge / degree scan + edge softmax           */
#define DAGL_STAGE_GATHER    6   /* neighbour gather + weighted sum                                 */
#define DAGL_STAGE_FOLD      7   /* fold + overlap normalisation                                    */
int dagl_profile_create(int max_calls, dagl_profile** out);
int dagl_profile_destroy(dagl_profile* prof);
int dagl_profile_reset(dagl_profile* prof);
/* stage >= 0: record only the two events around that stage (the others read back as 0 ms); -1 = all boundaries.
 * Also resets the recorded calls. */
int dagl_profile_select_stage(dagl_profile* prof, int stage);
/* stage_ms [capacity_calls][DAGL_N_STAGES] (host memory, may be NULL to query n_calls only) */
int dagl_profile_read(dagl_profile* prof, int* n_calls, float* stage_ms, int capacity_calls);
int dagl_ce_forward_profiled(void* stream, int B, int H, int W,
                             const float* b1, const float* b2, const float* thr, const float* bias,
                             const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                             int mode, int k, float* out,
                             void* workspace, size_t ws_bytes, dagl_ce_info* info, dagl_profile* prof);

/* ---- training: graph core with the features given, and its backward ---------------------------
 * Replaces what autograd records for dagl.py:250-272 (score matrix, adaptive mask, non-renormalised softmax,
 * aggregation, fold) when the block is trained (DN_Gray/trainer.py:44-50 loss.backward()).  The host computes
 * the projections itself (under its own autograd: wq_rows = relu(fc1(unfold4(b1))) [B,L,196],
 * x_rows = relu(fc2(unfold1(b1))) [B,N,196], dagl.py:240-249) and gets back the fixed-width neighbour lists
 * (width = dagl_ce_list_width(mode,k)) the backward needs.  Sparse neighbourhoods only: an adaptive mask that
 * keeps more than DAGL_FAST_CAP keys for some query returns DAGL_ERR_UNSUPPORTED.
 * Workspace of the forward: dagl_ce_workspace_bytes(B,H,W,mode,k).                                          */
int    dagl_ce_list_width(int mode, int k);
int    dagl_ce_core_forward(void* stream, int B, int H, int W,
                            const float* wq_rows, const float* x_rows, const float* b2 /* [B,16,H,W] */,
                            const float* thr, const float* bias /* [B,L], NULL in top-k mode */,
                            int mode, int k, float* out /* [B,16,H,W] */,
                            int32_t* nb_idx, float* nb_wgt, float* nb_s /* [B,L,width] each */,
                            int32_t* nb_cnt /* [B,L] */, float* mu /* [B,L] row means, adaptive modes */,
                            void* workspace, size_t ws_bytes, dagl_ce_info* info);
size_t dagl_ce_core_backward_workspace_bytes(int B, int H, int W, int mode, int k);
/* Gradients of a scalar loss w.r.t. wq_rows, x_rows, b2, thr, bias given d_out = dL/d out.  d_x_rows and d_b2
 * are gathered over the edge list sorted by key (stable radix sort: bit-reproducible); d_thr / d_bias may be NULL
 * in top-k mode.  The selection itself (which keys are neighbours) carries no gradient, as in the reference.  */
int    dagl_ce_core_backward(void* stream, int B, int H, int W, int mode, int k,
                             const float* wq_rows, const float* x_rows, const float* b2,
                             const float* thr, const float* bias,
                             const int32_t* nb_idx, const float* nb_wgt, const float* nb_s, const int32_t* nb_cnt,
                             const float* mu, const float* d_out,
                             float* d_wq_rows, float* d_x_rows, float* d_b2, float* d_thr, float* d_bias,
                             void* workspace, size_t ws_bytes);

/* Dense neighbourhoods under autograd (an adaptive mask that keeps more than DAGL_FAST_CAP keys for some query -- the
 * regime of default-initialised thr/bias heads, i.e. where a training run starts): the reference's dense formulation
 * (dagl.py:250-264) and the gradients autograd derives from it, chunked over the queries so that the [L,N] matrices
 * exist one chunk at a time; matrix products on the fp32 matrix cores (bitwise fmaf chains) or, by default in the backward, on
 * the fp16 ones with split operands.  Adaptive mode only
 * (the top-k modes always have fixed-width lists).  Same operands as dagl_ce_core_forward / _backward; instead of
 * neighbour lists the forward hands back `lse` [B,L,2] = (softmax shift, denominator) per query and `mu` [B,L].
 * info (may be NULL; non-NULL costs one host synchronisation): path 5, total_edges, max_degree.
 * flags: DAGL_FLAG_EXACT_SCAN = the chunked fp32 GEMM form whatever the size (no split-fp16 range limit); 0 = the
 * streamed split-fp16 kernel for images of >= 2048 keys (|feature| < 937; beyond it `out` is NaN-filled, and a call
 * with info != NULL re-runs itself in the GEMM form and sets info->range_fallback).                              */
size_t dagl_ce_core_dense_workspace_bytes(int B, int H, int W, int backward);
int    dagl_ce_core_dense_forward(void* stream, int B, int H, int W, int flags /* 0 or DAGL_FLAG_EXACT_SCAN */,
                                  const float* wq_rows, const float* x_rows, const float* b2,
                                  const float* thr, const float* bias, float* out, float* lse, float* mu,
                                  void* workspace, size_t ws_bytes, dagl_ce_info* info);
/* backward flags: 0 = the five matrix products of the gradients on the fp16 matrix cores with split operands (every tensor scaled
 * by a power of two from its own largest magnitude: no range limit; shapes whose [L,N] matrices fit one chunk, else fp32);
 * DAGL_FLAG_EXACT_SCAN = on the fp32 matrix cores.                                                                         */
int    dagl_ce_core_dense_backward(void* stream, int B, int H, int W, int flags,
                                   const float* wq_rows, const float* x_rows, const float* b2,
                                   const float* thr, const float* bias, const float* lse, const float* mu,
                                   const float* d_out,
                                   float* d_wq_rows, float* d_x_rows, float* d_b2, float* d_thr, float* d_bias,
                                   void* workspace, size_t ws_bytes);

/* (ABI 410) A testing and tuning hook: the chunk budget of the four entry points above and below -- how many floats one [chunk, N]
 * matrix may hold.  From it follow the queries per chunk (a multiple of 128, at least 128), the chunks per image, the images per group
 * (only when an image is one chunk) and with them the split-K factor of d Wq and whether the backward's products may run on the fp16
 * matrix cores (one chunk per image only).  dagl_ce_core_dense_chunk_floats sets it process-wide (0 or less restores the built-in 128 Mi floats
 * = 512 MiB) and returns the value previously in force; it is a relaxed atomic that every call reads once, so a call in flight on another
 * thread runs wholly under the old or wholly under the new value.  dagl_ce_core_dense_workspace_bytes follows the budget: a workspace
 * sized under one budget and offered under a larger one is refused with DAGL_ERR_WORKSPACE before anything is launched.
 * dagl_ce_core_dense_plan reports the launch plan the budget in force gives [B, H, W] (host only, no device access):
 * out = { queries per chunk, chunks per image, images per group, split-K factor of d Wq, K extent of the key-major operand copies
 * (N rounded up to 32 x that factor), 1 if the backward's products may run on the fp16 matrix cores else 0 }.                        */
long long dagl_ce_core_dense_chunk_floats(long long floats);
int       dagl_ce_core_dense_plan(int B, int H, int W, int backward, int32_t out[6]);

/* The top-k modes with min(k, N) > DAGL_MAX_TOPK under autograd (the fixed-k variant takes any num_edge: top_k = min(num_edge, N),
 * GReccR2b_3mh_1-checkpoint.py:242-250; CA_model-checkpoint.py:134-143 uses 500): no lists -- the dense formulation above with
 * the row-wise selection as its mask: per query the k best scores (ties at the k-th place to the lower key index, as everywhere),
 * DAGL_MODE_TOPK: logits 10 S on them, a 0/1 mask (thr / bias and their gradients may be NULL); DAGL_MODE_ADAPTIVE_TOPK: the k best of
 * the keys that pass the adaptive test, m = relu(S - mean thr + bias).  Matrix products on the fp32 matrix cores (the backward
 * re-selects from the recomputed scores, which are the forward's bit for bit).  Workspace: dagl_ce_core_dense_workspace_bytes.
 * info (may be NULL; non-NULL costs one host synchronisation): path 5, total_edges, max_degree.                                    */
int    dagl_ce_core_wide_forward(void* stream, int B, int H, int W, int mode, int k,
                                 const float* wq_rows, const float* x_rows, const float* b2,
                                 const float* thr, const float* bias, float* out,
                                 void* workspace, size_t ws_bytes, dagl_ce_info* info);
int    dagl_ce_core_wide_backward(void* stream, int B, int H, int W, int mode, int k,
                                  const float* wq_rows, const float* x_rows, const float* b2,
                                  const float* thr, const float* bias, const float* d_out,
                                  float* d_wq_rows, float* d_x_rows, float* d_b2, float* d_thr, float* d_bias,
                                  void* workspace, size_t ws_bytes);

/* ---- stages (each callable on its own: unit parity tests and the benchmark use them) --------- */

/* Batched fp32 matrix product on the matrix cores, the building block of the dense training stages:
 * C[b] = alpha * A[b] B[b] + beta * C[b] (+ bias[n], relu).  A is logically M x K, stored row-major
 * (a_k_contiguous: element (m,k) at A[m*lda + k]) or K-major (A[k*lda + m]); B is logically K x N, stored
 * as N x K rows (b_k_contiguous: B[n*ldb + k]) or K x N rows (B[k*ldb + n]).  Replaces torch.matmul / torch.mm
 * of dagl.py:250,263 and their autograd counterparts.  chunk_tiles > 0: partial sums over chunk_tiles * 16 products
 * added in fp32 (shorter rounding chains).  scratch (batch == 1 only, may be NULL): dagl_gemm_f32_scratch_floats()
 * floats; when given, a product with few output tiles and a long K (a weight gradient) is cut into K slices that fill
 * the chip, summed in slice order.  Deterministic either way (no atomics).                                        */
size_t dagl_gemm_f32_scratch_floats(int batch, int M, int N, int K);
int dagl_gemm_f32(void* stream, int batch, int M, int N, int K,
                  const float* A, long long lda, long long stride_a, int a_k_contiguous,
                  const float* B, long long ldb, long long stride_b, int b_k_contiguous,
                  float* C, long long ldc, long long stride_c, float alpha, float beta, const float* bias, int relu,
                  int chunk_tiles, float* scratch);

/* Stages of the differentiable path besides the matrix products (train_ops.hip): a convolution / Linear over patches
 * under autograd is  unfold -> dagl_gemm_f32 (+ bias, ReLU);  d weight = d Z^T rows,  d rows = d Z weight,
 * d map = fold(d rows).  Replaces nn.Conv2d / nn.Linear / nn.Unfold of dagl.py:208-249 in the training path.
 *   unfold: rows[b, (py,px), (kh,kw,c)] = map[b, oy + py*stride + kh, ox + px*stride + kw, c]   (map [B,Hp,Wp,C], C % 4 == 0)
 *   fold:   the adjoint, written for every pixel of the [B,Hp,Wp,C] map (gather form, no atomics)
 *   copy4:  generic strided 4-D copy (layout changes NCHW <-> zero-bordered NHWC and their adjoints)             */
int dagl_unfold_patches(void* stream, int B, int Hp, int Wp, int C, int k, int stride, int oy, int ox, int oh, int ow,
                        const float* map, float* rows);
int dagl_fold_patches(void* stream, int B, int Hp, int Wp, int C, int k, int stride, int oy, int ox, int oh, int ow,
                      const float* d_rows, float* d_map);
int dagl_copy4(void* stream, int n0, int n1, int n2, int n3, const float* src, long long s0, long long s1, long long s2,
               long long s3, float* dst, long long d0, long long d1, long long d2, long long d3);
int dagl_relu_backward(void* stream, size_t n, const float* y, const float* dy, float* dz);   /* dz = dy * (y > 0)   */
/* single-parameter PReLU of the trunk's ResBlocks (DN_Gray/model/common.py:59-79, act = nn.PReLU(); DN_Gray/model/dagl.py:27-35,
 * 76-90): y = x > 0 ? x : a x; backward dx = dy (x > 0 ? 1 : a), da = sum dy x [x <= 0] with a fixed-order fp64 reduction
 * (deterministic).  n = element count, a multiple of 4; tensors contiguous and 16-byte aligned.                            */
int    dagl_prelu_forward(void* stream, size_t n, const float* x, const float* a, float* y);
size_t dagl_prelu_scratch_bytes(size_t n);
int    dagl_prelu_backward(void* stream, size_t n, const float* x, const float* dy, const float* a, float* dx, float* da, void* scratch);
size_t dagl_col_sum_scratch_bytes(size_t rows, int cols);
int dagl_col_sum(void* stream, size_t rows, int cols, const float* src, float* out, void* scratch);   /* out[c] = sum_r src[r,c], cols <= 256 */

/* The two gradient products of a patch projection (fc1 / fc2 under autograd, dagl.py:248-249) on the fp16 matrix cores with
 * split operands (gemm16s.hip) -- what dagl_unfold_patches + two dagl_gemm_f32 calls compute, at several times the rate:
 *   d_w    [196,784]   = dz^T rows            (rows = the 7x7x16 patches of map_nhwc on the grid (stride, oy, ox, oh, ow),
 *                                              element order (kh,kw,c); they are never materialised in fp32)
 *   d_rows [B*oh*ow,784] = dz w_rows          (the caller folds them back: dagl_fold_patches)
 *   d_b    [196]       = column sums of dz
 * dz = dy (y > 0) when the layer's output y is given (ReLU backward, fused with the pass that takes dz's largest magnitude
 * and its column sums), dz = dy when y is NULL; y, dy [B*oh*ow,196]; w_rows [196,784] in (kh,kw,c) order; any output may be NULL.
 * Holds for |16 map|, |1024 w| < 65504 (the forward projection's own range); dz is rescaled per call by a power of two taken
 * from its largest magnitude.  Fixed summation order (split-K slices added in slice order): bit-reproducible.             */
size_t dagl_fc_grad16_scratch_bytes(int B, int oh, int ow);
int dagl_fc_grad16(void* stream, int B, int Hp, int Wp, int stride, int oy, int ox, int oh, int ow, const float* map_nhwc,
                   const float* w_rows, const float* y, const float* dy, float* d_w, float* d_b, float* d_rows, void* scratch,
                   size_t scratch_bytes);
/* (ABI 405) The same with the gradient of the MAP as its output: d_map [B,Hp,Wp,16] = fold(d_rows) as dagl_fold_patches computes it
 * (autograd through `fc(unfold(map))`, dagl.py:240-249), the rows folded inside the product -- over kw in the block's LDS, over kh by a
 * light second kernel, every sum in a fixed order -- so that the [n, 784] fp32 rows (411 MB at n = 131 072) are neither written nor read
 * back.  Geometries: dagl_fc_grad16_dmap_ok(stride, ow) (stride 1 and 16 / 32 / 64 or a multiple of 128 patches per row); others:
 * dagl_fc_grad16 + dagl_fold_patches.                                                                                          */
int    dagl_fc_grad16_dmap_ok(int stride, int ow);
size_t dagl_fc_grad16_dmap_scratch_bytes(int B, int oh, int ow);
int dagl_fc_grad16_dmap(void* stream, int B, int Hp, int Wp, int stride, int oy, int ox, int oh, int ow, const float* map_nhwc,
                        const float* w_rows, const float* y, const float* dy, float* d_w, float* d_b, float* d_map, void* scratch,
                        size_t scratch_bytes);
/* (detected by symbol) A read-out for tests: the launch plan one call of the two entries above would run, computed on the host by the
 * functions the call itself plans with (no device access).  want_w / want_rows / want_map: which of d_w, d_rows (dagl_fc_grad16) and
 * d_map (dagl_fc_grad16_dmap) the call asks for -- at most one of the last two; all three 0 is the bias-only call.
 * out = { n = B oh ow patches, n_pad (the K extent of the weight gradient's operands), K slices of d_w, patches per slice,
 *         image rows per slice when d_w reads shifted planes of the map (0: transposed patch rows),
 *         tile rows of d_w's kernel (256 or 128; 0: no d_w), 1 if that kernel is the instantiation that reads shifted planes,
 *         tile rows of the d rows product's kernel (0: neither d_rows nor d_map), column tiles one of its blocks walks,
 *         patches per folded row segment and segments per 128-patch tile (both 0 unless want_map),
 *         1 if one pass over d z writes both of its split copies }.                                                            */
int dagl_fc_grad16_plan(int B, int Hp, int Wp, int stride, int oy, int ox, int oh, int ow, int want_w, int want_rows, int want_map,
                        int32_t out[12]);

/* Backward of the first two convolutions of the block (g 3x3 and theta 1x1, 64 -> 16: dagl.py:208-209 under loss.backward(),
 * DN_Gray/trainer.py:48-57) straight on the maps -- no patch rows (conv_grad.hip): tap-wise products on the fp32 matrix cores,
 * fixed summation order (bit-reproducible).
 *   x [B,64,H,W] (the forward's input), d_b1p / d_b2p [B,H+6,W+6,16] = gradients of the zero-bordered NHWC maps (interior read),
 *   g_w [16,64,3,3], th_w [16,64] (needed for d_x only)
 *   d_x [B,64,H,W] or NULL;  d_g_w [16,64,3,3], d_g_b [16], d_th_w [16,64], d_th_b [16]: all four or all NULL
 *   scratch: dagl_conv_pair_backward_scratch_bytes(B,H,W) bytes (parameter gradients only)
 * dagl_conv_pair_backward_supported: W a multiple of 4 and <= 256 (rows are staged whole); other shapes: unfold + dagl_gemm_f32. */
int    dagl_conv_pair_backward_supported(int B, int H, int W);
size_t dagl_conv_pair_backward_scratch_bytes(int B, int H, int W);
int    dagl_conv_pair_backward(void* stream, int B, int H, int W, const float* x, const float* d_b1p, const float* d_b2p,
                               const float* g_w, const float* th_w, float* d_x, float* d_g_w, float* d_g_b, float* d_th_w,
                               float* d_th_b, void* scratch);
/* (detected by symbol) A read-out for tests: the strips of the two launches of one call, computed on the host by the function the
 * launcher and dagl_conv_pair_backward_scratch_bytes plan with (no device access):
 * out = { rows per block and strips per image of the parameter gradients' launch, the same two of the input gradient's launch };
 * the scratch holds B * strips partial sums of (4 * 2560 + 32) floats.  -1 for a shape that is not supported or a NULL out.   */
int    dagl_conv_pair_backward_plan(int B, int H, int W, int32_t out[4]);

/* The four prologue convolutions alone (dagl.py:208-215): b1/b2 as zero-bordered NHWC maps
 * [B,H+6,W+6,16], thr/bias [B,L] (both NULL = skip the two 7x7 heads).  `scratch` = 8*B*L floats of
 * caller-owned device memory for the heads' partial sums (may be NULL without the heads): like every
 * entry point, nothing is allocated in here.                                                       */
int dagl_ce_prologue(void* stream, int B, int H, int W, const float* x,
                     const float* g_w, const float* g_b, const float* theta_w, const float* theta_b,
                     const float* thr_w, const float* thr_b, const float* bias_w, const float* bias_b,
                     float* b1_nhwc, float* b2_nhwc, float* thr, float* bias, float* scratch);

/* (ABI 405) The same with g / theta on the fp16 matrix cores (split operands: >= 21 significant bits, a third of the fp32 kernel's time):
 * the differentiable path's forward.  No range on x (per-block power-of-two input scale); |w_conv| < 234.  `scratch`: 256-byte aligned,
 * dagl_ce_prologue16_scratch_bytes(B, H, W) bytes (packed weights, per-block statistics, the heads' partial sums).                  */
size_t dagl_ce_prologue16_scratch_bytes(int B, int H, int W);
int dagl_ce_prologue16(void* stream, int B, int H, int W, const float* x,
                       const float* g_w, const float* g_b, const float* theta_w, const float* theta_b,
                       const float* thr_w, const float* thr_b, const float* bias_w, const float* bias_b,
                       float* b1_nhwc, float* b2_nhwc, float* thr, float* bias, void* scratch, size_t scratch_bytes);

/* (detected by symbol) Read-outs for tests of the split-fp16 g / theta kernel (csrc/prologue.hip, conv_pair16_kernel).
 * dagl_ce_prologue16_plan: the launch plan of one call on heads (1..4) x imgs images of [H, W], computed on the host by the function the
 * launcher and the workspace carves plan with:  out = { strips of 64 columns, row chunks, rows per block, |b1| slots per head
 * (= 4 waves x strips x chunks x imgs) }; the grid is (strips, chunks, heads * imgs).
 * dagl_ce_prologue16_debug: the inference flavour of the kernel, through the fused forward's launcher, with every output in the caller's
 * buffers.  x, g_w, g_b, theta_w, theta_b: HOST arrays of `heads` device pointers (x[h]: [imgs,64,H,W]); batch index b = h * imgs + image.
 *   tag         != 0: written to *range_word when the call leaves the split-fp16 range (else the word keeps what the caller put there)
 *   scratch     256-byte aligned, dagl_ce_prologue16_debug_scratch_bytes(heads) bytes (the heads' packed weights)
 *   b1_nhwc     [heads*imgs, H+6, W+6, 16] fp32 key / query map, or NULL;  b2_nhwc likewise (required)
 *   b1_hi/b1_lo [heads*imgs, H+6, W+6, 16] fp16 bits, 16 b1 = hi + lo;  b1_hi2 / b1_lo2: 2^-8 b1 = hi2 + lo2, both or neither
 *   amax        [heads][slots] floats: largest |b1| of every wave of every block (+inf for a non-finite value), slot
 *               ((image * chunks + chunk) * strips + strip) * 4 + wave of its head
 *   clear_a     n 32-bit words the first block zeroes (the fused forward's per-call counters), or NULL with n = 0
 * The 3-pixel borders of all maps are zeroed by the launchers the forward uses.                                                      */
int    dagl_ce_prologue16_plan(int heads, int imgs, int H, int W, int32_t out[4]);
size_t dagl_ce_prologue16_debug_scratch_bytes(int heads);
int    dagl_ce_prologue16_debug(void* stream, int heads, int imgs, int H, int W, const float* const* x, const float* const* g_w,
                                const float* const* g_b, const float* const* theta_w, const float* const* theta_b, int32_t tag,
                                void* scratch, size_t scratch_bytes, float* b1_nhwc, float* b2_nhwc, uint16_t* b1_hi, uint16_t* b1_lo,
                                uint16_t* b1_hi2, uint16_t* b1_lo2, float* amax, int32_t* range_word, uint32_t* clear_a, int n);

/* (detected by symbol) Read-outs for tests of the split-fp16 patch projection (csrc/project16.hip, project16_kernel).
 * dagl_project16_plan: the launch plan of one call on B images of [H, W], which = 1 keys, 2 queries, 3 both, for a device of `cus` compute
 * units (<= 0: the current device's, 256 without one), computed on the host by the function the launcher plans with:
 *   out = { key items (32 patches each), query items, keys in row-major order across row ends (W >= 32), query units per image (8 items
 *   each), key units per image, two-group blocks n_full, the ids among them mapped by XCD (n_full & ~15), key units of the last image cut
 *   into 14 single-tile blocks each, projection blocks n_full + 14 groups, resident blocks 2 cus, key items per row, query items per row }
 * dagl_ce_project16_debug: the inference launch of the kernel (the fused forward's launcher) on heads (1..4) x imgs images, with every
 * output in the caller's buffers; nothing is cleared or padded in here, so what the kernel does not store keeps the caller's bytes.
 * B = heads * imgs, batch index b = h * imgs + image; N = H W keys, L queries; rows = dagl_feat_rows(n), rows_h = round_up(n, 64) + 64.
 *   map_hi/map_lo [B, H+6, W+6, 16] fp16 bits, 16 a = hi + lo;  map_hi2 / map_lo2: 2^-8 a = hi2 + lo2, both or neither, and with them
 *               amax [heads][slots] (slots a multiple of 4, >= 4): a head whose largest slot s has 16 s < 60000 reads the fine pair
 *   fc1_w/fc1_b queries, fc2_w/fc2_b keys: HOST arrays of `heads` device pointers, weights [196][16][49] (Linear order), biases [196];
 *               only the sides of `which` are read, the outputs of the other side must be NULL
 *   tag         != 0: written to *range_word when the call leaves the split-fp16 range (else the word keeps what the caller put there)
 *   scratch     256-byte aligned, dagl_ce_project16_debug_scratch_bytes(heads) bytes (the heads' packed weights)
 *   x_feat      [B, rows(N), 204] fp32 key features, wq_feat [B, rows(L), 204] query features
 *   x_bf16/wq_bf16  optional [B, rows_h, 216] bf16 copies; q_tiled != 0: the query copy in the screen's fragment order
 *   x_hi/x_lo, wq_hi/wq_lo  optional split copies [B, rows_h, 216] fp16 bits, 64 v = hi + lo (a pair is both or neither)
 *   colsum      optional [B, 204] doubles with colpart [B, 2 key units, 224] floats (keys)
 *   rowsum      optional [B, N, 8] floats (keys), not written while *rowsum_policy != 0 (the word may be NULL: always written)
 *   thr_x/thr_w/bias_w + thr_part  optional ride-along blocks of the thr / bias heads: HOST arrays of `heads` device pointers
 *               (x[h]: [imgs,64,H,W], 16-byte aligned, W % 4 == 0; weights [64][7][7]) and the partials [heads][4][imgs][L][2]   */
int    dagl_project16_plan(int B, int H, int W, int which, int cus, int32_t out[12]);
size_t dagl_ce_project16_debug_scratch_bytes(int heads);
int    dagl_ce_project16_debug(void* stream, int heads, int imgs, int H, int W, int which, const uint16_t* map_hi, const uint16_t* map_lo,
                               const uint16_t* map_hi2, const uint16_t* map_lo2, const float* amax, int slots, const float* const* fc1_w,
                               const float* const* fc1_b, const float* const* fc2_w, const float* const* fc2_b, int32_t tag,
                               int32_t* range_word, void* scratch, size_t scratch_bytes, float* x_feat, float* wq_feat, uint16_t* x_bf16,
                               uint16_t* wq_bf16, int q_tiled, uint16_t* x_hi, uint16_t* x_lo, uint16_t* wq_hi, uint16_t* wq_lo,
                               double* colsum, float* colpart, float* rowsum, const int32_t* rowsum_policy, const float* const* thr_x,
                               const float* const* thr_w, const float* const* bias_w, float* thr_part);

/* NCHW [B,16,H,W] -> zero-bordered NHWC [B,H+6,W+6,16]  (patch unfold without materialising
 * patches: replaces same_padding/extract_image_patches, dagl.py:123-169, for all three uses).    */
int dagl_pad_nhwc(void* stream, int B, int H, int W, const float* src_nchw, float* dst_nhwc);

/* fc weight [196,784] in the reference's (c,kh,kw) column order -> 208*784 floats in the packed
 * layout the projection kernel streams: [49 (kh,kw)][208 outputs, rows 196.. zero][16 channels,
 * 16-byte quads XOR-swizzled for conflict-free LDS reads].                                       */
int dagl_pack_fc_weight(void* stream, const float* w, float* w_packed);

/* Patch projection = Linear(784->196)+ReLU applied to every 7x7x16 patch of the padded map
 * (dagl.py:248 for queries, :249 for keys), as an implicit GEMM.
 *   queries != 0 : stride-4 SAME grid (L rows);  0 : stride-1 grid (N = H*W rows)
 *   feat   [B, rows_alloc, 204]  rows_alloc = dagl_feat_rows(rows); columns 196..203 and the
 *          rows beyond `rows` are written as zero
 *   colsum [B,204] (keys only, may be NULL): sum over the N rows of each column (for the row
 *          mean of the score matrix, dagl.py:256)                                                */
int dagl_project_patches(void* stream, int B, int H, int W, int queries,
                         const float* map_nhwc, const float* w_packed, const float* fc_bias,
                         float* feat, double* colsum);
int dagl_feat_rows(int rows);          /* rows rounded up to the streaming tile + 1 guard tile     */

/* The same Linear(784->196)+ReLU over patches on the split-fp16 matrix cores (the inference kernels: the map is split into
 * fp16 hi / lo, the weight packed, no unfolded patch rows exist), for the FORWARD of the differentiable path:
 *   map_nhwc  zero-bordered [B,H+6,W+6,16] fp32;  w_rows [196, 49 taps, 16 c] (the patch order of dagl_unfold_patches);
 *   rows_out  [B, n, 196] dense (n = L for queries != 0, N = H*W otherwise);  scratch: 256-byte aligned device memory of
 *   dagl_project_patches16_scratch_bytes(B,H,W,queries) bytes.  Holds for |16 map| < 65504, |1024 w| < 65504.  */
size_t dagl_project_patches16_scratch_bytes(int B, int H, int W, int queries);
int dagl_project_patches16(void* stream, int B, int H, int W, int queries, const float* map_nhwc, const float* w_rows,
                           const float* fc_bias, float* rows_out, void* scratch, size_t scratch_bytes);

/* Per-query threshold pieces of the adaptive mask (dagl.py:256):
 *   mt[b,l] = mean_j S[l,j] * thr[b,l]   with mean_j S[l,j] = Wq[l,:] . (colsum/N)
 *   (bias is used as is).                                                                        */
int dagl_query_thresholds(void* stream, int B, int L, int N, const float* wq, const double* colsum,
                          const float* thr, float* mt);

/* Gather + weighted sum over fixed-width neighbour lists: the sparse form of torch.mm(yi, pi)
 * (dagl.py:263-264; the north-star's batched_index_select + weighted sum).
 *   idx [L,k] int32 (row index into values, <0 = empty slot), wgt [L,k], values [n_rows,P],
 *   out [L,P];  P must be a multiple of 4, pointers 16-byte aligned.
 * Algorithmic bytes per query: k*P*4 (rows) + k*8 (idx,wgt) + P*4 (out).                        */
int dagl_gather_aggregate(void* stream, int L, int k, int P,
                          const int32_t* idx, const float* wgt, const float* values, float* out);

/* Materialise value rows [B,N,784] (element order (kh,kw,c)) from the padded NHWC value map --
 * what Unfold does at dagl.py:224-231; only the stand-alone gather benchmark / tests need it.   */
int dagl_unfold_values(void* stream, int B, int H, int W, const float* b2_nhwc, float* rows);

/* Fold the aggregated query patches back and divide by the overlap count (dagl.py:265-272).
 *   agg [B,L,784] element order (kh,kw,c);  out [B,16,H,W]                                       */
int dagl_fold_normalize(void* stream, int B, int H, int W, const float* agg, float* out);

/* Dense score matrix S = Wq . X^T for tests (dagl.py:250): s [B,L,N].                            */
int dagl_scores_dense(void* stream, int B, int L, int N, const float* wq, const float* x, float* s);

/* (ABI 406) CE.forward for ANY patch geometry.  ksize, stride_1, stride_2 and inter_channels are constructor arguments of the
 * reference block (DN_Gray/model/dagl.py:175-176; its own builders, dagl.py:94-109, never override them, so every tuned kernel has
 * (7, 4, 1, 16) compiled in).  This entry runs the reference's dense formulation, dagl.py:207-275, with the geometry as run-time
 * arguments -- unfold + fp32 matrix-core products, one chunk of score rows (<= 256 MiB) at a time, row-wise mask / softmax, fold
 * with the reference's padding rule (dagl.py:243: the stride_2 SAME grid's left pad) -- csrc/generic.hip.  Replaces the Python
 * call self.cX_Y(x) of a CE built with non-default arguments (dagl.py:114-118).
 *   x [B,Cin,H,W] fp32 NCHW;  g_w [c,Cin,3,3], theta_w [c,Cin,1,1], thr_w / bias_w [1,Cin,ksize,ksize] (may be NULL in
 *   DAGL_MODE_TOPK), fc1_w / fc2_w [P/4, P] over Unfold's (c,kh,kw) patch order with P = ksize^2 c -- the state_dict's own
 *   layouts, nothing pre-packed;  out [B,c,H,W];  degree [B*L] int32 or NULL (neighbours per query);  Cin and c multiples of 4.
 *   softmax_scale: dagl.py:175 (10 by default), any positive value.  k: the fixed-k modes' num_edge (min(k, N) keys are kept).
 * A geometry whose F.fold block grid does not hold exactly the L query patches raises in the reference; here DAGL_ERR_INVALID.
 * Non-finite input: a query whose score row holds a NaN / inf score, or a NaN / +inf mask value, gets NaN weights for every key,
 * as the reference's softmax over all keys does (so a NaN or inf pixel makes its whole image NaN); the ReLUs keep NaN.  */
size_t dagl_ce_generic_workspace_bytes(int B, int Cin, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels);
int dagl_ce_generic_forward(void* stream, int B, int Cin, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels,
                            float softmax_scale, int mode, int k, const float* x,
                            const float* g_w, const float* g_b, const float* theta_w, const float* theta_b,
                            const float* thr_w, const float* thr_b, const float* bias_w, const float* bias_b,
                            const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                            float* out, int32_t* degree, void* workspace, size_t workspace_bytes);

/* (ABI 406) The differentiable graph core, dagl.py:250-272, for any patch geometry (autograd through a CE built with non-default
 * arguments; the convolutions and patch projections around it are dagl_unfold_patches + dagl_gemm_f32 with their adjoints):
 *   wq_rows [B,L,P/4], x_rows [B,N,P/4] the feature rows (relu(fc(patches)), dagl.py:248-249);  b2p the value map, zero-bordered NHWC
 *   [B, H+2*border, W+2*border, c] with border = dagl_ce_generic_border(ksize);  thr / bias [B,L] (NULL in DAGL_MODE_TOPK);
 *   out / d_out [B,c,H,W].  The backward recomputes S and A chunk by chunk; it writes d_wq, d_x, d_b2p (every element) and, in the
 *   adaptive modes, d_thr / d_bias.  Workspace: dagl_ce_generic_core_workspace_bytes(..., backward).                                 */
int    dagl_ce_generic_border(int ksize);
size_t dagl_ce_generic_core_workspace_bytes(int B, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels, int backward);
int dagl_ce_generic_core_forward(void* stream, int B, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels,
                                 float softmax_scale, int mode, int k, const float* wq_rows, const float* x_rows, const float* b2p,
                                 const float* thr, const float* bias, float* out, int32_t* degree, void* workspace, size_t workspace_bytes);
int dagl_ce_generic_core_backward(void* stream, int B, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels,
                                  float softmax_scale, int mode, int k, const float* wq_rows, const float* x_rows, const float* b2p,
                                  const float* thr, const float* bias, const float* d_out, float* d_wq, float* d_x, float* d_b2p,
                                  float* d_thr, float* d_bias, void* workspace, size_t workspace_bytes);

/* (ABI 407) The residual trunk's convolutions (csrc/trunk.hip): 2-D convolution, stride 1, padding ksize / 2, ksize 1 or 3,
 * dilation 1, groups 1, 1 <= Cin, Cout <= 64, fp32 NCHW contiguous at any B, H, W >= 1, on the fp32 matrix cores (exact fp32
 * products, fp32 accumulation: the stock layer's arithmetic, no range limits).  w is the layer's weight [Cout, Cin, ksize, ksize].
 * Launches are stream-ordered; nothing is read back.
 *   pack_weights: w -> the kernels' fragment layout, dagl_trunk_packed_floats(...) floats; transposed = 1 gives the layout of the
 *     input gradient (taps mirrored, channels swapped).  Callers cache it until the weight changes.
 *   conv_forward: out = conv(x) (+ bias[o]); with slope (one float): PReLU, pre_out (may be NULL) = the value before it; with
 *     residual: out = out * res_scale + residual.  bias / slope / pre_out / residual may be NULL.
 *   conv_input_grad: d_in [B,Cin,H,W] = alpha * conv_transposed(d_out); with slope: the PReLU backward from the saved pre-activation
 *     pre [B,Cin,H,W] (d_in = pre > 0 ? g : slope g) and slope_part = dagl_trunk_input_grad_blocks(B,H,W) fp64 partial sums of the
 *     slope gradient; with skip_grad: d_in += skip_grad.
 *   conv_weight_grad: d_w = alpha * sum_pix x (x) d_out, d_b (may be NULL) = alpha * column sums of d_out, per-block partials in
 *     scratch (16-byte aligned, dagl_trunk_weight_grad_scratch_bytes) added in a fixed order: the same bits on every call.  With
 *     d_slope: d_slope[0] = the fixed-order sum of n_slope_part slope partials of an earlier conv_input_grad.                 */
size_t dagl_trunk_packed_floats(int Cin, int Cout, int ksize, int transposed);
int dagl_trunk_pack_weights(void* stream, int Cin, int Cout, int ksize, int transposed, const float* w, float* packed);
int dagl_trunk_conv_forward(void* stream, int B, int Cin, int Cout, int H, int W, int ksize, const float* x, const float* packed,
                            const float* bias, const float* slope, float* pre_out, float res_scale, const float* residual, float* out);
int dagl_trunk_input_grad_blocks(int B, int H, int W);
int dagl_trunk_conv_input_grad(void* stream, int B, int Cin, int Cout, int H, int W, int ksize, const float* d_out,
                               const float* packed_t, float alpha, const float* slope, const float* pre, double* slope_part,
                               const float* skip_grad, float* d_in);
size_t dagl_trunk_weight_grad_scratch_bytes(int B, int Cin, int Cout, int H, int W, int ksize);
int dagl_trunk_conv_weight_grad(void* stream, int B, int Cin, int Cout, int H, int W, int ksize, const float* x, const float* d_out,
                                float alpha, float* d_w, float* d_b, const double* slope_part, int n_slope_part, float* d_slope,
                                void* scratch, size_t scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DAGL_CE_H */
