// Refresh of a patch graph on a new input (ABI 412, detected by symbol): the structure update that costs O(edges).  Every query row looks
// only at the keys in a (2 radius + 1)^2 window around each of its previous neighbours, scores those candidates exactly, applies the
// module's selection rule to them and leaves a new CSR -- the PatchMatch / NN-descent propagation step on the PatchGraph.  With
// Wq [B L, 196] / X [B N, 196] the fc1 / fc2 features, per row r (image b = r / L):
//   candidates   the SET of keys (y + dy) W + (x + dx), (y, x) = (key_e / W, key_e % W) over the row's edges with key_e in [0, N),
//                |dy|, |dx| <= radius, clipped at the map border (never wrapped); a key outside [0, N) contributes nothing
//   S_j          <Wq[r], X[b N + j]> by gt_edge_dot (graph_rows.h): the bits dagl_graph_attend computes for the same pair, whatever k,
//                tau, the flags or the rest of the row are
//   selection    tau given: j passes iff S_j - tau_r > 0 (gt_logit);  k > 0: the min(k, passing) passing candidates with the largest S,
//                a tie at the last place to the lower key;  DAGL_GRAPH_REFRESH_KEEP_ALL: every candidate (the dilated graph)
//   weight       dagl_graph_attend's on the OUTPUT structure: z = scale S m, M = max(max z, 0 if deg < N),
//                D = sum e^(z - M) + (N - deg) e^(-M) (DAGL_GRAPH_ATTEND_EDGES_ONLY: over the edges alone), w = on e^(z - M) / D
//
//   graph_refresh_rows_kernel     a block per row (a wavefront per row where rows are short): expand into the LDS, bitonic sort, drop the
//                                 repeats, score the distinct candidates (a candidate per 16 lanes, two in flight per group), margin,
//                                 rank counting, fp32 maximum, fp64 sum in a fixed order, then the kept (key, score, weight) in ascending
//                                 key order to the front of the row's staging region -- it starts at row_off[r] (2 radius + 1)^2, a place
//                                 known without a scan -- and the degree
//   row_scan_kernel               select.hip: int32 degrees -> int64 offsets, row_off_out[B L] = E
//   graph_refresh_compact_kernel  a wavefront per row copies its staged entries to row_off_out[r]: ordered, no atomics
//
// The route's second entry, dagl_graph_step, is the refresh AND the block's output on its result: graph_step_rows_kernel is the same row
// body (rf_row) with an epilogue -- the kept entries' weights and the offsets of their value patches stay in the LDS in ascending key
// order, and the row's sum_c weight_c V[key_c] goes to agg [B L, 784] (ga_gather_run: one fmaf chain per element, the same bits from a
// wavefront and a block); every exit of the body writes a row of zeros first, the workspace is never cleared.  launch_fold follows.
// Without graph outputs the degree, the staging, the scan and the copy are left out: nothing then depends on a count the host reads.
//
// The third entry, dagl_graph_stage_step, is that step for the four heads of a CES stage: one CSR over the 4 B L head-major rows,
// graph_step_rows_kernel launched once per head on its slice (launch_graph_stage_step), one scan, one copy, and
// launch_stage_fold_mix (aggregate.hip) in the place of the fold: out = conv1x1(cat_h(fold(agg_h) / cnt)) + mix_b + x.
//
// The search entries, dagl_graph_search / dagl_graph_search_step, are the first two with the other two candidate sources of that
// algorithm (rf_row's SEARCH flavour, kernels of their own: the instantiations above keep their arguments and their device code):
//   propagate    the windows around (y - 4 dqy, x - 4 dqx) for every edge (y, x) of the query at (qy + dqy, qx + dqx), (dqy, dqx) in
//                {(0, -1), (0, 1), (-1, 0), (1, 0)}, inside the Lh x Lw query grid of the same image -- never across a grid-row end or an
//                image boundary --, clipped cell by cell; the adjacent rows come from the INPUT graph (Jacobi: no scheduling dependence)
//   explore = m  m keys ((uint64) h_t N) >> 32, h_t = lowbias32(lowbias32(row ^ seed) + t): a counter hash, no state, no window
// so a graph can improve from step to step, recover from drift and be built from a trivial start without an L N scan.  Everything
// after the expansion is the same code, a pair's score has the same bits.  A row runs when it has any raw candidate; it comes out
// empty when its own or an adjacent row's degree exceeds max_row_edges (counted once).  A row can keep more than deg (2 radius + 1)^2
// entries now, so the flavour stages at r k under a rank cut and else at the prefix sum of the rows' bounds (rs_region_start: from
// row_off alone, no scan), and graph_search_compact_kernel copies from there.  Both sources off: the plain launches.
//
// The stage search entries, dagl_graph_stage_search / dagl_graph_stage_search_step, are the search entries for the four heads of a CES
// stage on the stage step's operands: graph_stage_search_rows_kernel runs rf_row's SEARCH flavour over all 4 B L rows in ONE launch (the
// heads' operands by value in its arguments, head = row / (B L)), the staging laid out over the whole CSR, then one scan, one
// graph_search_compact_kernel and launch_stage_fold_mix.  The random keys are hashed from the head-local row: the four heads explore
// the same keys, as four calls with one seed do.
//
// The fixed-width entry, dagl_graph_step_fixed, is the step (or, without a value map, the refresh; with propagate / explore the search
// forms) on a graph held as `width` slots per row and a degree per row: rf_row's FIXED flavour reads row r's edges at r width_in
// (deg_in[r] of them, clamped to [0, width_in]) and writes the kept entries straight to r width_out, the degree, and (-1, 0, 0) into the
// slots behind them -- every exit writes the whole row, the outputs are never cleared.  No staging, no scan, no copy: the sizes are
// known before the launch, nothing is read on the host and the call with its graph output can be captured.  A row that keeps more
// than width_out entries (possible only without a rank cut) comes out EMPTY and is counted in status[0].
//
// The fixed-width stage entry, dagl_graph_stage_step_fixed, is that entry for the four heads of a CES stage: graph_stage_fixed_rows_kernel
// runs rf_row's FIXED flavour over the 4 B L head-major rows of the stage's slot arrays in ONE launch (the heads' operands by value, as in
// the stage search; the hash and the features from the head-local row), then launch_stage_fold_mix -- or, without the value operands,
// the graph alone.  The memset of the status words, the row launch, the fold + mix: capturable with its graph output.
//
// A row longer than max_row_edges comes out EMPTY and is counted in status[0] (integer atomics on the two status words are the only
// atomics); it is never truncated.  Every offset is clamped to [0, E], every key is range-tested before an address is formed, a row's
// candidates are bounded by the LDS arrays and its kept entries by its own staging region, the compaction by `capacity`: no array content
// makes a kernel leave its buffers.  Nothing is read on the host; the same arrays give the same bits on every call.
#include "dagl_common.h"
#include "graph_rows.h"

namespace dagl {

constexpr int RF_CAP = 2048;                  // candidates (before the repeats are dropped) a row may expand into: dagl_graph_refresh_max_candidates()
constexpr int RF_WAVE_CAP = 128;              // up to here a row is a wavefront's work (measured: DESIGN.md section 7; launch_graph_refresh)
constexpr int RF_MAX_RADIUS = 8;
constexpr int RF_EMPTY = 0x7fffffff;          // sorts behind every key
constexpr int RF_COPY_ROWS = 4;               // rows (wavefronts) per block of the compaction
constexpr int RS_MAX_EXPLORE = 256;           // random keys a row of the SEARCH flavour may ask for

struct RfArgs {
    int W, H, radius, max_row_edges, k, keep_all;
    int32_t* deg;                             // [B L] kept candidates per row
    int32_t* st_key; float* st_score; float* st_weight;     // [E (2 radius + 1)^2] staging
    unsigned long long* status;               // [2]: rows longer than max_row_edges, largest number of distinct candidates of a row
};

// what the SEARCH flavour of the row body adds (dagl_graph_search*): a struct of its own, so that the kernels above it keep their arguments
struct RsArgs {
    int propagate, explore;                   // the adjacent queries' edges as candidate sources (0 / 1); random keys per row (0 .. 256)
    unsigned seed;
    int Lw;                                   // queries per grid row (a.L / Lw grid rows per image)
    int k_region;                             // > 0: row r stages at r k_region (it keeps at most k);  0: at rs_region_start's prefix sum
    long long staged;                         // entries of each staging array
};

// what the FIXED flavour of the row body adds (dagl_graph_step_fixed).  The graph comes as width_in slots per row and a degree per row:
// GtArgs::key is the slot array, GtArgs::E = rows width_in, GtArgs::row_off is not used.  It leaves as width_out slots per row:
// RfArgs::st_key / st_score / st_weight are the OUTPUT arrays [rows, width_out] and RfArgs::deg the output degrees
struct RxArgs {
    const int32_t* deg_in;                    // [B L], read clamped to [0, width_in]
    int width_in, width_out;
};

__device__ __forceinline__ int rx_deg(const RxArgs& fx, int row) {
    const int d = fx.deg_in[row];
    return d < 0 ? 0 : (d > fx.width_in ? fx.width_in : d);
}

// lowbias32: the counter hash of the random candidates
__device__ __forceinline__ unsigned rs_hash(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// the offset of row r (r clamped to [0, n_rows]), clamped to [0, E]
__device__ __forceinline__ long long rs_off(const int64_t* __restrict__ row_off, int n_rows, long long E, long long r) {
    return gt_clamp(row_off[r < 0 ? 0 : (r > n_rows ? n_rows : r)], E);
}

// where row r of the SEARCH flavour stages, from row_off alone (no scan, no host read).  k_region = 0: the prefix sum over the rows
// before r of the bound  w2 (deg_r + the degrees of rows r - 1, r + 1, r - Lw, r + Lw) + explore  -- rows r + s that lie outside
// [0, n_rows) count 0, rows that are no grid neighbour (a grid-row end, an image boundary) are counted though never read: the sum of
// the regions is <= (5 E w2 + explore n_rows), what the entry allocates.  (With offsets that do not ascend the result is not a
// partition; rf_row tests its region against `staged` before it writes.)
__device__ __forceinline__ long long rs_region_start(const int64_t* __restrict__ row_off, int n_rows, long long E, int w2, const RsArgs& sr,
                                                     int row) {
    if (sr.k_region > 0) return (long long)row * sr.k_region;
    long long v = rs_off(row_off, n_rows, E, row);
    if (sr.propagate) {
        v += rs_off(row_off, n_rows, E, (long long)row - 1) - rs_off(row_off, n_rows, E, -1);
        v += rs_off(row_off, n_rows, E, (long long)row + 1) - rs_off(row_off, n_rows, E, 1);
        v += rs_off(row_off, n_rows, E, (long long)row - sr.Lw) - rs_off(row_off, n_rows, E, -sr.Lw);
        v += rs_off(row_off, n_rows, E, (long long)row + sr.Lw) - rs_off(row_off, n_rows, E, sr.Lw);
    }
    return v * w2 + (long long)sr.explore * row;
}

// a float as an unsigned that orders the same way: -0 = +0, NaN below everything (a strict total order with the key as tie-break: a rank
// cut keeps exactly min(k, passing) entries whatever the scores hold).  (Not in graph_rows.h: no other graph route ranks.)
__device__ __forceinline__ unsigned rf_ord(float s) {
    if (s != s) return 0u;
    const unsigned u = __float_as_uint(s == 0.f ? 0.f : s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rf_scan / rf_max / rf_sum stay here, not on dagl_common.h's block reductions: they are templated on the block size (a wavefront or four
// per row) and add the waves' partials one after the other where block_sum_f64 adds (w0 + w1) + (w2 + w3) -- other bits.
// exclusive prefix of v over the block's threads and the total, the same in every thread
template <int T>
__device__ __forceinline__ int rf_scan(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < T / 64; ++i) {
        base += i < w ? sh[i] : 0;
        total += sh[i];
    }
    return base + inc - v;
}

// maximum / sum over the block, fixed order: the xor butterfly inside each wave, then the waves one after the other
template <int T>
__device__ __forceinline__ float rf_max(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = sh[0];
#pragma unroll
    for (int i = 1; i < T / 64; ++i) m = fmaxf(m, sh[i]);
    return m;
}
template <int T>
__device__ __forceinline__ double rf_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = sh[0];
#pragma unroll
    for (int i = 1; i < T / 64; ++i) s += sh[i];
    return s;
}

// a row of zeros to agg [B L, 784]: what every exit of the aggregating flavour leaves before it returns (the workspace is not cleared)
template <int T>
__device__ __forceinline__ void rf_zero_row(float* agg, int row) {
    float4* o = reinterpret_cast<float4*>(agg + (size_t)row * P);
    for (int c = threadIdx.x; c < GA_C4; c += T) o[c] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// the slots from..width_out-1 of a FIXED output row: key -1, score 0, weight 0
template <int T>
__device__ __forceinline__ void rx_fill(const RfArgs& f, const RxArgs& fx, int row, int from) {
    const long long base = (long long)row * fx.width_out;
    for (int i = from + (int)threadIdx.x; i < fx.width_out; i += T) {
        f.st_key[base + i] = -1;
        f.st_score[base + i] = 0.f;
        f.st_weight[base + i] = 0.f;
    }
}

// the row body of the kernels below.  AGG (dagl_graph_step): the row's weighted sum of value patches goes to v.out [B L, 784] as well,
// and the graph outputs may be absent (f.st_key null: no degree, no staging writes).  SEARCH (dagl_graph_search*): step 1 takes the
// row's candidates from up to three sources -- (a) the windows around its own edges, as without SEARCH; (b) sr.propagate: the windows
// around (y - 4 dqy, x - 4 dqx) for every edge (y, x) of the query at (qy + dqy, qx + dqx), (dqy, dqx) in {(0, -1), (0, 1), (-1, 0),
// (1, 0)}, where that query lies in the Lh x Lw grid of the same image (the adjacent rows are read from the INPUT graph: Jacobi, no
// dependence on scheduling; the centre may lie off the map, the window is clipped cell by cell); (c) sr.explore keys
// (lowbias32(lowbias32(row ^ seed) + t) N) >> 32 of the row's image, no window -- and the row stages at rs_region_start; every step
// after the expansion is the same code.  `row` is the row of the CSR (row_off, deg, the staging region, v.out); `lrow` the row of the
// head's own operands (a.wq, a.x, a.tau, the value map, the hash of the random keys): the same row but in the stage kernel below, where
// the CSR holds four heads' rows and lrow = row - h B L.  FIXED (dagl_graph_step_fixed; RxArgs above): the input row is the slots
// row width_in .. + deg_in[row] (the adjacent queries' rows likewise), the kept entries go straight to row width_out + pos of the
// output arrays with the filler behind them, and every exit writes degree 0 and a whole filler row; a row that keeps more than
// width_out entries leaves empty, counted in status[0].  No staging region: rs_region_start, sr.staged and the room test are not used
template <int T, int CAP, bool AGG, bool SEARCH = false, bool FIXED = false>
__device__ __forceinline__ void rf_row(const GtArgs& a, const RfArgs& f, const GaArgs& v, const int row, const int lrow,
                                       const RsArgs& sr = RsArgs{}, const RxArgs& fx = RxArgs{}) {
    __shared__ long long s_of[CAP];           // two int arrays (below); AGG: at the end the float4 offset of each kept entry's value patch
                                              // in the map, compacted -- no array of its own: at 2048 candidates 16 KiB more LDS halve the
                                              // blocks per CU, and the row body lives on them
    __shared__ float s_sc[CAP];               // the scores of the distinct candidates; AGG: at the end the kept entries' weights, compacted
    __shared__ unsigned char s_flag[CAP];     // bits 0-1: the margin is not 0 (the candidate passes), bit 2: kept
    __shared__ int sh_i[T / 64];
    __shared__ float sh_f[T / 64];
    __shared__ double sh_d[T / 64];
    int* const s_sort = reinterpret_cast<int*>(s_of);     // the expanded candidates, sorted; then the order word of a passing candidate
    int* const s_key = s_sort + CAP;                      // the distinct candidates, ascending
    const bool graph_out = FIXED || !AGG || f.st_key != nullptr;
    const int t = threadIdx.x;
    const long long lo = FIXED ? (long long)row * fx.width_in : gt_clamp(a.row_off[row], a.E);
    const long long hi = FIXED ? lo + rx_deg(fx, row) : gt_clamp(a.row_off[row + 1], a.E);
    const long long deg_in = hi - lo;
    const int wd = 2 * f.radius + 1, w2 = wd * wd;
    // SEARCH: the sources' first edges and the running sums of their degrees (0 the row itself, 1-4 the adjacent queries; a source that
    // does not exist holds no edge), the raw candidate count and the row's staging region
    long long src_lo[5] = {lo, 0, 0, 0, 0}, stage_at = 0;
    int src_end[5] = {0, 0, 0, 0, 0}, raw_n = 0;
    if (SEARCH) {
        const int q = row % a.L, qy = q / sr.Lw, qx = q - qy * sr.Lw, Lh = a.L / sr.Lw;
        long long dg[5] = {deg_in > 0 ? deg_in : 0, 0, 0, 0, 0};
        if (sr.propagate) {
#pragma unroll
            for (int s = 1; s < 5; ++s) {
                const int dqy = s == 3 ? -1 : (s == 4 ? 1 : 0), dqx = s == 1 ? -1 : (s == 2 ? 1 : 0);
                if ((unsigned)(qy + dqy) < (unsigned)Lh && (unsigned)(qx + dqx) < (unsigned)sr.Lw) {
                    const int r2 = row + dqy * sr.Lw + dqx;                      // (the same image: in [0, n_rows))
                    src_lo[s] = FIXED ? (long long)r2 * fx.width_in : gt_clamp(a.row_off[r2], a.E);
                    const long long d = FIXED ? (long long)rx_deg(fx, r2) : gt_clamp(a.row_off[r2 + 1], a.E) - src_lo[s];
                    dg[s] = d > 0 ? d : 0;
                }
            }
        }
        bool overlong = false;
        long long sum = 0;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            overlong |= dg[s] > f.max_row_edges;
            sum += dg[s];
        }
        const long long raw_ll = overlong ? 0 : sum * w2 + sr.explore;           // (<= 5 max_row_edges w2 + 256: no overflow)
        stage_at = !FIXED && graph_out ? rs_region_start(a.row_off, a.n_rows, a.E, w2, sr, row) : 0;
        const long long region = sr.k_region > 0 ? sr.k_region : raw_ll;
        const bool room = FIXED || !graph_out || (stage_at >= 0 && stage_at + region <= sr.staged);
        if (overlong || raw_ll <= 0 || raw_ll > CAP || !room) {                  // (the same in every thread)
            if (t == 0) {
                if (graph_out) f.deg[row] = 0;
                if (overlong || raw_ll > CAP) atomicAdd(f.status, 1ull);
            }
            if (FIXED) rx_fill<T>(f, fx, row, 0);
            if (AGG) rf_zero_row<T>(v.out, row);
            return;
        }
        raw_n = (int)raw_ll;
        int run = 0;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            run += (int)dg[s];
            src_end[s] = run;
        }
    } else if (deg_in <= 0 || deg_in > f.max_row_edges || deg_in * w2 > CAP) {   // (the same in every thread)
        if (t == 0) {
            if (graph_out) f.deg[row] = 0;
            if (deg_in > 0) atomicAdd(f.status, 1ull);
        }
        if (FIXED) rx_fill<T>(f, fx, row, 0);
        if (AGG) rf_zero_row<T>(v.out, row);
        return;
    }
    // 1. expand: entry idx = (edge, window offset); what falls off the map or comes from a key off the map sorts to the end
    const int raw = SEARCH ? raw_n : (int)deg_in * w2;
    int n_pad = 64;
    while (n_pad < raw) n_pad <<= 1;                                              // <= CAP: CAP is a power of two >= raw
    if (SEARCH) {
        const int windowed = src_end[4] * w2;                                     // entries (edge of a source, window offset); then the random keys
        const unsigned h0 = rs_hash((unsigned)lrow ^ sr.seed);
        for (int idx = t; idx < n_pad; idx += T) {
            int c = RF_EMPTY;
            if (idx < windowed) {
                const int e = idx / w2, o = idx - e * w2;
                long long at = src_lo[0] + e;
                int sy = 0, sx = 0;                                               // the shift of the source's keys: 4 (dqy, dqx)
#pragma unroll
                for (int s = 1; s < 5; ++s) {
                    if (e >= src_end[s - 1]) {
                        at = src_lo[s] + (e - src_end[s - 1]);
                        sy = s == 3 ? -QS : (s == 4 ? QS : 0);
                        sx = s == 1 ? -QS : (s == 2 ? QS : 0);
                    }
                }
                const int key = a.key[at];
                if ((unsigned)key < (unsigned)a.N) {
                    const int oy = o / wd;
                    const int y = key / f.W - sy + oy - f.radius, x = key % f.W - sx + (o - oy * wd) - f.radius;
                    if ((unsigned)y < (unsigned)f.H && (unsigned)x < (unsigned)f.W) c = y * f.W + x;
                }
            } else if (idx < raw) {
                const unsigned h = rs_hash(h0 + (unsigned)(idx - windowed));
                c = (int)(((unsigned long long)h * (unsigned long long)(unsigned)a.N) >> 32);      // < N
            }
            s_sort[idx] = c;
        }
    } else {
        for (int idx = t; idx < n_pad; idx += T) {
            int c = RF_EMPTY;
            if (idx < raw) {
                const int e = idx / w2, o = idx - e * w2;
                const int key = a.key[lo + e];
                if ((unsigned)key < (unsigned)a.N) {
                    const int oy = o / wd;
                    const int y = key / f.W + oy - f.radius, x = key % f.W + (o - oy * wd) - f.radius;
                    if ((unsigned)y < (unsigned)f.H && (unsigned)x < (unsigned)f.W) c = y * f.W + x;
                }
            }
            s_sort[idx] = c;
        }
    }
    __syncthreads();
    // 2. bitonic sort, ascending
    for (int kk = 2; kk <= n_pad; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = t; i < n_pad; i += T) {
                const int p = i ^ j;
                if (p > i) {
                    const int u = s_sort[i], v = s_sort[p];
                    if ((u > v) == ((i & kk) == 0)) { s_sort[i] = v; s_sort[p] = u; }
                }
            }
            __syncthreads();
        }
    }
    // 3. the distinct candidates, in order: a run of consecutive entries per thread, an exclusive scan of the counts
    const int per = n_pad / T > 0 ? n_pad / T : 1;
    const int i0 = min(n_pad, t * per), i1 = min(n_pad, i0 + per);
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += s_sort[i] != RF_EMPTY && (i == 0 || s_sort[i] != s_sort[i - 1]);
    int n;
    int pos = rf_scan<T>(cnt, sh_i, n);
    for (int i = i0; i < i1; ++i)
        if (s_sort[i] != RF_EMPTY && (i == 0 || s_sort[i] != s_sort[i - 1])) s_key[pos++] = s_sort[i];
    __syncthreads();
    if (t == 0 && (unsigned long long)n > f.status[1]) atomicMax(f.status + 1, (unsigned long long)n);
    // 4. scores and margins: a candidate per 16 lanes, two in flight per group
    {
        const int l = t & 15, grp = t >> 4, G = T / 16;
        const float4* q = reinterpret_cast<const float4*>(a.wq) + (size_t)lrow * GT_C4;
        const float4* xk = reinterpret_cast<const float4*>(a.x) + (size_t)(lrow / a.L) * a.N * GT_C4;
        for (int c0 = grp; c0 < n; c0 += 2 * G) {
            const int c1 = c0 + G < n ? c0 + G : c0;
            const float v0 = gt_edge_dot(q, xk + (size_t)s_key[c0] * GT_C4, l);
            const float v1 = gt_edge_dot(q, xk + (size_t)s_key[c1] * GT_C4, l);
            if (l == 0) {
                float mg;
                gt_logit(a, lrow, v0, mg);
                s_sc[c0] = v0;
                s_flag[c0] = mg != 0.f ? 3 : 0;
                if (c1 != c0) {
                    gt_logit(a, lrow, v1, mg);
                    s_sc[c1] = v1;
                    s_flag[c1] = mg != 0.f ? 3 : 0;
                }
            }
        }
    }
    __syncthreads();
    // 5. the rank cut among the passing candidates: better = a larger score, or an equal one with a lower key
    unsigned* s_ord = reinterpret_cast<unsigned*>(s_sort);
    if (f.keep_all) {
        for (int c = t; c < n; c += T) s_flag[c] |= 4;
    } else if (f.k <= 0) {
        for (int c = t; c < n; c += T) s_flag[c] |= (s_flag[c] & 2) << 1;
    } else {
        for (int c = t; c < n; c += T) s_ord[c] = rf_ord(s_sc[c]);
        __syncthreads();
        for (int c = t; c < n; c += T) {
            if (!(s_flag[c] & 2)) continue;
            const unsigned oc = s_ord[c];
            int rank = 0;
            for (int j = 0; j < n; ++j) {                        // (ascending keys: j < c is the lower key)
                const unsigned oj = s_ord[j];
                rank += (s_flag[j] & 2) && (oj > oc || (oj == oc && j < c));
            }
            if (rank < f.k) s_flag[c] |= 4;
        }
    }
    __syncthreads();
    // 6. the output row: its degree, the maximum, the sum, the weights
    cnt = 0;
    const int pr = (n + T - 1) / T;
    const int c0 = min(n, t * pr), c1 = min(n, c0 + pr);
    for (int c = c0; c < c1; ++c) cnt += (s_flag[c] >> 2) & 1;
    int kept;
    pos = rf_scan<T>(cnt, sh_i, kept);
    if (FIXED && kept > fx.width_out) {                          // (the same in every thread) more than the output row holds: empty, counted
        if (t == 0) {
            f.deg[row] = 0;
            atomicAdd(f.status, 1ull);
        }
        rx_fill<T>(f, fx, row, 0);
        if (AGG) rf_zero_row<T>(v.out, row);
        return;
    }
    if (t == 0 && graph_out) f.deg[row] = kept;
    if (kept == 0) {                                             // (the same in every thread)
        if (FIXED) rx_fill<T>(f, fx, row, 0);
        if (AGG) rf_zero_row<T>(v.out, row);
        return;
    }
    const bool off_graph = !a.edges_only && kept < a.N;
    float mx = -INFINITY;
    for (int c = c0; c < c1; ++c) {
        float mg;
        if (s_flag[c] & 4) mx = fmaxf(mx, gt_logit(a, lrow, s_sc[c], mg));
    }
    mx = rf_max<T>(mx, sh_f);
    const float M = off_graph ? fmaxf(mx, 0.f) : mx;
    double sum = 0.0;
    for (int c = c0; c < c1; ++c) {
        float mg;
        if (s_flag[c] & 4) sum += (double)expf(gt_logit(a, lrow, s_sc[c], mg) - M);
    }
    sum = rf_sum<T>(sum, sh_d);
    if (off_graph) sum += (double)(a.N - kept) * exp(-(double)M);
    // 7. the kept entries, ascending keys, to the front of the row's staging region (kept <= n <= raw = its size; SEARCH with a rank
    //    cut: kept <= k = its size).  FIXED: to the front of the row's own width_out slots (kept <= width_out), the filler behind them
    const long long base = FIXED ? (long long)row * fx.width_out : (SEARCH ? stage_at : lo * w2);
    //    AGG: a thread also keeps the weight and the patch offset of its kept entries (at most PER = CAP / T >= pr of them) in registers
    constexpr int PER = CAP / T;
    float my_w[AGG ? PER : 1];
    long long my_of[AGG ? PER : 1];
    const int pos0 = pos;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = c0 + i;
        if (c >= c1) break;
        if (!(s_flag[c] & 4)) continue;
        float mg;
        const float z = gt_logit(a, lrow, s_sc[c], mg);
        const float wgt = mg != 0.f ? (float)((double)expf(z - M) / sum) : 0.f;
        if (graph_out) {
            f.st_key[base + pos] = s_key[c];
            f.st_score[base + pos] = s_sc[c];
            f.st_weight[base + pos] = wgt;
        }
        if (AGG) {
            my_w[i] = wgt;
            my_of[i] = ga_source<true>(v, lrow, s_key[c]);        // (a candidate is a key of the map: never -1)
        }
        ++pos;
    }
    if (FIXED) rx_fill<T>(f, fx, row, kept);
    if (!AGG) return;
    // 8. the kept entries' weights and patch offsets to the LDS in compacted (ascending-key) order, over the scores and the two int
    //    arrays -- every thread has read its own entries of those above: a barrier, the stores (pos0 .. < kept <= n <= CAP), a barrier
    __syncthreads();
    pos = pos0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = c0 + i;
        if (c < c1 && (s_flag[c] & 4)) {
            s_sc[pos] = my_w[i];
            s_of[pos] = my_of[i];
            ++pos;
        }
    }
    __syncthreads();
    // 9. agg[row] = sum_c weight_c V[key_c] over the kept entries in ascending key order: a float4 column of the 784-float row at a time,
    //    one fmaf chain per element (ga_gather_run), so a wavefront (columns lane, lane + 64, ...) and a block (a column per thread of
    //    0..195) give the same bits
    const float4* src = reinterpret_cast<const float4*>(v.src);
    float4* o = reinterpret_cast<float4*>(v.out + (size_t)row * P);
    for (int c = t; c < GA_C4; c += T) o[c] = ga_gather_run(src + (c / 28) * v.Wp * (CH / 4) + c % 28, s_of, s_sc, 0, kept);
}

template <int T, int CAP>
__global__ __launch_bounds__(T) void graph_refresh_rows_kernel(GtArgs a, RfArgs f) {
    rf_row<T, CAP, false>(a, f, GaArgs{}, blockIdx.x, blockIdx.x);
}

// dagl_graph_step's: the refresh's row and its aggregated output row from the same kept entries
template <int T, int CAP>
__global__ __launch_bounds__(T) void graph_step_rows_kernel(GtArgs a, RfArgs f, GaArgs v) {
    rf_row<T, CAP, true>(a, f, v, blockIdx.x, blockIdx.x);
}

// dagl_graph_search's and dagl_graph_search_step's: the same two bodies with the SEARCH candidate sources (kernels of their own: the
// four above keep their arguments and their device code)
template <int T, int CAP>
__global__ __launch_bounds__(T) void graph_search_rows_kernel(GtArgs a, RfArgs f, RsArgs sr) {
    rf_row<T, CAP, false, true>(a, f, GaArgs{}, blockIdx.x, blockIdx.x, sr);
}

template <int T, int CAP>
__global__ __launch_bounds__(T) void graph_search_step_rows_kernel(GtArgs a, RfArgs f, GaArgs v, RsArgs sr) {
    rf_row<T, CAP, true, true>(a, f, v, blockIdx.x, blockIdx.x, sr);
}

// dagl_graph_step_fixed's: the FIXED flavour of the four bodies above (kernels of their own: those keep their arguments and their
// device code)
template <int T, int CAP>
__global__ __launch_bounds__(T) void graph_fixed_rows_kernel(GtArgs a, RfArgs f, RxArgs fx) {
    rf_row<T, CAP, false, false, true>(a, f, GaArgs{}, blockIdx.x, blockIdx.x, RsArgs{}, fx);
}

template <int T, int CAP>
__global__ __launch_bounds__(T) void graph_fixed_step_rows_kernel(GtArgs a, RfArgs f, GaArgs v, RxArgs fx) {
    rf_row<T, CAP, true, false, true>(a, f, v, blockIdx.x, blockIdx.x, RsArgs{}, fx);
}

template <int T, int CAP>
__global__ __launch_bounds__(T) void graph_fixed_search_rows_kernel(GtArgs a, RfArgs f, RsArgs sr, RxArgs fx) {
    rf_row<T, CAP, false, true, true>(a, f, GaArgs{}, blockIdx.x, blockIdx.x, sr, fx);
}

template <int T, int CAP>
__global__ __launch_bounds__(T) void graph_fixed_search_step_rows_kernel(GtArgs a, RfArgs f, GaArgs v, RsArgs sr, RxArgs fx) {
    rf_row<T, CAP, true, true, true>(a, f, v, blockIdx.x, blockIdx.x, sr, fx);
}

// dagl_graph_stage_search's and dagl_graph_stage_search_step's: the SEARCH flavour over the 4 B L head-major rows of a CES stage's CSR in
// ONE launch.  The four heads' own operands come by value in the arguments; row r belongs to head h = r / (B L) and is row r - h B L of
// that head's features, margins, value map and hash, while the offsets, the adjacent rows, the degree, the staging region (the prefix
// sum over the WHOLE CSR: a.n_rows = 4 B L) and the aggregated row are those of r.  row0: the first row of the launch (0 but where the
// heads are launched one by one, for measurements)
struct RsHeads { const float* wq[4]; const float* x[4]; const float* tau[4]; const float* b2p[4]; };

template <int T, int CAP, bool AGG>
__global__ __launch_bounds__(T) void graph_stage_search_rows_kernel(GtArgs a, RfArgs f, GaArgs v, RsArgs sr, RsHeads hd, int head_rows,
                                                                    int row0) {
    const int row = row0 + (int)blockIdx.x;                      // < 4 head_rows (the launch)
    const int h = row / head_rows;
    // (selects, not an index: the table stays in scalar registers)
    a.wq = h == 0 ? hd.wq[0] : (h == 1 ? hd.wq[1] : (h == 2 ? hd.wq[2] : hd.wq[3]));
    a.x = h == 0 ? hd.x[0] : (h == 1 ? hd.x[1] : (h == 2 ? hd.x[2] : hd.x[3]));
    a.tau = h == 0 ? hd.tau[0] : (h == 1 ? hd.tau[1] : (h == 2 ? hd.tau[2] : hd.tau[3]));
    if (AGG) v.src = h == 0 ? hd.b2p[0] : (h == 1 ? hd.b2p[1] : (h == 2 ? hd.b2p[2] : hd.b2p[3]));
    rf_row<T, CAP, AGG, true>(a, f, v, row, row - h * head_rows, sr);
}

// dagl_graph_stage_step_fixed's: the FIXED flavour over the 4 B L head-major rows of a CES stage's fixed-width graph in ONE launch (a
// kernel of its own: those above keep their arguments and their device code).  The heads' operands come as in the kernel above; row r
// addresses its input slots, the adjacent rows' (r +- 1, r +- Lw: the grid position is r % L and head_rows is a multiple of L, so a
// source never lies in another image or head), its output slots, its degree and its aggregated row; lrow = r - h head_rows the features,
// the margin, the value map and the hash.  a.n_rows = 4 head_rows
template <int T, int CAP, bool AGG, bool SEARCH>
__global__ __launch_bounds__(T) void graph_stage_fixed_rows_kernel(GtArgs a, RfArgs f, GaArgs v, RsArgs sr, RxArgs fx, RsHeads hd,
                                                                   int head_rows) {
    const int row = (int)blockIdx.x;                             // < 4 head_rows (the launch)
    const int h = row / head_rows;
    // (selects, not an index: the table stays in scalar registers)
    a.wq = h == 0 ? hd.wq[0] : (h == 1 ? hd.wq[1] : (h == 2 ? hd.wq[2] : hd.wq[3]));
    a.x = h == 0 ? hd.x[0] : (h == 1 ? hd.x[1] : (h == 2 ? hd.x[2] : hd.x[3]));
    a.tau = h == 0 ? hd.tau[0] : (h == 1 ? hd.tau[1] : (h == 2 ? hd.tau[2] : hd.tau[3]));
    if (AGG) v.src = h == 0 ? hd.b2p[0] : (h == 1 ? hd.b2p[1] : (h == 2 ? hd.b2p[2] : hd.b2p[3]));
    rf_row<T, CAP, AGG, SEARCH, true>(a, f, v, row, row - h * head_rows, sr, fx);
}

// graph_refresh_compact_kernel (below) for the SEARCH flavour: a row's staged entries start at rs_region_start.  deg[row] > 0 only where
// rf_row found the whole region inside the staging arrays
__global__ __launch_bounds__(RF_COPY_ROWS * 64) void graph_search_compact_kernel(int n_rows, int w2, long long E, RsArgs sr,
                                                                                 const int64_t* __restrict__ row_off,
                                                                                 const int32_t* __restrict__ deg,
                                                                                 const int64_t* __restrict__ row_off_out,
                                                                                 const int32_t* __restrict__ st_key, const float* __restrict__ st_score,
                                                                                 const float* __restrict__ st_weight, int32_t* __restrict__ key,
                                                                                 float* __restrict__ weight, float* __restrict__ score,
                                                                                 long long capacity) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * RF_COPY_ROWS + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const long long src = rs_region_start(row_off, n_rows, E, w2, sr, row), dst = row_off_out[row];
    const int n = deg[row];
    if (n <= 0 || src < 0 || src + n > sr.staged) return;
    for (int i = lane; i < n; i += 64) {
        if (dst + i >= capacity) break;                          // (offsets that overlap: more staged than the caller's bound)
        key[dst + i] = st_key[src + i];
        score[dst + i] = st_score[src + i];
        weight[dst + i] = st_weight[src + i];
    }
}

// a wavefront per row: its staged entries to their place in the output
__global__ __launch_bounds__(RF_COPY_ROWS * 64) void graph_refresh_compact_kernel(int n_rows, int w2, long long E, const int64_t* __restrict__ row_off,
                                                                                  const int32_t* __restrict__ deg,
                                                                                  const int64_t* __restrict__ row_off_out,
                                                                                  const int32_t* __restrict__ st_key, const float* __restrict__ st_score,
                                                                                  const float* __restrict__ st_weight, int32_t* __restrict__ key,
                                                                                  float* __restrict__ weight, float* __restrict__ score,
                                                                                  long long capacity) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * RF_COPY_ROWS + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const long long src = gt_clamp(row_off[row], E) * w2, dst = row_off_out[row];
    const int n = deg[row];                                      // <= the row's staging region (graph_refresh_rows_kernel)
    for (int i = lane; i < n; i += 64) {
        if (dst + i >= capacity) break;                          // (offsets that overlap: more staged than the caller's bound)
        key[dst + i] = st_key[src + i];
        score[dst + i] = st_score[src + i];
        weight[dst + i] = st_weight[src + i];
    }
}

struct RefreshWs { float* agg; int32_t* deg; int32_t* st_key; float* st_score; float* st_weight; size_t bytes; };

// agg: the step's [B L, 784] aggregated rows; graph: the degrees and the staging region (the step without graph outputs has neither)
static RefreshWs refresh_carve(void* ws, size_t n_rows, size_t staged, bool agg = false, bool graph = true) {
    Carver cv(ws);
    RefreshWs w{};
    if (agg) w.agg = cv.take<float>(n_rows * P);
    if (graph) {
        w.deg = cv.take<int32_t>(n_rows);
        w.st_key = cv.take<int32_t>(staged + 1);
        w.st_score = cv.take<float>(staged + 1);
        w.st_weight = cv.take<float>(staged + 1);
    }
    w.bytes = cv.bytes();
    return w;
}

// b2p / out: the step's value map and output, both null for the refresh;  row_off_out null (the step alone): no graph comes out
// search: the SEARCH flavour (dagl_graph_search*: propagate or explore set) with its candidate sources and its staging layout
struct RefreshCall {
    GraphAttendCall c; int max_row_edges, radius, k; bool keep_all, block_rows;
    int64_t* row_off_out; int32_t* key_out; float* weight_out; float* score_out; int64_t capacity; int64_t* status;
    const float* b2p; float* out;
    bool search; int propagate, explore; uint32_t seed;
};

// the candidates a row may expand into, before the repeats are dropped: its own edges' windows; SEARCH: the four adjacent rows' too, and
// the random keys
static long long rf_row_bound(int max_row_edges, int radius, int propagate, int explore) {
    const long long wd = 2 * radius + 1;
    return (long long)(1 + 4 * propagate) * max_row_edges * wd * wd + explore;
}

// the entries of each staging array and the most edges a call may produce.  Without SEARCH: E w2.  SEARCH: a region of k per row
// under a rank cut, else rs_region_start's prefix sums
static int64_t rf_staged(int64_t n_rows, int64_t E, int radius, int propagate, int explore, int k_region) {
    const int64_t w2 = (int64_t)(2 * radius + 1) * (2 * radius + 1);
    if (!propagate && !explore) return E * w2;
    return k_region > 0 ? n_rows * k_region : (1 + 4 * propagate) * E * w2 + explore * n_rows;
}

// short rows (top-k 8 at radius 1: 72 candidates) take a wavefront each, longer ones a block of four
static bool rf_wave_rows(const RefreshCall& r) {
    return !r.block_rows && rf_row_bound(r.max_row_edges, r.radius, r.search ? r.propagate : 0, r.search ? r.explore : 0) <= RF_WAVE_CAP;
}

// the SEARCH flavour's row kernel, with or without the aggregation epilogue (v null), in either form
static int launch_search_rows(hipStream_t s, int n_rows, bool wave, const GtArgs& a, const RfArgs& f, const GaArgs* v, const RsArgs& sr) {
    if (v) {
        if (wave) {
            hipLaunchKernelGGL((graph_search_step_rows_kernel<64, RF_WAVE_CAP>), dim3((unsigned)n_rows), dim3(64), 0, s, a, f, *v, sr);
        } else {
            hipLaunchKernelGGL((graph_search_step_rows_kernel<256, RF_CAP>), dim3((unsigned)n_rows), dim3(256), 0, s, a, f, *v, sr);
        }
        DAGL_LAUNCH_CHECK("graph_search_step_rows_kernel");
    } else {
        if (wave) {
            hipLaunchKernelGGL((graph_search_rows_kernel<64, RF_WAVE_CAP>), dim3((unsigned)n_rows), dim3(64), 0, s, a, f, sr);
        } else {
            hipLaunchKernelGGL((graph_search_rows_kernel<256, RF_CAP>), dim3((unsigned)n_rows), dim3(256), 0, s, a, f, sr);
        }
        DAGL_LAUNCH_CHECK("graph_search_rows_kernel");
    }
    return DAGL_OK;
}

// the step's row kernel over n_rows rows: a block per row of a.row_off, in either form
static int launch_step_rows(hipStream_t s, int n_rows, bool wave, const GtArgs& a, const RfArgs& f, const GaArgs& v) {
    if (wave) {
        hipLaunchKernelGGL((graph_step_rows_kernel<64, RF_WAVE_CAP>), dim3((unsigned)n_rows), dim3(64), 0, s, a, f, v);
    } else {
        hipLaunchKernelGGL((graph_step_rows_kernel<256, RF_CAP>), dim3((unsigned)n_rows), dim3(256), 0, s, a, f, v);
    }
    DAGL_LAUNCH_CHECK("graph_step_rows_kernel");
    return DAGL_OK;
}

static int launch_graph_refresh(hipStream_t s, int B, const Grid& g, const RefreshCall& r, void* workspace) {
    const int n_rows = B * g.L, wd = 2 * r.radius + 1, w2 = wd * wd;
    const bool agg = r.out != nullptr, graph = r.row_off_out != nullptr;
    DAGL_HIP_TRY(hipMemsetAsync(r.status, 0, 2 * sizeof(int64_t), s));
    if (r.c.E == 0 && !(r.search && r.explore > 0)) {            // (random keys populate an empty graph)
        if (graph) DAGL_HIP_TRY(hipMemsetAsync(r.row_off_out, 0, ((size_t)n_rows + 1) * sizeof(int64_t), s));
        if (agg) DAGL_HIP_TRY(hipMemsetAsync(r.out, 0, (size_t)B * CH * g.N * sizeof(float), s));      // fold(0) / cnt
        return DAGL_OK;
    }
    const int k_region = r.keep_all ? 0 : r.k;
    const int64_t staged = rf_staged(n_rows, r.c.E, r.radius, r.search ? r.propagate : 0, r.search ? r.explore : 0, k_region);
    const RefreshWs w = refresh_carve(workspace, (size_t)n_rows, (size_t)staged, agg, graph);
    const GtArgs a = gt_args(B, g, r.c);
    RfArgs f{};
    f.W = g.W; f.H = g.H; f.radius = r.radius; f.max_row_edges = r.max_row_edges; f.k = r.keep_all ? 0 : r.k; f.keep_all = r.keep_all ? 1 : 0;
    f.deg = w.deg; f.st_key = w.st_key; f.st_score = w.st_score; f.st_weight = w.st_weight;
    f.status = reinterpret_cast<unsigned long long*>(r.status);
    const bool wave = rf_wave_rows(r);
    RsArgs sr{};
    sr.propagate = r.propagate; sr.explore = r.explore; sr.seed = r.seed; sr.Lw = g.Lw; sr.k_region = k_region; sr.staged = staged;
    if (r.search) {
        GaArgs v = ga_map_args(B, g, r.b2p, nullptr, nullptr, nullptr, 0);
        v.out = w.agg;
        const int rc = launch_search_rows(s, n_rows, wave, a, f, agg ? &v : nullptr, sr);
        if (rc) return rc;
    } else if (agg) {
        GaArgs v = ga_map_args(B, g, r.b2p, nullptr, nullptr, nullptr, 0);
        v.out = w.agg;
        const int rc = launch_step_rows(s, n_rows, wave, a, f, v);
        if (rc) return rc;
    } else {
        if (wave) {
            hipLaunchKernelGGL((graph_refresh_rows_kernel<64, RF_WAVE_CAP>), dim3((unsigned)n_rows), dim3(64), 0, s, a, f);
        } else {
            hipLaunchKernelGGL((graph_refresh_rows_kernel<256, RF_CAP>), dim3((unsigned)n_rows), dim3(256), 0, s, a, f);
        }
        DAGL_LAUNCH_CHECK("graph_refresh_rows_kernel");
    }
    if (graph) {
        const int rc = launch_row_scan(s, n_rows, w.deg, r.row_off_out);
        if (rc) return rc;
        const dim3 copy_grid((unsigned)((n_rows + RF_COPY_ROWS - 1) / RF_COPY_ROWS));
        if (r.search) {
            hipLaunchKernelGGL(graph_search_compact_kernel, copy_grid, dim3(RF_COPY_ROWS * 64), 0, s, n_rows, w2, (long long)r.c.E, sr,
                               r.c.row_off, w.deg, r.row_off_out, w.st_key, w.st_score, w.st_weight, r.key_out, r.weight_out, r.score_out,
                               (long long)r.capacity);
            DAGL_LAUNCH_CHECK("graph_search_compact_kernel");
        } else {
            hipLaunchKernelGGL(graph_refresh_compact_kernel, copy_grid, dim3(RF_COPY_ROWS * 64), 0, s, n_rows, w2, (long long)r.c.E,
                               r.c.row_off, w.deg, r.row_off_out, w.st_key, w.st_score, w.st_weight, r.key_out, r.weight_out, r.score_out,
                               (long long)r.capacity);
            DAGL_LAUNCH_CHECK("graph_refresh_compact_kernel");
        }
    }
    return agg ? launch_fold(s, B, g, w.agg, r.out) : DAGL_OK;
}

// The step of a whole CES stage: r.c.row_off / key are ONE CSR over the 4 B L head-major rows, head h has features, value map and tau
// of its own.  The row kernel runs once per head on that head's slice of the offsets, degrees and aggregated rows -- a row addresses the
// keys and its staging region by the absolute row_off[r], so nothing is rebased and no feature is copied --, the status words add up
// over the launches; then one scan and one ordered copy over all the rows, and the fold + mix + residual of the four heads' rows.
struct StageStepCall { const float* const* wq4; const float* const* x4; const float* const* b2p4; const float* const* tau4;
                       const float* x; const float* mix_w; const float* mix_b; };

static int launch_graph_stage_step(hipStream_t s, int B, const Grid& g, const RefreshCall& r, const StageStepCall& st, void* workspace) {
    const int head_rows = B * g.L, n_rows = 4 * head_rows, wd = 2 * r.radius + 1, w2 = wd * wd;
    const bool graph = r.row_off_out != nullptr;
    DAGL_HIP_TRY(hipMemsetAsync(r.status, 0, 2 * sizeof(int64_t), s));
    const RefreshWs w = refresh_carve(workspace, (size_t)n_rows, (size_t)r.c.E * w2, true, graph);
    if (r.c.E == 0) {
        if (graph) DAGL_HIP_TRY(hipMemsetAsync(r.row_off_out, 0, ((size_t)n_rows + 1) * sizeof(int64_t), s));
        DAGL_HIP_TRY(hipMemsetAsync(w.agg, 0, (size_t)n_rows * P * sizeof(float), s));                  // fold(0) / cnt: out = mix_b + x
        return launch_stage_fold_mix(s, B, g, w.agg, st.x, st.mix_w, st.mix_b, r.out);
    }
    RfArgs f{};
    f.W = g.W; f.H = g.H; f.radius = r.radius; f.max_row_edges = r.max_row_edges; f.k = r.keep_all ? 0 : r.k; f.keep_all = r.keep_all ? 1 : 0;
    f.st_key = w.st_key; f.st_score = w.st_score; f.st_weight = w.st_weight;
    f.status = reinterpret_cast<unsigned long long*>(r.status);
    const bool wave = rf_wave_rows(r);
    for (int h = 0; h < 4; ++h) {
        GraphAttendCall c = r.c;
        c.wq_rows = st.wq4[h]; c.x_rows = st.x4[h]; c.tau = st.tau4 ? st.tau4[h] : nullptr;
        c.row_off = r.c.row_off + (size_t)h * head_rows;
        const GtArgs a = gt_args(B, g, c);                       // (E stays the whole array's: the clamp of an offset)
        f.deg = graph ? w.deg + (size_t)h * head_rows : nullptr;
        GaArgs v = ga_map_args(B, g, st.b2p4[h], nullptr, nullptr, nullptr, 0);
        v.out = w.agg + (size_t)h * head_rows * P;
        const int rc = launch_step_rows(s, head_rows, wave, a, f, v);
        if (rc) return rc;
    }
    if (graph) {
        const int rc = launch_row_scan(s, n_rows, w.deg, r.row_off_out);
        if (rc) return rc;
        hipLaunchKernelGGL(graph_refresh_compact_kernel, dim3((unsigned)((n_rows + RF_COPY_ROWS - 1) / RF_COPY_ROWS)), dim3(RF_COPY_ROWS * 64), 0,
                           s, n_rows, w2, (long long)r.c.E, r.c.row_off, w.deg, r.row_off_out, w.st_key, w.st_score, w.st_weight, r.key_out,
                           r.weight_out, r.score_out, (long long)r.capacity);
        DAGL_LAUNCH_CHECK("graph_refresh_compact_kernel");
    }
    return launch_stage_fold_mix(s, B, g, w.agg, st.x, st.mix_w, st.mix_b, r.out);
}

// the entries of each staging array of the stage search: 4 B L k under a rank cut, else rs_region_start's prefix sums over the whole CSR
// (also with both sources off: the flavour's own layout)
static int64_t rs_stage_staged(int64_t n_rows, int64_t E, int radius, int propagate, int explore, int k_region) {
    const int64_t w2 = (int64_t)(2 * radius + 1) * (2 * radius + 1);
    return k_region > 0 ? n_rows * k_region : (1 + 4 * propagate) * E * w2 + explore * n_rows;
}

template <bool AGG>
static void launch_stage_search_rows(hipStream_t s, int rows, bool wave, const GtArgs& a, const RfArgs& f, const GaArgs& v, const RsArgs& sr,
                                     const RsHeads& hd, int head_rows, int row0) {
    if (wave) {
        hipLaunchKernelGGL((graph_stage_search_rows_kernel<64, RF_WAVE_CAP, AGG>), dim3((unsigned)rows), dim3(64), 0, s, a, f, v, sr, hd,
                           head_rows, row0);
    } else {
        hipLaunchKernelGGL((graph_stage_search_rows_kernel<256, RF_CAP, AGG>), dim3((unsigned)rows), dim3(256), 0, s, a, f, v, sr, hd,
                           head_rows, row0);
    }
}

// The search step of a whole CES stage (dagl_graph_stage_search*): the CSR, the operand tables and the end of launch_graph_stage_step,
// but ONE row launch over the 4 B L rows (graph_stage_search_rows_kernel), and the staging laid out over the whole CSR: without a rank
// cut a head's rows may need up to 5 E_h w2 entries, which no slice of an E w2 array holds.  st.b2p4 / r.out null: the graph alone.
// head_launches: the same kernel once per head on its rows (for measurements: the same bits)
static int launch_graph_stage_search(hipStream_t s, int B, const Grid& g, const RefreshCall& r, const StageStepCall& st, void* workspace,
                                     bool head_launches) {
    const int head_rows = B * g.L, n_rows = 4 * head_rows, wd = 2 * r.radius + 1, w2 = wd * wd;
    const bool agg = r.out != nullptr, graph = r.row_off_out != nullptr;
    DAGL_HIP_TRY(hipMemsetAsync(r.status, 0, 2 * sizeof(int64_t), s));
    const int k_region = r.keep_all ? 0 : r.k;
    const int64_t staged = rs_stage_staged(n_rows, r.c.E, r.radius, r.propagate, r.explore, k_region);
    const RefreshWs w = refresh_carve(workspace, (size_t)n_rows, (size_t)staged, agg, graph);
    if (r.c.E == 0 && r.explore == 0) {                          // (random keys populate an empty graph)
        if (graph) DAGL_HIP_TRY(hipMemsetAsync(r.row_off_out, 0, ((size_t)n_rows + 1) * sizeof(int64_t), s));
        if (!agg) return DAGL_OK;
        DAGL_HIP_TRY(hipMemsetAsync(w.agg, 0, (size_t)n_rows * P * sizeof(float), s));                  // fold(0) / cnt: out = mix_b + x
        return launch_stage_fold_mix(s, B, g, w.agg, st.x, st.mix_w, st.mix_b, r.out);
    }
    GraphAttendCall c = r.c;
    c.wq_rows = st.wq4[0]; c.x_rows = st.x4[0];                  // (the kernel takes every head's from the table)
    const GtArgs a = gt_args(4 * B, g, c);                       // n_rows = 4 B L: the rows rs_region_start sums over
    RfArgs f{};
    f.W = g.W; f.H = g.H; f.radius = r.radius; f.max_row_edges = r.max_row_edges; f.k = k_region; f.keep_all = r.keep_all ? 1 : 0;
    f.deg = w.deg; f.st_key = w.st_key; f.st_score = w.st_score; f.st_weight = w.st_weight;
    f.status = reinterpret_cast<unsigned long long*>(r.status);
    RsArgs sr{};
    sr.propagate = r.propagate; sr.explore = r.explore; sr.seed = r.seed; sr.Lw = g.Lw; sr.k_region = k_region; sr.staged = staged;
    RsHeads hd{};
    for (int h = 0; h < 4; ++h) {
        hd.wq[h] = st.wq4[h]; hd.x[h] = st.x4[h]; hd.tau[h] = st.tau4 ? st.tau4[h] : nullptr; hd.b2p[h] = agg ? st.b2p4[h] : nullptr;
    }
    GaArgs v{};
    if (agg) {
        v = ga_map_args(B, g, st.b2p4[0], nullptr, nullptr, nullptr, 0);
        v.out = w.agg;
    }
    const bool wave = rf_wave_rows(r);
    for (int row0 = 0; row0 < n_rows; row0 += head_launches ? head_rows : n_rows) {
        const int rows = head_launches ? head_rows : n_rows;
        if (agg) launch_stage_search_rows<true>(s, rows, wave, a, f, v, sr, hd, head_rows, row0);
        else launch_stage_search_rows<false>(s, rows, wave, a, f, v, sr, hd, head_rows, row0);
        DAGL_LAUNCH_CHECK("graph_stage_search_rows_kernel");
    }
    if (graph) {
        const int rc = launch_row_scan(s, n_rows, w.deg, r.row_off_out);
        if (rc) return rc;
        hipLaunchKernelGGL(graph_search_compact_kernel, dim3((unsigned)((n_rows + RF_COPY_ROWS - 1) / RF_COPY_ROWS)), dim3(RF_COPY_ROWS * 64), 0,
                           s, n_rows, w2, (long long)r.c.E, sr, r.c.row_off, w.deg, r.row_off_out, w.st_key, w.st_score, w.st_weight,
                           r.key_out, r.weight_out, r.score_out, (long long)r.capacity);
        DAGL_LAUNCH_CHECK("graph_search_compact_kernel");
    }
    return agg ? launch_stage_fold_mix(s, B, g, w.agg, st.x, st.mix_w, st.mix_b, r.out) : DAGL_OK;
}

static int refresh_shape_ok(const char* who, int B, int H, int W, int64_t total_edges, int radius) {
    int rc = graph_dims_ok(who, B, H, W);
    if (rc) return rc;
    DAGL_REQUIRE(radius >= 0 && radius <= RF_MAX_RADIUS, "%s: radius=%d outside [0, %d]", who, radius, RF_MAX_RADIUS);
    if ((rc = graph_edges_ok(who, total_edges))) return rc;
    const int64_t w2 = (int64_t)(2 * radius + 1) * (2 * radius + 1);
    DAGL_REQUIRE(total_edges * w2 < (1ll << 31), "%s: total_edges (2 radius + 1)^2 = %lld staged candidates, 2^31 or more", who,
                 (long long)(total_edges * w2));
    return DAGL_OK;
}

// what the SEARCH entries add to the refusals (both 0: the plain refresh)
static int search_args_ok(const char* who, int propagate, int explore) {
    DAGL_REQUIRE(propagate == 0 || propagate == 1, "%s: propagate=%d, expected 0 or 1", who, propagate);
    DAGL_REQUIRE(explore >= 0 && explore <= RS_MAX_EXPLORE, "%s: explore=%d outside [0, %d]", who, explore, RS_MAX_EXPLORE);
    return DAGL_OK;
}

// the checks and the call of the refresh, step and search entries.  b2p / out null: the refresh.  Else the step, where the four graph outputs may all be null
// (the output alone: capacity_edges is not looked at)
static int graph_refresh_entry(const char* who, void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                               const int64_t* row_off, const int32_t* key, int64_t total_edges, int max_row_edges, int radius,
                               const float* tau, int k, float scale, int flags, float* out, int64_t* row_off_out, int32_t* key_out,
                               float* weight_out, float* score_out, int64_t capacity_edges, int64_t* status_out, void* workspace,
                               size_t ws_bytes, bool step, int propagate = 0, int explore = 0, uint32_t seed = 0) {
    int rc = refresh_shape_ok(who, B, H, W, total_edges, radius);
    if (rc) return rc;
    if ((rc = search_args_ok(who, propagate, explore))) return rc;
    const bool search = propagate || explore;
    const bool graph = !step || row_off_out || key_out || weight_out || score_out;
    const bool outputs = status_out && (!graph || (row_off_out && ((total_edges == 0 && !explore) || (key_out && weight_out && score_out))));
    if ((rc = graph_operands_ok(who, wq_rows, x_rows, row_off, key, total_edges, scale, flags, outputs,
                                DAGL_GRAPH_REFRESH_KEEP_ALL | DAGL_GRAPH_REFRESH_BLOCK_ROWS)))
        return rc;
    if (step) {
        DAGL_REQUIRE(b2p && out, "%s: null tensor pointer", who);
        DAGL_REQUIRE(((uintptr_t)b2p % 16) == 0, "%s: b2p must be 16-byte aligned", who);
    }
    DAGL_REQUIRE(k >= 0, "%s: k=%d < 0", who, k);
    DAGL_REQUIRE(max_row_edges >= 0, "%s: max_row_edges=%d < 0", who, max_row_edges);
    const int64_t w2 = (int64_t)(2 * radius + 1) * (2 * radius + 1);
    if ((int64_t)max_row_edges * w2 > RF_CAP) {
        set_error("%s: max_row_edges (2 radius + 1)^2 = %lld candidates per row, more than the %d a row may expand into", who,
                  (long long)((int64_t)max_row_edges * w2), RF_CAP);
        return DAGL_ERR_UNSUPPORTED;
    }
    if (search && rf_row_bound(max_row_edges, radius, propagate, explore) > RF_CAP) {
        set_error("%s: (1 + 4 propagate) max_row_edges (2 radius + 1)^2 + explore = %lld candidates per row, more than the %d a row may "
                  "expand into", who, rf_row_bound(max_row_edges, radius, propagate, explore), RF_CAP);
        return DAGL_ERR_UNSUPPORTED;
    }
    const Grid g = make_grid(H, W);
    const bool keep_all = (flags & DAGL_GRAPH_REFRESH_KEEP_ALL) != 0;
    // what the call may produce: the raw bound, or B L k under a rank cut where that is smaller; SEARCH without a rank cut: the
    // staging bound (the same number)
    int64_t may = rf_staged((int64_t)B * g.L, total_edges, radius, propagate, explore, 0);
    if (!keep_all && k > 0 && (int64_t)B * g.L * k < may) may = (int64_t)B * g.L * k;
    if (graph && capacity_edges < may) {
        set_error("%s: capacity %lld edges < the %lld this call may produce", who, (long long)capacity_edges, (long long)may);
        return DAGL_ERR_WORKSPACE;
    }
    const size_t need = refresh_carve(nullptr, (size_t)B * g.L,
                                      (size_t)rf_staged((int64_t)B * g.L, total_edges, radius, propagate, explore, keep_all ? 0 : k), step,
                                      graph).bytes;
    if ((rc = check_workspace(who, workspace, ws_bytes, need))) return rc;
    RefreshCall r{};
    r.c = graph_attend_call(wq_rows, x_rows, row_off, key, total_edges, tau, scale, flags);
    r.max_row_edges = max_row_edges; r.radius = radius; r.k = k; r.keep_all = keep_all;
    r.block_rows = (flags & DAGL_GRAPH_REFRESH_BLOCK_ROWS) != 0;
    r.row_off_out = graph ? row_off_out : nullptr; r.key_out = key_out; r.weight_out = weight_out; r.score_out = score_out;
    r.capacity = capacity_edges; r.status = status_out; r.b2p = b2p; r.out = out;
    r.search = search; r.propagate = propagate; r.explore = explore; r.seed = seed;
    return launch_graph_refresh((hipStream_t)stream, B, g, r, workspace);
}

// a stage holds four heads of B images: its rows are those of 4 B images
static int stage_shape_ok(const char* who, int B, int H, int W, int64_t total_edges, int radius) {
    int rc = graph_dims_ok(who, B, H, W);
    if (rc) return rc;
    DAGL_REQUIRE((int64_t)4 * B * H * W < (1ll << 30), "%s: batch too large for 32-bit row ids", who);
    return refresh_shape_ok(who, 4 * B, H, W, total_edges, radius);
}

static int stage_mix_operands_ok(const char* who, const float* x, const float* mix_w, const float* mix_b, const float* out) {
    DAGL_REQUIRE(x && mix_w && mix_b && out, "%s: null tensor pointer", who);
    return DAGL_OK;
}

// the checks and the call of the stage search entries.  step: b2p4, x, mix_w, mix_b and out are given, and the four graph outputs may all
// be null (the output alone: capacity_edges is not looked at)
static int graph_stage_search_entry(const char* who, void* stream, int B, int H, int W, const float* const* wq_rows4,
                                    const float* const* x_rows4, const float* const* b2p4, const int64_t* row_off, const int32_t* key,
                                    int64_t total_edges, int max_row_edges, int radius, const float* const* tau4, int k, float scale,
                                    int flags, const float* x, const float* mix_w, const float* mix_b, float* out, int64_t* row_off_out,
                                    int32_t* key_out, float* weight_out, float* score_out, int64_t capacity_edges, int64_t* status_out,
                                    void* workspace, size_t ws_bytes, bool step, int propagate, int explore, uint32_t seed) {
    int rc = stage_shape_ok(who, B, H, W, total_edges, radius);
    if (rc) return rc;
    if ((rc = search_args_ok(who, propagate, explore))) return rc;
    DAGL_REQUIRE(wq_rows4 && x_rows4 && (!step || b2p4), "%s: null pointer table", who);
    const bool graph = !step || row_off_out || key_out || weight_out || score_out;
    const bool outputs = status_out && (!graph || (row_off_out && ((total_edges == 0 && !explore) || (key_out && weight_out && score_out))));
    int with_tau = 0;
    for (int h = 0; h < 4; ++h) {
        if ((rc = graph_operands_ok(who, wq_rows4[h], x_rows4[h], row_off, key, total_edges, scale, flags, outputs && (!step || b2p4[h]),
                                    DAGL_GRAPH_REFRESH_KEEP_ALL | DAGL_GRAPH_REFRESH_BLOCK_ROWS | DAGL_GRAPH_STAGE_SEARCH_HEAD_LAUNCHES)))
            return rc;
        if (step) DAGL_REQUIRE(((uintptr_t)b2p4[h] % 16) == 0, "%s: b2p must be 16-byte aligned", who);
        with_tau += tau4 && tau4[h];
    }
    DAGL_REQUIRE(with_tau == 0 || with_tau == 4, "%s: tau given for %d of the four heads (all or none)", who, with_tau);
    if (step && (rc = stage_mix_operands_ok(who, x, mix_w, mix_b, out))) return rc;
    DAGL_REQUIRE(k >= 0, "%s: k=%d < 0", who, k);
    DAGL_REQUIRE(max_row_edges >= 0, "%s: max_row_edges=%d < 0", who, max_row_edges);
    if (rf_row_bound(max_row_edges, radius, propagate, explore) > RF_CAP) {
        set_error("%s: (1 + 4 propagate) max_row_edges (2 radius + 1)^2 + explore = %lld candidates per row, more than the %d a row may "
                  "expand into", who, rf_row_bound(max_row_edges, radius, propagate, explore), RF_CAP);
        return DAGL_ERR_UNSUPPORTED;
    }
    const Grid g = make_grid(H, W);
    const int64_t n_rows = (int64_t)4 * B * g.L;
    const bool keep_all = (flags & DAGL_GRAPH_REFRESH_KEEP_ALL) != 0;
    int64_t may = rf_staged(n_rows, total_edges, radius, propagate, explore, 0);
    if (!keep_all && k > 0 && n_rows * k < may) may = n_rows * k;
    if (graph && capacity_edges < may) {
        set_error("%s: capacity %lld edges < the %lld this call may produce", who, (long long)capacity_edges, (long long)may);
        return DAGL_ERR_WORKSPACE;
    }
    const size_t need = refresh_carve(nullptr, (size_t)n_rows,
                                      (size_t)rs_stage_staged(n_rows, total_edges, radius, propagate, explore, keep_all ? 0 : k), step,
                                      graph).bytes;
    if ((rc = check_workspace(who, workspace, ws_bytes, need))) return rc;
    RefreshCall r{};
    r.c = graph_attend_call(nullptr, nullptr, row_off, key, total_edges, nullptr, scale, flags);
    r.max_row_edges = max_row_edges; r.radius = radius; r.k = k; r.keep_all = keep_all;
    r.block_rows = (flags & DAGL_GRAPH_REFRESH_BLOCK_ROWS) != 0;
    r.row_off_out = graph ? row_off_out : nullptr; r.key_out = key_out; r.weight_out = weight_out; r.score_out = score_out;
    r.capacity = capacity_edges; r.status = status_out; r.out = step ? out : nullptr;
    r.search = true; r.propagate = propagate; r.explore = explore; r.seed = seed;
    const StageStepCall st{wq_rows4, x_rows4, step ? b2p4 : nullptr, with_tau ? tau4 : nullptr, x, mix_w, mix_b};
    return launch_graph_stage_search((hipStream_t)stream, B, g, r, st, workspace, (flags & DAGL_GRAPH_STAGE_SEARCH_HEAD_LAUNCHES) != 0);
}

// ---- the fixed-width step (dagl_graph_step_fixed) ----------------------------------------------------------------------------------
struct FixedCall {
    GraphAttendCall c;                        // row_off null, key = key_in, E = B L width_in
    const int32_t* deg_in; int width_in, width_out, radius, k; bool keep_all, block_rows;
    int propagate, explore; uint32_t seed;
    const float* b2p; float* out;             // both null: the refresh alone
    int32_t* key_out; float* weight_out; float* score_out; int32_t* deg_out; int64_t* status;
};

#define DAGL_FIXED_LAUNCH(kernel, ...)                                                                                          \
    do {                                                                                                                        \
        if (wave) hipLaunchKernelGGL((kernel<64, RF_WAVE_CAP>), dim3((unsigned)n_rows), dim3(64), 0, s, __VA_ARGS__);           \
        else hipLaunchKernelGGL((kernel<256, RF_CAP>), dim3((unsigned)n_rows), dim3(256), 0, s, __VA_ARGS__);                   \
        DAGL_LAUNCH_CHECK(#kernel);                                                                                             \
    } while (0)

// one row launch (every row leaves whole, also from an empty input: nothing to clear, no count to know), then the fold
static int launch_graph_step_fixed(hipStream_t s, int B, const Grid& g, const FixedCall& r, void* workspace) {
    const int n_rows = B * g.L;
    const bool agg = r.out != nullptr, search = r.propagate || r.explore;
    DAGL_HIP_TRY(hipMemsetAsync(r.status, 0, 2 * sizeof(int64_t), s));
    const RefreshWs w = refresh_carve(workspace, (size_t)n_rows, 0, agg, false);
    const GtArgs a = gt_args(B, g, r.c);
    RfArgs f{};
    f.W = g.W; f.H = g.H; f.radius = r.radius; f.max_row_edges = r.width_in; f.k = r.keep_all ? 0 : r.k; f.keep_all = r.keep_all ? 1 : 0;
    f.deg = r.deg_out; f.st_key = r.key_out; f.st_score = r.score_out; f.st_weight = r.weight_out;
    f.status = reinterpret_cast<unsigned long long*>(r.status);
    const RxArgs fx{r.deg_in, r.width_in, r.width_out};
    RsArgs sr{};
    sr.propagate = r.propagate; sr.explore = r.explore; sr.seed = r.seed; sr.Lw = g.Lw;
    GaArgs v{};
    if (agg) {
        v = ga_map_args(B, g, r.b2p, nullptr, nullptr, nullptr, 0);
        v.out = w.agg;
    }
    const bool wave = !r.block_rows && rf_row_bound(r.width_in, r.radius, r.propagate, r.explore) <= RF_WAVE_CAP;
    if (search && agg) DAGL_FIXED_LAUNCH(graph_fixed_search_step_rows_kernel, a, f, v, sr, fx);
    else if (search) DAGL_FIXED_LAUNCH(graph_fixed_search_rows_kernel, a, f, sr, fx);
    else if (agg) DAGL_FIXED_LAUNCH(graph_fixed_step_rows_kernel, a, f, v, fx);
    else DAGL_FIXED_LAUNCH(graph_fixed_rows_kernel, a, f, fx);
    return agg ? launch_fold(s, B, g, w.agg, r.out) : DAGL_OK;
}
#undef DAGL_FIXED_LAUNCH

template <bool AGG, bool SEARCH>
static void launch_stage_fixed_rows(hipStream_t s, int n_rows, bool wave, const GtArgs& a, const RfArgs& f, const GaArgs& v, const RsArgs& sr,
                                    const RxArgs& fx, const RsHeads& hd, int head_rows) {
    if (wave) {
        hipLaunchKernelGGL((graph_stage_fixed_rows_kernel<64, RF_WAVE_CAP, AGG, SEARCH>), dim3((unsigned)n_rows), dim3(64), 0, s, a, f, v, sr,
                           fx, hd, head_rows);
    } else {
        hipLaunchKernelGGL((graph_stage_fixed_rows_kernel<256, RF_CAP, AGG, SEARCH>), dim3((unsigned)n_rows), dim3(256), 0, s, a, f, v, sr,
                           fx, hd, head_rows);
    }
}

// The fixed-width step of a whole CES stage (dagl_graph_stage_step_fixed): r's slot arrays and degrees run over the 4 B L head-major
// rows, st holds the heads' operands (st.b2p4 / r.out null: the graph alone).  The status words, ONE row launch
// (graph_stage_fixed_rows_kernel: every row leaves whole, nothing to clear), then the fold + mix + residual of the four heads' rows
static int launch_graph_stage_step_fixed(hipStream_t s, int B, const Grid& g, const FixedCall& r, const StageStepCall& st, void* workspace) {
    const int head_rows = B * g.L, n_rows = 4 * head_rows;
    const bool agg = r.out != nullptr, search = r.propagate || r.explore;
    DAGL_HIP_TRY(hipMemsetAsync(r.status, 0, 2 * sizeof(int64_t), s));
    const RefreshWs w = refresh_carve(workspace, (size_t)n_rows, 0, agg, false);
    GraphAttendCall c = r.c;
    c.wq_rows = st.wq4[0]; c.x_rows = st.x4[0];                  // (the kernel takes every head's from the table)
    const GtArgs a = gt_args(4 * B, g, c);                       // n_rows = 4 B L
    RfArgs f{};
    f.W = g.W; f.H = g.H; f.radius = r.radius; f.max_row_edges = r.width_in; f.k = r.keep_all ? 0 : r.k; f.keep_all = r.keep_all ? 1 : 0;
    f.deg = r.deg_out; f.st_key = r.key_out; f.st_score = r.score_out; f.st_weight = r.weight_out;
    f.status = reinterpret_cast<unsigned long long*>(r.status);
    const RxArgs fx{r.deg_in, r.width_in, r.width_out};
    RsArgs sr{};
    sr.propagate = r.propagate; sr.explore = r.explore; sr.seed = r.seed; sr.Lw = g.Lw;
    RsHeads hd{};
    for (int h = 0; h < 4; ++h) {
        hd.wq[h] = st.wq4[h]; hd.x[h] = st.x4[h]; hd.tau[h] = st.tau4 ? st.tau4[h] : nullptr; hd.b2p[h] = agg ? st.b2p4[h] : nullptr;
    }
    GaArgs v{};
    if (agg) {
        v = ga_map_args(B, g, st.b2p4[0], nullptr, nullptr, nullptr, 0);      // (L, the map geometry: a head's; src from the table)
        v.out = w.agg;
    }
    const bool wave = !r.block_rows && rf_row_bound(r.width_in, r.radius, r.propagate, r.explore) <= RF_WAVE_CAP;
    if (search && agg) launch_stage_fixed_rows<true, true>(s, n_rows, wave, a, f, v, sr, fx, hd, head_rows);
    else if (search) launch_stage_fixed_rows<false, true>(s, n_rows, wave, a, f, v, sr, fx, hd, head_rows);
    else if (agg) launch_stage_fixed_rows<true, false>(s, n_rows, wave, a, f, v, sr, fx, hd, head_rows);
    else launch_stage_fixed_rows<false, false>(s, n_rows, wave, a, f, v, sr, fx, hd, head_rows);
    DAGL_LAUNCH_CHECK("graph_stage_fixed_rows_kernel");
    return agg ? launch_stage_fold_mix(s, B, g, w.agg, st.x, st.mix_w, st.mix_b, r.out) : DAGL_OK;
}

static bool ranges_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + qn && b < a + pn;
}

// the checks and the call of the fixed-width entries, written once.  heads = 1: dagl_graph_step_fixed -- the tables hold one pointer,
// mix_x / mix_w / mix_b are not looked at; heads = 4: dagl_graph_stage_step_fixed -- the slot arrays run over the 4 B L head-major rows.
// b2p / out null: the graph alone.  tau: null, or a table (heads = 4: set for all the heads or for none)
static int graph_fixed_entry(const char* who, void* stream, int heads, int B, int H, int W, const float* const* wq, const float* const* x,
                             const float* const* b2p, const int32_t* key_in, const int32_t* deg_in, int width_in, int radius,
                             const float* const* tau, int k, float scale, int flags, int propagate, int explore, uint32_t seed,
                             const float* mix_x, const float* mix_w, const float* mix_b, float* out, int32_t* key_out, float* weight_out,
                             float* score_out, int32_t* deg_out, int width_out, int64_t* status, void* workspace, size_t workspace_bytes) {
    const bool stage = heads == 4;
    int rc = graph_dims_ok(who, B, H, W);
    if (rc) return rc;
    if (stage) DAGL_REQUIRE((int64_t)4 * B * H * W < (1ll << 30), "%s: batch too large for 32-bit row ids", who);
    DAGL_REQUIRE(radius >= 0 && radius <= RF_MAX_RADIUS, "%s: radius=%d outside [0, %d]", who, radius, RF_MAX_RADIUS);
    DAGL_REQUIRE(width_in >= 1 && width_out >= 1, "%s: width_in=%d, width_out=%d: each at least 1", who, width_in, width_out);
    const Grid g = make_grid(H, W);
    const int64_t n_rows = (int64_t)heads * B * g.L;
    DAGL_REQUIRE(n_rows * width_in < (1ll << 31) && n_rows * width_out < (1ll << 31), "%s: %sB L width = %lld slots, 2^31 or more", who,
                 stage ? "4 " : "", (long long)(n_rows * (width_in > width_out ? width_in : width_out)));
    if ((rc = search_args_ok(who, propagate, explore))) return rc;
    if (stage) {
        DAGL_REQUIRE(wq && x, "%s: null pointer table", who);
        const int given = (b2p != nullptr) + (mix_x != nullptr) + (mix_w != nullptr) + (mix_b != nullptr) + (out != nullptr);
        DAGL_REQUIRE(given == 0 || given == 5, "%s: b2p4, x, mix_w, mix_b and out come together (all null: the graph alone)", who);
    } else {
        DAGL_REQUIRE((b2p == nullptr) == (out == nullptr), "%s: b2p and out come together (both null: the refresh alone)", who);
    }
    const bool step = out != nullptr;
    static const int64_t no_offsets = 0;      // (the shared null test asks for offsets; this form has none)
    int with_tau = 0;
    for (int h = 0; h < heads; ++h) {
        if ((rc = graph_operands_ok(who, wq[h], x[h], &no_offsets, key_in, n_rows * width_in, scale, flags,
                                    deg_in && key_out && weight_out && score_out && deg_out && status && (!step || b2p[h]),
                                    DAGL_GRAPH_REFRESH_KEEP_ALL | DAGL_GRAPH_REFRESH_BLOCK_ROWS)))
            return rc;
        if (step) DAGL_REQUIRE(((uintptr_t)b2p[h] % 16) == 0, "%s: b2p must be 16-byte aligned", who);
        with_tau += tau && tau[h];
    }
    DAGL_REQUIRE(with_tau == 0 || with_tau == heads, "%s: tau given for %d of the four heads (all or none)", who, with_tau);
    if (stage && step && (rc = stage_mix_operands_ok(who, mix_x, mix_w, mix_b, out))) return rc;
    DAGL_REQUIRE(k >= 0, "%s: k=%d < 0", who, k);
    const bool keep_all = (flags & DAGL_GRAPH_REFRESH_KEEP_ALL) != 0;
    if (k > 0 && !keep_all) {
        const int most = k < g.N ? k : g.N;
        DAGL_REQUIRE(width_out >= most, "%s: width_out=%d < min(k, N) = %d entries a row may keep", who, width_out, most);
    }
    if (rf_row_bound(width_in, radius, propagate, explore) > RF_CAP) {
        set_error("%s: (1 + 4 propagate) width_in (2 radius + 1)^2 + explore = %lld candidates per row, more than the %d a row may "
                  "expand into", who, rf_row_bound(width_in, radius, propagate, explore), RF_CAP);
        return DAGL_ERR_UNSUPPORTED;
    }
    {
        // every output array against every input array (every head's; the stage's mix operands too)
        const size_t rows = (size_t)n_rows, head_rows = (size_t)B * g.L;
        const void* in_p[4 * 4 + 5];
        size_t in_n[4 * 4 + 5];
        int n_in = 0;
        for (int h = 0; h < heads; ++h) {
            in_p[n_in] = wq[h]; in_n[n_in++] = head_rows * D * sizeof(float);
            in_p[n_in] = x[h]; in_n[n_in++] = (size_t)B * g.N * D * sizeof(float);
            in_p[n_in] = step ? b2p[h] : nullptr; in_n[n_in++] = (size_t)B * g.Hp * g.Wp * CH * sizeof(float);
            in_p[n_in] = with_tau ? tau[h] : nullptr; in_n[n_in++] = head_rows * sizeof(float);
        }
        in_p[n_in] = key_in; in_n[n_in++] = rows * width_in * sizeof(int32_t);
        in_p[n_in] = deg_in; in_n[n_in++] = rows * sizeof(int32_t);
        if (stage) {
            in_p[n_in] = mix_x; in_n[n_in++] = (size_t)B * 4 * CH * g.N * sizeof(float);
            in_p[n_in] = mix_w; in_n[n_in++] = (size_t)(4 * CH) * (4 * CH) * sizeof(float);
            in_p[n_in] = mix_b; in_n[n_in++] = (size_t)(4 * CH) * sizeof(float);
        }
        const void* out_p[5] = {out, key_out, weight_out, score_out, deg_out};
        const size_t out_n[5] = {(size_t)B * heads * CH * g.N * sizeof(float), rows * width_out * sizeof(int32_t),
                                 rows * width_out * sizeof(float), rows * width_out * sizeof(float), rows * sizeof(int32_t)};
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < n_in; ++j)
                DAGL_REQUIRE(!ranges_overlap(out_p[i], out_n[i], in_p[j], in_n[j]), "%s: an output array overlaps an input array", who);
    }
    const size_t need = refresh_carve(nullptr, (size_t)n_rows, 0, step, false).bytes;
    if (need > 0 && (rc = check_workspace(who, workspace, workspace_bytes, need))) return rc;
    FixedCall r{};
    r.c = graph_attend_call(wq[0], x[0], nullptr, key_in, n_rows * width_in, with_tau ? tau[0] : nullptr, scale, flags);
    r.deg_in = deg_in; r.width_in = width_in; r.width_out = width_out; r.radius = radius; r.k = k; r.keep_all = keep_all;
    r.block_rows = (flags & DAGL_GRAPH_REFRESH_BLOCK_ROWS) != 0;
    r.propagate = propagate; r.explore = explore; r.seed = seed; r.b2p = step ? b2p[0] : nullptr; r.out = out;
    r.key_out = key_out; r.weight_out = weight_out; r.score_out = score_out; r.deg_out = deg_out; r.status = status;
    if (!stage) return launch_graph_step_fixed((hipStream_t)stream, B, g, r, workspace);
    const StageStepCall st{wq, x, step ? b2p : nullptr, with_tau ? tau : nullptr, mix_x, mix_w, mix_b};
    return launch_graph_stage_step_fixed((hipStream_t)stream, B, g, r, st, workspace);
}

}  // namespace dagl

using namespace dagl;

extern "C" {

int dagl_graph_refresh_max_candidates(void) { return RF_CAP; }

size_t dagl_graph_refresh_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius) {
    if (refresh_shape_ok("dagl_graph_refresh_workspace_bytes", B, H, W, total_edges, radius)) return 0;
    return refresh_carve(nullptr, (size_t)B * make_grid(H, W).L, (size_t)total_edges * (2 * radius + 1) * (2 * radius + 1)).bytes;
}

int dagl_graph_refresh(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const int64_t* row_off,
                       const int32_t* key, int64_t total_edges, int max_row_edges, int radius, const float* tau, int k, float scale,
                       int flags, int64_t* row_off_out, int32_t* key_out, float* weight_out, float* score_out, int64_t capacity_edges,
                       int64_t* status_out, void* workspace, size_t ws_bytes) {
    return graph_refresh_entry("dagl_graph_refresh", stream, B, H, W, wq_rows, x_rows, nullptr, row_off, key, total_edges, max_row_edges,
                               radius, tau, k, scale, flags, nullptr, row_off_out, key_out, weight_out, score_out, capacity_edges,
                               status_out, workspace, ws_bytes, false);
}

// the refresh and the block's output on its result in one call (no ABI bump: found by symbol)
size_t dagl_graph_step_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius, int want_graph) {
    if (refresh_shape_ok("dagl_graph_step_workspace_bytes", B, H, W, total_edges, radius)) return 0;
    return refresh_carve(nullptr, (size_t)B * make_grid(H, W).L, (size_t)total_edges * (2 * radius + 1) * (2 * radius + 1), true,
                         want_graph != 0).bytes;
}

int dagl_graph_step(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p, const int64_t* row_off,
                    const int32_t* key, int64_t total_edges, int max_row_edges, int radius, const float* tau, int k, float scale, int flags,
                    float* out, int64_t* row_off_out, int32_t* key_out, float* weight_out, float* score_out, int64_t capacity_edges,
                    int64_t* status_out, void* workspace, size_t ws_bytes) {
    return graph_refresh_entry("dagl_graph_step", stream, B, H, W, wq_rows, x_rows, b2p, row_off, key, total_edges, max_row_edges, radius,
                               tau, k, scale, flags, out, row_off_out, key_out, weight_out, score_out, capacity_edges, status_out,
                               workspace, ws_bytes, true);
}

// the search step on a patch graph: the refresh / the step with the adjacent queries' edges and random keys as further candidate
// sources (no ABI bump: found by symbol).  propagate = explore = 0: the plain entries' launches, workspace and bits
size_t dagl_graph_search_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius, int propagate, int explore, int k,
                                         int want_graph, int aggregate) {
    const char* who = "dagl_graph_search_workspace_bytes";
    if (refresh_shape_ok(who, B, H, W, total_edges, radius) || search_args_ok(who, propagate, explore)) return 0;
    if (k < 0) { set_error("%s: k=%d < 0", who, k); return 0; }
    const int64_t n_rows = (int64_t)B * make_grid(H, W).L;
    return refresh_carve(nullptr, (size_t)n_rows, (size_t)rf_staged(n_rows, total_edges, radius, propagate, explore, k), aggregate != 0,
                         want_graph != 0 || aggregate == 0).bytes;
}

int dagl_graph_search(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const int64_t* row_off,
                      const int32_t* key, int64_t total_edges, int max_row_edges, int radius, const float* tau, int k, float scale,
                      int flags, int64_t* row_off_out, int32_t* key_out, float* weight_out, float* score_out, int64_t capacity_edges,
                      int64_t* status_out, void* workspace, size_t ws_bytes, int propagate, int explore, uint32_t seed) {
    return graph_refresh_entry("dagl_graph_search", stream, B, H, W, wq_rows, x_rows, nullptr, row_off, key, total_edges, max_row_edges,
                               radius, tau, k, scale, flags, nullptr, row_off_out, key_out, weight_out, score_out, capacity_edges,
                               status_out, workspace, ws_bytes, false, propagate, explore, seed);
}

int dagl_graph_search_step(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                           const int64_t* row_off, const int32_t* key, int64_t total_edges, int max_row_edges, int radius,
                           const float* tau, int k, float scale, int flags, float* out, int64_t* row_off_out, int32_t* key_out,
                           float* weight_out, float* score_out, int64_t capacity_edges, int64_t* status_out, void* workspace,
                           size_t ws_bytes, int propagate, int explore, uint32_t seed) {
    return graph_refresh_entry("dagl_graph_search_step", stream, B, H, W, wq_rows, x_rows, b2p, row_off, key, total_edges, max_row_edges,
                               radius, tau, k, scale, flags, out, row_off_out, key_out, weight_out, score_out, capacity_edges, status_out,
                               workspace, ws_bytes, true, propagate, explore, seed);
}

// the fold + 1x1 mix + residual of a CES stage from its four heads' aggregated rows, on its own (no ABI bump: found by symbol)
int dagl_ces_stage_fold_mix(void* stream, int B, int H, int W, const float* agg, const float* x, const float* mix_w, const float* mix_b,
                            float* out) {
    const char* who = "dagl_ces_stage_fold_mix";
    int rc = graph_dims_ok(who, B, H, W);
    if (rc) return rc;
    DAGL_REQUIRE((int64_t)4 * B * H * W < (1ll << 30), "%s: batch too large for 32-bit row ids", who);
    DAGL_REQUIRE(agg != nullptr, "%s: null tensor pointer", who);
    if ((rc = stage_mix_operands_ok(who, x, mix_w, mix_b, out))) return rc;
    DAGL_REQUIRE(((uintptr_t)agg % 16) == 0, "%s: agg must be 16-byte aligned", who);
    return launch_stage_fold_mix((hipStream_t)stream, B, make_grid(H, W), agg, x, mix_w, mix_b, out);
}

// the launch dagl_ces_stage_fold_mix saves, on its own: the mix + residual of a STORED concat map (stage_mix_kernel, what
// dagl_ces_stage_forward ends with) -- with dagl_fold_normalize on [4 B] rows in front, the two-launch form to measure against
int dagl_ces_stage_mix(void* stream, int B, int H, int W, const float* cat, const float* x, const float* mix_w, const float* mix_b,
                       float* out) {
    const char* who = "dagl_ces_stage_mix";
    int rc = graph_dims_ok(who, B, H, W);
    if (rc) return rc;
    DAGL_REQUIRE(B <= 65535, "%s: B=%d beyond the 65535 images of one launch", who, B);
    DAGL_REQUIRE(cat != nullptr, "%s: null tensor pointer", who);
    if ((rc = stage_mix_operands_ok(who, x, mix_w, mix_b, out))) return rc;
    return launch_stage_mix((hipStream_t)stream, B, H * W, cat, x, mix_w, mix_b, out);
}

// the step of a whole CES stage: four heads' rows in one CSR, one scan, one copy, the fused fold + mix (no ABI bump: found by symbol)
size_t dagl_graph_stage_step_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius, int want_graph) {
    if (stage_shape_ok("dagl_graph_stage_step_workspace_bytes", B, H, W, total_edges, radius)) return 0;
    return refresh_carve(nullptr, (size_t)4 * B * make_grid(H, W).L, (size_t)total_edges * (2 * radius + 1) * (2 * radius + 1), true,
                         want_graph != 0).bytes;
}

int dagl_graph_stage_step(void* stream, int B, int H, int W, const float* const* wq_rows4, const float* const* x_rows4,
                          const float* const* b2p4, const int64_t* row_off, const int32_t* key, int64_t total_edges, int max_row_edges,
                          int radius, const float* const* tau4, int k, float scale, int flags, const float* x, const float* mix_w,
                          const float* mix_b, float* out, int64_t* row_off_out, int32_t* key_out, float* weight_out, float* score_out,
                          int64_t capacity_edges, int64_t* status_out, void* workspace, size_t ws_bytes) {
    const char* who = "dagl_graph_stage_step";
    int rc = stage_shape_ok(who, B, H, W, total_edges, radius);
    if (rc) return rc;
    DAGL_REQUIRE(wq_rows4 && x_rows4 && b2p4, "%s: null pointer table", who);
    const bool graph = row_off_out || key_out || weight_out || score_out;
    const bool outputs = status_out && (!graph || (row_off_out && (total_edges == 0 || (key_out && weight_out && score_out))));
    int with_tau = 0;
    for (int h = 0; h < 4; ++h) {
        if ((rc = graph_operands_ok(who, wq_rows4[h], x_rows4[h], row_off, key, total_edges, scale, flags, outputs && b2p4[h],
                                    DAGL_GRAPH_REFRESH_KEEP_ALL | DAGL_GRAPH_REFRESH_BLOCK_ROWS)))
            return rc;
        DAGL_REQUIRE(((uintptr_t)b2p4[h] % 16) == 0, "%s: b2p must be 16-byte aligned", who);
        with_tau += tau4 && tau4[h];
    }
    DAGL_REQUIRE(with_tau == 0 || with_tau == 4, "%s: tau given for %d of the four heads (all or none)", who, with_tau);
    if ((rc = stage_mix_operands_ok(who, x, mix_w, mix_b, out))) return rc;
    DAGL_REQUIRE(k >= 0, "%s: k=%d < 0", who, k);
    DAGL_REQUIRE(max_row_edges >= 0, "%s: max_row_edges=%d < 0", who, max_row_edges);
    const int64_t w2 = (int64_t)(2 * radius + 1) * (2 * radius + 1);
    if ((int64_t)max_row_edges * w2 > RF_CAP) {
        set_error("%s: max_row_edges (2 radius + 1)^2 = %lld candidates per row, more than the %d a row may expand into", who,
                  (long long)((int64_t)max_row_edges * w2), RF_CAP);
        return DAGL_ERR_UNSUPPORTED;
    }
    const Grid g = make_grid(H, W);
    const bool keep_all = (flags & DAGL_GRAPH_REFRESH_KEEP_ALL) != 0;
    int64_t may = total_edges * w2;
    if (!keep_all && k > 0 && (int64_t)4 * B * g.L * k < may) may = (int64_t)4 * B * g.L * k;
    if (graph && capacity_edges < may) {
        set_error("%s: capacity %lld edges < the %lld this call may produce", who, (long long)capacity_edges, (long long)may);
        return DAGL_ERR_WORKSPACE;
    }
    const size_t need = refresh_carve(nullptr, (size_t)4 * B * g.L, (size_t)(total_edges * w2), true, graph).bytes;
    if ((rc = check_workspace(who, workspace, ws_bytes, need))) return rc;
    RefreshCall r{};
    r.c = graph_attend_call(nullptr, nullptr, row_off, key, total_edges, nullptr, scale, flags);
    r.max_row_edges = max_row_edges; r.radius = radius; r.k = k; r.keep_all = keep_all;
    r.block_rows = (flags & DAGL_GRAPH_REFRESH_BLOCK_ROWS) != 0;
    r.row_off_out = graph ? row_off_out : nullptr; r.key_out = key_out; r.weight_out = weight_out; r.score_out = score_out;
    r.capacity = capacity_edges; r.status = status_out; r.out = out;
    const StageStepCall st{wq_rows4, x_rows4, b2p4, with_tau ? tau4 : nullptr, x, mix_w, mix_b};
    return launch_graph_stage_step((hipStream_t)stream, B, g, r, st, workspace);
}

// the search step of a whole CES stage: the four heads' rows in one row launch (no ABI bump: found by symbol)
size_t dagl_graph_stage_search_workspace_bytes(int B, int H, int W, int64_t total_edges, int radius, int propagate, int explore, int k,
                                               int want_graph, int aggregate) {
    const char* who = "dagl_graph_stage_search_workspace_bytes";
    if (stage_shape_ok(who, B, H, W, total_edges, radius) || search_args_ok(who, propagate, explore)) return 0;
    if (k < 0) { set_error("%s: k=%d < 0", who, k); return 0; }
    const int64_t n_rows = (int64_t)4 * B * make_grid(H, W).L;
    return refresh_carve(nullptr, (size_t)n_rows, (size_t)rs_stage_staged(n_rows, total_edges, radius, propagate, explore, k),
                         aggregate != 0, want_graph != 0 || aggregate == 0).bytes;
}

int dagl_graph_stage_search(void* stream, int B, int H, int W, const float* const* wq_rows4, const float* const* x_rows4,
                            const int64_t* row_off, const int32_t* key, int64_t total_edges, int max_row_edges, int radius,
                            const float* const* tau4, int k, float scale, int flags, int64_t* row_off_out, int32_t* key_out,
                            float* weight_out, float* score_out, int64_t capacity_edges, int64_t* status_out, void* workspace,
                            size_t ws_bytes, int propagate, int explore, uint32_t seed) {
    return graph_stage_search_entry("dagl_graph_stage_search", stream, B, H, W, wq_rows4, x_rows4, nullptr, row_off, key, total_edges,
                                    max_row_edges, radius, tau4, k, scale, flags, nullptr, nullptr, nullptr, nullptr, row_off_out, key_out,
                                    weight_out, score_out, capacity_edges, status_out, workspace, ws_bytes, false, propagate, explore, seed);
}

int dagl_graph_stage_search_step(void* stream, int B, int H, int W, const float* const* wq_rows4, const float* const* x_rows4,
                                 const float* const* b2p4, const int64_t* row_off, const int32_t* key, int64_t total_edges,
                                 int max_row_edges, int radius, const float* const* tau4, int k, float scale, int flags, const float* x,
                                 const float* mix_w, const float* mix_b, float* out, int64_t* row_off_out, int32_t* key_out,
                                 float* weight_out, float* score_out, int64_t capacity_edges, int64_t* status_out, void* workspace,
                                 size_t ws_bytes, int propagate, int explore, uint32_t seed) {
    return graph_stage_search_entry("dagl_graph_stage_search_step", stream, B, H, W, wq_rows4, x_rows4, b2p4, row_off, key, total_edges,
                                    max_row_edges, radius, tau4, k, scale, flags, x, mix_w, mix_b, out, row_off_out, key_out, weight_out,
                                    score_out, capacity_edges, status_out, workspace, ws_bytes, true, propagate, explore, seed);
}

// the step on a fixed-width graph: one row launch, the graph output at a size known before the call (no ABI bump: found by symbol)
size_t dagl_graph_step_fixed_workspace_bytes(int B, int H, int W, int want_out) {
    if (graph_dims_ok("dagl_graph_step_fixed_workspace_bytes", B, H, W)) return 0;
    return refresh_carve(nullptr, (size_t)B * make_grid(H, W).L, 0, want_out != 0, false).bytes;
}

int dagl_graph_step_fixed(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2p,
                          const int32_t* key_in, const int32_t* deg_in, int width_in, int radius, const float* tau, int k, float scale,
                          int flags, int propagate, int explore, uint32_t seed, float* out, int32_t* key_out, float* weight_out,
                          float* score_out, int32_t* deg_out, int width_out, int64_t* status, void* workspace, size_t workspace_bytes) {
    return graph_fixed_entry("dagl_graph_step_fixed", stream, 1, B, H, W, &wq_rows, &x_rows, b2p ? &b2p : nullptr, key_in, deg_in, width_in,
                             radius, tau ? &tau : nullptr, k, scale, flags, propagate, explore, seed, nullptr, nullptr, nullptr, out, key_out,
                             weight_out, score_out, deg_out, width_out, status, workspace, workspace_bytes);
}

// the fixed-width step of a whole CES stage: the four heads' rows in ONE row launch, the fused fold + mix; no staging, scan, copy or
// host read, so the call with its graph output can be captured (no ABI bump: found by symbol)
size_t dagl_graph_stage_step_fixed_workspace_bytes(int B, int H, int W, int want_out) {
    const char* who = "dagl_graph_stage_step_fixed_workspace_bytes";
    if (graph_dims_ok(who, B, H, W)) return 0;
    if ((int64_t)4 * B * H * W >= (1ll << 30)) { set_error("%s: batch too large for 32-bit row ids", who); return 0; }
    return refresh_carve(nullptr, (size_t)4 * B * make_grid(H, W).L, 0, want_out != 0, false).bytes;
}

int dagl_graph_stage_step_fixed(void* stream, int B, int H, int W, const float* const* wq_rows4, const float* const* x_rows4,
                                const float* const* b2p4, const int32_t* key_in, const int32_t* deg_in, int width_in, int radius,
                                const float* const* tau4, int k, float scale, int flags, int propagate, int explore, uint32_t seed,
                                const float* x, const float* mix_w, const float* mix_b, float* out, int32_t* key_out, float* weight_out,
                                float* score_out, int32_t* deg_out, int width_out, int64_t* status, void* workspace,
                                size_t workspace_bytes) {
    return graph_fixed_entry("dagl_graph_stage_step_fixed", stream, 4, B, H, W, wq_rows4, x_rows4, b2p4, key_in, deg_in, width_in, radius,
                             tau4, k, scale, flags, propagate, explore, seed, x, mix_w, mix_b, out, key_out, weight_out, score_out, deg_out,
                             width_out, status, workspace, workspace_bytes);
}

}  // extern "C"
