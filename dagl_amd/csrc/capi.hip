// extern "C" boundary (include/dagl_ce.h) and the orchestration of one block forward.
#include <stdarg.h>
#include <string.h>

#include <atomic>

#include "dagl_common.h"
#include "thr_bias4.h"

namespace dagl {

static thread_local char g_err[512] = "";
// tags the calls of this process for the range guard (RangeTag): the only process-wide state of the library
static std::atomic<uint32_t> g_call_tag{1};
int32_t next_call_tag() {
    uint32_t t = g_call_tag.fetch_add(1, std::memory_order_relaxed) & 0x7fffffffu;
    return (int32_t)(t ? t : 1u);
}

// A call captured into a HIP graph carries its tag as a kernel argument: every replay has the SAME tag, and a sticky word that holds
// it (one replay left the fp16 range / was not served in-stream) would poison every later replay.  The first launch of a captured call
// therefore turns "this tag" into "some earlier call" -- still non-zero: the poll still reports it -- before the call's own kernels run.
constexpr int32_t STALE_TAG = 0x7ffffffe;
__global__ void retag_kernel(int32_t* word, int32_t* veto, int32_t tag) {
    if (word != nullptr && *word == tag) *word = STALE_TAG;
    if (veto != nullptr && *veto == tag) *veto = STALE_TAG;
}

// Top-k threshold policy words of a workspace (STAT_POLICY, STAT_GATE, STAT_OWNER).  A call that is not
// "prepared" (first call, another shape, a train / eval alternation) used to clear the policy: a module that alternates between
// two shapes forgot "tight" on every call and paid sampled pass + policy kernel + tight re-run each time.  The learnt word now
// survives as long as the workspace still carries the cookie of this very geometry (a fresh or re-used buffer does not).
__global__ void policy_init_kernel(int64_t* stats, int64_t cookie, int32_t start_tight) {
    if (stats[STAT_OWNER] != cookie) { stats[STAT_POLICY] = start_tight; stats[STAT_OWNER] = cookie; }
    // sticky "a DAGL_FLAG_NO_REDO call went unserved" -- only prepared (weights-packed) calls set or report it, and this kernel runs
    // on the non-prepared ones: cleared every time, so that a workspace handed on by torch's caching allocator, or shared by modules of
    // one shape (the cookie hashes the geometry, not the owner), cannot pass a stale bit to CE.range_ok()
    stats[STAT_NO_REDO_STICKY] = 0;
    stats[STAT_GATE] = 0;
}

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
    set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
    (void)hipGetLastError();
    return DAGL_ERR_HIP;
}

// 128 bytes of pinned host memory per calling thread for the small device->host read-backs (a pageable
// destination would make every hipMemcpyAsync a blocking staged copy).  Allocated once, never freed.
static int64_t* pinned_scratch() {
    static thread_local int64_t* p = nullptr;
    if (p == nullptr) {
        void* q = nullptr;
        if (hipHostMalloc(&q, 128, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        p = static_cast<int64_t*>(q);
    }
    return p;
}
static int read_back(hipStream_t s, const int64_t* dev, int n, int64_t* out) {
    int64_t* pin = pinned_scratch();
    int64_t* dst = pin ? pin : out;
    DAGL_HIP_TRY(hipMemcpyAsync(dst, dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DAGL_HIP_TRY(hipStreamSynchronize(s));
    if (pin) for (int i = 0; i < n; ++i) out[i] = pin[i];
    return DAGL_OK;
}

// Early verdict: the copy is queued behind the kernels that produce the words and followed by an event; the caller queues
// the rest of its launches and then waits for the EVENT only, so the device keeps working through the host round trip
// (a stream synchronise would drain it, and the next call's first kernels would start on an idle device).
static hipEvent_t verdict_event() {
    static thread_local hipEvent_t ev[16] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return nullptr; }
    if (ev[dev] == nullptr && hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError(); ev[dev] = nullptr;
    }
    return ev[dev];
}
static int read_back_begin(hipStream_t s, const int64_t* dev, int n, bool* pending) {
    int64_t* pin = pinned_scratch();
    hipEvent_t ev = pin ? verdict_event() : nullptr;
    *pending = false;
    if (ev == nullptr) return DAGL_OK;                      // no pinned memory / event: read_back_end synchronises the stream
    DAGL_HIP_TRY(hipMemcpyAsync(pin, dev, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DAGL_HIP_TRY(hipEventRecord(ev, s));
    *pending = true;
    return DAGL_OK;
}
static int read_back_end(hipStream_t s, const int64_t* dev, int n, bool pending, int64_t* out) {
    if (!pending) return read_back(s, dev, n, out);
    DAGL_HIP_TRY(hipEventSynchronize(verdict_event()));
    const int64_t* pin = pinned_scratch();
    for (int i = 0; i < n; ++i) out[i] = pin[i];
    return DAGL_OK;
}

// ---- optional stage profile: hipEvents recorded at stage boundaries on the caller's stream ------------------
struct Profile {
    int max_calls = 0, n_calls = 0;
    int only_stage = -1;                 // >= 0: record just the two events around that stage (an event record costs
                                         // ~4 us of stream time; nine per call are 12 % of a 256^2 forward)
    hipEvent_t* ev = nullptr;            // [max_calls][DAGL_N_STAGES + 1]
};
static inline void prof_mark(Profile* p, hipStream_t s, int stage_boundary) {
    if (p && p->n_calls < p->max_calls &&
        (p->only_stage < 0 || stage_boundary == p->only_stage || stage_boundary == p->only_stage + 1))
        (void)hipEventRecord(p->ev[(size_t)p->n_calls * (DAGL_N_STAGES + 1) + stage_boundary], s);
}

// ---- execution plan: chunking of the key stream + workspace carve ---------------------------------------
struct Plan {
    Grid g;
    int B, mode, k, kslots;
    bool screen;                    // bf16 screen + exact refine (default) vs. the all-fp32 scan
    bool split16;                   // fp16 split-operand projection (default) vs. the fp32 MFMA projection
    int splits, tiles_per_split, n_tiles;                 // fp32 scan (select.hip)
    int s_splits, s_steps_per_split, s_steps, s_sample, s_qblock;   // bf16 screen (screen.hip)
    int s_gkeep = 4;                                      // group maxima per (query, chunk, half) segment handed to the threshold kernel (ScreenArgs::gkeep)
    int capseg, capseg_alloc;
    int s_sample_tight = 0, capseg_tight = 0;             // top-k modes behind the screen: the tight threshold's pair (DAGL_FLAG_TIGHT_TOPK)
    bool pivot = false;                                   // the sampled threshold comes from the pivot keys (pivot.hip): regions laid out
    bool pivot_policy = false;                            // ... also for calls under the workspace's policy word (DAGL_FLAG_SAMPLED_TOPK: p.pivot alone)
    int pv_steps = 0, pv_steps_per_split = 0;             // 64-row steps of the pivot matrix, per image / per key chunk of the sampling launch
    int width;                      // neighbour-list width of the fixed-width paths
    int ovf_cap;                    // adaptive lists behind the screen: queries that may be redone one by one (overflow.hip)
    bool wide = false;              // top-k modes, k > DAGL_MAX_TOPK: row-wise dense form (topk_wide.hip), no lists
    size_t o_wide = 0;
    // byte offsets into the workspace
    size_t o_b1p, o_b2p, o_wp1, o_wp2, o_x, o_wq, o_xh, o_wqh, o_colsum, o_mt, o_cnt, o_segcnt, o_segoff, o_rowoff,
        o_deg, o_stats, o_lidx, o_lval, o_cidx, o_cval, o_nbidx, o_nbwgt, o_nbcnt, o_agg, o_gmax, o_rowsum, o_xp, o_pidx, o_theta, o_smax, o_traw, o_scand, o_spill, o_spillcnt,
        o_redo, o_ovflist, o_heavy, o_ovfq, o_ovfscores, o_ovfpart, o_thr, o_bias, o_thrpart, o_maphi, o_maplo, o_maphi2, o_maplo2, o_b1amax, o_wp1h, o_wp2h, o_convw, o_colpart, o_end;
};

static bool g_N_small(int H, int W);

constexpr int SCREEN_MIN_KEYS = 2048;     // below this the fp32 scan is launch-bound anyway
constexpr int SCREEN_CAPSEG = 16;
static bool g_N_small(int H, int W) { return (int64_t)H * W < SCREEN_MIN_KEYS; }

static int make_plan(int B, int H, int W, int mode_flags, int k, Plan& p, bool core = false) {
    p = Plan{};                     // (offsets of regions this plan does not carve stay 0)
    const int mode = mode_flags & 0xff;
    const bool exact = (mode_flags & DAGL_FLAG_EXACT_SCAN) != 0;
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1, "dagl: bad shape B=%d H=%d W=%d", B, H, W);
    DAGL_REQUIRE((mode_flags & ~(0xff | DAGL_FLAG_EXACT_SCAN | DAGL_FLAG_WEIGHTS_PACKED | DAGL_FLAG_DENSE_HINT | DAGL_FLAG_NO_WAIT | DAGL_FLAG_TIGHT_TOPK | DAGL_FLAG_SAMPLED_TOPK | DAGL_FLAG_NO_REDO)) == 0 &&
                 (mode == DAGL_MODE_ADAPTIVE || mode == DAGL_MODE_TOPK || mode == DAGL_MODE_ADAPTIVE_TOPK),
                 "dagl: unknown mode 0x%x", mode_flags);
    if (mode != DAGL_MODE_ADAPTIVE) DAGL_REQUIRE(k >= 1, "dagl: k=%d < 1", k);
    DAGL_REQUIRE((int64_t)H * W < (1ll << 30), "dagl: image too large");
    if (mode != DAGL_MODE_ADAPTIVE && (int64_t)k > (int64_t)H * W) k = H * W;     // top_k = min(num_edge, N), GReccR2b_3mh_1-checkpoint.py:243
    // neighbourhoods wider than the lists: every query in the row-wise dense form (inference entry points only)
    p.wide = mode != DAGL_MODE_ADAPTIVE && k > DAGL_MAX_TOPK;
    if (p.wide) DAGL_REQUIRE(!core, "dagl_ce_core_forward: k=%d > %d: the differentiable path keeps lists of at most %d neighbours", k,
                             DAGL_MAX_TOPK, DAGL_MAX_TOPK);
    p.g = make_grid(H, W);
    p.B = B; p.mode = mode; p.k = k;
    p.kslots = (mode == DAGL_MODE_ADAPTIVE || p.wide) ? 0 : topk_slots(k);
    const Grid& g = p.g;
    p.screen = !exact && !p.wide && g.N >= SCREEN_MIN_KEYS;
    p.split16 = !exact;
    p.n_tiles = (g.N + KT - 1) / KT;
    const int n_qgroups = (g.L + 127) / 128;
    // fp32 scan: enough blocks for ~4 per CU, chunks of at least 8 tiles, candidate merge bounded for top-k
    int splits = (1024 + n_qgroups * B - 1) / (n_qgroups * B);
    const int max_by_tiles = (p.n_tiles + 7) / 8;
    if (splits > max_by_tiles) splits = max_by_tiles;
    if (p.kslots) { const int cap = 1024 / (2 * p.kslots); if (splits > cap) splits = cap; }
    if (splits < 1) splits = 1;
    p.tiles_per_split = (p.n_tiles + splits - 1) / splits;
    p.splits = (p.n_tiles + p.tiles_per_split - 1) / p.tiles_per_split;
    // adaptive lists: 256 slots behind the screen (mean degrees of ~8 come with maxima of ~100), 64 for the exact scan and for
    // the training entry point (its backward keeps one neighbour per lane)
    p.width = (mode == DAGL_MODE_ADAPTIVE) ? ((core || exact || g_N_small(H, W)) ? DAGL_FAST_CAP : DAGL_LIST_CAP) : (p.wide ? 1 : k);
    // bf16 screen: the key stream from L2 into LDS is what bounds it (LDS-DMA lands ~25 GB/s per CU, 6.4 TB/s over the chip;
    // at 256^2 sixteen groups of 256 queries stream the 28 MB of bf16 keys 16 times = 453 MB = 71 us against 46 us of matrix
    // work), so a block covers 512 queries (16 waves, one block per CU: every key tile is fetched half as often) whenever
    // that still gives one block per CU; otherwise 256 queries (8 waves, two blocks per CU).  Key chunks of >= 4 steps of 64
    // keys, <= 64 chunks.
    p.s_steps = (g.N + SKEYS - 1) / SKEYS;
    {
        const int mx = (p.s_steps + 3) / 4 > 64 ? 64 : (p.s_steps + 3) / 4;
        // 512-, 384- or 256-query blocks: whichever leaves the fewest idle query slots (a 72 x 72 tile has L = 324: 12 waves
        // instead of 16), the larger block on a tie; the 16- and 12-wave blocks only when they still give one block per CU
        int qb = 256;
        long long slots = (long long)((g.L + 255) / 256) * 256;
        for (int cand = 384; cand <= 512; cand += 128) {
            const long long nq = (g.L + cand - 1) / cand;
            if (nq * B * mx < 256) continue;
            if (nq * cand <= slots) { qb = cand; slots = nq * cand; }
        }
#ifdef DAGL_ABLATION
        { static const int e = [] { const char* v = getenv("DAGL_SCREEN_QBLOCK"); return v ? atoi(v) : 0; }(); if (e == 256 || e == 384 || e == 512) qb = e; }
        static const int target_env = [] { const char* e = getenv("DAGL_SCREEN_BLOCKS"); return e ? atoi(e) : 0; }();
        const int target = target_env > 0 ? target_env : (qb >= 384 ? 256 : 512);
#else
        const int target = (qb >= 384) ? 256 : 512;   // one resident round
#endif
        const int nqg = (g.L + qb - 1) / qb;
        int sp = (target + nqg * B - 1) / (nqg * B);
        // top-k modes: the threshold is the k-th largest of chunks x 2 x 16 group maxima per query -- large batches of small maps
        // (256 leaf tiles: ONE chunk) left fewer values than k = 50 (theta = 0: every key a candidate, every group on the redo pass)
        // -- and the fewer keys a group holds, the closer its maximum lies to the query's best keys: k / 4 chunks (k = 50: 416 groups
        // of a dozen keys on a 72 x 72 tile instead of 128 groups of forty: a third of the candidates)
        if (mode != DAGL_MODE_ADAPTIVE && sp < (k + 3) / 4) sp = (k + 3) / 4;
        if (sp > mx) sp = mx;
        if (sp < 1) sp = 1;
        p.s_qblock = qb;
        p.s_steps_per_split = (p.s_steps + sp - 1) / sp;
        p.s_splits = (p.s_steps + p.s_steps_per_split - 1) / p.s_steps_per_split;
        // top-k threshold from every 8th key tile: ~2 k s candidates per query reach refine, which thins them out with their
        // screened scores before any feature row is fetched (every 4th: 8 us more sampling for 3 us less filtering at 256^2)
        // (the candidate count grows like k x stride: the stride is kept at <= 64 / k so that a query's candidates stay well
        // inside its slots -- 1024^2, k = 16, every 8th tile sent most queries to the exact redo: 165 ms instead of 27)
        p.s_sample = p.s_steps_per_split >= 16 ? 8 : (p.s_steps_per_split >= 8 ? 4 : (p.s_steps_per_split >= 4 ? 2 : 1));
        { const int kk = (k > 8) ? k : 8; int cap = 64 / kk; if (cap < 1) cap = 1; if (p.s_sample > cap) p.s_sample = cap; }
#ifdef DAGL_ABLATION
        { static const int smp = [] { const char* e = getenv("DAGL_SCREEN_SAMPLE"); return e ? atoi(e) : 0; }(); if (smp > 0) p.s_sample = smp; }
#endif
    }
    // candidate slots per (query, chunk, half) segment: 16 when a query has many segments, up to 256 when it has few
    // (short key streams): ~1024 slots per query in total
    p.capseg = SCREEN_CAPSEG;
    while (p.capseg < 256 && 2 * p.capseg * p.s_splits * 2 <= 1024) p.capseg *= 2;
#ifdef DAGL_ABLATION
    { static const int cs = [] { const char* e = getenv("DAGL_SCREEN_CAPSEG"); return e ? atoi(e) : 0; }(); if (cs >= 4) p.capseg = cs; }
#endif
    // DAGL_FLAG_TIGHT_TOPK: the threshold from every second key tile and eight times the slots per segment (as far as 2 GiB of
    // records go; with fewer slots: from every tile) -- on the Set12 feature maps every 2nd tile + 128 slots serves six of
    // seven images at 0.25 ms, every tile + 64 slots the same six at 0.27, every 4th tile two (profiles/r03_real_features_topk.log).
    // The records are ALWAYS laid out for the larger count, so that a workspace serves both kinds of call with one layout.
    p.capseg_alloc = p.capseg;
    if (p.screen && mode != DAGL_MODE_ADAPTIVE) {
        while (p.capseg_alloc < 8 * p.capseg && p.capseg_alloc < 256 &&
               (size_t)B * g.L * p.s_splits * 2 * (2 * (size_t)p.capseg_alloc) * sizeof(int2) <= ((size_t)2 << 30))
            p.capseg_alloc *= 2;
        // the tight pair: forced by the flag, or taken by the kernels themselves once the workspace's policy word says so
        p.s_sample_tight = (p.capseg_alloc >= 8 * p.capseg && p.s_sample >= 2) ? 2 : 1;
        p.capseg_tight = p.capseg_alloc;
        // The sampled threshold from the PIVOT keys (pivot.hip) instead of every s_sample-th key tile: where the sampled stride skips
        // tiles at all (>= 2: long key streams), k <= 16, and the N / 32 pivots leave the k-th largest of their group maxima room
        // (>= 32 k keys).  Laid out whatever the call's flags, like the records; the training entry point (features given, no
        // projection in the call) keeps the tile sampling.
        p.pivot = !core && p.split16 && p.s_sample >= 2 && k <= 16 && g.N / 32 >= 32 * k;
        p.pivot_policy = p.s_sample >= 4;      // under the policy word: only where the tile sampling is long (a stride of 2 is a few steps)
        if (p.pivot) { p.pv_steps = pivot_steps(g.N); p.pv_steps_per_split = (p.pv_steps + p.s_splits - 1) / p.s_splits; }
        if (mode_flags & DAGL_FLAG_TIGHT_TOPK) { p.s_sample = p.s_sample_tight; p.capseg = p.capseg_tight; }
    }

    const size_t BL = (size_t)B * g.L;
    Carver cv;
    const size_t map_b = (size_t)B * g.Hp * g.Wp * CH * sizeof(float);
    p.o_b1p = cv.reserve(map_b);
    p.o_b2p = cv.reserve(map_b);
    p.o_wp1 = cv.reserve((size_t)DPAD * P * sizeof(float));
    p.o_wp2 = cv.reserve((size_t)DPAD * P * sizeof(float));
    p.o_x = cv.reserve((size_t)B * feat_rows(g.N) * DS * sizeof(float));
    p.o_wq = cv.reserve((size_t)B * feat_rows(g.L) * DS * sizeof(float));
    p.o_colsum = cv.reserve((size_t)B * DS * sizeof(double));
    p.o_mt = cv.reserve(BL * sizeof(float));
    p.o_cnt = cv.reserve(BL * sizeof(int32_t));                // LIFETIME: scan_adaptive only.  Top-k modes behind the screen keep the pivot indices
                                                               // here (o_pidx below): a top-k path that starts using `cnt` must move them
    p.o_segcnt = cv.reserve(BL * p.splits * 2 * sizeof(int32_t));
    p.o_segoff = cv.reserve(BL * p.splits * 2 * sizeof(int32_t));
    p.o_rowoff = cv.reserve((BL + 1) * sizeof(int64_t));
    p.o_deg = cv.reserve(BL * sizeof(int32_t));
    p.o_stats = cv.reserve(STAT_WORDS * sizeof(int64_t));     // (StatWord, dagl_common.h)
    if (mode == DAGL_MODE_ADAPTIVE) {
        p.o_lidx = cv.reserve(BL * DAGL_FAST_CAP * sizeof(int32_t));
        p.o_lval = cv.reserve(BL * DAGL_FAST_CAP * sizeof(float));
    } else {
        p.o_cidx = cv.reserve(BL * p.splits * 2 * p.kslots * sizeof(int32_t));
        p.o_cval = cv.reserve(BL * p.splits * 2 * p.kslots * sizeof(float));
    }
    p.o_nbidx = cv.reserve(BL * p.width * sizeof(int32_t));
    p.o_nbwgt = cv.reserve(BL * p.width * sizeof(float));
    p.o_nbcnt = cv.reserve(BL * sizeof(int32_t));
    p.o_agg = cv.reserve(BL * P * sizeof(float));              // LIFETIME: written from the gather stage on (stage_tail / fold_out / select_wide /
                                                               // select_dense / overflow rows).  Top-k modes behind the screen keep the pivot row sums and
                                                               // the pivot matrix here between the projection and the sampling launch (o_rowsum, o_xp
                                                               // below): anything that writes `agg` BEFORE the sampling launch of a top-k call corrupts them
    p.o_thr = cv.reserve(BL * sizeof(float));
    p.o_bias = cv.reserve(BL * sizeof(float));
    p.o_thrpart = cv.reserve(8 * BL * sizeof(float));                       // prologue: partial thr/bias sums of 4 channel groups
    if (!exact) {
        p.o_maphi = cv.reserve((size_t)B * g.Hp * g.Wp * CH * sizeof(uint16_t));
        p.o_maplo = cv.reserve((size_t)B * g.Hp * g.Wp * CH * sizeof(uint16_t));
        // the coarse tier of the key / query map and the conv blocks' |b1| slots (B1Tiers, dagl_common.h): written by conv_pair16_kernel,
        // read by project16_kernel, so that activations beyond the fine tier's |b1| < 3750 are served by the same launches
        p.o_maphi2 = cv.reserve((size_t)B * g.Hp * g.Wp * CH * sizeof(uint16_t));
        p.o_maplo2 = cv.reserve((size_t)B * g.Hp * g.Wp * CH * sizeof(uint16_t));
        p.o_b1amax = cv.reserve((size_t)conv16_blocks_per_head(g, 1, B) * sizeof(float));
        p.o_wp1h = cv.reserve(4 * P16_PACKED_HALFS * sizeof(uint16_t));          // up to 4 heads (stage entry point)
        p.o_wp2h = cv.reserve(4 * P16_PACKED_HALFS * sizeof(uint16_t));
        p.o_convw = cv.reserve(4 * CONV_W16_BYTES);                                       // packed g / theta weights per head
        p.o_colpart = cv.reserve((size_t)B * project16_key_blocks(g) * 224 * sizeof(float));
    }
    if (p.screen) {
        p.o_xh = cv.reserve((size_t)B * feat_rows_h(g.N) * DSH * sizeof(uint16_t));
        p.o_wqh = cv.reserve((size_t)B * feat_rows_h(g.L) * DSH * sizeof(uint16_t));
        p.s_gkeep = (p.s_splits * 2 * 16 <= 512) ? 16 : 4;       // (screen_theta_kernel takes up to 512 values per query)
        p.o_gmax = cv.reserve(BL * p.s_splits * 2 * p.s_gkeep * sizeof(float));
        if (p.pivot) {
            // The pivot regions take no workspace of their own.  Row sums and pivot matrix live from the projection to the sampling
            // launch, the aggregated rows `agg` (196 B per key against their 46) from the gather on -- and only in calls that
            // materialise them (debug read-out, variable-length lists); the indices sit in `cnt`, which only the adaptive mode's
            // fp32 scan uses.  Both fit whenever the screen runs (N >= 2048); a layout where they do not keeps the tile sampling.
            const size_t rs_b = align_up((size_t)B * g.N * PIVOT_SLOTS * sizeof(float), 256);
            const size_t xp_b = (size_t)B * pivot_rows(g.N) * DSH * sizeof(uint16_t);
            const size_t px_b = (size_t)B * ((g.N + 63) / 64) * 2 * sizeof(int32_t);
            p.o_rowsum = p.o_agg; p.o_xp = p.o_agg + rs_b; p.o_pidx = p.o_cnt;
            if (rs_b + xp_b > BL * P * sizeof(float) || px_b > BL * sizeof(int32_t)) p.pivot = false;
        }
        p.o_theta = cv.reserve(BL * sizeof(float));
        p.o_scand = cv.reserve(BL * p.s_splits * 2 * p.capseg_alloc * sizeof(int2));     // candidate records (count in slot 0)
        if (mode != DAGL_MODE_ADAPTIVE) {       // top-k modes: a query's shared area behind its segments (ScreenArgs::spill)
            p.o_spill = cv.reserve(BL * SCREEN_SPILL * sizeof(int2));
            p.o_spillcnt = cv.reserve(BL * sizeof(unsigned));
        }
        if (mode == DAGL_MODE_ADAPTIVE) {
            p.o_smax = cv.reserve(BL * sizeof(float));       // dense formulation: the rows' shifts (as scores)
            p.o_traw = cv.reserve(BL * sizeof(float));       // ... and their largest sampled screened scores
        }
        p.o_redo = cv.reserve((size_t)B * n_qgroups * sizeof(int32_t));
    }
    if (p.screen && mode == DAGL_MODE_ADAPTIVE && !core) {
        p.ovf_cap = overflow_cap(g.N, B);
        p.o_ovflist = cv.reserve((size_t)p.ovf_cap * sizeof(int32_t));
        p.o_heavy = cv.reserve((size_t)refine_heavy_cap() * sizeof(int32_t));
        p.o_ovfq = cv.reserve((size_t)p.ovf_cap * DS * sizeof(float));
        p.o_ovfscores = cv.reserve((size_t)B * p.ovf_cap * ((g.N + 31) / 32 * 32) * sizeof(float));
        p.o_ovfpart = cv.reserve((size_t)p.ovf_cap * OVF_CHUNKS * OVF_PART_FLOATS * sizeof(float));
    }
    if (p.wide) p.o_wide = cv.reserve(topk_wide_workspace_bytes(g.N, g.L));
    p.o_end = cv.bytes();
    return DAGL_OK;
}

static int check_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("dagl: no HIP device"); (void)hipGetLastError(); return DAGL_ERR_NO_DEVICE; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { set_error("dagl: cannot query device"); (void)hipGetLastError(); return DAGL_ERR_NO_DEVICE; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("dagl: device arch %s is not gfx950", prop.gcnArchName);
        return DAGL_ERR_NO_DEVICE;
    }
    return DAGL_OK;
}

// the streamed dense formulation's workspace (dense.hip), carved behind the plan: the end of it, and its offset
static size_t dense_ws_end(const Plan& p, size_t* o_dense = nullptr) {
    if (o_dense) *o_dense = p.o_end;
    return p.o_end + dense_workspace_bytes(p.B, p.g);
}

// every field of a call's info "not known" but the workspace it needs and the path
static void reset_info(dagl_ce_info* info, int64_t required_bytes, int path) {
    if (!info) return;
    info->required_bytes = required_bytes; info->total_edges = -1; info->max_degree = -1; info->redone_queries = -1;
    info->path = path; info->range_fallback = 0; info->dense_rerun_blocks = 0;
}

static int32_t* stat32(int64_t* stats, StatWord w) { return reinterpret_cast<int32_t*>(stats + w); }

// ---- one block forward: what an entry point asks for, the state of the call, its stages in launch order ----------------------

struct MapsIn {                  // input of dagl_ce_forward*: the conv outputs (all device pointers)
    const float *b1, *b2;        // [B,16,H,W] key / query map, value map
    const float *thr, *bias;     // [B,L] (adaptive modes)
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};

struct FusedIn {                 // input of the fused-prologue entry points (all device pointers), one per head
    const float* x;              // [B,64,H,W] (shared by the heads of a stage)
    const float *g_w, *g_b, *th_w, *th_b, *thr_w, *thr_b, *bias_w, *bias_b;
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};

struct CoreIn {                  // training entry point: features given, neighbour lists handed back for the backward
    const float* wq_rows; const float* x_rows;                   // [B,L,196], [B,N,196] dense rows (post-ReLU)
    const float* b2; const float* thr; const float* bias;        // [B,16,H,W] value map; [B,L] (adaptive modes)
    int32_t* nb_idx; float* nb_wgt; float* nb_s; int32_t* nb_cnt; // [B,L,width] x3, [B,L]
    float* mu;                                                   // [B,L] row means of S (adaptive modes)
    float* lse;                                                  // dense core (streamed dense formulation): [B,L,2] = {softmax shift M, sum Z};
                                                                 // the list outputs are then unused (null)
};

struct ForwardRequest {
    hipStream_t s;
    int B, H, W, mode_flags, k;
    float* out; void* ws; size_t ws_bytes; dagl_ce_info* info;
    // the input: exactly one of the three
    const MapsIn* maps = nullptr;
    const FusedIn* fin = nullptr;
    int heads = 1;               // > 1 (stage entry point): `B` counts head x image pairs, batch entry = head * (B / heads) + image;
                                 // fin[h] carries head h's weights, `out` is the [B/heads, heads*16, H, W] concat map
    const CoreIn* core = nullptr;
    int32_t* dbg_deg = nullptr; float* dbg_rowsum = nullptr; float* dbg_agg = nullptr;     // debug entry point
    Profile* prof = nullptr;
    ForwardRequest(void* stream, int B_, int H_, int W_, int mode_flags_, int k_, float* out_, void* ws_, size_t ws_bytes_,
                   dagl_ce_info* info_)
        : s((hipStream_t)stream), B(B_), H(H_), W(W_), mode_flags(mode_flags_), k(k_), out(out_), ws(ws_), ws_bytes(ws_bytes_),
          info(info_) {}
};

// the request's pointers and workspace, checked against its plan before anything reaches the device
static int check_request(const ForwardRequest& r, const Plan& p) {
    const bool thresholds = p.mode != DAGL_MODE_TOPK;          // the adaptive modes take per-query thresholds and biases
    if (const CoreIn* c = r.core) {
        DAGL_REQUIRE(r.out, "dagl_ce_forward: null tensor pointer");
        DAGL_REQUIRE(c->wq_rows && c->x_rows && c->b2 && (c->lse || (c->nb_idx && c->nb_wgt && c->nb_s && c->nb_cnt)),
                     "dagl_ce_core_forward: null tensor pointer");
        if (thresholds) DAGL_REQUIRE(c->thr && c->bias && c->mu, "dagl_ce_core_forward: thr/bias/mu required in adaptive modes");
    } else if (const FusedIn* f = r.fin) {
        DAGL_REQUIRE(r.out && f->fc1_w && f->fc1_b && f->fc2_w && f->fc2_b, "dagl_ce_forward: null tensor pointer");
        DAGL_REQUIRE(f->x && f->g_w && f->g_b && f->th_w && f->th_b, "dagl_ce_forward_fused: null tensor pointer");
        if (thresholds)
            DAGL_REQUIRE(f->thr_w && f->thr_b && f->bias_w && f->bias_b, "dagl_ce_forward_fused: thr/bias heads required in adaptive modes");
    } else {
        const MapsIn* m = r.maps;
        DAGL_REQUIRE(r.out && m->fc1_w && m->fc1_b && m->fc2_w && m->fc2_b, "dagl_ce_forward: null tensor pointer");
        DAGL_REQUIRE(m->b1 && m->b2, "dagl_ce_forward: null tensor pointer");
        if (thresholds) DAGL_REQUIRE(m->thr && m->bias, "dagl_ce_forward: thr/bias required in adaptive modes");
    }
    return check_workspace("dagl_ce_forward", r.ws, r.ws_bytes, p.o_end);
}

// One forward call: its plan, the workspace carve resolved to pointers, and what its stages share.  Built once per call.
struct Call {
    const ForwardRequest& r;
    const Plan& p;
    const Grid& g;
    hipStream_t s;
    int B, mode, k, heads;
    size_t BL;
    int n_qgroups;                                   // query groups of 128 per image (the fp32 scan's redo unit)
    const FusedIn* fin; const CoreIn* core;
    const float *fc1_w, *fc1_b, *fc2_w, *fc2_b;      // head 0's fc weights (null on the training entry point)
    const float *thr, *bias;                         // per-query heads: the caller's, or the fused prologue's in the workspace
    float *b1p, *b2p, *wp1, *wp2, *X, *Wq, *mt, *agg;
    uint16_t *Xh, *Wqh;                              // bf16 features (screen)
    double* colsum;
    int64_t* stats;                                  // statistics block (StatWord)
    int32_t* redo;                                   // screen: query groups the fp32 scan redoes
    int32_t* nbidx; float* nbwgt; int32_t* nbcnt;    // neighbour lists: the workspace's, or the training entry point's outputs
    RangeTag rt;                                     // range guard of the split-fp16 kernels (dagl_common.h)
    // "prepared": the caller vouches that this workspace last served an identical call (same geometry, mode, weights):
    // packed weights, the maps' zero borders and the zero guard rows of the feature matrices are still in place, and
    // the few per-call counters are cleared by the prologue kernel itself -- three launches fewer
    bool prepared;
    bool topk_policy;                                // top-k modes behind the screen: the threshold policy lives in the workspace
    bool pivot;                                      // a sampled threshold of this call comes from the pivot keys (pivot.hip)
    bool fused_theta;                                // the adaptive screen's threshold comes out of query_thresholds_kernel
    bool no_wait, no_redo;                           // DAGL_FLAG_NO_WAIT / _NO_REDO honoured on this call
    int q_tiled;                                     // the projection writes the bf16 queries in the screen's fragment order
    long long ovf_edge_limit;
    ThrHeadSet thr_all; bool thr_in_proj;            // fused entry points: the thr / bias heads' blocks ride in the projection's launch
    Split16Out split_out; const Split16Out* split_p; // DAGL_FLAG_DENSE_HINT: the projection also writes dense.hip's split features
    // set by the stages
    SelectArgs sa; EdgeArgs ea; AggArgs ag;
    bool ovf_active = false;         // set once the refine kernel has listed its overflowed queries (adaptive, screened)
    bool agg_done = false;           // the gather + weighted sum over the lists ran inside the overflow launches (adaptive, screened)
    bool left_range = false;         // a statistics read-back found this call's tag in the range word

    Call(const ForwardRequest& r_, const Plan& p_);
};

Call::Call(const ForwardRequest& r_, const Plan& p_) : r(r_), p(p_), g(p_.g) {
    void* ws = r.ws;
    const int flags = r.mode_flags;
    s = r.s; B = r.B; mode = p.mode; k = p.k; heads = r.heads;            // (k clamped to the number of keys)
    BL = (size_t)B * g.L;
    n_qgroups = (g.L + 127) / 128;
    fin = r.fin; core = r.core;
    fc1_w = fin ? fin->fc1_w : core ? nullptr : r.maps->fc1_w;
    fc1_b = fin ? fin->fc1_b : core ? nullptr : r.maps->fc1_b;
    fc2_w = fin ? fin->fc2_w : core ? nullptr : r.maps->fc2_w;
    fc2_b = fin ? fin->fc2_b : core ? nullptr : r.maps->fc2_b;
    thr = fin ? at<float>(ws, p.o_thr) : core ? core->thr : r.maps->thr;
    bias = fin ? at<float>(ws, p.o_bias) : core ? core->bias : r.maps->bias;
    b1p = at<float>(ws, p.o_b1p); b2p = at<float>(ws, p.o_b2p);
    wp1 = at<float>(ws, p.o_wp1); wp2 = at<float>(ws, p.o_wp2);
    X = at<float>(ws, p.o_x); Wq = at<float>(ws, p.o_wq);
    mt = at<float>(ws, p.o_mt); agg = at<float>(ws, p.o_agg);
    Xh = p.screen ? at<uint16_t>(ws, p.o_xh) : nullptr;
    Wqh = p.screen ? at<uint16_t>(ws, p.o_wqh) : nullptr;
    colsum = at<double>(ws, p.o_colsum);
    stats = at<int64_t>(ws, p.o_stats);
    redo = p.screen ? at<int32_t>(ws, p.o_redo) : nullptr;
    nbidx = core ? core->nb_idx : at<int32_t>(ws, p.o_nbidx);
    nbwgt = core ? core->nb_wgt : at<float>(ws, p.o_nbwgt);
    nbcnt = core ? core->nb_cnt : at<int32_t>(ws, p.o_nbcnt);
    // (every path has the guard: the fp32 path has no range, but a NaN feature must not become a 0 behind its ReLU, nor an
    // inf-poisoned key drop out of the selection -- dagl.py:207-275 returns NaN for a non-finite input, and so does every path here;
    // the training entry points: the streamed dense core splits the features into fp16 halves too)
    rt.word = stat32(stats, STAT_RANGE); rt.done = stat32(stats, STAT_DONE); rt.tag = next_call_tag();

    const bool dbg = r.dbg_deg || r.dbg_rowsum || r.dbg_agg;
    prepared = fin && p.split16 && (flags & DAGL_FLAG_WEIGHTS_PACKED);
    topk_policy = p.screen && mode != DAGL_MODE_ADAPTIVE && !(flags & (DAGL_FLAG_TIGHT_TOPK | DAGL_FLAG_SAMPLED_TOPK)) &&
                  p.capseg_tight > 0 && (p.capseg_tight != p.capseg || p.s_sample_tight != p.s_sample);
    // Pivot threshold: forced by DAGL_FLAG_SAMPLED_TOPK, or a call under the workspace's policy word on a PREPARED workspace (the word
    // then has the last say, on the device).  The first call of a shape under the policy keeps the tile sampling: it is that call's
    // overflow under the UNIFORM sample that decides, as before, whether the workspace moves to the tight threshold for good
    pivot = p.pivot && !(flags & DAGL_FLAG_TIGHT_TOPK) && ((flags & DAGL_FLAG_SAMPLED_TOPK) || (p.pivot_policy && (!topk_policy || prepared)));
    fused_theta = p.screen && mode == DAGL_MODE_ADAPTIVE;
    no_wait = (flags & DAGL_FLAG_NO_WAIT) && p.ovf_cap > 0 && !dbg && !core && heads == 1;
    no_redo = p.screen && (flags & DAGL_FLAG_NO_REDO) && fin && heads == 1 && !core && !dbg;
    q_tiled = (p.screen && p.split16 && !core) ? 1 : 0;
    // the per-query redo gathers one value patch per edge of a flagged row (~1 ns each), the dense formulation costs ~9 ps per
    // (query, key) PAIR whatever the mask: a call whose flagged rows hold more than 1/96 of all pairs goes dense
    ovf_edge_limit = (long long)((double)BL * (double)g.N / 96.0);
    // the thr / bias heads' partial sums are first read by query_thresholds_kernel, behind the projection: on the split-fp16 path their
    // blocks ride in the projection's launch (round 5; 13 us of every adaptive-mode call as a launch of their own)
    thr_all = {};
    thr_in_proj = false;
    if (fin && mode != DAGL_MODE_TOPK) {
        for (int h = 0; h < heads; ++h) { thr_all.x[h] = fin[h].x; thr_all.thr_w[h] = fin[h].thr_w; thr_all.bias_w[h] = fin[h].bias_w; }
        thr_all.imgs = B / heads;
        thr_in_proj = p.split16 && thr_bias4_ok(g, thr_all, heads);
    }
    // a call that goes straight to the streamed dense formulation (DAGL_FLAG_DENSE_HINT): the projection writes the split-fp16
    // features dense.hip consumes as well -- no separate splitting pass over the fp32 rows
    split_p = nullptr;
    if (!core && p.split16 && p.screen && mode == DAGL_MODE_ADAPTIVE && (flags & DAGL_FLAG_DENSE_HINT)) {
        size_t o_dn = 0;
        if (r.ws_bytes >= dense_ws_end(p, &o_dn)) { split_out = dense_split_buffers(at<char>(ws, o_dn), B, g); split_p = &split_out; }
    }
}

static inline void mark(const Call& c, int stage_boundary) { prof_mark(c.r.prof, c.s, stage_boundary); }

// ---- stage 0: layout: zero-bordered NHWC maps, packed fc weights ------------------------------------

// the fused entry points: the g / theta / thr / bias convolutions of every head (prologue.hip); on the split-fp16 path the key /
// query map leaves them as fp16 halves only
static int prologue_fused(Call& c) {
    const Plan& p = c.p; const Grid& g = c.g; const FusedIn* fin = c.fin; void* ws = c.r.ws;
    const int heads = c.heads, imgs = c.B / heads;
    const bool thr_heads = c.mode != DAGL_MODE_TOPK;
    const size_t map_f = (size_t)imgs * g.Hp * g.Wp * CH;
    const bool conv_merged = heads > 1 && p.split16;       // a stage's heads: their g / theta convolutions are ONE launch
    // a prepared call's per-call counters and redo flags are cleared by the first block of the conv kernel
    uint32_t* clear_stats = c.prepared ? reinterpret_cast<uint32_t*>(c.stats) : nullptr;
    const int clear_stats_words = c.prepared ? 2 * STAT_N_COUNTERS : 0;
    uint32_t* clear_redo = (c.prepared && p.screen) ? reinterpret_cast<uint32_t*>(c.redo) : nullptr;
    const int clear_redo_words = (c.prepared && p.screen) ? c.B * c.n_qgroups : 0;
    uint16_t* map_hi = p.split16 ? at<uint16_t>(ws, p.o_maphi) : nullptr;
    uint16_t* map_lo = p.split16 ? at<uint16_t>(ws, p.o_maplo) : nullptr;
    float* thr_part = at<float>(ws, p.o_thrpart);
    // the map's two tiers (B1Tiers): all heads of the call share the slot array, [head][blocks of that head]
    B1Tiers tiers_all;
    if (p.split16) {
        tiers_all.hi2 = at<uint16_t>(ws, p.o_maphi2); tiers_all.lo2 = at<uint16_t>(ws, p.o_maplo2);
        tiers_all.amax = at<float>(ws, p.o_b1amax); tiers_all.slots = conv16_blocks_per_head(g, heads, imgs);
    }
    int rc;
    for (int hd = 0; hd < heads; ++hd) {
        const FusedIn& f = fin[hd];
        unsigned char* convw = p.split16 ? at<unsigned char>(ws, p.o_convw) + (size_t)hd * CONV_W16_BYTES : nullptr;
        if (convw && !(c.r.mode_flags & DAGL_FLAG_WEIGHTS_PACKED) && (rc = launch_pack_conv_weight16(c.s, f.g_w, f.th_w, convw))) return rc;
        if (conv_merged && hd == heads - 1) {
            ConvHeadSet hs = {};
            for (int h2 = 0; h2 < heads; ++h2) {
                hs.x[h2] = fin[h2].x; hs.w[h2] = at<unsigned char>(ws, p.o_convw) + (size_t)h2 * CONV_W16_BYTES;
                hs.gb[h2] = fin[h2].g_b; hs.tb[h2] = fin[h2].th_b;
            }
            hs.imgs = imgs;
            hs.tiers = tiers_all;
            if ((rc = launch_conv_pair16_heads(c.s, heads, imgs, g, hs, c.b2p, nullptr, map_hi, map_lo, clear_stats, clear_stats_words, clear_redo,
                                               clear_redo_words, c.rt))) return rc;
            if (thr_heads && !c.thr_in_proj && (rc = launch_thr_bias_heads(c.s, heads, imgs, g, c.thr_all, thr_part))) return rc;
        }
        PrologueLaunch pl;
        pl.B = imgs; pl.g = g; pl.x = f.x;
        pl.g_w = f.g_w; pl.g_b = f.g_b; pl.th_w = f.th_w; pl.th_b = f.th_b;
        pl.thr_w = f.thr_w; pl.thr_b = f.thr_b; pl.bias_w = f.bias_w; pl.bias_b = f.bias_b;
        pl.b2p = c.b2p + hd * map_f;
        if (p.split16) {
            // default path: the key/query map is only ever consumed as split fp16 (project16), so the prologue
            // writes the hi / lo maps itself and no fp32 copy exists
            pl.conv = conv_merged ? ConvPath::DoneByCaller : ConvPath::Split16;
            pl.conv_w16 = convw;
            pl.b1_hi = map_hi + hd * map_f; pl.b1_lo = map_lo + hd * map_f;
            pl.tiers = B1Tiers{tiers_all.hi2 + hd * map_f, tiers_all.lo2 + hd * map_f, tiers_all.amax, tiers_all.slots};
        } else {
            pl.b1p = c.b1p + hd * map_f;
        }
        if (thr_heads && !c.thr_in_proj) pl.thr = at<float>(ws, p.o_thr) + (size_t)hd * imgs * g.L;
        pl.bias = at<float>(ws, p.o_bias) + (size_t)hd * imgs * g.L;
        pl.thr_part = thr_part + (size_t)hd * 8 * imgs * g.L;
        pl.borders_zero = c.prepared; pl.defer_thr_reduce = thr_heads;
        if (hd == 0) {
            pl.clear_a = clear_stats; pl.clear_a_words = clear_stats_words;
            pl.clear_b = clear_redo; pl.clear_b_words = clear_redo_words;
        }
        pl.range = c.rt;
        if ((rc = launch_prologue(c.s, pl))) return rc;
    }
    return DAGL_OK;
}

// the fc weights packed for the projection (and dagl_ce_forward's key / query map split into fp16 halves)
static int pack_fc_weights(Call& c) {
    const Plan& p = c.p; const Grid& g = c.g; void* ws = c.r.ws;
    const bool packed = (c.r.mode_flags & DAGL_FLAG_WEIGHTS_PACKED) != 0;
    int rc;
    if (!p.split16) {
        DAGL_REQUIRE(c.heads == 1, "dagl: the stage entry point needs the default (screened) scan");
        if (packed) return DAGL_OK;
        if ((rc = launch_pack_fc_weight(c.s, c.fc1_w, c.wp1))) return rc;
        return launch_pack_fc_weight(c.s, c.fc2_w, c.wp2);
    }
    uint16_t* wp1h = at<uint16_t>(ws, p.o_wp1h);
    uint16_t* wp2h = at<uint16_t>(ws, p.o_wp2h);
    if (!c.fin)                                              // stock-conv entry point: split the padded fp32 map
        if ((rc = launch_split_map(c.s, (size_t)c.B * g.Hp * g.Wp * CH, c.b1p, at<uint16_t>(ws, p.o_maphi), at<uint16_t>(ws, p.o_maplo),
                                   c.rt))) return rc;
    for (int hd = 0; hd < c.heads && !packed; ++hd) {
        if ((rc = launch_pack_fc_weight16(c.s, c.fin ? c.fin[hd].fc1_w : c.fc1_w, wp1h + (size_t)hd * P16_PACKED_HALFS))) return rc;
        if ((rc = launch_pack_fc_weight16(c.s, c.fin ? c.fin[hd].fc2_w : c.fc2_w, wp2h + (size_t)hd * P16_PACKED_HALFS))) return rc;
    }
    return DAGL_OK;
}

static int stage_layout(Call& c) {
    const Plan& p = c.p; const Grid& g = c.g;
    hipStream_t s = c.s;
    int rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    if (cap == hipStreamCaptureStatusActive) {
        hipLaunchKernelGGL(retag_kernel, dim3(1), dim3(1), 0, s, c.rt.word,
                           c.mode == DAGL_MODE_ADAPTIVE ? stat32(c.stats, STAT_VETO) : nullptr, c.rt.tag);
        DAGL_LAUNCH_CHECK("retag_kernel");
    }
    mark(c, 0);
    if (!c.prepared) DAGL_HIP_TRY(hipMemsetAsync(c.stats + STAT_RANGE, 0, 2 * sizeof(int64_t), s));   // fresh workspace: range, done
    if (!c.prepared && c.mode == DAGL_MODE_ADAPTIVE) DAGL_HIP_TRY(hipMemsetAsync(c.stats + STAT_VETO, 0, sizeof(int64_t), s));
    if (p.screen && c.mode != DAGL_MODE_ADAPTIVE && !c.prepared) {
        // (include/dagl_ce.h DAGL_FLAG_TIGHT_TOPK; forced thresholds -- DAGL_FLAG_TIGHT_TOPK / _SAMPLED_TOPK -- do not read the policy
        // word; the cookie and the sticky words are kept all the same).  A cold workspace starts with the sampled threshold and a closed
        // gate -- but maps of up to 16 384 keys (128^2; the 72 x 72 leaf tiles of the tiled driver) START on the tight threshold: there it
        // costs nothing measurable on synthetic maps (sampling every second key tile of <= 256 is a few steps) and its better threshold
        // saves 12 % on natural-image leaf tiles even when nothing overflows (0.64 against 0.73 ms per batch of 64 tiles,
        // profiles/r04_topk_policy_real_features.log).  The word is kept while the workspace carries this geometry's cookie.
        uint64_t ck = 0x5DA6ull;
        for (const int v : {c.B, c.r.H, c.r.W, c.mode, c.k, p.s_splits, p.capseg, p.capseg_tight}) ck = ck * 0x100000001B3ull ^ (uint64_t)(uint32_t)v;
        hipLaunchKernelGGL(policy_init_kernel, dim3(1), dim3(1), 0, s, c.stats, (int64_t)(ck | 1ull), g.N <= 16384 ? 1 : 0);
        DAGL_LAUNCH_CHECK("policy_init_kernel");
    }
    if (c.core) {                       // (nothing to pack: the projections were done by the caller, under autograd)
        if ((rc = launch_pad_nhwc(s, c.B, g.H, g.W, c.core->b2, c.b2p))) return rc;
    } else {
        if (c.fin) {
            if ((rc = prologue_fused(c))) return rc;
        } else {
            if ((rc = launch_pad_nhwc(s, c.B, g.H, g.W, c.r.maps->b1, c.b1p))) return rc;
            if ((rc = launch_pad_nhwc(s, c.B, g.H, g.W, c.r.maps->b2, c.b2p))) return rc;
        }
        if ((rc = pack_fc_weights(c))) return rc;
    }
    ZeroList zl;
    if (c.split_p) dense_guard_rows(zl, c.B, g, c.split_out);
    if (c.prepared && c.split_p) { if ((rc = launch_zero_regions(s, zl))) return rc; }
    if (!c.prepared) {   // rows past the last patch (partial tile + guard tile) are streamed by the scans: keep them zero
        const int rx = feat_rows(g.N), rq = feat_rows(g.L);
        const int hx = feat_rows_h(g.N), hq = feat_rows_h(g.L);
        zl.add(c.X + (size_t)g.N * DS, (size_t)(rx - g.N) * DS * sizeof(float), c.B, (size_t)rx * DS * sizeof(float));
        zl.add(c.Wq + (size_t)g.L * DS, (size_t)(rq - g.L) * DS * sizeof(float), c.B, (size_t)rq * DS * sizeof(float));
        if (p.screen) {
            zl.add(c.Xh + (size_t)g.N * DSH, (size_t)(hx - g.N) * DSH * sizeof(uint16_t), c.B, (size_t)hx * DSH * sizeof(uint16_t));
            // (from the last PARTIAL 32-query tile on: in the fragment order its unused rows sit between the used ones)
            const int lq = g.L & ~31;
            zl.add(c.Wqh + (size_t)lq * DSH, (size_t)(hq - lq) * DSH * sizeof(uint16_t), c.B, (size_t)hq * DSH * sizeof(uint16_t));
        }
        zl.add(c.colsum, align_up((size_t)c.B * DS * sizeof(double), 16));
        zl.add(c.stats, STAT_N_COUNTERS * sizeof(int64_t));
        if (p.screen) zl.add(c.redo, align_up((size_t)c.B * c.n_qgroups * sizeof(int32_t), 16));
        if ((rc = launch_zero_regions(s, zl))) return rc;
    }
    return DAGL_OK;
}

// ---- stage 1: both projections, one launch -------------------------------------------------------------
static int stage_project(Call& c) {
    const Plan& p = c.p; const Grid& g = c.g; void* ws = c.r.ws;
    int rc;
    mark(c, 1);
    if (c.core) {
        if ((rc = launch_rows_to_feat(c.s, c.B, g.N, c.core->x_rows, c.X, c.Xh, c.rt))) return rc;
        if ((rc = launch_rows_to_feat(c.s, c.B, g.L, c.core->wq_rows, c.Wq, c.Wqh, c.rt))) return rc;
        return c.mode != DAGL_MODE_TOPK ? launch_colsum_rows(c.s, c.B, g.N, c.core->x_rows, c.colsum) : DAGL_OK;
    }
    if (!p.split16) {
        ProjectLaunch pj;
        pj.B = c.B; pj.g = g; pj.which = 3; pj.map = c.b1p; pj.colsum = c.colsum; pj.range = c.rt;
        pj.keys.wp = c.wp2; pj.keys.bias = c.fc2_b; pj.keys.feat = c.X; pj.keys.feat_bf16 = c.Xh;
        pj.queries.wp = c.wp1; pj.queries.bias = c.fc1_b; pj.queries.feat = c.Wq; pj.queries.feat_bf16 = c.Wqh;
        return launch_project(c.s, pj);
    }
    Project16Launch pj;
    pj.B = c.B; pj.g = g; pj.which = 3; pj.heads = c.heads; pj.range = c.rt;
    pj.map_hi = at<uint16_t>(ws, p.o_maphi); pj.map_lo = at<uint16_t>(ws, p.o_maplo);
    if (c.fin) {       // (the fused entry points: conv_pair16_kernel wrote both tiers; dagl_ce_forward's split_map_kernel only the fine one)
        pj.tiers.hi2 = at<uint16_t>(ws, p.o_maphi2); pj.tiers.lo2 = at<uint16_t>(ws, p.o_maplo2);
        pj.tiers.amax = at<float>(ws, p.o_b1amax); pj.tiers.slots = conv16_blocks_per_head(g, c.heads, c.B / c.heads);
    }
    const float* b1s[4]; const float* b2s[4];
    for (int hd = 0; hd < 4; ++hd) {
        b1s[hd] = (c.fin && hd < c.heads) ? c.fin[hd].fc1_b : c.fc1_b;
        b2s[hd] = (c.fin && hd < c.heads) ? c.fin[hd].fc2_b : c.fc2_b;
    }
    pj.keys.wp = at<uint16_t>(ws, p.o_wp2h); pj.keys.bias = b2s; pj.keys.feat = c.X; pj.keys.feat_bf16 = c.Xh;
    pj.queries.wp = at<uint16_t>(ws, p.o_wp1h); pj.queries.bias = b1s; pj.queries.feat = c.Wq; pj.queries.feat_bf16 = c.Wqh;
    if (c.mode != DAGL_MODE_TOPK) pj.colsum = c.colsum;
    pj.colpart = at<float>(ws, p.o_colpart);
    pj.q_tiled = c.q_tiled; pj.split = c.split_p;
    if (c.pivot) { pj.rowsum = at<float>(ws, p.o_rowsum); if (c.topk_policy) pj.rowsum_policy = stat32(c.stats, STAT_POLICY); }
    if (c.thr_in_proj) { pj.thr_hs = &c.thr_all; pj.thr_head_imgs = c.B; pj.thr_part = at<float>(ws, p.o_thrpart); }
    return launch_project16(c.s, pj);
}

// ---- stage 2: adaptive thresholds ----------------------------------------------------------------------
static int stage_thresholds(Call& c) {
    const Plan& p = c.p; const Grid& g = c.g; void* ws = c.r.ws;
    mark(c, 2);
    SelectArgs& sa = c.sa;
    memset(&sa, 0, sizeof(sa));
    sa.B = c.B; sa.L = g.L; sa.N = g.N; sa.W = g.W; sa.wq = c.Wq; sa.x = c.X; sa.mode = c.mode; sa.k = c.k;
    sa.splits = p.splits; sa.tiles_per_split = p.tiles_per_split;
    EdgeArgs& ea = c.ea;
    memset(&ea, 0, sizeof(ea));
    ea.B = c.B; ea.L = g.L; ea.N = g.N; ea.mode = c.mode; ea.k = c.k; ea.splits = p.splits;
    ea.nb_idx = c.nbidx; ea.nb_wgt = c.nbwgt; ea.nb_cnt = c.nbcnt; ea.width = p.width;
    ea.nb_s = c.core ? c.core->nb_s : nullptr;
    AggArgs& ag = c.ag;
    memset(&ag, 0, sizeof(ag));
    ag.B = c.B; ag.g = g; ag.b2p = c.b2p; ag.nb_idx = c.nbidx; ag.nb_wgt = c.nbwgt; ag.nb_cnt = c.nbcnt; ag.width = p.width;
    ag.agg = c.agg;
    if (c.mode == DAGL_MODE_TOPK) return DAGL_OK;
    ThrFuse tf;
    if (c.fin) {                                 // finish the thr / bias heads here (their partial sums are per head)
        tf.part = at<float>(ws, p.o_thrpart); tf.imgs_per_head = c.B / c.heads;
        for (int hd = 0; hd < c.heads; ++hd) { tf.thr_b[hd] = c.fin[hd].thr_b; tf.bias_b[hd] = c.fin[hd].bias_b; }
        tf.thr_out = at<float>(ws, p.o_thr); tf.bias_out = at<float>(ws, p.o_bias);
    } else {
        tf.bias_out = const_cast<float*>(c.bias);   // read only in this case
    }
    if (c.fused_theta) {
        tf.theta_out = at<float>(ws, p.o_theta);
        tf.zero_out = at<float>(ws, p.o_traw);      // (select_dense's sampled pass takes maxima into it)
    }
    const int rc = launch_query_thresholds(c.s, c.B, g.L, g.N, c.Wq, c.colsum, c.thr, c.mt, c.core ? c.core->mu : nullptr, &tf);
    sa.mt = c.mt; sa.bs = c.bias; ea.mt = c.mt; ea.bs = c.bias;
    return rc;
}

// ---- stages 6-7: gather + weighted sum, fold ---------------------------------------------------------------

// the end of every path: the aggregated rows (the debug entry point: a copy of them) folded into the output map
static int fold_out(Call& c) {
    mark(c, 7);
    if (c.r.dbg_agg) DAGL_HIP_TRY(hipMemcpyAsync(c.r.dbg_agg, c.agg, c.BL * P * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    const int rc = launch_fold(c.s, c.B, c.g, c.agg, c.r.out, c.heads, c.rt);
    if (rc == DAGL_OK) mark(c, 8);
    return rc;
}

// arguments of the per-query redo of the rows that overflowed the screened adaptive lists (overflow.hip)
static OvfArgs overflow_args(const Call& c) {
    const Plan& p = c.p; const Grid& g = c.g; void* ws = c.r.ws;
    OvfArgs oa;
    memset(&oa, 0, sizeof(oa));
    oa.B = c.B; oa.g = g; oa.x = c.X; oa.rows_x = feat_rows(g.N);
    oa.mt = c.mt; oa.bs = c.bias; oa.b2p = c.b2p; oa.list = at<int32_t>(ws, p.o_ovflist);
    oa.count = stat32(c.stats, STAT_OVF_COUNT); oa.cap = p.ovf_cap;
    oa.qrows = at<float>(ws, p.o_ovfq); oa.scores = at<float>(ws, p.o_ovfscores); oa.ldn = (g.N + 31) / 32 * 32; oa.part = at<float>(ws, p.o_ovfpart);
    oa.agg = c.agg; oa.nb_cnt = c.nbcnt; oa.dbg_deg = c.r.dbg_deg; oa.dbg_rowsum = c.r.dbg_rowsum;
    oa.edges_run = c.stats + STAT_EDGES;     // (zero since the start of the call, overwritten with the total by the statistics block)
    oa.flagged_edges = c.stats + STAT_REDONE_EDGES; oa.edge_limit = c.ovf_edge_limit;
    return oa;
}

static int stage_tail(Call& c) {
    const ForwardRequest& r = c.r; const AggArgs& ag = c.ag;
    int rc;
    if (r.dbg_deg || r.dbg_rowsum)
        if ((rc = launch_row_stats(c.s, c.BL, ag.nb_wgt, ag.nb_cnt, ag.row_off, ag.width, r.dbg_deg, r.dbg_rowsum))) return rc;
    mark(c, 6);
    // short fixed-width lists and nobody asking for the aggregated rows: gather, weighted sum and fold in one kernel
    if (c.mode != DAGL_MODE_ADAPTIVE && ag.row_off == nullptr && !c.ovf_active && !r.dbg_agg && !c.core) {
        if ((rc = launch_aggregate_fold(c.s, ag, r.out, c.heads, c.rt))) return rc;
        mark(c, 7);                              // (the whole tail is booked on the gather stage)
        mark(c, 8);
        return DAGL_OK;
    }
    // (the few queries whose neighbourhood overflowed the lists are redone one by one, dense rows, overflow.hip; the list gather
    // skips them.  A call that does not wait had both done in the overflow launches; one that waits has its statistics on their
    // way to the host by now and queues the gathers here, under the round trip)
    if (!c.agg_done) {
        if ((rc = launch_aggregate_direct(c.s, ag))) return rc;
        if (c.ovf_active) {           // (a call that waited for its verdict: the flagged rows' gathers behind the read-back)
            OvfArgs oa = overflow_args(c);
            oa.edges_run = nullptr;                     // (their edges are known: ovf_attend_kernel looks at flagged_edges)
            if ((rc = launch_overflow_apply(c.s, oa))) return rc;
        }
    }
    return fold_out(c);
}

// ---- stages 3-5: neighbour selection + edge softmax, one function per path ----------------------------------

// a read-back of the first n (> STAT_RANGE) statistics words; the range word tells whether the call left the split-fp16 range
static int read_stats(Call& c, int n, int64_t* hs) {
    const int rc = read_back(c.s, c.stats, n, hs);
    c.left_range = rc == DAGL_OK && (int32_t)hs[STAT_RANGE] == c.rt.tag;
    return rc;
}

// path 6: top-k modes with neighbourhoods wider than the lists -- scores, k-th largest, mask, softmax and weighted sum row by row
static int select_wide(Call& c) {
    dagl_ce_info* info = c.r.info;
    int rc;
    mark(c, 3); mark(c, 4); mark(c, 5);
    if (c.heads > 1) { set_error("dagl_ces_stage_forward: k=%d > %d: use the per-head entry point", c.k, DAGL_MAX_TOPK); return DAGL_ERR_UNSUPPORTED; }
    int32_t* deg = at<int32_t>(c.r.ws, c.p.o_deg);
    if ((rc = launch_topk_wide(c.s, c.B, c.g, c.mode, c.k, c.Wq, c.X, c.mt, c.bias, c.b2p, at<char>(c.r.ws, c.p.o_wide), c.agg, deg,
                               c.r.dbg_rowsum, c.rt))) return rc;
    mark(c, 6);
    if (c.r.dbg_deg) DAGL_HIP_TRY(hipMemcpyAsync(c.r.dbg_deg, deg, c.BL * sizeof(int32_t), hipMemcpyDeviceToDevice, c.s));
    if ((rc = fold_out(c))) return rc;
    if (!info) return DAGL_OK;
    if ((rc = launch_degree_stats(c.s, c.BL, deg, c.stats))) return rc;
    int64_t hs[STAT_RANGE + 1] = {0};
    if ((rc = read_stats(c, STAT_RANGE + 1, hs)) || c.left_range) return rc;
    info->path = 6; info->total_edges = hs[STAT_EDGES]; info->max_degree = (int32_t)hs[STAT_MAX_DEGREE];
    return DAGL_OK;
}

static ScreenArgs screen_args(const Call& c) {
    const Plan& p = c.p; const Grid& g = c.g; void* ws = c.r.ws;
    ScreenArgs sc;
    memset(&sc, 0, sizeof(sc));
    sc.B = c.B; sc.L = g.L; sc.N = g.N; sc.mode = c.mode; sc.wqh = c.Wqh; sc.xh = c.Xh; sc.q_tiled = c.q_tiled;
    sc.rows_qh = feat_rows_h(g.L); sc.rows_xh = feat_rows_h(g.N);
    sc.splits = p.s_splits; sc.steps_per_split = p.s_steps_per_split; sc.n_steps = p.s_steps; sc.sample = p.s_sample; sc.qblock = p.s_qblock;
    sc.gmax = at<float>(ws, p.o_gmax); sc.gkeep = p.s_gkeep; sc.theta = at<float>(ws, p.o_theta); sc.mt = c.mt; sc.bs = c.bias;
    sc.capseg = p.capseg; sc.cand = at<int2>(ws, p.o_scand);
    if (c.mode != DAGL_MODE_ADAPTIVE) { sc.spill = at<int2>(ws, p.o_spill); sc.spill_cnt = at<unsigned>(ws, p.o_spillcnt); }
    if (c.topk_policy) { sc.policy = stat32(c.stats, STAT_POLICY); sc.sample_tight = p.s_sample_tight; sc.capseg_tight = p.capseg_tight; }
    if (c.pivot && c.mode != DAGL_MODE_ADAPTIVE) {
        sc.xp = at<uint16_t>(ws, p.o_xp); sc.rows_xp = pivot_rows(g.N); sc.pv_steps = p.pv_steps; sc.pv_steps_per_split = p.pv_steps_per_split;
    }
#ifdef DAGL_ABLATION
    { static const int var = [] { const char* e = getenv("DAGL_SCREEN_VARIANT"); return e ? atoi(e) : 0; }(); sc.variant = var; }
#endif
    return sc;
}

// path 4: most queries keep more keys than the screen has candidate slots for -- the dense regime.  Lists are pointless there;
// the dense formulation is streamed instead (dense.hip).  Reached after the screen found out, or directly when the caller passes
// DAGL_FLAG_DENSE_HINT (its previous call on this module ended here): always correct, only slower than the lists when the
// neighbourhoods are in fact sparse.
static int select_dense(Call& c, bool features_split) {
    const Plan& p = c.p; const Grid& g = c.g; void* ws = c.r.ws; dagl_ce_info* info = c.r.info;
    size_t o_dn = 0;
    const size_t end = dense_ws_end(p, &o_dn);
    if (info) { info->required_bytes = (int64_t)end; info->path = 4; }
    if (c.core && !c.core->lse) {
        if (info) info->required_bytes = -1;
        set_error("dagl_ce_core_forward: dense neighbourhoods (most queries keep more than %d keys) do not fit fixed-width lists: "
                  "use dagl_ce_core_dense_forward", DAGL_FAST_CAP);
        return DAGL_ERR_UNSUPPORTED;
    }
    if (c.r.ws_bytes < end) {
        set_error("dagl_ce_forward: dense neighbourhoods need workspace %zu B, have %zu B", end, c.r.ws_bytes);
        return DAGL_ERR_WORKSPACE;
    }
    // the softmax's shift, known up front: every row's largest score, exactly -- a top-1 screen (sampled pass -> theta = the
    // largest sampled S~ less the band -> filter pass) and the exact scores of its few candidates (rowmax_exact_kernel).  Up to
    // round 4: an upper bound from one full bf16 scan, whose 1.6 % became > 18 units of a logit beyond ~580 and sent whole
    // blocks through dense_attend_kernel a second time (every block of bench.py's default map: 1.52 ms for 0.81)
    ScreenArgs s1 = screen_args(c);
    s1.mode = DAGL_MODE_TOPK; s1.mt = nullptr; s1.bs = nullptr; s1.policy = nullptr; s1.gate = nullptr;
    s1.spill = nullptr; s1.spill_cnt = nullptr; s1.seg_max = 1;      // (no spill: a row with more candidates than slots keeps its upper bound)
    s1.theta_max = at<int>(ws, p.o_traw); s1.theta = at<float>(ws, p.o_traw);     // (zeroed by query_thresholds_kernel)
    int rc;
    if ((rc = launch_screen(c.s, s1, 0))) return rc;
    if ((rc = launch_screen(c.s, s1, 1))) return rc;
    float* smax = at<float>(ws, p.o_smax);
    RefineArgs r1;
    memset(&r1, 0, sizeof(r1));
    r1.B = c.B; r1.L = g.L; r1.N = g.N; r1.mode = DAGL_MODE_TOPK; r1.k = 1; r1.splits = p.s_splits; r1.capseg = p.capseg;
    r1.wq = c.Wq; r1.x = c.X; r1.rows_q = feat_rows(g.L); r1.rows_x = feat_rows(g.N);
    r1.cand = s1.cand; r1.theta = s1.theta; r1.mt = c.mt; r1.bs = c.bias;
    if ((rc = launch_rowmax_exact(c.s, r1, smax))) return rc;
    mark(c, 6);          // (stage "gather" of a dense call = value-map split + dense_attend_kernel + combine)
    if ((rc = launch_dense_attend(c.s, c.B, g, c.Wq, c.X, c.mt, c.bias, smax, c.b2p, at<char>(ws, o_dn), c.agg, c.r.dbg_deg,
                                  c.r.dbg_rowsum, c.stats, c.rt, c.core ? c.core->lse : nullptr, features_split, info != nullptr))) return rc;
    if ((rc = fold_out(c))) return rc;
    if (!info) return DAGL_OK;
    int64_t hs[STAT_DENSE_RERUN + 1] = {0};
    if ((rc = read_stats(c, STAT_DENSE_RERUN + 1, hs)) || c.left_range) return rc;
    info->total_edges = hs[STAT_EDGES]; info->max_degree = (int32_t)hs[STAT_MAX_DEGREE];
    info->redone_queries = hs[STAT_FLAGGED];                          // queries whose degree exceeds the lists' width
    info->dense_rerun_blocks = (int32_t)hs[STAT_DENSE_RERUN];         // blocks of 64 queries dense_attend_kernel ran a second time
    return DAGL_OK;
}

// paths 0 / 1, adaptive mode: one fp32 scan into per-lane lists; a degree beyond them takes the two-pass CSR form (1)
static int scan_adaptive(Call& c) {
    const Plan& p = c.p; void* ws = c.r.ws; dagl_ce_info* info = c.r.info;
    SelectArgs& sa = c.sa; EdgeArgs& ea = c.ea;
    int32_t* lidx = at<int32_t>(ws, p.o_lidx);
    float* lval = at<float>(ws, p.o_lval);
    int32_t* cnt = at<int32_t>(ws, p.o_cnt);
    int32_t* segcnt = at<int32_t>(ws, p.o_segcnt);
    int32_t* segrel = at<int32_t>(ws, p.o_segoff);
    int32_t* deg = at<int32_t>(ws, p.o_deg);
    int rc;
    DAGL_HIP_TRY(hipMemsetAsync(cnt, 0, c.BL * sizeof(int32_t), c.s));
    sa.cnt = cnt; sa.seg_cnt = segcnt; sa.list_idx = lidx; sa.list_val = lval;
    if ((rc = launch_score_select(c.s, sa, 0))) return rc;
    if (!p.screen) mark(c, 5);
    if ((rc = launch_row_degree(c.s, (int)c.BL, p.splits * 2, segcnt, segrel, deg, c.stats))) return rc;
    int64_t hs[STAT_MAX_DEGREE + 1] = {0};
    if ((rc = read_back(c.s, c.stats, STAT_MAX_DEGREE + 1, hs))) return rc;
    const int64_t edges = hs[STAT_EDGES], max_deg = hs[STAT_MAX_DEGREE];
    if (info) { info->total_edges = edges; info->max_degree = (int32_t)max_deg; info->path = 0; }
    if (max_deg <= DAGL_FAST_CAP) {
        ea.cnt = deg; ea.list_idx = lidx; ea.list_val = lval; ea.row_off = nullptr;
        return launch_edge_softmax(c.s, ea);
    }
    // two-pass CSR: exact degrees are known, refill deterministically at per-lane cursors
    Carver cv(ws, p.o_end);
    const size_t e = (size_t)edges;
    int32_t* csr_idx = cv.take<int32_t>(e);
    float* csr_val = cv.take<float>(e);
    int32_t* csr_nb_idx = cv.take<int32_t>(e);
    float* csr_nb_wgt = cv.take<float>(e);
    const size_t off = cv.bytes();
    if (info) { info->required_bytes = (int64_t)off; info->path = 1; }
    if (c.core) {
        if (info) info->required_bytes = -1;
        set_error("dagl_ce_core_forward: dense neighbourhoods (max degree %lld > %d) do not fit fixed-width lists: "
                  "use dagl_ce_core_dense_forward", (long long)max_deg, DAGL_FAST_CAP);
        return DAGL_ERR_UNSUPPORTED;
    }
    if (c.r.ws_bytes < off) {
        set_error("dagl_ce_forward: dense neighbourhoods (max degree %lld, %lld edges) need workspace %zu B, have %zu B",
                  (long long)max_deg, (long long)edges, off, c.r.ws_bytes);
        return DAGL_ERR_WORKSPACE;
    }
    int64_t* rowoff = at<int64_t>(ws, p.o_rowoff);
    if ((rc = launch_row_scan(c.s, (int)c.BL, deg, rowoff))) return rc;
    sa.list_idx = csr_idx; sa.list_val = csr_val; sa.seg_rel = segrel; sa.row_off = rowoff;
    if ((rc = launch_score_select(c.s, sa, 1))) return rc;
    ea.cnt = deg; ea.list_idx = sa.list_idx; ea.list_val = sa.list_val; ea.row_off = rowoff;
    ea.nb_idx = csr_nb_idx; ea.nb_wgt = csr_nb_wgt;
    if ((rc = launch_edge_softmax(c.s, ea))) return rc;
    c.ag.nb_idx = ea.nb_idx; c.ag.nb_wgt = ea.nb_wgt; c.ag.row_off = rowoff;
    return DAGL_OK;
}

// path 2, top-k modes: per-lane top-k lists of the fp32 scan; behind the screen only the query groups it flagged
static int scan_topk(Call& c) {
    const Plan& p = c.p; void* ws = c.r.ws;
    SelectArgs& sa = c.sa; EdgeArgs& ea = c.ea;
    int rc;
    sa.cand_idx = at<int32_t>(ws, p.o_cidx); sa.cand_val = at<float>(ws, p.o_cval);
    ea.cand_idx = sa.cand_idx; ea.cand_val = sa.cand_val;
    if (c.no_redo) {
        // DAGL_FLAG_NO_REDO: the caller has seen this workspace's recent calls without redo work and does without the launch (4.7 us
        // that find nothing); a call that flagged a group after all is NaN-filled by the gather kernel and reported (sticky)
        c.ag.unserved = c.stats + STAT_FLAGGED; c.ag.unserved_sticky = stat32(c.stats, STAT_NO_REDO_STICKY);
    } else if (p.screen) {
        // redo pass behind the screen: scan + merge of the flagged groups in one launch (exits after one load when nothing
        // is flagged); its grid barrier counts in STAT_OVF_COUNT (cleared with the call's counters, unused by the top-k modes)
        if ((rc = launch_topk_redo(c.s, sa, ea, c.mode == DAGL_MODE_TOPK ? 2 : 3, reinterpret_cast<unsigned*>(c.stats + STAT_OVF_COUNT),
                                   c.topk_policy ? stat32(c.stats, STAT_POLICY) : nullptr))) return rc;
    } else {
        if ((rc = launch_score_select(c.s, sa, c.mode == DAGL_MODE_TOPK ? 2 : 3))) return rc;
        mark(c, 5);
        if ((rc = launch_edge_softmax(c.s, ea))) return rc;
    }
    if (c.r.info && !p.screen) { c.r.info->path = 2; c.r.info->max_degree = c.k; }
    return DAGL_OK;
}

// the fp32 scan (select.hip) and the tail: every call without the screen, and the screened calls it redoes
static int select_scan(Call& c) {
    const int rc = (c.mode == DAGL_MODE_ADAPTIVE) ? scan_adaptive(c) : scan_topk(c);
    return rc ? rc : stage_tail(c);
}

// The adaptive mode's verdict on a screened call.  Dense neighbourhoods need host-side CSR sizing, so the verdict must be read
// back.  Everything it consists of is known once the flagged queries' chunk statistics exist (their true degrees): the copy is
// queued there, the optimistic gather, the flagged rows' weighted sums and the fold behind it, and the host waits for the copy
// alone -- the device works through the round trip and through the caller's next launches.
// DAGL_FLAG_NO_WAIT: the verdict is formed on the device, the call returns without reading it (no host round trip: the adaptive
// forward can be captured into a HIP graph); an unserved call is NaN-filled, never wrong
static int screened_verdict(Call& c) {
    const Plan& p = c.p; dagl_ce_info* info = c.r.info;
    int rc;
    if (c.no_wait) c.rt.veto = stat32(c.stats, STAT_VETO);
    if (c.ovf_active) {           // the flagged rows redone (three launches that exit at once when there are none) + the call's statistics
        // (a call that does not wait shares the scores' launch with the gather over the lists; one that waits keeps the gather
        // behind the read-back: the host round trip runs under it)
        if ((rc = launch_overflow_rows(c.s, overflow_args(c), c.no_wait ? &c.ag : nullptr, c.BL, c.stats,
                                       c.no_wait ? stat32(c.stats, STAT_VETO) : nullptr, c.rt.tag))) return rc;
        c.agg_done = c.no_wait;
    } else {
        if ((rc = launch_degree_stats(c.s, c.BL, c.nbcnt, c.stats))) return rc;
    }
    if (c.no_wait) return stage_tail(c);                 // info: path 3, statistics not read (-1)
    constexpr int n = STAT_REDONE_EDGES + 1;
    int64_t hs[n] = {0};
    bool pending = false;
    if ((rc = read_back_begin(c.s, c.stats, n, &pending))) return rc;
    if ((rc = stage_tail(c))) return rc;
    if ((rc = read_back_end(c.s, c.stats, n, pending, hs))) return rc;
    if ((c.left_range = (int32_t)hs[STAT_RANGE] == c.rt.tag)) return DAGL_OK;
    const int64_t flagged = hs[STAT_FLAGGED];
    if (info) info->redone_queries = flagged;
    // most queries overflow, or the flagged rows are too heavy to redo one by one (the attend kernels saw the same
    // word and left them alone): dense regime
    const bool heavy_rows = c.ovf_active && flagged > 0 && flagged <= p.ovf_cap && hs[STAT_REDONE_EDGES] > c.ovf_edge_limit;
    const bool mostly = flagged * 2 > (int64_t)c.BL || heavy_rows;
    if (flagged == 0 || (!mostly && c.ovf_active && flagged <= p.ovf_cap)) {   // (few overflowed queries: redone in-stream)
        if (info) { info->total_edges = hs[STAT_EDGES]; info->max_degree = (int32_t)hs[STAT_MAX_DEGREE]; }
        return DAGL_OK;
    }
    c.ovf_active = false; c.agg_done = false;
    if (mostly) return select_dense(c, false);
    return select_scan(c);                               // redo everything with the fp32 scan (CSR capable)
}

// path 3: bf16 screen + exact refine (screen.hip)
static int select_screened(Call& c) {
    const Plan& p = c.p; void* ws = c.r.ws; dagl_ce_info* info = c.r.info;
    int rc;
    if (c.mode == DAGL_MODE_ADAPTIVE && (c.r.mode_flags & DAGL_FLAG_DENSE_HINT) && (!c.core || c.core->lse)) {
        mark(c, 3); mark(c, 4); mark(c, 5);
        return select_dense(c, c.split_p != nullptr);
    }
    const ScreenArgs sc = screen_args(c);
    float* theta = at<float>(ws, p.o_theta);
    int32_t* policy = stat32(c.stats, STAT_POLICY);
    mark(c, 3);
    if (c.mode != DAGL_MODE_ADAPTIVE) {                     // top-k threshold from the sampling pass
        bool fused = false;
        if (c.pivot) {                                      // ... over the two heaviest keys of every 64 (pivot.hip)
            PivotArgs pv;
            memset(&pv, 0, sizeof(pv));
            pv.B = c.B; pv.N = c.g.N; pv.n_blk = (c.g.N + 63) / 64; pv.steps = p.pv_steps;
            pv.rowsum = at<float>(ws, p.o_rowsum); pv.xh = c.Xh; pv.rows_xh = sc.rows_xh;
            pv.xp = at<uint16_t>(ws, p.o_xp); pv.rows_xp = sc.rows_xp; pv.pidx = at<int32_t>(ws, p.o_pidx); pv.policy = sc.policy;
            // one launch picks, fetches and scores them (pivot_sample_kernel); DAGL_PIVOT_SAMPLE=0 keeps the two launches with the
            // pivot matrix between them: the same results, for comparing the two
            static const bool one_launch = [] { const char* e = getenv("DAGL_PIVOT_SAMPLE"); return !(e && atoi(e) == 0); }();
            fused = one_launch && pivot_sample_serves(sc);
            if ((rc = fused ? launch_pivot_sample(c.s, sc, pv) : launch_pivot_keys(c.s, pv))) return rc;
        }
        if (!fused && (rc = launch_screen(c.s, sc, 0))) return rc;
        if ((rc = launch_screen_theta(c.s, (int)c.BL, p.s_splits * 2 * p.s_gkeep, c.k, sc.gmax, theta, nullptr, sc.spill_cnt))) return rc;
    }
    if (c.mode != DAGL_MODE_TOPK && !c.fused_theta)         // adaptive threshold; the intersection mode takes the larger
        if ((rc = launch_adaptive_theta(c.s, c.BL, c.mt, c.bias, theta, c.mode == DAGL_MODE_ADAPTIVE_TOPK))) return rc;
    mark(c, 4);
    if ((rc = launch_screen(c.s, sc, 1))) return rc;
    mark(c, 5);
    RefineArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.B = c.B; ra.L = c.g.L; ra.N = c.g.N; ra.mode = c.mode; ra.k = c.k; ra.splits = p.s_splits; ra.capseg = p.capseg;
    ra.width = p.width; ra.wq = c.Wq; ra.x = c.X; ra.rows_q = feat_rows(c.g.L); ra.rows_x = feat_rows(c.g.N);
    ra.mt = c.mt; ra.bs = c.bias; ra.cand = sc.cand; ra.theta = sc.theta; ra.spill = sc.spill; ra.spill_cnt = sc.spill_cnt;
    ra.nb_idx = c.nbidx; ra.nb_wgt = c.nbwgt; ra.nb_cnt = c.nbcnt; ra.redo_flags = c.redo; ra.n_qgroups_exact = c.n_qgroups;
    ra.stats = c.stats; ra.nb_s = c.core ? c.core->nb_s : nullptr;
    if (p.ovf_cap > 0) {
        ra.ovf_list = at<int32_t>(ws, p.o_ovflist); ra.ovf_count = stat32(c.stats, STAT_OVF_COUNT); ra.ovf_cap = p.ovf_cap;
        ra.ovf_qrows = at<float>(ws, p.o_ovfq);
        ra.heavy_list = at<int32_t>(ws, p.o_heavy); ra.heavy_count = stat32(c.stats, STAT_OVF_COUNT) + 1;   // (cleared with the counters)
        c.ovf_active = true;
    }
    if (c.topk_policy) { ra.policy = policy; ra.capseg_tight = p.capseg_tight; }
    if ((rc = launch_refine(c.s, ra))) return rc;
    if (c.topk_policy && !c.prepared) {
        // cold workspace: did the sampled threshold overflow most queries' slots (natural-image features)?  Then the policy word
        // flips here and sampling, threshold, filter and refine run once more, tight, in this very call -- four launches that
        // exit at once otherwise -- instead of every query group taking the fp32 redo pass (2.7 ms at 256^2)
        int32_t* gate = stat32(c.stats, STAT_GATE);
        if ((rc = launch_topk_policy(c.s, c.stats, policy, gate, c.redo, (int)(c.B * c.n_qgroups), (long long)c.BL))) return rc;
        ScreenArgs sc2 = sc; sc2.gate = gate;
        if ((rc = launch_screen(c.s, sc2, 0))) return rc;
        if ((rc = launch_screen_theta(c.s, (int)c.BL, p.s_splits * 2 * p.s_gkeep, c.k, sc2.gmax, theta, gate, sc2.spill_cnt))) return rc;
        // (the intersection mode takes the larger of the two thresholds: max(adaptive, theta) is idempotent, so the ungated
        // kernel is harmless when the re-run did not run)
        if (c.mode != DAGL_MODE_TOPK && !c.fused_theta)
            if ((rc = launch_adaptive_theta(c.s, c.BL, c.mt, c.bias, theta, true))) return rc;
        if ((rc = launch_screen(c.s, sc2, 1))) return rc;
        RefineArgs ra2 = ra; ra2.gate = gate;
        if ((rc = launch_refine(c.s, ra2))) return rc;
    }
    if (info) info->path = 3;
    if (c.mode == DAGL_MODE_ADAPTIVE) return screened_verdict(c);
    // top-k modes: query groups whose candidate slots overflowed are redone by the fp32 scan; it exits at once for every other
    // group, so no host round trip is needed
    c.sa.run_flags = c.redo; c.ea.run_flags = c.redo; c.sa.run_count = c.stats + STAT_FLAGGED; c.ea.run_count = c.stats + STAT_FLAGGED;
    if (info && (c.r.dbg_deg || c.r.dbg_rowsum || c.r.dbg_agg)) {        // debug entry point: report the overflow count
        int64_t hs[STAT_N_COUNTERS] = {0};
        if ((rc = read_back(c.s, c.stats, STAT_N_COUNTERS, hs))) return rc;
        info->redone_queries = hs[STAT_FLAGGED];
    }
    return select_scan(c);
}

// One forward: plan, checks, stages.  `left_range`: a statistics read-back found that an operand left the split-fp16 range
static int forward_once(const ForwardRequest& r, bool& left_range) {
    Plan p;
    int rc = make_plan(r.B, r.H, r.W, r.mode_flags, r.k, p, r.core != nullptr);
    if (rc) return rc;
    reset_info(r.info, (int64_t)p.o_end, 0);
    if ((rc = check_request(r, p))) return rc;
    Call c(r, p);
    if ((rc = stage_layout(c)) || (rc = stage_project(c)) || (rc = stage_thresholds(c))) return rc;
    if (p.wide) rc = select_wide(c);
    else if (p.screen) rc = select_screened(c);
    else { mark(c, 3); mark(c, 4); rc = select_scan(c); }
    left_range = c.left_range;
    return rc;
}

// Every forward entry point ends here: the profile counts the call, and a call that left the split-fp16 range -- which only the
// statistics read-backs see; without one the poisoned output and dagl_ce_range_check report it -- is re-run once on the fp32 path
// (same arguments, DAGL_FLAG_EXACT_SCAN).  Neither a fallback call nor its re-run is counted.
static int ce_forward(const ForwardRequest& r) {
    bool left_range = false;
    int rc = forward_once(r, left_range);
    if (rc != DAGL_OK) return rc;
    if (!left_range) {
        if (r.prof && r.prof->n_calls < r.prof->max_calls) ++r.prof->n_calls;
        return DAGL_OK;
    }
    if (r.info) r.info->range_fallback = 1;
    // the training entry point: non-finite features, `out` NaN-filled (dagl_ce_core_dense_forward re-runs the GEMM form).  Already the
    // fp32 path: the word was set by a NON-FINITE feature (round 6), the output is NaN-filled as the reference's would be.  Nothing to re-run
    if (r.core || (r.mode_flags & DAGL_FLAG_EXACT_SCAN)) return DAGL_OK;
    if (r.heads > 1) {            // stage entry point: no fp32 form of the four-head launch set; hand the call back (per-head path)
        if (r.info) r.info->required_bytes = -1;
        set_error("dagl_ces_stage_forward: an operand left the split-fp16 range: use the per-head entry point");
        return DAGL_ERR_WORKSPACE;
    }
    ForwardRequest exact = r;
    exact.mode_flags = (r.mode_flags | DAGL_FLAG_EXACT_SCAN) & ~(DAGL_FLAG_WEIGHTS_PACKED | DAGL_FLAG_DENSE_HINT);
    exact.prof = nullptr;
    rc = forward_once(exact, left_range);      // (left_range again: a non-finite input -- the output is NaN-filled)
    if (r.info) r.info->range_fallback = 1;
    return rc;
}

}  // namespace dagl

using namespace dagl;

extern "C" {

int dagl_version(void) { return DAGL_ABI_VERSION; }

const char* dagl_last_error(void) { return g_err; }

int dagl_device_check(void) { return check_device(); }

size_t dagl_ce_workspace_bytes(int B, int H, int W, int mode, int k) {
    Plan p;
    if (make_plan(B, H, W, mode, k, p)) return 0;
    return p.o_end;
}

int dagl_ce_forward(void* stream, int B, int H, int W, const float* b1, const float* b2, const float* thr,
                    const float* bias, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                    const float* fc2_b, int mode, int k, float* out, void* workspace, size_t ws_bytes,
                    dagl_ce_info* info) {
    const MapsIn in{b1, b2, thr, bias, fc1_w, fc1_b, fc2_w, fc2_b};
    ForwardRequest r(stream, B, H, W, mode, k, out, workspace, ws_bytes, info);
    r.maps = &in;
    return ce_forward(r);
}

int dagl_ce_forward_debug(void* stream, int B, int H, int W, const float* b1, const float* b2, const float* thr,
                          const float* bias, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                          const float* fc2_b, int mode, int k, float* out, void* workspace, size_t ws_bytes,
                          dagl_ce_info* info, int32_t* deg_out, float* rowsum_out, float* agg_out) {
    const MapsIn in{b1, b2, thr, bias, fc1_w, fc1_b, fc2_w, fc2_b};
    ForwardRequest r(stream, B, H, W, mode, k, out, workspace, ws_bytes, info);
    r.maps = &in;
    r.dbg_deg = deg_out; r.dbg_rowsum = rowsum_out; r.dbg_agg = agg_out;
    return ce_forward(r);
}

int dagl_ce_pivot_debug(void* stream, int B, int H, int W, int mode, int k, void* workspace, size_t ws_bytes, int32_t* pivot_idx_out,
                        float* key_rowsum_out) {
    Plan p;
    int rc = make_plan(B, H, W, mode, k, p);
    if (rc) return rc;
    if (!p.pivot || (mode & DAGL_FLAG_TIGHT_TOPK)) {
        set_error("dagl_ce_pivot_debug: calls of this shape / mode / k do not take their threshold from pivot keys");
        return DAGL_ERR_UNSUPPORTED;
    }
    DAGL_REQUIRE(pivot_idx_out || key_rowsum_out, "dagl_ce_pivot_debug: null output pointers");
    if ((rc = check_workspace("dagl_ce_pivot_debug", workspace, ws_bytes, p.o_end))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (pivot_idx_out)
        DAGL_HIP_TRY(hipMemcpyAsync(pivot_idx_out, at<int32_t>(workspace, p.o_pidx), (size_t)B * ((p.g.N + 63) / 64) * 2 * sizeof(int32_t),
                                    hipMemcpyDeviceToDevice, s));
    if (key_rowsum_out && (rc = launch_pivot_rowsum(s, (size_t)B * p.g.N, at<float>(workspace, p.o_rowsum), key_rowsum_out))) return rc;
    return DAGL_OK;
}

int dagl_ce_wide_debug(void* stream, int B, int H, int W, int mode, int k, void* workspace, size_t ws_bytes, int32_t* served_out) {
    Plan p;
    int rc = make_plan(B, H, W, mode, k, p);
    if (rc) return rc;
    const int32_t* served = nullptr; int rows = 0;
    if (!p.wide || topk_wide_served(p.k, p.g.N, p.g.L, nullptr, &served, &rows)) {
        set_error("dagl_ce_wide_debug: calls of this mode / k run no list kernel (not the wide path, or k > 1024)");
        return DAGL_ERR_UNSUPPORTED;
    }
    DAGL_REQUIRE(served_out, "dagl_ce_wide_debug: null output pointer");
    if ((rc = check_workspace("dagl_ce_wide_debug", workspace, ws_bytes, p.o_end))) return rc;
    (void)topk_wide_served(p.k, p.g.N, p.g.L, at<char>(workspace, p.o_wide), &served, &rows);
    DAGL_HIP_TRY(hipMemcpyAsync(served_out, served, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return DAGL_OK;
}

int dagl_profile_create(int max_calls, dagl_profile** out) {
    DAGL_REQUIRE(max_calls >= 1 && max_calls <= 4096 && out, "dagl_profile_create: bad argument");
    Profile* p = new Profile();
    p->max_calls = max_calls;
    const size_t n = (size_t)max_calls * (DAGL_N_STAGES + 1);
    p->ev = new hipEvent_t[n];
    for (size_t i = 0; i < n; ++i) {
        hipError_t e = hipEventCreate(&p->ev[i]);
        if (e != hipSuccess) {
            for (size_t j = 0; j < i; ++j) (void)hipEventDestroy(p->ev[j]);
            delete[] p->ev; delete p;
            return hip_fail(e, "hipEventCreate");
        }
    }
    *out = reinterpret_cast<dagl_profile*>(p);
    return DAGL_OK;
}

int dagl_profile_destroy(dagl_profile* prof) {
    Profile* p = reinterpret_cast<Profile*>(prof);
    if (!p) return DAGL_OK;
    const size_t n = (size_t)p->max_calls * (DAGL_N_STAGES + 1);
    for (size_t i = 0; i < n; ++i) (void)hipEventDestroy(p->ev[i]);
    delete[] p->ev; delete p;
    return DAGL_OK;
}

int dagl_profile_select_stage(dagl_profile* prof, int stage) {
    Profile* p = reinterpret_cast<Profile*>(prof);
    DAGL_REQUIRE(p && stage >= -1 && stage < DAGL_N_STAGES, "dagl_profile_select_stage: bad argument");
    p->only_stage = stage;
    p->n_calls = 0;
    return DAGL_OK;
}

int dagl_profile_reset(dagl_profile* prof) {
    Profile* p = reinterpret_cast<Profile*>(prof);
    DAGL_REQUIRE(p, "dagl_profile_reset: null profile");
    p->n_calls = 0;
    return DAGL_OK;
}

int dagl_profile_read(dagl_profile* prof, int* n_calls, float* stage_ms, int capacity_calls) {
    Profile* p = reinterpret_cast<Profile*>(prof);
    DAGL_REQUIRE(p && n_calls, "dagl_profile_read: null argument");
    *n_calls = p->n_calls;
    if (!stage_ms) return DAGL_OK;
    const int n = p->n_calls < capacity_calls ? p->n_calls : capacity_calls;
    for (int c = 0; c < n; ++c) {
        hipEvent_t* e = p->ev + (size_t)c * (DAGL_N_STAGES + 1);
        DAGL_HIP_TRY(hipEventSynchronize(e[p->only_stage < 0 ? DAGL_N_STAGES : p->only_stage + 1]));
        for (int st = 0; st < DAGL_N_STAGES; ++st) {
            float ms = 0.f;
            if (p->only_stage < 0 || st == p->only_stage) DAGL_HIP_TRY(hipEventElapsedTime(&ms, e[st], e[st + 1]));
            stage_ms[(size_t)c * DAGL_N_STAGES + st] = ms;
        }
    }
    return DAGL_OK;
}

int dagl_ce_forward_profiled(void* stream, int B, int H, int W, const float* b1, const float* b2, const float* thr,
                             const float* bias, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                             const float* fc2_b, int mode, int k, float* out, void* workspace, size_t ws_bytes,
                             dagl_ce_info* info, dagl_profile* prof) {
    const MapsIn in{b1, b2, thr, bias, fc1_w, fc1_b, fc2_w, fc2_b};
    ForwardRequest r(stream, B, H, W, mode, k, out, workspace, ws_bytes, info);
    r.maps = &in;
    r.prof = reinterpret_cast<Profile*>(prof);
    return ce_forward(r);
}

int dagl_ce_forward_fused(void* stream, int B, int H, int W, const float* x, const float* g_w, const float* g_b,
                          const float* theta_w, const float* theta_b, const float* thr_w, const float* thr_b,
                          const float* bias_w, const float* bias_b, const float* fc1_w, const float* fc1_b,
                          const float* fc2_w, const float* fc2_b, int mode, int k, float* out, void* workspace,
                          size_t ws_bytes, dagl_ce_info* info, dagl_profile* prof) {
    const FusedIn fin{x, g_w, g_b, theta_w, theta_b, thr_w, thr_b, bias_w, bias_b, fc1_w, fc1_b, fc2_w, fc2_b};
    ForwardRequest r(stream, B, H, W, mode, k, out, workspace, ws_bytes, info);
    r.fin = &fin;
    r.prof = reinterpret_cast<Profile*>(prof);
    return ce_forward(r);
}

size_t dagl_ces_stage_workspace_bytes(int B, int H, int W, int mode, int k) {
    Plan p;
    if (B < 1 || make_plan(4 * B, H, W, mode, k, p)) return 0;
    return p.o_end + align_up((size_t)B * 64 * H * W * sizeof(float), 256);
}

int dagl_ces_stage_forward(void* stream, int B, int H, int W, const float* x, const dagl_ce_weights* heads4,
                           const float* mix_w, const float* mix_b, int mode, int k, float* out, void* workspace,
                           size_t ws_bytes, dagl_ce_info* info, dagl_profile* prof) {
    DAGL_REQUIRE(B >= 1 && x && heads4 && mix_w && mix_b && out, "dagl_ces_stage_forward: bad argument");
    Plan p;
    int rc = make_plan(4 * B, H, W, mode, k, p);
    if (rc) return rc;
    const size_t cat_bytes = align_up((size_t)B * 64 * H * W * sizeof(float), 256);
    if (info) info->required_bytes = (int64_t)(p.o_end + cat_bytes);
    if ((rc = check_workspace("dagl_ces_stage_forward", workspace, ws_bytes, p.o_end + cat_bytes))) return rc;
    FusedIn fin[4];
    for (int h = 0; h < 4; ++h) {
        const dagl_ce_weights& w = heads4[h];
        fin[h] = FusedIn{x, w.g_w, w.g_b, w.theta_w, w.theta_b, w.thr_w, w.thr_b, w.bias_w, w.bias_b,
                         w.fc1_w, w.fc1_b, w.fc2_w, w.fc2_b};
        DAGL_REQUIRE(w.g_w && w.g_b && w.theta_w && w.theta_b && w.fc1_w && w.fc1_b && w.fc2_w && w.fc2_b,
                     "dagl_ces_stage_forward: head %d has a null weight pointer", h);
    }
    float* cat = at<float>(workspace, p.o_end);       // [B,64,H,W]
    // a dense adaptive neighbourhood asks for more workspace than planned: give the block everything up to the concat map
    ForwardRequest r(stream, 4 * B, H, W, mode, k, cat, workspace, p.o_end, info);
    r.fin = fin; r.heads = 4;
    r.prof = reinterpret_cast<Profile*>(prof);
    rc = ce_forward(r);
    if (rc) {
        if (rc == DAGL_ERR_WORKSPACE && info) info->required_bytes = -1;    // dense neighbourhoods: use the per-head entry point
        return rc;
    }
    return launch_stage_mix((hipStream_t)stream, B, H * W, cat, x, mix_w, mix_b, out);
}

int dagl_ce_range_check(void* stream, int B, int H, int W, int mode, int k, void* workspace, size_t ws_bytes,
                        int* violated) {
    DAGL_REQUIRE(workspace && violated, "dagl_ce_range_check: null pointer");
    Plan p;
    int rc = make_plan(B, H, W, mode, k, p);
    if (rc) return rc;
    DAGL_REQUIRE(ws_bytes >= p.o_end && ((uintptr_t)workspace % 256) == 0, "dagl_ce_range_check: not the workspace of such a call");
    *violated = 0;
    if (mode & DAGL_FLAG_EXACT_SCAN) return DAGL_OK;                      // the fp32 path has no such range (and always waits)
    // ONE read-back (one synchronisation) of the statistics words STAT_FLAGGED .. STAT_NO_REDO_STICKY
    int64_t hw[STAT_WORDS] = {0};
    int64_t* st = at<int64_t>(workspace, p.o_stats);
    if ((rc = read_back((hipStream_t)stream, st + STAT_FLAGGED, STAT_NO_REDO_STICKY + 1 - STAT_FLAGGED, hw + STAT_FLAGGED))) return rc;
    const bool topk_screen = (mode & 0xff) != DAGL_MODE_ADAPTIVE && p.screen;
    // sticky: the word keeps the tag of the last call that left the range until it is read here (calls that reuse a
    // prepared workspace do not clear it), so a poll every n-th call sees a violation of ANY call since the last poll
    if ((int32_t)hw[STAT_RANGE] != 0) { *violated |= 1; DAGL_HIP_TRY(hipMemsetAsync(st + STAT_RANGE, 0, sizeof(int64_t), (hipStream_t)stream)); }
    // bit 2 (not sticky: the count is cleared by every call): the last call's redo pass of the top-k modes had work
    if (topk_screen && hw[STAT_FLAGGED] > 0) *violated |= 4;
    if (topk_screen && (int32_t)hw[STAT_POLICY] != 0) *violated |= 8;            // bit 3: the workspace's threshold policy word says "tight"
    // bit 4 (sticky): a DAGL_FLAG_NO_REDO call had flagged groups (its output is NaN-filled)
    if (topk_screen && (int32_t)hw[STAT_NO_REDO_STICKY] != 0) { *violated |= 16; DAGL_HIP_TRY(hipMemsetAsync(st + STAT_NO_REDO_STICKY, 0, sizeof(int64_t), (hipStream_t)stream)); }
    // bit 1: a DAGL_FLAG_NO_WAIT call was not served in-stream (likewise sticky)
    if ((mode & 0xff) == DAGL_MODE_ADAPTIVE && (int32_t)hw[STAT_VETO] != 0) {
        *violated |= 2; DAGL_HIP_TRY(hipMemsetAsync(st + STAT_VETO, 0, sizeof(int64_t), (hipStream_t)stream));
    }
    return DAGL_OK;
}

int dagl_ce_list_width(int mode, int k) {
    const int m = mode & 0xff;
    if (m == DAGL_MODE_ADAPTIVE) return DAGL_FAST_CAP;
    if ((m == DAGL_MODE_TOPK || m == DAGL_MODE_ADAPTIVE_TOPK) && k >= 1 && k <= DAGL_MAX_TOPK) return k;
    set_error("dagl_ce_list_width: bad mode 0x%x / k=%d", mode, k);
    return DAGL_ERR_INVALID;
}

int dagl_ce_core_forward(void* stream, int B, int H, int W, const float* wq_rows, const float* x_rows, const float* b2,
                         const float* thr, const float* bias, int mode, int k, float* out, int32_t* nb_idx,
                         float* nb_wgt, float* nb_s, int32_t* nb_cnt, float* mu, void* workspace, size_t ws_bytes,
                         dagl_ce_info* info) {
    const CoreIn core{wq_rows, x_rows, b2, thr, bias, nb_idx, nb_wgt, nb_s, nb_cnt, mu, nullptr};
    ForwardRequest r(stream, B, H, W, mode, k, out, workspace, ws_bytes, info);
    r.core = &core;
    return ce_forward(r);
}

// the list backward's workspace: the one walk that sizes it (null base) and hands its regions to the launch
struct BwdWs { float* dagg; float* b2p; float* dS; float* dmu; double* colsum; float* dxbar; BwdSortWs sort; size_t bytes; };
static BwdWs backward_carve(void* ws, int B, const Grid& g, int width) {
    Carver cv(ws);
    const size_t BL = (size_t)B * g.L, E = BL * width, n_keys = (size_t)B * g.N;
    BwdWs w;
    w.dagg = cv.take<float>(BL * P);
    w.b2p = cv.take<float>((size_t)B * g.Hp * g.Wp * CH);                       // b2 padded NHWC
    w.dS = cv.take<float>(E);
    w.dmu = cv.take<float>(BL);
    w.colsum = reinterpret_cast<double*>(cv.take<char>((size_t)B * DS * sizeof(double) + (size_t)B * D * sizeof(float)));
    w.dxbar = reinterpret_cast<float*>(w.colsum + (size_t)B * DS);              // (d Xbar shares the column sums' region)
    w.sort.keys_in = cv.take<uint32_t>(E); w.sort.keys_out = cv.take<uint32_t>(E);      // sort keys / edge ids, in and out
    w.sort.vals_in = cv.take<uint32_t>(E); w.sort.vals_out = cv.take<uint32_t>(E);
    w.sort.seg = cv.take<uint32_t>(2 * n_keys);                                 // run of every key
    w.sort.temp_bytes = edge_sort_temp_bytes(E, n_keys);
    w.sort.temp = cv.take<char>(w.sort.temp_bytes);
    w.sort.rowbuf = cv.take<float>(edge_rowbuf_floats(E));
    w.sort.part = cv.take<float>(edge_part_floats(E));
    w.bytes = cv.bytes();
    return w;
}

size_t dagl_ce_core_backward_workspace_bytes(int B, int H, int W, int mode, int k) {
    const int width = dagl_ce_list_width(mode, k);
    if (B < 1 || H < 1 || W < 1 || width < 0) return 0;
    return backward_carve(nullptr, B, make_grid(H, W), width).bytes;
}

int dagl_ce_core_backward(void* stream, int B, int H, int W, int mode, int k, const float* wq_rows, const float* x_rows,
                          const float* b2, const float* thr, const float* bias, const int32_t* nb_idx,
                          const float* nb_wgt, const float* nb_s, const int32_t* nb_cnt, const float* mu,
                          const float* d_out, float* d_wq_rows, float* d_x_rows, float* d_b2, float* d_thr,
                          float* d_bias, void* workspace, size_t ws_bytes) {
    const int width = dagl_ce_list_width(mode, k);
    if (width < 0) return width;
    const int m = mode & 0xff;
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1, "dagl_ce_core_backward: bad shape");
    DAGL_REQUIRE(wq_rows && x_rows && b2 && nb_idx && nb_wgt && nb_s && nb_cnt && d_out && d_wq_rows && d_x_rows && d_b2,
                 "dagl_ce_core_backward: null tensor pointer");
    if (m != DAGL_MODE_TOPK)
        DAGL_REQUIRE(thr && bias && mu && d_thr && d_bias, "dagl_ce_core_backward: thr/bias/mu and their gradients required in adaptive modes");
    int rc;
    if ((rc = check_workspace("dagl_ce_core_backward", workspace, ws_bytes, 0))) return rc;
    const Grid g = make_grid(H, W);
    DAGL_REQUIRE((size_t)B * g.L * width < (1ull << 31) && (size_t)B * g.N < (1ull << 31), "dagl_ce_core_backward: batch too large for 32-bit edge ids");
    const BwdWs w = backward_carve(workspace, B, g, width);
    if ((rc = check_workspace("dagl_ce_core_backward", workspace, ws_bytes, w.bytes))) return rc;
    hipStream_t s = (hipStream_t)stream;
    BwdArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.g = g; a.mode = m; a.width = width;
    a.wq_rows = wq_rows; a.x_rows = x_rows; a.thr = thr; a.bs = bias; a.mu = mu;
    a.nb_idx = nb_idx; a.nb_wgt = nb_wgt; a.nb_s = nb_s; a.nb_cnt = nb_cnt; a.dout = d_out;
    a.dagg = w.dagg; a.b2p = w.b2p; a.dS = w.dS; a.dmu = w.dmu; a.colsum = w.colsum;
    a.dwq_rows = d_wq_rows; a.dx_rows = d_x_rows; a.dthr = d_thr; a.dbias = d_bias;
    if ((rc = launch_pad_nhwc(s, B, H, W, b2, w.b2p))) return rc;
    if (m != DAGL_MODE_TOPK)
        if ((rc = launch_colsum_rows(s, B, g.N, x_rows, w.colsum))) return rc;
    return launch_core_backward(s, a, w.sort, w.dxbar, d_b2);
}

// total edges / largest degree of a dense-core call, from the two statistics words behind its workspace (info == NULL: not read)
static int read_edge_stats(hipStream_t s, const int64_t* stats, dagl_ce_info* info) {
    if (!info) return DAGL_OK;
    int64_t hs[STAT_MAX_DEGREE + 1] = {0};
    const int rc = read_back(s, stats, STAT_MAX_DEGREE + 1, hs);
    if (rc) return rc;
    info->total_edges = hs[STAT_EDGES]; info->max_degree = (int32_t)hs[STAT_MAX_DEGREE];
    return DAGL_OK;
}

// the chunked fp32 GEMM form of a dense-core forward (a.ws / a.ws_bytes: the caller's buffer): the plan's bytes, then the statistics words
static int dense_train_forward_call(const char* who, hipStream_t s, DenseTrainForward& a, dagl_ce_info* info) {
    const size_t plan_bytes = dense_train_workspace_bytes(a.B, a.g, false), need = plan_bytes + DENSE_TRAIN_STATS_BYTES;
    int rc;
    if ((rc = check_workspace(who, a.ws, a.ws_bytes, need))) {
        if (info) info->required_bytes = (int64_t)need;
        return rc;
    }
    int64_t* stats = at<int64_t>(a.ws, plan_bytes);
    a.ws_bytes = plan_bytes; a.stats = info ? stats : nullptr;
    if ((rc = launch_dense_train_forward(s, a))) return rc;
    return read_edge_stats(s, stats, info);
}

// forward on the inference path's streamed kernel (split-fp16 S and A V in one pass over the keys) when the image has enough
// keys for the screen's machinery it borrows (row-maximum scan); the chunked fp32 GEMM formulation otherwise
static bool dense_core_streamed(int H, int W) { return (int64_t)H * W >= SCREEN_MIN_KEYS; }
static size_t dense_core_streamed_bytes(int B, int H, int W) {
    Plan p;
    if (make_plan(B, H, W, DAGL_MODE_ADAPTIVE | DAGL_FLAG_DENSE_HINT, 0, p, true)) return 0;
    return dense_ws_end(p);
}

size_t dagl_ce_core_dense_workspace_bytes(int B, int H, int W, int backward) {
    if (B < 1 || H < 1 || W < 1) return 0;
    const size_t gemm_form = dense_train_workspace_bytes(B, make_grid(H, W), backward != 0);
    if (backward || !dense_core_streamed(H, W)) return gemm_form;
    const size_t streamed = dense_core_streamed_bytes(B, H, W);
    return streamed > gemm_form ? streamed : gemm_form;
}

long long dagl_ce_core_dense_chunk_floats(long long floats) { return dense_train_chunk_floats(floats); }

int dagl_ce_core_dense_plan(int B, int H, int W, int backward, int32_t out[6]) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && out, "dagl_ce_core_dense_plan: bad argument");
    dense_train_plan(B, make_grid(H, W), backward != 0, out);
    return DAGL_OK;
}

int dagl_ce_core_dense_forward(void* stream, int B, int H, int W, int flags, const float* wq_rows, const float* x_rows,
                               const float* b2, const float* thr, const float* bias, float* out, float* lse, float* mu,
                               void* workspace, size_t ws_bytes, dagl_ce_info* info) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && wq_rows && x_rows && b2 && thr && bias && out && lse && mu &&
                 (flags & ~DAGL_FLAG_EXACT_SCAN) == 0, "dagl_ce_core_dense_forward: bad argument");
    int rc;
    if ((rc = check_workspace("dagl_ce_core_dense_forward", workspace, ws_bytes, 0))) return rc;
    const Grid g = make_grid(H, W);
    bool left_range = false;
    if (dense_core_streamed(H, W) && !(flags & DAGL_FLAG_EXACT_SCAN)) {
        const CoreIn core{wq_rows, x_rows, b2, thr, bias, nullptr, nullptr, nullptr, nullptr, mu, lse};
        ForwardRequest r(stream, B, H, W, DAGL_MODE_ADAPTIVE | DAGL_FLAG_DENSE_HINT, 0, out, workspace, ws_bytes, info);
        r.core = &core;
        const int rc0 = ce_forward(r);
        // a feature outside the split-fp16 range (|feature| >= 937): the streamed kernels NaN-filled `out`; a call that reads
        // its statistics back (info != NULL) notices and is re-run right here in the fp32 GEMM form, which has no such range
        if (rc0 != DAGL_OK || info == nullptr || !info->range_fallback) return rc0;
        left_range = true;
    }
    reset_info(info, (int64_t)dense_train_workspace_bytes(B, g, false), 5);
    DenseTrainForward a;
    a.B = B; a.g = g; a.wq_rows = wq_rows; a.x_rows = x_rows; a.b2 = b2; a.thr = thr; a.bias = bias;
    a.out = out; a.lse = lse; a.mu = mu; a.ws = workspace; a.ws_bytes = ws_bytes;
    if ((rc = dense_train_forward_call("dagl_ce_core_dense_forward", (hipStream_t)stream, a, info))) return rc;
    if (info) info->range_fallback = left_range ? 1 : 0;
    return DAGL_OK;
}

int dagl_ce_core_dense_backward(void* stream, int B, int H, int W, int flags, const float* wq_rows, const float* x_rows, const float* b2,
                                const float* thr, const float* bias, const float* lse, const float* mu, const float* d_out,
                                float* d_wq_rows, float* d_x_rows, float* d_b2, float* d_thr, float* d_bias, void* workspace,
                                size_t ws_bytes) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && wq_rows && x_rows && b2 && thr && bias && lse && mu && d_out && d_wq_rows &&
                 d_x_rows && d_b2 && d_thr && d_bias && (flags & ~DAGL_FLAG_EXACT_SCAN) == 0, "dagl_ce_core_dense_backward: bad argument");
    const int rc = check_workspace("dagl_ce_core_dense_backward", workspace, ws_bytes, 0);
    if (rc) return rc;
    DenseTrainBackward a;
    a.B = B; a.g = make_grid(H, W); a.wq_rows = wq_rows; a.x_rows = x_rows; a.b2 = b2; a.thr = thr; a.bias = bias;
    a.lse = lse; a.dout = d_out; a.dwq_rows = d_wq_rows; a.dx_rows = d_x_rows; a.db2 = d_b2; a.dthr = d_thr; a.dbias = d_bias;
    a.ws = workspace; a.ws_bytes = ws_bytes; a.fp32_products = (flags & DAGL_FLAG_EXACT_SCAN) != 0;
    return launch_dense_train_backward((hipStream_t)stream, a);
}

// ---- top-k modes whose neighbourhoods exceed the lists (min(k, N) > DAGL_MAX_TOPK) under autograd: the dense formulation of
// dense_train.hip with the row-wise selection of topk_wide.hip as its mask ------------------------------------------------------
int dagl_ce_core_wide_forward(void* stream, int B, int H, int W, int mode, int k, const float* wq_rows, const float* x_rows,
                              const float* b2, const float* thr, const float* bias, float* out, void* workspace, size_t ws_bytes,
                              dagl_ce_info* info) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && wq_rows && x_rows && b2 && out && k >= 1 &&
                 (mode == DAGL_MODE_TOPK || mode == DAGL_MODE_ADAPTIVE_TOPK), "dagl_ce_core_wide_forward: bad argument");
    DAGL_REQUIRE(mode == DAGL_MODE_TOPK || (thr && bias), "dagl_ce_core_wide_forward: the intersection mode needs thr and bias");
    int rc;
    if ((rc = check_workspace("dagl_ce_core_wide_forward", workspace, ws_bytes, 0))) return rc;
    const Grid g = make_grid(H, W);
    if (k > g.N) k = g.N;                                              // top_k = min(num_edge, N)
    reset_info(info, (int64_t)(dense_train_workspace_bytes(B, g, false) + DENSE_TRAIN_STATS_BYTES), 5);
    DenseTrainForward a;
    a.B = B; a.g = g; a.mode = mode; a.k = k; a.wq_rows = wq_rows; a.x_rows = x_rows; a.b2 = b2; a.thr = thr; a.bias = bias;
    a.out = out; a.ws = workspace; a.ws_bytes = ws_bytes;
    return dense_train_forward_call("dagl_ce_core_wide_forward", (hipStream_t)stream, a, info);
}

int dagl_ce_core_wide_backward(void* stream, int B, int H, int W, int mode, int k, const float* wq_rows, const float* x_rows,
                               const float* b2, const float* thr, const float* bias, const float* d_out, float* d_wq_rows,
                               float* d_x_rows, float* d_b2, float* d_thr, float* d_bias, void* workspace, size_t ws_bytes) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && wq_rows && x_rows && b2 && d_out && d_wq_rows && d_x_rows && d_b2 && k >= 1 &&
                 (mode == DAGL_MODE_TOPK || mode == DAGL_MODE_ADAPTIVE_TOPK), "dagl_ce_core_wide_backward: bad argument");
    DAGL_REQUIRE(mode == DAGL_MODE_TOPK || (thr && bias && d_thr && d_bias),
                 "dagl_ce_core_wide_backward: the intersection mode needs thr, bias and their gradients");
    const int rc = check_workspace("dagl_ce_core_wide_backward", workspace, ws_bytes, 0);
    if (rc) return rc;
    const Grid g = make_grid(H, W);
    if (k > g.N) k = g.N;
    DenseTrainBackward a;
    a.B = B; a.g = g; a.mode = mode; a.k = k; a.wq_rows = wq_rows; a.x_rows = x_rows; a.b2 = b2; a.thr = thr; a.bias = bias;
    a.dout = d_out; a.dwq_rows = d_wq_rows; a.dx_rows = d_x_rows; a.db2 = d_b2; a.dthr = d_thr; a.dbias = d_bias;
    a.ws = workspace; a.ws_bytes = ws_bytes; a.fp32_products = true;
    return launch_dense_train_backward((hipStream_t)stream, a);
}

size_t dagl_gemm_f32_scratch_floats(int batch, int M, int N, int K) {
    if (batch != 1 || M < 1 || N < 1 || K < 1) return 0;
    const int sl = gemm32_auto_slices(M, N, K);
    return sl > 1 ? (size_t)sl * M * N : 0;
}

int dagl_gemm_f32(void* stream, int batch, int M, int N, int K, const float* A, long long lda, long long stride_a, int a_k_contiguous,
                  const float* B, long long ldb, long long stride_b, int b_k_contiguous, float* C, long long ldc, long long stride_c,
                  float alpha, float beta, const float* bias, int relu, int chunk_tiles, float* scratch) {
    DAGL_REQUIRE(batch >= 1 && M >= 0 && N >= 0 && K >= 1 && lda >= 1 && ldb >= 1 && ldc >= N && chunk_tiles >= 0, "dagl_gemm_f32: bad shape");
    Gemm32 g;
    g.M = M; g.N = N; g.K = K; g.batch = batch; g.A = A; g.lda = lda; g.sA = stride_a; g.a_kc = a_k_contiguous;
    g.B = B; g.ldb = ldb; g.sB = stride_b; g.b_kc = b_k_contiguous; g.C = C; g.ldc = ldc; g.sC = stride_c;
    g.alpha = alpha; g.beta = beta; g.bias = bias; g.relu = relu; g.chunk_tiles = chunk_tiles;
    if (scratch != nullptr && batch == 1) { g.slices = gemm32_auto_slices(M, N, K); g.scratch = scratch; }
    return launch_gemm32((hipStream_t)stream, g);
}

int dagl_ce_prologue(void* stream, int B, int H, int W, const float* x, const float* g_w, const float* g_b,
                     const float* theta_w, const float* theta_b, const float* thr_w, const float* thr_b,
                     const float* bias_w, const float* bias_b, float* b1_nhwc, float* b2_nhwc, float* thr, float* bias,
                     float* scratch) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && x && g_w && g_b && theta_w && theta_b && b1_nhwc && b2_nhwc,
                 "dagl_ce_prologue: bad argument");
    if (thr || bias)
        DAGL_REQUIRE(thr && bias && thr_w && thr_b && bias_w && bias_b && scratch,
                     "dagl_ce_prologue: thr/bias heads incomplete (weights, outputs and 8*B*L floats of scratch)");
    PrologueLaunch pl;
    pl.B = B; pl.g = make_grid(H, W); pl.x = x;
    pl.g_w = g_w; pl.g_b = g_b; pl.th_w = theta_w; pl.th_b = theta_b;
    pl.thr_w = thr_w; pl.thr_b = thr_b; pl.bias_w = bias_w; pl.bias_b = bias_b;
    pl.conv = ConvPath::Fp32;
    pl.b1p = b1_nhwc; pl.b2p = b2_nhwc; pl.thr = thr; pl.bias = bias; pl.thr_part = scratch;
    return launch_prologue((hipStream_t)stream, pl);
}

// (ABI 405) the same four convolutions with g / theta on the fp16 matrix cores (split operands, conv_pair16_kernel: a third of the fp32
// kernel's time) and the key / query map out in fp32 -- the differentiable path's forward.  The input is split with a power-of-two scale
// of each block's own (a second run of the strip when its rows leave |16 x| < 60000): no range on x; |w_conv| < 234 as everywhere.
struct Pro16Ws { unsigned char* convw; float* amax; int slots; float* thr_part; size_t bytes; };
static Pro16Ws prologue16_carve(void* scratch, int B, const Grid& g) {
    Carver cv(scratch);
    Pro16Ws w;
    w.convw = cv.take<unsigned char>(CONV_W16_BYTES);
    w.slots = conv16_blocks_per_head(g, 1, B);
    w.amax = cv.take<float>((size_t)w.slots);
    w.thr_part = cv.take<float>(8 * (size_t)B * g.L);
    w.bytes = cv.bytes();
    return w;
}

size_t dagl_ce_prologue16_scratch_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return prologue16_carve(nullptr, B, make_grid(H, W)).bytes;
}

int dagl_ce_prologue16(void* stream, int B, int H, int W, const float* x, const float* g_w, const float* g_b,
                       const float* theta_w, const float* theta_b, const float* thr_w, const float* thr_b,
                       const float* bias_w, const float* bias_b, float* b1_nhwc, float* b2_nhwc, float* thr, float* bias,
                       void* scratch, size_t scratch_bytes) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && x && g_w && g_b && theta_w && theta_b && b1_nhwc && b2_nhwc && scratch,
                 "dagl_ce_prologue16: bad argument");
    if (thr || bias)
        DAGL_REQUIRE(thr && bias && thr_w && thr_b && bias_w && bias_b, "dagl_ce_prologue16: thr/bias heads incomplete");
    DAGL_REQUIRE(scratch_bytes >= dagl_ce_prologue16_scratch_bytes(B, H, W) && ((uintptr_t)scratch % 256) == 0,
                 "dagl_ce_prologue16: scratch %zu B (256-byte aligned), need %zu B", scratch_bytes, dagl_ce_prologue16_scratch_bytes(B, H, W));
    hipStream_t s = (hipStream_t)stream;
    const Grid g = make_grid(H, W);
    const Pro16Ws w = prologue16_carve(scratch, B, g);
    int rc;
    if ((rc = launch_pack_conv_weight16(s, g_w, theta_w, w.convw))) return rc;
    PrologueLaunch pl;
    pl.B = B; pl.g = g; pl.x = x;
    pl.g_w = g_w; pl.g_b = g_b; pl.th_w = theta_w; pl.th_b = theta_b;
    pl.thr_w = thr_w; pl.thr_b = thr_b; pl.bias_w = bias_w; pl.bias_b = bias_b;
    pl.conv = ConvPath::Split16; pl.conv_w16 = w.convw;
    pl.tiers.amax = w.amax; pl.tiers.slots = w.slots;   // (slots only: the fp32 map has no tiers; they switch the per-block input scale on)
    pl.b1p = b1_nhwc; pl.b2p = b2_nhwc; pl.thr = thr; pl.bias = bias; pl.thr_part = w.thr_part;
    return launch_prologue(s, pl);
}

// (detected by symbol) the launch plan of conv_pair16_kernel, by the function its launcher and the carves of its slots plan with
int dagl_ce_prologue16_plan(int heads, int imgs, int H, int W, int32_t out[4]) {
    DAGL_REQUIRE(heads >= 1 && heads <= 4 && imgs >= 1 && H >= 1 && W >= 1 && out, "dagl_ce_prologue16_plan: bad argument");
    const Conv16Plan p = conv16_plan(make_grid(H, W), heads, imgs);
    out[0] = p.strips; out[1] = p.chunks; out[2] = p.rows_per_block; out[3] = p.slots;
    return DAGL_OK;
}

// (detected by symbol) read-out of the inference flavour of conv_pair16_kernel for tests: the launcher of the fused forward on heads x imgs
// images, every output in the caller's buffers -- the planes, the |b1| slots, the range word and the words the first block clears
size_t dagl_ce_prologue16_debug_scratch_bytes(int heads) {
    return heads >= 1 && heads <= 4 ? (size_t)heads * CONV_W16_BYTES : 0;
}

int dagl_ce_prologue16_debug(void* stream, int heads, int imgs, int H, int W, const float* const* x, const float* const* g_w,
                             const float* const* g_b, const float* const* theta_w, const float* const* theta_b, int32_t tag,
                             void* scratch, size_t scratch_bytes, float* b1_nhwc, float* b2_nhwc, uint16_t* b1_hi, uint16_t* b1_lo,
                             uint16_t* b1_hi2, uint16_t* b1_lo2, float* amax, int32_t* range_word, uint32_t* clear_a, int n) {
    DAGL_REQUIRE(heads >= 1 && heads <= 4 && imgs >= 1 && H >= 1 && W >= 1, "dagl_ce_prologue16_debug: bad shape (1..4 heads)");
    DAGL_REQUIRE(x && g_w && g_b && theta_w && theta_b, "dagl_ce_prologue16_debug: null pointer table");
    for (int h = 0; h < heads; ++h)
        DAGL_REQUIRE(x[h] && g_w[h] && g_b[h] && theta_w[h] && theta_b[h], "dagl_ce_prologue16_debug: null input of head %d", h);
    DAGL_REQUIRE(b2_nhwc && b1_hi && b1_lo && amax && range_word, "dagl_ce_prologue16_debug: null output");
    DAGL_REQUIRE((b1_hi2 == nullptr) == (b1_lo2 == nullptr), "dagl_ce_prologue16_debug: the coarse tier is both planes or neither");
    DAGL_REQUIRE(tag != 0, "dagl_ce_prologue16_debug: the tag must not be 0");
    DAGL_REQUIRE(n >= 0 && (n == 0 || clear_a), "dagl_ce_prologue16_debug: %d words to clear, null clear_a", n);
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
    DAGL_REQUIRE(al16(b1_nhwc) && al16(b2_nhwc) && al16(b1_hi) && al16(b1_lo) && al16(b1_hi2) && al16(b1_lo2),
                 "dagl_ce_prologue16_debug: maps and planes must be 16-byte aligned");
    int rc;
    if ((rc = check_workspace("dagl_ce_prologue16_debug", scratch, scratch_bytes, dagl_ce_prologue16_debug_scratch_bytes(heads)))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Grid g = make_grid(H, W);
    const int B = heads * imgs;
    ConvHeadSet hs = {};
    for (int h = 0; h < heads; ++h) {
        unsigned char* convw = static_cast<unsigned char*>(scratch) + (size_t)h * CONV_W16_BYTES;
        if ((rc = launch_pack_conv_weight16(s, g_w[h], theta_w[h], convw))) return rc;
        hs.x[h] = x[h]; hs.w[h] = convw; hs.gb[h] = g_b[h]; hs.tb[h] = theta_b[h];
    }
    hs.imgs = imgs;
    hs.tiers.hi2 = b1_hi2; hs.tiers.lo2 = b1_lo2; hs.tiers.amax = amax; hs.tiers.slots = conv16_plan(g, heads, imgs).slots;
    if ((rc = launch_zero_borders(s, B, H, W, b1_nhwc ? b1_nhwc : b2_nhwc, b2_nhwc))) return rc;
    if ((rc = launch_zero_borders16(s, B, H, W, b1_hi, b1_lo))) return rc;
    if (b1_hi2 && (rc = launch_zero_borders16(s, B, H, W, b1_hi2, b1_lo2))) return rc;
    RangeTag range;
    range.word = range_word; range.tag = tag;
    return launch_conv_pair16_heads(s, heads, imgs, g, hs, b2_nhwc, b1_nhwc, b1_hi, b1_lo, clear_a, n, nullptr, 0, range);
}

// (detected by symbol) the launch plan of project16_kernel on B images of [H, W], by the function its launcher plans with
int dagl_project16_plan(int B, int H, int W, int which, int cus, int32_t out[12]) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && which >= 1 && which <= 3 && out, "dagl_project16_plan: bad argument");
    const Project16Plan p = project16_plan(make_grid(H, W), B, which, cus);
    out[0] = p.n_items[0]; out[1] = p.n_items[1]; out[2] = p.lin[0]; out[3] = p.units_q; out[4] = p.units_k;
    out[5] = p.n_full; out[6] = p.n_full & ~15; out[7] = p.n_split_groups; out[8] = p.n_proj; out[9] = p.cap;
    out[10] = p.segs[0]; out[11] = p.segs[1];
    return DAGL_OK;
}

// (detected by symbol) read-out of the inference launch of project16_kernel for tests: the launcher of the fused forward on heads x imgs
// images of fp16 planes, every output -- feature rows, bf16 and split copies, column and row sums, the thr / bias partials -- in the
// caller's buffers, none of them touched outside the kernel's own stores
size_t dagl_ce_project16_debug_scratch_bytes(int heads) {
    return heads >= 1 && heads <= 4 ? (size_t)heads * 2 * P16_PACKED_HALFS * sizeof(uint16_t) : 0;
}

int dagl_ce_project16_debug(void* stream, int heads, int imgs, int H, int W, int which, const uint16_t* map_hi, const uint16_t* map_lo,
                            const uint16_t* map_hi2, const uint16_t* map_lo2, const float* amax, int slots, const float* const* fc1_w,
                            const float* const* fc1_b, const float* const* fc2_w, const float* const* fc2_b, int32_t tag,
                            int32_t* range_word, void* scratch, size_t scratch_bytes, float* x_feat, float* wq_feat, uint16_t* x_bf16,
                            uint16_t* wq_bf16, int q_tiled, uint16_t* x_hi, uint16_t* x_lo, uint16_t* wq_hi, uint16_t* wq_lo,
                            double* colsum, float* colpart, float* rowsum, const int32_t* rowsum_policy, const float* const* thr_x,
                            const float* const* thr_w, const float* const* bias_w, float* thr_part) {
    DAGL_REQUIRE(heads >= 1 && heads <= 4 && imgs >= 1 && H >= 1 && W >= 1 && which >= 1 && which <= 3,
                 "dagl_ce_project16_debug: bad shape (1..4 heads, which 1..3)");
    const bool keys = (which & 1) != 0, queries = (which & 2) != 0;
    if (keys) DAGL_REQUIRE(fc2_w && fc2_b, "dagl_ce_project16_debug: null pointer table");
    if (queries) DAGL_REQUIRE(fc1_w && fc1_b, "dagl_ce_project16_debug: null pointer table");
    const bool thr = thr_x || thr_w || bias_w || thr_part;
    if (thr) DAGL_REQUIRE(thr_x && thr_w && bias_w && thr_part, "dagl_ce_project16_debug: the thr / bias ride-along is x, both weights and the partials, or none");
    for (int h = 0; h < heads; ++h) {
        DAGL_REQUIRE((!keys || (fc2_w[h] && fc2_b[h])) && (!queries || (fc1_w[h] && fc1_b[h])) && (!thr || (thr_x[h] && thr_w[h] && bias_w[h])),
                     "dagl_ce_project16_debug: null input of head %d", h);
    }
    DAGL_REQUIRE(map_hi && map_lo, "dagl_ce_project16_debug: null plane");
    DAGL_REQUIRE(range_word && (!keys || x_feat) && (!queries || wq_feat), "dagl_ce_project16_debug: null output");
    DAGL_REQUIRE((keys || !(x_feat || x_bf16 || x_hi || x_lo || colsum || colpart || rowsum)) && (queries || !(wq_feat || wq_bf16 || wq_hi || wq_lo)),
                 "dagl_ce_project16_debug: an output of a side `which` leaves out");
    DAGL_REQUIRE((map_hi2 == nullptr) == (map_lo2 == nullptr), "dagl_ce_project16_debug: the coarse tier is both planes or neither");
    DAGL_REQUIRE((amax != nullptr) == (map_hi2 != nullptr), "dagl_ce_project16_debug: the slots come with the coarse tier and only with it");
    if (amax) DAGL_REQUIRE(slots >= 4 && slots % 4 == 0, "dagl_ce_project16_debug: %d slots per head (a multiple of 4, at least 4)", slots);
    DAGL_REQUIRE((x_hi == nullptr) == (x_lo == nullptr) && (wq_hi == nullptr) == (wq_lo == nullptr),
                 "dagl_ce_project16_debug: a split copy is both halves or neither");
    DAGL_REQUIRE((colsum == nullptr) == (colpart == nullptr), "dagl_ce_project16_debug: colsum and colpart come together");
    DAGL_REQUIRE(rowsum || !rowsum_policy, "dagl_ce_project16_debug: a policy word without rowsum");
    DAGL_REQUIRE(tag != 0, "dagl_ce_project16_debug: the tag must not be 0");
    auto al16 = [](const void* p) { return ((uintptr_t)p & 15u) == 0; };
    DAGL_REQUIRE(al16(map_hi) && al16(map_lo) && al16(map_hi2) && al16(map_lo2) && al16(amax) && al16(x_feat) && al16(wq_feat) && al16(x_bf16) &&
                 al16(wq_bf16) && al16(x_hi) && al16(x_lo) && al16(wq_hi) && al16(wq_lo) && al16(colsum) && al16(colpart) && al16(rowsum),
                 "dagl_ce_project16_debug: planes, slots, feature rows, copies and sums must be 16-byte aligned");
    const Grid g = make_grid(H, W);
    ThrHeadSet ths = {};
    if (thr) {
        for (int h = 0; h < heads; ++h) { ths.x[h] = thr_x[h]; ths.thr_w[h] = thr_w[h]; ths.bias_w[h] = bias_w[h]; }
        ths.imgs = imgs;
        DAGL_REQUIRE(thr_bias4_ok(g, ths, heads), "dagl_ce_project16_debug: the thr / bias ride-along needs W %% 4 == 0 and 16-byte aligned x");
    }
    int rc;
    if ((rc = check_workspace("dagl_ce_project16_debug", scratch, scratch_bytes, dagl_ce_project16_debug_scratch_bytes(heads)))) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint16_t* wp2 = static_cast<uint16_t*>(scratch);                       // [heads] fc2 (keys), then [heads] fc1 (queries)
    uint16_t* wp1 = wp2 + (size_t)heads * P16_PACKED_HALFS;
    for (int h = 0; h < heads; ++h) {
        if (keys && (rc = launch_pack_fc_weight16(s, fc2_w[h], wp2 + (size_t)h * P16_PACKED_HALFS))) return rc;
        if (queries && (rc = launch_pack_fc_weight16(s, fc1_w[h], wp1 + (size_t)h * P16_PACKED_HALFS))) return rc;
    }
    const float* b1s[4]; const float* b2s[4];
    for (int h = 0; h < 4; ++h) { b1s[h] = queries ? fc1_b[h < heads ? h : 0] : nullptr; b2s[h] = keys ? fc2_b[h < heads ? h : 0] : nullptr; }
    Project16Launch pj;
    pj.B = heads * imgs; pj.g = g; pj.which = which; pj.heads = heads;
    pj.range.word = range_word; pj.range.tag = tag;
    pj.map_hi = map_hi; pj.map_lo = map_lo;
    pj.tiers.hi2 = const_cast<uint16_t*>(map_hi2); pj.tiers.lo2 = const_cast<uint16_t*>(map_lo2);
    pj.tiers.amax = const_cast<float*>(amax); pj.tiers.slots = slots;
    if (keys) { pj.keys.wp = wp2; pj.keys.bias = b2s; pj.keys.feat = x_feat; pj.keys.feat_bf16 = x_bf16; }
    if (queries) { pj.queries.wp = wp1; pj.queries.bias = b1s; pj.queries.feat = wq_feat; pj.queries.feat_bf16 = wq_bf16; }
    pj.colsum = colsum; pj.colpart = colpart; pj.q_tiled = q_tiled ? 1 : 0;
    Split16Out so;
    so.hi[0] = x_hi; so.lo[0] = x_lo; so.hi[1] = wq_hi; so.lo[1] = wq_lo;
    so.rows_alloc[0] = feat_rows_h(g.N); so.rows_alloc[1] = feat_rows_h(g.L);
    if (x_hi || wq_hi) pj.split = &so;
    pj.rowsum = rowsum; pj.rowsum_policy = rowsum_policy;
    if (thr) { pj.thr_hs = &ths; pj.thr_head_imgs = heads * imgs; pj.thr_part = thr_part; }
    return launch_project16(s, pj);
}

// ---- the 7x7x16 -> 196 patch Linear (+ReLU) of the differentiable path's FORWARD on the inference kernels: split the map,
// pack the weight, project (split-fp16 matrix cores, no unfolded rows), copy the feature rows out densely ---------------
struct Pp16Ws { uint16_t *hi, *lo, *wp; float* feat; int64_t* words; size_t bytes; };
static Pp16Ws pp16_carve(void* scratch, int B, const Grid& g, int n) {
    Carver cv(scratch);
    const size_t map_h = (size_t)B * g.Hp * g.Wp * CH;
    Pp16Ws w;
    w.hi = cv.take<uint16_t>(map_h); w.lo = cv.take<uint16_t>(map_h);
    w.wp = cv.take<uint16_t>(P16_PACKED_HALFS);
    w.feat = cv.take<float>((size_t)B * feat_rows(n) * DS);
    w.words = cv.take<int64_t>(2);                                    // range word, completion word (RangeTag)
    w.bytes = cv.bytes();
    return w;
}

size_t dagl_project_patches16_scratch_bytes(int B, int H, int W, int queries) {
    if (B < 1 || H < 1 || W < 1) return 0;
    const Grid g = make_grid(H, W);
    return pp16_carve(nullptr, B, g, queries ? g.L : g.N).bytes;
}

int dagl_project_patches16(void* stream, int B, int H, int W, int queries, const float* map_nhwc, const float* w_rows,
                           const float* fc_bias, float* rows_out, void* scratch, size_t scratch_bytes) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && map_nhwc && w_rows && fc_bias && rows_out && scratch,
                 "dagl_project_patches16: bad argument");
    DAGL_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "dagl_project_patches16: scratch must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const Grid g = make_grid(H, W);
    const int n = queries ? g.L : g.N;
    const Pp16Ws w = pp16_carve(scratch, B, g, n);
    DAGL_REQUIRE(scratch_bytes >= w.bytes, "dagl_project_patches16: scratch %zu B, need %zu B", scratch_bytes, w.bytes);
    int rc;
    // range guard (|16 map| , |1024 w| < 65504): the split / pack / projection kernels store this call's tag into the range
    // word when they meet a larger value, and the copy-out below then writes NaN instead of numbers formed from inf halves
    RangeTag rt;
    DAGL_HIP_TRY(hipMemsetAsync(w.words, 0, 2 * sizeof(int64_t), s));
    rt.word = reinterpret_cast<int32_t*>(w.words); rt.done = reinterpret_cast<int32_t*>(w.words + 1); rt.tag = next_call_tag();
    if ((rc = launch_split_map(s, (size_t)B * g.Hp * g.Wp * CH, map_nhwc, w.hi, w.lo, rt))) return rc;
    if ((rc = launch_pack_fc_weight16(s, w_rows, w.wp, /*rows_order=*/true))) return rc;
    const float* bias1[1] = {fc_bias};
    Project16Launch pj;
    pj.B = B; pj.g = g; pj.which = queries ? 2 : 1; pj.map_hi = w.hi; pj.map_lo = w.lo; pj.range = rt;
    auto& side = queries ? pj.queries : pj.keys;
    side.wp = w.wp; side.bias = bias1; side.feat = w.feat;
    if ((rc = launch_project16(s, pj))) return rc;
    // [B, feat_rows(n), DS] -> [B, n, 196]
    return launch_feat_rows_out(s, B, n, w.feat, rows_out, rt);
}

int dagl_pad_nhwc(void* stream, int B, int H, int W, const float* src_nchw, float* dst_nhwc) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && src_nchw && dst_nhwc, "dagl_pad_nhwc: bad argument");
    return launch_pad_nhwc((hipStream_t)stream, B, H, W, src_nchw, dst_nhwc);
}

int dagl_pack_fc_weight(void* stream, const float* w, float* w_packed) {
    DAGL_REQUIRE(w && w_packed, "dagl_pack_fc_weight: null pointer");
    return launch_pack_fc_weight((hipStream_t)stream, w, w_packed);
}

int dagl_feat_rows(int rows) { return feat_rows(rows); }

int dagl_project_patches(void* stream, int B, int H, int W, int queries, const float* map_nhwc,
                         const float* w_packed, const float* fc_bias, float* feat, double* colsum) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && map_nhwc && w_packed && fc_bias && feat,
                 "dagl_project_patches: bad argument");
    const Grid g = make_grid(H, W);
    hipStream_t s = (hipStream_t)stream;
    const int rows = queries ? g.L : g.N, ra = feat_rows(rows);
    for (int b = 0; b < B; ++b)
        DAGL_HIP_TRY(hipMemsetAsync(feat + ((size_t)b * ra + rows) * DS, 0, (size_t)(ra - rows) * DS * sizeof(float), s));
    if (colsum) DAGL_HIP_TRY(hipMemsetAsync(colsum, 0, (size_t)B * DS * sizeof(double), s));
    ProjectLaunch pj;
    pj.B = B; pj.g = g; pj.which = queries ? 2 : 1; pj.map = map_nhwc;
    auto& side = queries ? pj.queries : pj.keys;
    side.wp = w_packed; side.bias = fc_bias; side.feat = feat;
    if (!queries) pj.colsum = colsum;
    return launch_project(s, pj);
}

int dagl_query_thresholds(void* stream, int B, int L, int N, const float* wq, const double* colsum,
                          const float* thr, float* mt) {
    DAGL_REQUIRE(B >= 1 && L >= 1 && N >= 1 && wq && colsum && thr && mt, "dagl_query_thresholds: bad argument");
    return launch_query_thresholds((hipStream_t)stream, B, L, N, wq, colsum, thr, mt);
}

int dagl_gather_aggregate(void* stream, int L, int k, int P_, const int32_t* idx, const float* wgt,
                          const float* values, float* out) {
    DAGL_REQUIRE(L >= 0 && k >= 1 && P_ >= 4 && (P_ % 4) == 0, "dagl_gather_aggregate: bad shape L=%d k=%d P=%d", L, k, P_);
    if (L == 0) return DAGL_OK;
    DAGL_REQUIRE(idx && wgt && values && out, "dagl_gather_aggregate: null pointer");
    DAGL_REQUIRE(((uintptr_t)values % 16) == 0 && ((uintptr_t)out % 16) == 0, "dagl_gather_aggregate: 16-byte alignment required");
    return launch_gather_fixed((hipStream_t)stream, L, k, P_, idx, wgt, values, out);
}

int dagl_unfold_values(void* stream, int B, int H, int W, const float* b2_nhwc, float* rows) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && b2_nhwc && rows, "dagl_unfold_values: bad argument");
    return launch_unfold_values((hipStream_t)stream, B, make_grid(H, W), b2_nhwc, rows);
}

int dagl_fold_normalize(void* stream, int B, int H, int W, const float* agg, float* out) {
    DAGL_REQUIRE(B >= 1 && H >= 1 && W >= 1 && agg && out, "dagl_fold_normalize: bad argument");
    return launch_fold((hipStream_t)stream, B, make_grid(H, W), agg, out);
}

int dagl_scores_dense(void* stream, int B, int L, int N, const float* wq, const float* x, float* sc) {
    DAGL_REQUIRE(B >= 1 && L >= 1 && N >= 1 && wq && x && sc, "dagl_scores_dense: bad argument");
    return launch_scores_dense((hipStream_t)stream, B, L, N, wq, x, sc);
}

// (ABI 406) any patch geometry: csrc/generic.hip
size_t dagl_ce_generic_workspace_bytes(int B, int Cin, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels) {
    if (B < 1 || Cin < 4 || H < 1 || W < 1 || ksize < 1 || ksize > 31 || stride_1 < 1 || stride_2 < 1 || inter_channels < 4) return 0;
    return dagl::ce_generic_workspace_bytes(B, Cin, H, W, ksize, stride_1, stride_2, inter_channels);
}

int dagl_ce_generic_forward(void* stream, int B, int Cin, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels,
                            float softmax_scale, int mode, int k, const float* x, const float* g_w, const float* g_b,
                            const float* theta_w, const float* theta_b, const float* thr_w, const float* thr_b, const float* bias_w,
                            const float* bias_b, const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                            float* out, int32_t* degree, void* workspace, size_t workspace_bytes) {
    int rc = dagl::ce_generic_check(B, Cin, H, W, ksize, stride_1, stride_2, inter_channels, mode, k);
    if (rc) return rc;
    DAGL_REQUIRE(softmax_scale > 0.f, "dagl_ce_generic_forward: softmax_scale must be positive");
    DAGL_REQUIRE(x && g_w && g_b && theta_w && theta_b && fc1_w && fc1_b && fc2_w && fc2_b && out && workspace,
                 "dagl_ce_generic_forward: null pointer");
    if (mode != DAGL_MODE_TOPK) DAGL_REQUIRE(thr_w && thr_b && bias_w && bias_b, "dagl_ce_generic_forward: thr / bias heads missing");
    const size_t need = dagl::ce_generic_workspace_bytes(B, Cin, H, W, ksize, stride_1, stride_2, inter_channels);
    if (workspace_bytes < need) { dagl::set_error("dagl_ce_generic_forward: workspace %zu bytes, %zu needed", workspace_bytes, need); return DAGL_ERR_WORKSPACE; }
    if ((rc = check_device())) return rc;
    return dagl::launch_ce_generic((hipStream_t)stream, B, Cin, H, W, ksize, stride_1, stride_2, inter_channels, softmax_scale, mode, k, x,
                                   g_w, g_b, theta_w, theta_b, thr_w, thr_b, bias_w, bias_b, fc1_w, fc1_b, fc2_w, fc2_b, out, degree, workspace);
}

int dagl_ce_generic_border(int ksize) { return dagl::ce_generic_border(ksize); }

size_t dagl_ce_generic_core_workspace_bytes(int B, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels, int backward) {
    if (B < 1 || H < 1 || W < 1 || ksize < 1 || ksize > 31 || stride_1 < 1 || stride_2 < 1 || inter_channels < 4) return 0;
    return dagl::ce_generic_core_workspace_bytes(B, H, W, ksize, stride_1, stride_2, inter_channels, backward);
}

int dagl_ce_generic_core_forward(void* stream, int B, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels,
                                 float softmax_scale, int mode, int k, const float* wq_rows, const float* x_rows, const float* b2p,
                                 const float* thr, const float* bias, float* out, int32_t* degree, void* workspace, size_t workspace_bytes) {
    int rc = dagl::ce_generic_check(B, 4, H, W, ksize, stride_1, stride_2, inter_channels, mode, k);
    if (rc) return rc;
    DAGL_REQUIRE(softmax_scale > 0.f && wq_rows && x_rows && b2p && out && workspace, "dagl_ce_generic_core_forward: bad argument");
    if (mode != DAGL_MODE_TOPK) DAGL_REQUIRE(thr && bias, "dagl_ce_generic_core_forward: thr / bias missing");
    const size_t need = dagl::ce_generic_core_workspace_bytes(B, H, W, ksize, stride_1, stride_2, inter_channels, 0);
    if (workspace_bytes < need) { dagl::set_error("dagl_ce_generic_core_forward: workspace %zu bytes, %zu needed", workspace_bytes, need); return DAGL_ERR_WORKSPACE; }
    if ((rc = check_device())) return rc;
    return dagl::launch_ce_generic_core_forward((hipStream_t)stream, B, H, W, ksize, stride_1, stride_2, inter_channels, softmax_scale, mode, k,
                                                wq_rows, x_rows, b2p, thr, bias, out, degree, workspace);
}

int dagl_ce_generic_core_backward(void* stream, int B, int H, int W, int ksize, int stride_1, int stride_2, int inter_channels,
                                  float softmax_scale, int mode, int k, const float* wq_rows, const float* x_rows, const float* b2p,
                                  const float* thr, const float* bias, const float* d_out, float* d_wq, float* d_x, float* d_b2p,
                                  float* d_thr, float* d_bias, void* workspace, size_t workspace_bytes) {
    int rc = dagl::ce_generic_check(B, 4, H, W, ksize, stride_1, stride_2, inter_channels, mode, k);
    if (rc) return rc;
    DAGL_REQUIRE(softmax_scale > 0.f && wq_rows && x_rows && b2p && d_out && d_wq && d_x && d_b2p && workspace,
                 "dagl_ce_generic_core_backward: bad argument");
    if (mode != DAGL_MODE_TOPK) DAGL_REQUIRE(thr && bias && d_thr && d_bias, "dagl_ce_generic_core_backward: thr / bias (and their gradients) missing");
    const size_t need = dagl::ce_generic_core_workspace_bytes(B, H, W, ksize, stride_1, stride_2, inter_channels, 1);
    if (workspace_bytes < need) { dagl::set_error("dagl_ce_generic_core_backward: workspace %zu bytes, %zu needed", workspace_bytes, need); return DAGL_ERR_WORKSPACE; }
    if ((rc = check_device())) return rc;
    return dagl::launch_ce_generic_core_backward((hipStream_t)stream, B, H, W, ksize, stride_1, stride_2, inter_channels, softmax_scale, mode, k,
                                                 wq_rows, x_rows, b2p, thr, bias, d_out, d_wq, d_x, d_b2p, d_thr, d_bias, workspace);
}

// (ABI 408) the learned patch graph as CSR: csrc/graph.hip
size_t dagl_ce_graph_workspace_bytes(int B, int H, int W, int mode, int k, int rows_per_chunk) {
    GraphPlan p;
    if (graph_plan(B, H, W, mode, k, rows_per_chunk, p)) return 0;
    return p.o_end;
}

int dagl_ce_graph_count(void* stream, int B, int H, int W, const float* b1, const float* thr, const float* bias, const float* fc1_w,
                        const float* fc1_b, const float* fc2_w, const float* fc2_b, int mode, int k, int rows_per_chunk,
                        int64_t* row_off_out, void* workspace, size_t ws_bytes, dagl_ce_info* info) {
    GraphPlan p;
    int rc = graph_plan(B, H, W, mode, k, rows_per_chunk, p);
    if (rc) return rc;
    reset_info(info, (int64_t)p.o_end, 8);
    DAGL_REQUIRE(row_off_out && b1 && fc1_w && fc1_b && fc2_w && fc2_b, "dagl_ce_graph_count: null tensor pointer");
    if (mode != DAGL_MODE_TOPK) DAGL_REQUIRE(thr && bias, "dagl_ce_graph_count: thr/bias required in adaptive modes");
    if ((rc = check_workspace("dagl_ce_graph_count", workspace, ws_bytes, p.o_end))) return rc;
    return launch_graph_count((hipStream_t)stream, p, b1, thr, bias, fc1_w, fc1_b, fc2_w, fc2_b, row_off_out, workspace);
}

int dagl_ce_graph_fill(void* stream, int B, int H, int W, int mode, int k, int rows_per_chunk, const int64_t* row_off,
                       int32_t* key_out, float* weight_out, float* score_out, int64_t total_edges, int64_t capacity_edges,
                       void* workspace, size_t ws_bytes) {
    GraphPlan p;
    int rc = graph_plan(B, H, W, mode, k, rows_per_chunk, p);
    if (rc) return rc;
    DAGL_REQUIRE(total_edges >= 0 && total_edges <= (int64_t)B * p.g.L * p.g.N, "dagl_ce_graph_fill: total_edges=%lld is not a count of this graph's edges",
                 (long long)total_edges);
    if (capacity_edges < total_edges) {
        set_error("dagl_ce_graph_fill: capacity %lld edges < the graph's %lld edges", (long long)capacity_edges, (long long)total_edges);
        return DAGL_ERR_WORKSPACE;
    }
    DAGL_REQUIRE(row_off && (total_edges == 0 || (key_out && weight_out)), "dagl_ce_graph_fill: null tensor pointer");
    if ((rc = check_workspace("dagl_ce_graph_fill", workspace, ws_bytes, p.o_end))) return rc;
    if (total_edges == 0) return DAGL_OK;
    return launch_graph_fill((hipStream_t)stream, p, row_off, key_out, weight_out, score_out, (long long)capacity_edges, workspace);
}

// the routes on a GIVEN patch graph (dagl_graph_apply*, _attend*, _forward*, _refresh*, _from_lists*) have their entries beside their
// kernels: csrc/graph_apply.hip, graph_attend.hip, graph_forward.hip, graph_refresh.hip, graph_lists.hip

}  // extern "C"
