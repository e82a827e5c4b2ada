// binning_host.h -- the host side of K3..K7: which kernels of binning.hip, binning_persist.h and binning_rows.h run,
// and where in the two workspaces they work.  Host code only; included by binning.hip behind the device headers.
// In order: switches and BinHooks, BinFrame, the layouts and their views, SortPlan, BinDevice.
#pragma once

namespace {

// ------------------------------------------------------------------------------------ switches and environment hooks
// The three switch accessors read their hook once per process; BinHooks and bin_frame() (GSR_BINNING) read theirs once
// per launching call (tests setenv between calls).  Defaults: DESIGN.md 3.1.
enum { PERSIST_OFF = 0, PERSIST_P = 1, PERSIST_S = 2 };
constexpr long long PERSIST_SORT_MAX_PAIRS = 6ll << 20;  // above: the look-back tile sort
// ... and the row-major pipeline from ~5 million pairs on: below, its four launches (three latency chains of one tile
// each) lose to the persistent sort kernel / the two look-back passes -- measured (tools/binbench.py, K5-K7 alone, exact
// sizes): 1.8 M pairs 71 against 54 us, 5.6 M 107 against 101 us, 13.6 M 157 against 188 us (profiles/r06_rows_pipeline.txt)
constexpr long long ROWS_MIN_PAIRS = 5ll << 20;

std::atomic<int> g_persist_override{-1};  // gsr_set_bin_persistent: -1 = environment
std::atomic<int> g_rows_override{-1};     // gsr_set_bin_rowmajor: -1 = environment
// Exact tile culling (binning_persist.h: gsr_tile_mask).  Its cost is K3's -- per Gaussian and tile row of the rect,
// +27 us per 10^6 Gaussians at 1080p, +37 us at 4K -- its return the D-sized passes' and the composite kernels'.
// Measured (profiles/r05_tile_cull.txt): D -9..19 %; K3-K7 327 -> 330 us at c1, 713 -> 694 us at 4K; the training steps
// 1.206 -> 1.204 ms and 2.811 -> 2.799 ms: the composite kernels skip such pairs with one box test per quadrant anyway.
// Hence OFF by default; "auto" is a static rule for scenes whose splats cover many tiles -- not a function of earlier views.
std::atomic<int> g_tile_cull{-1};  // gsr_set_tile_cull: -1 = environment
std::atomic<int> g_tie_order{0};   // gsr_set_depth_tie_order: 0 arrival index (the reference), 1 screen position

int persist_effective_mode() {  // GSR_BIN_PERSIST = 0 | 1 (default) | p | s
    const int o = g_persist_override.load(std::memory_order_relaxed);
    if (o >= 0) return o;
    static const int env_mode = [] {
        const char *e = getenv("GSR_BIN_PERSIST");
        if (!e || !*e || strcmp(e, "1") == 0) return PERSIST_P | PERSIST_S;
        if (strcmp(e, "p") == 0) return (int)PERSIST_P;
        if (strcmp(e, "s") == 0) return (int)PERSIST_S;
        return (int)PERSIST_OFF;
    }();
    return env_mode;
}
bool rows_switch_on() {  // GSR_BIN_ROWS = 0 | 1 (default)
    const int mode = g_rows_override.load(std::memory_order_relaxed);
    if (mode >= 0) return mode == 1;
    static const bool env_on = [] {
        const char *e = getenv("GSR_BIN_ROWS");
        return !(e && *e == '0');
    }();
    return env_on;
}
int tile_cull_on(int tiles) {  // GSR_TILE_CULL = 0 (default) | 1 | auto: frames above GSR_TILE_CULL_TILES (16384) tiles
    int mode = g_tile_cull.load(std::memory_order_relaxed);
    if (mode < 0) {
        static const int env_mode = [] {
            const char *e = getenv("GSR_TILE_CULL");
            if (!e || !*e || strcmp(e, "0") == 0) return 0;
            return strcmp(e, "auto") == 0 ? 2 : 1;
        }();
        mode = env_mode;
    }
    if (mode != 2) return mode;
    static const int min_tiles = [] {
        const char *e = getenv("GSR_TILE_CULL_TILES");
        const int v = e ? atoi(e) : 0;
        return v > 0 ? v : 16384;
    }();
    return tiles > min_tiles ? 1 : 0;
}

int lowered(int v, int dflt) { return v > 0 && v < dflt ? v : dflt; }  // a hook that may only LOWER a figure
int env_int(const char *name) {
    const char *e = getenv(name);
    return e && *e ? atoi(e) : 0;
}
struct BinHooks {
    long long persist_maxd;   // GSR_BIN_PERSIST_MAXD: most pairs the persistent sort kernel takes (6 << 20)
    long long rows_min;       // GSR_BIN_ROWS_MIN: fewest pairs the row-major pipeline takes (5 << 20; tests set 1)
    int rows_fill_d;          // GSR_ROWS_FILL_D: pair_scatter workgroups per CU (4; lower only; A/B measurements)
    int max_tpw;              // GSR_BIN_MAX_TPW: tiles per workgroup of the prepare kernel, 1..PP_MAX_TPW (1)
    int owners;               // GSR_BIN_OWNERS: caps the chunk-owner table (PS_OWNERS; lower only)
    int sort_timeout_ms;      // GSR_BIN_SORT_TIMEOUT_MS: first-barrier time-out of the sort kernel (250; lower only)
    int grid_p, grid_s;       // GSR_BIN_GRID_P / _S: cap the persistent grids; as given (0: unset), lowered() at their use
    bool depth_buckets;       // GSR_BIN_DEPTH_SORT = lsd clears it: four global LSD depth passes in the prepare kernel
    bool abort_p, abort_s;    // GSR_BIN_FORCE_ABORT = p | s | ps: the named kernels' first barrier aborts (tests)
    bool timeline;            // GSR_BIN_TIMELINE = 1: phase stamps of the persistent kernels (gsr_bin_timeline)
};
BinHooks read_hooks() {
    BinHooks h;
    const int maxd = env_int("GSR_BIN_PERSIST_MAXD");
    h.persist_maxd = maxd > 0 && maxd < 0x7fffffff ? maxd : PERSIST_SORT_MAX_PAIRS;
    const char *e = getenv("GSR_BIN_ROWS_MIN");
    const long long rows_min = e ? atoll(e) : 0;
    h.rows_min = rows_min > 0 ? rows_min : ROWS_MIN_PAIRS;
    h.rows_fill_d = lowered(env_int("GSR_ROWS_FILL_D"), 4);
    h.max_tpw = lowered(env_int("GSR_BIN_MAX_TPW"), PP_MAX_TPW + 1);
    if (h.max_tpw > PP_MAX_TPW) h.max_tpw = 1;
    h.owners = lowered(env_int("GSR_BIN_OWNERS"), PS_OWNERS);
    h.sort_timeout_ms = lowered(env_int("GSR_BIN_SORT_TIMEOUT_MS"), 250);
    h.grid_p = env_int("GSR_BIN_GRID_P");
    h.grid_s = env_int("GSR_BIN_GRID_S");
    e = getenv("GSR_BIN_DEPTH_SORT");
    h.depth_buckets = !(e && strcmp(e, "lsd") == 0);
    e = getenv("GSR_BIN_FORCE_ABORT");
    h.abort_p = e && strchr(e, 'p') != nullptr;
    h.abort_s = e && strchr(e, 's') != nullptr;
    e = getenv("GSR_BIN_TIMELINE");
    h.timeline = e && *e == '1';
    return h;
}

// ------------------------------------------------------------------------------------------------------- the frame
int bits_for(long long n) {  // bits needed for the values 0 .. n-1 (at least 1)
    int b = 1;
    while ((1ll << b) < n) b++;
    return b;
}
int tile_bits(int tiles) { return bits_for((long long)tiles + 1); }  // (the largest key value is the sentinel `tiles`)
struct BinFrame {
    int width, height, gx, gy, tiles;
    int xbits, ybits;  // of the (row << xbits | column) keys
    bool yx;           // (row, column) keys + fused emission: <= 256 x 256 tiles, unless GSR_BINNING=generic (A/B, tests)
    int cull;          // exact tile culling; only on the (row, column) path
};
BinFrame bin_frame(int width, int height) {
    BinFrame f;
    f.width = width; f.height = height;
    f.gx = (width + GSR_BLOCK_X - 1) / GSR_BLOCK_X;
    f.gy = (height + GSR_BLOCK_Y - 1) / GSR_BLOCK_Y;
    f.tiles = f.gx * f.gy;
    f.xbits = bits_for(f.gx); f.ybits = bits_for(f.gy);
    const char *e = getenv("GSR_BINNING");
    f.yx = !(e && strcmp(e, "generic") == 0) && f.gx <= RADIX_DIGITS && f.gy <= RADIX_DIGITS;
    f.cull = f.yx ? tile_cull_on(f.tiles) : 0;
    return f;
}

// ------------------------------------------------------------------------------------------------ workspace layouts
constexpr int PERSIST_MAX_GRID_P = 1024;  // upper bounds used to size workspaces (CUs x workgroups per CU of any part)
constexpr int PERSIST_MAX_GRID_S = 4096;
template <class T>
T *at(void *base, size_t off) { return reinterpret_cast<T *>(reinterpret_cast<char *>(base) + off); }
GridSync sync_view(void *sync, int G) {
    uint32_t *leaf = at<uint32_t>(sync, 0), *root = leaf + (size_t)((G + GB_FAN - 1) / GB_FAN) * GB_LEAF_STRIDE;
    return {leaf, root, root + GB_LEAF_STRIDE};
}
struct PersistLayoutP {  // inside the control block of the prepare workspace
    size_t sync, grp, bins, cnt, wtot, zero_bytes, total;
};
PersistLayoutP persist_layout_p(int G) {
    PersistLayoutP L;
    const int ngroups = (G + GB_FAN - 1) / GB_FAN;
    size_t o = 0;
    L.sync = o; o += align_up(sizeof(uint32_t) * grid_sync_words(G));
    L.grp = o; o += align_up(sizeof(uint32_t) * (BK_PASS + 1) * (size_t)ngroups * RADIX_DIGITS);
    L.bins = o; o += align_up(sizeof(uint32_t) * (BK_BINS + 2));  // bin counts, { ~min, max } key (bucket path)
    L.zero_bytes = o;  // [0, zero_bytes) is cleared before every launch
    L.cnt = o; o += align_up(sizeof(uint32_t) * (BK_PASS + 1) * (size_t)G * RADIX_DIGITS);
    L.wtot = o; o += align_up(sizeof(unsigned long long) * (size_t)G);
    L.total = o;
    return L;
}
struct PersistLayoutS {  // inside the control block of the sort scratch
    size_t sync, grp, grp_solo, cnt, cnt_solo, zero_bytes, total;
};
PersistLayoutS persist_layout_s(int G) {
    PersistLayoutS L;
    const int ngroups = (G + GB_FAN - 1) / GB_FAN;
    size_t o = 0;
    L.sync = o; o += align_up(sizeof(uint32_t) * grid_sync_words(G));
    L.grp = o; o += align_up(sizeof(uint32_t) * 2 * (size_t)ngroups * RADIX_DIGITS);
    L.grp_solo = o; o += align_up(sizeof(uint32_t) * 2 * RADIX_DIGITS);  // (workgroup 0 alone after an aborted first barrier)
    L.zero_bytes = o;
    L.cnt = o; o += align_up(sizeof(uint32_t) * 2 * (size_t)G * RADIX_DIGITS);
    L.cnt_solo = o; o += align_up(sizeof(uint32_t) * 2 * RADIX_DIGITS);
    L.total = o;
    return L;
}
// the persistent kernels' control blocks share the space of the look-back pipeline's (one of the two runs per call):
// workspaces are sized for the largest grid any device may hold
int persist_grid_bound(long long n, int max_grid) {
    const long long nb = radix_blocks(n);
    return (int)(nb < max_grid ? (nb > 0 ? nb : 1) : max_grid);
}

struct PrepLayout {  // the prepare workspace (what K3-K4 leave for K5-K7)
    size_t tt, kA, vA, kB, vB, offsets, segoff, rects, hull, early, thist, ctrl, total;
    CtrlLayout C;
};
PrepLayout prep_layout(int P) {
    PrepLayout L;
    size_t o = 0;
    const size_t np = align_up((size_t)(P + 1) * 4);
    L.tt = o; o += np;      // pairs of each Gaussian (| the rows of its rect << 20 on the (row, column) path)
    L.segoff = o; o += np;  // exclusive scan of hh[sorted id]: the row segments (round 6, binning_rows.h)
    L.kA = o; o += np;
    L.vA = o; o += np;
    L.kB = o; o += np;
    L.vB = o; o += np;
    L.offsets = o; o += np;
    L.rects = o; o += align_up((size_t)(P + 1) * sizeof(TileRect));
    L.hull = o; o += 256;  // int32 [2]: the row hull of the mask (written by K3, copied into the range table by the sort)
    L.early = o; o += 256;  // { u64 sum of tiles_touched (K3's atomics), u32 workgroups that added theirs }: zeroed with ctrl
    L.thist = o; o += align_up(sizeof(uint32_t) * RADIX_REPLICAS * RADIX_MAX_PASSES * RADIX_DIGITS);  // zeroed with ctrl
    L.ctrl = o;
    L.C = ctrl_layout(P, 4, true);
    o += L.C.total;
    L.total = o;
    return L;
}
size_t prep_bytes_needed(int P) {  // ... with room for either pipeline's control block
    const PrepLayout L = prep_layout(P);
    const size_t need = persist_layout_p(persist_grid_bound(P, PERSIST_MAX_GRID_P)).total;
    return need > L.C.total ? L.total + (need - L.C.total) : L.total;
}
struct PrepViews {
    uint32_t *tt, *segoff, *kA, *vA, *kB, *vB, *offsets, *thist;
    TileRect *rects; int32_t *hull; unsigned long long *early; char *ctrl;
};
PrepViews views(const PrepLayout &L, void *b) {
    return {at<uint32_t>(b, L.tt), at<uint32_t>(b, L.segoff), at<uint32_t>(b, L.kA), at<uint32_t>(b, L.vA),
            at<uint32_t>(b, L.kB), at<uint32_t>(b, L.vB), at<uint32_t>(b, L.offsets), at<uint32_t>(b, L.thist),
            at<TileRect>(b, L.rects), at<int32_t>(b, L.hull), at<unsigned long long>(b, L.early), at<char>(b, L.ctrl)};
}

struct RowsLayout {  // the sort scratch as the row-major pipeline lays it out (binning_rows.h)
    size_t seg_key, seg_gid, pairoff, tdiff, tilebase, chunk_owner, ctrl, tickets, scan_state, seg_state, pair_state,
        ctrl_bytes, total;
};
RowsLayout rows_layout(int64_t D, int gx, int gy) {
    RowsLayout L;
    size_t o = 0;
    const size_t nr = align_up((size_t)(D + 1) * 4);  // R <= D segments
    L.seg_key = o; o += nr;
    L.seg_gid = o; o += nr;
    L.pairoff = o; o += nr;
    // (one replica per XCD, cleared by seg_scatter_kernel)
    L.tdiff = o; o += align_up(sizeof(int32_t) * RADIX_REPLICAS * (size_t)gy * (size_t)(gx + 1));
    L.tilebase = o; o += align_up(sizeof(uint32_t) * (size_t)gx * gy);
    L.chunk_owner = o; o += align_up(sizeof(int32_t) * (size_t)(radix_blocks(D) + gy + 1) * (RADIX_TILE / PS_CHUNK));
    L.ctrl = o;  // [ctrl, ctrl + ctrl_bytes) is zero before the first kernel
    L.tickets = o; o += 256;
    L.scan_state = o; o += align_up(sizeof(unsigned long long) * (size_t)((D + SEGSCAN_TILE - 1) / SEGSCAN_TILE + 2));
    L.seg_state = o; o += align_up(sizeof(uint32_t) * (size_t)(radix_blocks(D) + 1) * RADIX_DIGITS);
    L.pair_state = o; o += align_up(sizeof(uint32_t) * (size_t)(radix_blocks(D) + gy + 1) * RADIX_DIGITS);
    L.ctrl_bytes = o - L.ctrl;
    L.total = o;
    return L;
}
// the sort scratch of the two-pass forms: ping-pong pairs, then a control block that holds the look-back passes' words or
// the persistent sort kernel's; sized so that the row-major layout fits the same buffer where that pipeline can run
struct SortLayout {
    size_t kA, vA, kB, vB, ctrl, total;
    CtrlLayout C;
};
SortLayout sort_layout(const BinFrame &f, int64_t D) {
    SortLayout L;
    size_t o = 0;
    const size_t nd = align_up((size_t)(D + 1) * 4);
    L.kA = o; o += nd;
    L.vA = o; o += nd;
    L.kB = o; o += nd;
    L.vB = o; o += nd;
    L.ctrl = o;
    const int passes = radix_plan(0, tile_bits(f.tiles)).passes;
    L.C = ctrl_layout(D, passes < 2 ? 2 : passes, false);  // (the (row, column) path always runs 2)
    const size_t need = persist_layout_s(persist_grid_bound(D, PERSIST_MAX_GRID_S)).total;  // (either pipeline's control block)
    o += L.C.total > need ? L.C.total : need;
    if (f.yx) {
        const size_t rows = rows_layout(D, f.gx, f.gy).total;
        if (rows > o) o = rows;
    }
    L.total = o;
    return L;
}
struct SortViews {
    uint32_t *kA, *vA, *kB, *vB, *ghist, *tickets, *state;  // (the last three: the look-back passes' words, CtrlLayout)
    char *ctrl;
};
SortViews views(const SortLayout &L, void *b) {
    return {at<uint32_t>(b, L.kA), at<uint32_t>(b, L.vA), at<uint32_t>(b, L.kB), at<uint32_t>(b, L.vB),
            at<uint32_t>(b, L.ctrl + L.C.ghist), at<uint32_t>(b, L.ctrl + L.C.tickets),
            at<uint32_t>(b, L.ctrl + L.C.radix_state), at<char>(b, L.ctrl)};
}

// ------------------------------------------------------------------------------------------------------ the sort plan
// The form of K5-K7 for one frame and pair count (or, `bounded`, capacity), decided HERE and nowhere else: ROWS (the
// row-major pipeline: (row, column) path, uncut rects, from rows_min pairs on), else YX ((row, column) keys in two passes:
// the persistent sort kernel when the device admits it at launch time -- admission hands out a sequence number, so it
// cannot be asked earlier -- else the two look-back passes; the zero region covers the larger of their control blocks),
// else GENERIC (tile-id keys; no bounded launch).  [zero_off, +zero_bytes) of the scratch must be zero before the first
// kernel: the caller clears it, or hands it to the prepare step, whose first kernel clears it (16-byte aligned and a
// whole number of uint4: every layout total is a multiple of 256).
enum SortForm { SORT_ROWS, SORT_YX, SORT_GENERIC };
struct SortPlan {
    int err;  // what the call returns instead of sorting (0: go ahead, the fields below are set)
    SortForm form;
    size_t zero_off, zero_bytes;
};
SortPlan plan_sort(const BinFrame &f, int64_t D, size_t scratch_bytes, bool bounded, long long rows_min) {
    if (D > RADIX_MAX_N) return {GSR_EINVAL};
    const SortLayout S = sort_layout(f, D);
    if (scratch_bytes < S.total) return {GSR_ENOSPACE};
    if (bounded && !f.yx) return {GSR_EINVAL};
    if (f.yx && !f.cull && D >= rows_min && rows_switch_on()) {
        const RowsLayout R = rows_layout(D, f.gx, f.gy);
        return {0, SORT_ROWS, R.ctrl, R.ctrl_bytes};
    }
    if (!f.yx) return {0, SORT_GENERIC, S.ctrl, S.C.total};
    const size_t zp = persist_layout_s(persist_grid_bound(D, PERSIST_MAX_GRID_S)).zero_bytes;
    return {0, SORT_YX, S.ctrl, S.C.total > zp ? S.C.total : zp};
}

// ------------------------------------------------------------------------------------------------- per-device state
// Count slots: pinned, device-mapped, 64 per device, two words each.  K4's last workgroup stores the pair count and then
// the call's sequence tag; the host POLLS the tag (a few microseconds after the store lands) instead of paying a stream
// synchronise (interrupt + wake-up, ~30-40 us measured) -- everything the host launches after this point is on the
// critical path of the iteration.  If the tag does not show up within ~2 ms the host falls back to hipStreamSynchronize
// (which also surfaces a faulted kernel).  A call's ticket is its sequence number (process-wide, never 0); slot =
// ticket % 64, so up to 64 counts can be outstanding per device (gsr_bin_prepare_async / gsr_bin_count_wait).
constexpr int TOTAL_SLOTS = 64, MAX_DEVICES = 64;

// what a gsr_bin_prepare_async call was given: kept per count slot so that gsr_bin_count_wait can repeat the call on
// the look-back pipeline when the persistent kernel gave up at its first barrier (binning_persist.h)
struct PrepCall {
    int P, width, height;
    const float *means2D, *depths;
    const int32_t *radii;
    const float *conic_opacity;
    const uint8_t *compute_locally;
    void *prep;
    hipStream_t stream;
    bool persistent;
    void *zero_ptr;     // the zero region of the tile sort launched behind this prepare step (SortPlan), or null
    size_t zero_bytes;  // a multiple of 16
};

struct BinDevice {
    uint32_t *total_word;  // pinned: the count slots (set up by the first ticket)
    bool caps_init;
    int grid_p, grid_s;    // what the device holds at once, per persistent kernel (persist_caps); 0: unavailable
    uint32_t *done;        // pinned: { sequence number of the last launch past its last barrier, fault code, faults
                           // (barrier_fault), solo recoveries of the sort kernel }; null: no persistent launch tried yet
    uint32_t faults_seen;  // faults already reported to a caller
    uint32_t solo_seen;    // recoveries already answered with a back-off
    int backoff;           // sort calls that still take the look-back tile sort after a recovery
    bool faulted;          // a barrier after the first timed out once: look-back pipeline from then on
    uint32_t seq;          // last sequence number handed out
    hipStream_t stream;    // stream of that launch
    bool any;
    PrepCall calls[TOTAL_SLOTS];  // written by the thread that took the slot's ticket, read by whoever waits for it
};
// ONE mutex: lazy set-up, ticket counter, bookkeeping fields.  Admission waits (<= 250 us) holding it, as it always has;
// every launching call reads the fault count under it first, so a second mutex for tickets would spare nobody that wait.
std::mutex g_bin_mutex;
BinDevice g_bin_devices[MAX_DEVICES];
uint32_t g_ticket_seq = 0;

// the current device's record (a barrier fault of an earlier call is reported by persist_fault_check, once)
int bin_device(BinDevice **out) {
    int dev = 0;
    GSR_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= MAX_DEVICES) return GSR_EINVAL;
    *out = &g_bin_devices[dev];
    return 0;
}

// the grids the persistent kernels may use and the pinned done word, queried when a persistent launch is first tried
void persist_caps(BinDevice &d) {
    std::lock_guard<std::mutex> guard(g_bin_mutex);
    if (d.caps_init) return;
    d.caps_init = true;
    const int dev = (int)(&d - g_bin_devices);
    int cus = 0, per_p = 0, per_p8 = 0, per_s = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0 &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_p, bin_prepare_persist_kernel<4>, PP_THREADS, 0) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_p8, bin_prepare_persist_kernel<8>, PP_THREADS, 0) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_s, bin_sort_persist_kernel, PS_THREADS, 0) == hipSuccess) {
        // one prepare workgroup per CU (16 waves: the latency chain of a tile wants the CU to itself); the sort
        // fills the device (four per CU when the registers allow)
        d.grid_p = (per_p >= 1 && per_p8 >= 1) ? (cus < PERSIST_MAX_GRID_P ? cus : PERSIST_MAX_GRID_P) : 0;
        const long long gs = (long long)cus * (per_s < 4 ? per_s : 4);
        d.grid_s = per_s >= 1 ? (int)(gs < PERSIST_MAX_GRID_S ? gs : PERSIST_MAX_GRID_S) : 0;
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocDefault) == hipSuccess) {
        memset(p, 0, 64);
        d.done = reinterpret_cast<uint32_t *>(p);
    } else {
        d.grid_p = d.grid_s = 0;
    }
    (void)hipGetLastError();
}

int take_ticket(BinDevice &d, uint32_t **host, uint32_t *seq_out) {
    std::lock_guard<std::mutex> guard(g_bin_mutex);
    if (!d.total_word) {
        void *p = nullptr;
        GSR_HIP(hipHostMalloc(&p, sizeof(uint32_t) * 2 * TOTAL_SLOTS, hipHostMallocDefault));
        memset(p, 0, sizeof(uint32_t) * 2 * TOTAL_SLOTS);
        d.total_word = reinterpret_cast<uint32_t *>(p);
    }
    const uint32_t seq = ++g_ticket_seq ? g_ticket_seq : ++g_ticket_seq;  // never 0
    *seq_out = seq;
    *host = d.total_word + 2 * (seq % TOTAL_SLOTS);
    return 0;
}
uint32_t *slot_of_ticket(const BinDevice &d, uint32_t seq) { return d.total_word + 2 * (seq % TOTAL_SLOTS); }
int wait_total(hipStream_t stream, uint32_t *host_total, uint32_t seq, uint32_t *total) {
    volatile uint32_t *w = host_total;
    const auto t0 = std::chrono::steady_clock::now();
    for (long spins = 0;; spins++) {
        if (w[1] == seq) {
            std::atomic_thread_fence(std::memory_order_acquire);
            *total = w[0];
            return 0;
        }
        if ((spins & 1023) == 1023 &&
            std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2))
            break;
    }
    GSR_HIP(hipStreamSynchronize(stream));
    *total = w[0];
    return w[1] == seq ? 0 : GSR_EINVAL;
}

// May a barrier kernel be launched on `stream` now?  Yes when the previous one ran on the same stream (stream order
// serialises them) or has passed its last barrier.  -> sequence number to publish (0 inside a stream capture: a replay
// cannot be tracked -- graphs replay on the stream that owns the device's binning), or -1: use the look-back pipeline.
long long persist_admit(BinDevice &d, hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return 0;
    (void)hipGetLastError();
    std::lock_guard<std::mutex> guard(g_bin_mutex);
    if (d.faulted) return -1;
    if (d.any && d.stream != stream) {
        // (round 6: the host now has a view's pair count ~20 us into its prepare kernel, so a caller that alternates
        // views between two streams arrives here while the other stream's ~100 us kernel is still running; giving up at
        // once sent every second view down the nine launches of the look-back pipeline -- measured 2140 -> 1410 views/s.
        // A bounded wait for that kernel's last barrier costs the host what the count poll used to cost it.)
        const volatile uint32_t *done = reinterpret_cast<volatile uint32_t *>(d.done);
        if (*done != d.seq) {
            const auto t0 = std::chrono::steady_clock::now();
            while (*done != d.seq) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(250)) return -1;
            }
        }
    }
    uint32_t s = ++d.seq;
    if (s == 0) s = ++d.seq;
    d.stream = stream;
    d.any = true;
    return (long long)s;
}

// Has a persistent kernel of this device reported a barrier fault (barrier_fault) that no caller has been told about?
// -> GSR_EFAULT once per fault; the device keeps to the look-back pipeline afterwards.
int persist_fault_check(BinDevice &d) {
    if (!d.done) return 0;
    std::lock_guard<std::mutex> guard(g_bin_mutex);
    const uint32_t faults = reinterpret_cast<volatile uint32_t *>(d.done)[2];
    if (faults == d.faults_seen) return 0;
    d.faults_seen = faults;
    d.faulted = true;
    return GSR_EFAULT;
}

// The sort kernel finished a view with workgroup 0 alone (the grid could not become resident within the time-out): the
// next 64 calls take the look-back tile sort instead of waiting out the time-out again.
bool persist_sort_backoff(BinDevice &d, bool forced_abort) {
    std::lock_guard<std::mutex> guard(g_bin_mutex);
    const uint32_t solo = reinterpret_cast<volatile uint32_t *>(d.done)[3];
    if (solo != d.solo_seen) {
        d.solo_seen = solo;
        d.backoff = forced_abort ? 0 : 64;  // (a forced abort is a test: keep the kernel in use)
    }
    if (d.backoff > 0) {
        d.backoff--;
        return true;
    }
    return false;
}

// Diagnostics (GSR_BIN_TIMELINE=1): one device buffer per kernel, [grid][32] stamps of the 100 MHz clock taken by thread 0
// of every workgroup at the phase boundaries of the LAST launch; read with gsr_bin_timeline.
unsigned long long *g_timeline[2] = {nullptr, nullptr};
int g_timeline_grid[2] = {0, 0};
unsigned long long *timeline_buffer(bool on, int which, int G) {
    if (!on) return nullptr;
    if (!g_timeline[which]) {
        void *p = nullptr;
        if (hipMalloc(&p, sizeof(unsigned long long) * 32 * PERSIST_MAX_GRID_S) != hipSuccess) return nullptr;
        g_timeline[which] = reinterpret_cast<unsigned long long *>(p);
    }
    (void)hipMemset(g_timeline[which], 0, sizeof(unsigned long long) * 32 * (size_t)G);
    g_timeline_grid[which] = G;
    return g_timeline[which];
}

}  // namespace
