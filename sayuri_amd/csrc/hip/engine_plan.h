// engine_plan.h -- what the engine decides on the host before anything is launched: the kernel registries, the switches read
// from the environment, the batch geometry, the tile plans and the routing of a convolution to its kernel family, the launch
// parameters and the layers' device images that Engine<T> and the layer-level test taps share, the tower code object's loader.
// (One translation unit: engine.hip includes engine_plan.h, engine_graph.h and engine_taps.h in this order.)
#pragma once
namespace sayuri {

static thread_local std::string g_err;
static std::atomic<unsigned> g_host_free_gen{0};  // sayuri_hip_host_free calls so far (Engine::zc_device_pointer)
static thread_local int g_test_conv_kind = 0;  // kernel family (ConvFamily) the last sayuri_hip_test_conv call ran
static thread_local int g_test_split_ring = 0; // weight stages of the last sayuri_hip_test_conv_split launch (0: none yet)
static int fail(const std::string& m) { g_err = m; return -1; }

#define HIP_OK(expr)                                                                      \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
            return -1;                                                                    \
        }                                                                                 \
    } while (0)

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
constexpr size_t kMaxLds = 160 * 1024;
constexpr int kNumCU = 256;

// ------------------------------------------------------------------ conv kernel registry
template <typename T> struct ConvKernelTable {
    typedef void (*Fn)(const ConvParams);
    struct Entry { int wmt, wnt; Fn fn; size_t (*lds)(int); int npos_cap; };
    static std::vector<Entry>& entries() {
        static std::vector<Entry> e;
        return e;
    }
};

template <typename T, int WMT, int WNT> static void register_conv() {
    typedef ConvCfg<T, WMT, WNT> Cfg;
    auto fn = &conv_mfma_kernel<T, WMT, WNT>;
    ConvKernelTable<T>::entries().push_back({WMT, WNT, fn, &Cfg::lds_bytes, Cfg::NPOS_CAP});
}

template <typename T> static void register_all_convs();
template <> void register_all_convs<f16>() {
    if (!ConvKernelTable<f16>::entries().empty()) return;
    register_conv<f16, 1, 4>(); register_conv<f16, 2, 4>(); register_conv<f16, 3, 4>();
    register_conv<f16, 4, 4>(); register_conv<f16, 6, 4>(); register_conv<f16, 8, 4>();
    register_conv<f16, 1, 2>(); register_conv<f16, 2, 2>(); register_conv<f16, 3, 2>();
    register_conv<f16, 4, 2>(); register_conv<f16, 6, 2>(); register_conv<f16, 8, 2>();
    register_conv<f16, 6, 3>(); register_conv<f16, 8, 3>();
}
template <> void register_all_convs<float>() {
    if (!ConvKernelTable<float>::entries().empty()) return;
    register_conv<float, 1, 4>(); register_conv<float, 2, 4>(); register_conv<float, 3, 4>();
    register_conv<float, 4, 4>();
    register_conv<float, 1, 2>(); register_conv<float, 2, 2>(); register_conv<float, 3, 2>();
    register_conv<float, 4, 2>();
}

// tuned fp16 3x3 kernels for any batch geometry (conv_glds.h): 192 / 128 / 64-pixel tiles across samples
struct GldsEntry {
    int wmt, wnt;
    void (*fn)(const GldsParams);
    void (*setup)(BatchGeom, int*, int2*);
    size_t lds;
    int npos_cap, npos, pt;
};
static std::vector<GldsEntry>& glds_entries() {
    static std::vector<GldsEntry> e;
    return e;
}
template <int WMT, int WNT> static void register_glds() {
    typedef GldsCfg<WMT, WNT> Cfg;
    glds_entries().push_back({WMT, WNT, &conv_glds_kernel<WMT, WNT>, &tile_setup_kernel<Cfg::PT, Cfg::NPOS>, Cfg::lds_bytes(),
                              Cfg::NPOS_CAP, Cfg::NPOS, Cfg::PT});
}
static void register_all_glds() {
    if (!glds_entries().empty()) return;
    register_glds<8, 3>(); register_glds<8, 2>(); register_glds<8, 1>();
    register_glds<4, 3>(); register_glds<4, 2>(); register_glds<4, 1>();
}
// The weight image of the board kernels with an even tile count: the same planes with their rows in board_row_channel order
// (conv_board.h: a lane then holds 8 consecutive channels of a row-tile pair without any exchange).
// `row` = elements per row: 8 for the image, 1 for the bias that goes with it.
template <typename T> static std::vector<T> board_row_order(const std::vector<T>& img, int ko_pad, int row = 8) {
    std::vector<T> out(img.size());
    const size_t planes = img.size() / ((size_t)ko_pad * row);
    for (size_t pl = 0; pl < planes; ++pl)
        for (int r = 0; r < ko_pad; ++r)
            std::copy_n(img.begin() + (pl * ko_pad + board_row_channel(r)) * row, row, out.begin() + (pl * ko_pad + r) * row);
    return out;
}
static bool board_uses_row_order(int kot) { return (kot / 64) % 2 == 0; }  // 256 / 128: yes; 192 (three row tiles per wave): natural order
// one-workgroup-per-board kernels (conv_board.h), by output-channel tile
typedef void (*BoardFn)(const BoardParams);
typedef void (*BoardSeFn)(const BoardSeParams);
struct BoardEntry { int kot; BoardFn fn; BoardSeFn fn_se; size_t (*lds)(int); };
static const BoardEntry kBoardEntries[] = {
    {256, &conv_board_kernel<4>, &conv_board_se_kernel<4>, &BoardCfg<4>::lds_bytes},  // SAYURI_BOARD_DBG=n swaps in <4, true> (timeline)
    {192, &conv_board_kernel<3>, nullptr, &BoardCfg<3>::lds_bytes},
    {128, &conv_board_kernel<2>, &conv_board_se_kernel<2>, &BoardCfg<2>::lds_bytes},
};
// many-small-workgroups kernels of the latency mode (conv_split.h), by column tiles per wave and weight stages: the
// three-stage ring for every width (ascending: split_plan takes the first that is wide enough), the deeper one for the thin ones
typedef void (*SplitFn)(const SplitParams);
struct SplitEntry { int nj, stages; SplitFn fn; };
static const SplitEntry kSplitEntries[] = {
    {1, kSplitStages, &conv_split_kernel<1, kSplitStages>}, {2, kSplitStages, &conv_split_kernel<2, kSplitStages>},
    {3, kSplitStages, &conv_split_kernel<3, kSplitStages>}, {6, kSplitStages, &conv_split_kernel<6, kSplitStages>},
    {12, kSplitStages, &conv_split_kernel<12, kSplitStages>},
    {1, kSplitDeepStages, &conv_split_kernel<1, kSplitDeepStages>}, {2, kSplitDeepStages, &conv_split_kernel<2, kSplitDeepStages>},
    {3, kSplitDeepStages, &conv_split_kernel<3, kSplitDeepStages>},
};
// the tower's 1x1 convolutions of bottleneck-family networks as many small workgroups (conv_pw.h), by column tiles per wave
// (ascending: pw_plan takes the first that is wide enough; a piece has at most kPwMaxCols = 24 column tiles)
typedef void (*PwFn)(const PwParams);
struct PwEntry { int nj; PwFn fn; };
static const PwEntry kPwEntries[] = {
    {1, &conv_pw_kernel<1>}, {2, &conv_pw_kernel<2>}, {3, &conv_pw_kernel<3>}, {6, &conv_pw_kernel<6>}, {12, &conv_pw_kernel<12>},
};
// the depthwise k x k convolution on LDS (conv_dw.h), by k
typedef void (*DwFn)(const DwParams);
struct DwEntry { int k; DwFn fn; };
static const DwEntry kDwEntries[] = {{3, &conv_dw_kernel<3>}, {5, &conv_dw_kernel<5>}, {7, &conv_dw_kernel<7>}};
// head_board_kernel variants: {row tiles, trunk chunks in flight}; the first that fits the LDS is used (head_board_fits)
typedef void (*HeadFn)(const HeadBoardParams);
struct HeadEntry { int rt, depth; HeadFn fn; };
static const HeadEntry kHeadEntries[] = {
    {2, 5, &head_board_kernel<2, 5>}, {4, 5, &head_board_kernel<4, 5>}, {4, 3, &head_board_kernel<4, 3>},
    {6, 3, &head_board_kernel<6, 3>}, {6, 2, &head_board_kernel<6, 2>},
};
static void enable_big_lds_glds() {
    register_all_glds();
    for (const auto& e : glds_entries())
        (void)hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)&conv_board_kernel<4, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    for (const auto& e : kHeadEntries) (void)hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    (void)hipFuncSetAttribute((const void*)&conv_board_sx_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    for (const auto& e : kSplitEntries) (void)hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    for (const auto& e : kPwEntries) (void)hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    for (const auto& e : kBoardEntries) {
        (void)hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
        if (e.fn_se) (void)hipFuncSetAttribute((const void*)e.fn_se, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
    }
}
// Switches of one engine, read from the environment ONCE, in sayuri_hip_create (and per call in the layer-level test
// taps): nothing on the launch path calls getenv.  They select between product paths that give the same results (A/B
// measurements, tests that check one path against the other), or turn on a debugging / measuring aid.  The measuring-only
// switches (in-kernel timelines, forced activation / channel tile) exist only in builds with -DSAYURI_EXPERIMENTS.
//   SAYURI_CONV=v0 | glds[:wnt]   3x3 layers on the generic / the LDS-DMA-tiles-across-samples kernel instead of one workgroup per board
//   SAYURI_TOWER=0                one launch per convolution instead of one persistent launch per run of board convolutions
//   SAYURI_SE_FUSED=0             SE unit as se_pool / se_fc / se_scale instead of inside the convolution
//   SAYURI_HEADS_FUSED=0          conv1x1 x2 + head_tail instead of head_board_kernel
//   SAYURI_NO_ARITH=1             board kernels read their index tables instead of computing the entries
//   SAYURI_CHAINS_SERIAL=1        debugging aid: the chains of a chained forward one after another (forward())
//   SAYURI_TOWER_SYNC=1           debugging aid: nothing overlaps a persistent tower launch (tower_flush())
//   SAYURI_HIP_FWDSTAT=1          measuring aid: device time of every forward sent through submit(), printed when the engine goes
//   SAYURI_LATENCY=1              a plain sayuri_hip_create of the fp16 engine makes a latency context (sayuri_hip_create_ex's
//                                 SAYURI_HIP_LATENCY; read in engine.hip, not here: the taps do not see it)
//   SAYURI_LATENCY_SPLIT=n        latency context: n strips per board in every split convolution instead of the engine's choice
//   SAYURI_LATENCY_RING=n         latency context: n weight stages in every split convolution instead of the engine's choice (split_ring);
//                                 3 is the three-stage ring everywhere; a depth the chosen variant does not have is refused
//   SAYURI_SE_ONE=0 | 1           the SE unit outside a convolution as se_pool / se_fc / se_scale everywhere | as one launch everywhere
//   SAYURI_PW=0 | 1               the tower's 1x1 convolutions on the generic kernel everywhere | on conv_pw.h wherever it applies,
//                                 instead of where the speed rule says it pays (pw_pays; same bits either way)
//   SAYURI_PW_PIECES=n            conv_pw.h: n pieces per sample in every launch instead of the engine's choice (pw_plan)
//   SAYURI_DW=0 | 1               the depthwise convolutions on depthwise_kernel everywhere | on conv_dw.h wherever it applies,
//                                 instead of where the speed rule says it pays (dw_pays; same bits either way)
//   SAYURI_DW_STRIPS=n            conv_dw.h: n strips per sample in every launch instead of the engine's choice (dw_plan)
// The other switches are described at their fields below.
struct ConvOverride {
    bool v0 = false, no_board = false;
    int wnt = 0;
};
struct EngineFlags {
    ConvOverride conv;
    bool tower = true, se_fused = true, heads_fused = true, arith = true;
    bool latency = false;              // a latency context (sayuri_hip_create_ex): every fp16 3x3 layer whose padded output channels are a
                                       // multiple of 64 runs as many small workgroups (conv_split.h), whatever the batch size; no persistent
                                       // launch, no chains, every SE unit as one launch behind its convolution (for_latency(), se_one,
                                       // Engine::se_unit())
    int latency_split = 0;             // SAYURI_LATENCY_SPLIT=n: strips per board (0: split_auto)
    int latency_ring = 0;              // SAYURI_LATENCY_RING=n: weight stages of the split kernels (0: split_ring)
    int pw = -1;                       // SAYURI_PW: unset (-1) a tower 1x1 takes conv_pw.h where the rule says it pays (route_conv, pw_pays);
                                       // 0: nowhere; 1: wherever the kernel applies
    int pw_pieces = 0;                 // SAYURI_PW_PIECES=n: pieces per sample (0: pw_auto)
    int dw = -1;                       // SAYURI_DW: unset (-1) a depthwise layer takes conv_dw.h where the rule says it pays
                                       // (Engine::depthwise, dw_pays); 0: nowhere; 1: wherever the kernel applies
    int dw_strips = 0;                 // SAYURI_DW_STRIPS=n: strips per sample (0: dw_auto)
    int se_one = -1;                   // SAYURI_SE_ONE: an SE unit that runs as kernels of its own is ONE launch (se_unit_kernel, small_ops.h)
                                       // instead of se_pool / se_fc / se_scale -- unset (-1): in a latency context (Engine::se_unit()'s
                                       // rule); 0: nowhere; 1: wherever Engine::se_unit() or the se_unit tap would run the three.  Same
                                       // bits either way.
    bool tower_chain = true;           // a layer of the persistent run fetches the next layer's first weight group (SAYURI_TOWER_CHAIN=0: off)
    bool tower_gen_epi = true;         // Mish layers of the run take the generated epilogue (SAYURI_TOWER_GEN_EPI=0: the compiled one)
    bool se_split = true;              // SAYURI_SE_SPLIT=0: SE units of layers split over several channel tiles (384 channels) as
                                       // se_pool / se_fc / se_scale again instead of inside the convolution (conv_board_sx.h)
    int tower_noepi_after = -1;        // SAYURI_TOWER_NOEPI_AFTER=n (measuring): from the n-th persistent launch on, the layers with the
                                       // generated epilogue skip it (row_order = 3): timing only, the outputs are stale
    unsigned dbg_sx_epoch0 = 0;        // SAYURI_DEBUG_SX_EPOCH0=n (tests): the exchange tags of a new context start at n (the wrap of the tags)
    bool dbg_sx_stall = false;         // SAYURI_DEBUG_SX_STALL=1 (tests): one sibling of every tile never publishes under the right tag
    int sx_dbg = 0;                    // SAYURI_SX_DBG=n: s_memtime timeline of the n-th split SE convolution of a profiled forward
    int dbg_recycle_input = 0;         // SAYURI_DEBUG_RECYCLE_INPUT=1: hand the packed input's buffer back to the pool after the input
                                       // convolution, as rounds 3-4 did (the row-stride table below then REFUSES the forward); =2: and
                                       // switch the table off -- the race of rounds 3-4 is back (tests/test_gpu_fuzz.py shows that it sees it)
    int chains = 0;                    // SAYURI_CHAINS: 0 = the engine decides, 1 = never, N = N chains whenever a batch qualifies (Engine::forward)
    bool chains_serial = false;        // SAYURI_CHAINS_SERIAL
    bool tower_sync = false;           // SAYURI_TOWER_SYNC
    bool fwdstat = false;              // SAYURI_HIP_FWDSTAT
    int board_kot = 0;                 // experiments: only this channel tile
    int act_override = -1;             // experiments: activation of every board convolution
    int board_dbg = 0, heads_dbg = 0;  // experiments: in-kernel timelines
    static bool off(const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; }
    static EngineFlags from_env() {
        EngineFlags f;
        if (const char* e = getenv("SAYURI_CONV")) {
            if (!strncmp(e, "v0", 2)) { f.conv.v0 = true; f.conv.no_board = true; }
            else if (!strncmp(e, "glds", 4)) { f.conv.no_board = true; (void)sscanf(e, "glds:%d", &f.conv.wnt); }
        }
        f.tower = !off("SAYURI_TOWER");
        f.tower_chain = !off("SAYURI_TOWER_CHAIN");
        f.tower_gen_epi = !off("SAYURI_TOWER_GEN_EPI");
        if (const char* e = getenv("SAYURI_DEBUG_RECYCLE_INPUT")) f.dbg_recycle_input = atoi(e);
        f.se_split = !off("SAYURI_SE_SPLIT");
        if (const char* e = getenv("SAYURI_SX_DBG")) f.sx_dbg = atoi(e);
        f.dbg_sx_stall = getenv("SAYURI_DEBUG_SX_STALL") != nullptr;
        if (const char* e = getenv("SAYURI_DEBUG_SX_EPOCH0")) f.dbg_sx_epoch0 = (unsigned)strtoul(e, nullptr, 0);
        if (const char* e = getenv("SAYURI_TOWER_NOEPI_AFTER")) f.tower_noepi_after = atoi(e);
        f.se_fused = !off("SAYURI_SE_FUSED");
        f.heads_fused = !off("SAYURI_HEADS_FUSED");
        f.arith = !getenv("SAYURI_NO_ARITH");
        if (const char* e = getenv("SAYURI_CHAINS")) f.chains = std::max(0, std::min(atoi(e), 4));
        f.chains_serial = getenv("SAYURI_CHAINS_SERIAL") != nullptr;
        f.tower_sync = getenv("SAYURI_TOWER_SYNC") != nullptr;
        f.fwdstat = getenv("SAYURI_HIP_FWDSTAT") != nullptr;
        if (const char* e = getenv("SAYURI_LATENCY_SPLIT")) f.latency_split = std::max(0, atoi(e));
        if (const char* e = getenv("SAYURI_LATENCY_RING")) f.latency_ring = atoi(e);  // (split_plan refuses what no kernel has)
        if (const char* e = getenv("SAYURI_SE_ONE")) f.se_one = atoi(e) != 0;
        if (const char* e = getenv("SAYURI_PW")) f.pw = atoi(e) != 0;
        if (const char* e = getenv("SAYURI_PW_PIECES")) f.pw_pieces = std::max(0, atoi(e));
        if (const char* e = getenv("SAYURI_DW")) f.dw = atoi(e) != 0;
        if (const char* e = getenv("SAYURI_DW_STRIPS")) f.dw_strips = std::max(0, atoi(e));
#ifdef SAYURI_EXPERIMENTS
        if (const char* e = getenv("SAYURI_BOARD_KOT")) f.board_kot = atoi(e);
        if (const char* e = getenv("SAYURI_ACT_OVERRIDE")) f.act_override = atoi(e);
        if (const char* e = getenv("SAYURI_BOARD_DBG")) f.board_dbg = atoi(e);
        if (getenv("SAYURI_HEADS_DBG")) f.heads_dbg = 1;
        if (f.board_dbg || f.heads_dbg || f.act_override >= 0) f.tower = false;
#endif
        return f;
    }
    // The same switches for a latency context: one launch per layer, one chain, and the SE unit always as kernels of its own
    // behind a split convolution -- the fused forms pool fp32 accumulators that no single workgroup holds here -- which
    // Engine::se_unit() runs as one launch (se_unit_kernel) unless SAYURI_SE_ONE=0 asks for se_pool / se_fc / se_scale.
    EngineFlags for_latency() const {
        EngineFlags f = *this;
        f.latency = true;
        f.tower = false; f.se_fused = false; f.se_split = false; f.chains = 1;
        return f;
    }
};

// allow > 64 KiB of dynamic LDS on the current device
template <typename T> static void se_unit_enable_lds() {
    (void)hipFuncSetAttribute((const void*)&se_unit_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
}
template <typename T> static void enable_big_lds() {
    register_all_convs<T>();
    se_unit_enable_lds<T>();
    for (const auto& e : ConvKernelTable<T>::entries())
        (void)hipFuncSetAttribute((const void*)e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
}

// candidate output-channel tiles, largest first
static int pick_wmt(int cout_s, bool fp16) {
    // KO_T = 32*WMT.  Smallest tile that covers cout_s, else the tile with least padding.
    const int opts16[] = {1, 2, 3, 4, 6, 8};
    const int opts32[] = {1, 2, 3, 4};
    const int* opts = fp16 ? opts16 : opts32;
    const int nopts = fp16 ? 6 : 4;
    for (int i = 0; i < nopts; ++i)
        if (opts[i] * 32 >= cout_s) return opts[i];
    int best = opts[nopts - 1], best_pad = 1 << 30;
    for (int i = nopts - 1; i >= 0; --i) {
        const int kot = opts[i] * 32, pad = round_up(cout_s, kot) - cout_s;
        if (pad < best_pad) { best_pad = pad; best = opts[i]; }
    }
    return best;
}

// ------------------------------------------------------------------ host-side geometry
struct HostGeom {
    std::vector<int> bsz, off;  // off has n+1 entries
    int n = 0, total = 0;
    // worst-case LDS halo positions / subregions of any PT-pixel tile
    void tile_bounds(int PT, int* npos_out, int* nsub_out) const {
        int max_pos = 0, max_sub = 0;
        int s = 0;
        for (int g0 = 0; g0 < total; g0 += PT) {
            const int g1 = std::min(g0 + PT, total);
            while (s + 1 < n && off[s + 1] <= g0) ++s;
            int pos = 0, sub = 0;
            for (int m = s; m < n && off[m] < g1; ++m) {
                const int bs = bsz[m];
                const int a = std::max(g0, off[m]) - off[m], b = std::min(g1, off[m + 1]) - off[m];
                const int rows = (b - 1) / bs - a / bs + 3;
                pos += rows * (bs + 2);
                ++sub;
            }
            max_pos = std::max(max_pos, pos);
            max_sub = std::max(max_sub, sub);
        }
        *npos_out = round_up(std::max(max_pos, 16), 16);
        *nsub_out = max_sub;
    }
};

// The geometry of n samples of the given board sizes (2 .. max_board each) as a plan query or a test tap receives them:
// bsz, off, total.  0, or the refusal under the caller's name.
static int host_geom(int n, const int* board_sizes, int max_board, const std::string& who, HostGeom* hg) {
    if (n <= 0 || !board_sizes || max_board < 2) return fail(who + ": bad argument");
    hg->n = n; hg->bsz.assign(board_sizes, board_sizes + n); hg->off.assign(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (hg->bsz[i] < 2 || hg->bsz[i] > max_board) return fail(who + ": bad board size");
        hg->off[i + 1] = hg->off[i] + hg->bsz[i] * hg->bsz[i];
    }
    hg->total = hg->off[n];
    return 0;
}

// A kernel variant with PT-pixel tiles across samples fits this geometry: the worst tile's halo positions (*npos, what its
// LDS is sized by) and samples.  Its cost: rounds of workgroups over the CUs times the time of a tile.
static bool tile_fits(const HostGeom& geom, int PT, int npos_cap, int* npos) {
    int nsub;
    geom.tile_bounds(PT, npos, &nsub);
    return *npos <= npos_cap && nsub <= kMaxSub;
}
static double tile_cost(const HostGeom& geom, int PT, int kot_tiles, int* ntiles) {
    *ntiles = (geom.total + PT - 1) / PT;
    return std::ceil((double)*ntiles * kot_tiles / kNumCU) * (PT + 24);
}
// The generic conv_mfma variant of channel tile `wmt` for this geometry: the cheapest that fits, or -- `widest`, the test
// taps -- the one with the widest pixel tile.  false: none fits.
template <typename T> struct TileChoice { int wnt, npos, ntiles; const typename ConvKernelTable<T>::Entry* e; };
template <typename T> static bool pick_tile(const HostGeom& geom, int wmt, int kot_tiles, bool widest, TileChoice<T>* out) {
    double best = 0;
    out->e = nullptr;
    for (const auto& e : ConvKernelTable<T>::entries()) {
        int npos, ntiles;
        if (e.wmt != wmt || !tile_fits(geom, 64 * e.wnt, e.npos_cap, &npos) || e.lds(npos) > kMaxLds) continue;
        const double cost = tile_cost(geom, 64 * e.wnt, kot_tiles, &ntiles), score = widest ? -e.wnt : cost;
        if (!out->e || score < best) { best = score; *out = TileChoice<T>{e.wnt, npos, ntiles, &e}; }
    }
    return out->e != nullptr;
}

// Choose the tuned LDS-DMA kernel variant for an fp16 3x3 layer with `ko_pad` weight rows on
// this batch geometry; nullptr when none applies (the generic conv_mfma kernel is used then).
static const GldsEntry* pick_glds(const HostGeom& geom, int ko_pad, int* ntiles_out, const ConvOverride& ov) {
    if (ko_pad % 128 != 0) return nullptr;
    if (ov.v0) return nullptr;
    const int wmt = ko_pad % 256 == 0 ? 8 : 4;
    const int kot_tiles = ko_pad / (wmt * 32);
    const GldsEntry* best = nullptr;
    double best_cost = 1e30;
    for (const auto& e : glds_entries()) {
        if (e.wmt != wmt) continue;
        if (ov.wnt && e.wnt != ov.wnt) continue;
        int npos, ntiles;
        if (!tile_fits(geom, e.pt, e.npos_cap, &npos) || e.lds > kMaxLds) continue;
        const double cost = tile_cost(geom, e.pt, kot_tiles, &ntiles);
        if (cost < best_cost) { best_cost = cost; best = &e; *ntiles_out = ntiles; }
    }
    return best;
}

// The one-workgroup-per-board plan of a batch geometry (conv_board.h): consecutive samples packed greedily.
struct BoardPlan {
    int ntiles = 0, npos = 0;
    bool ok = false, single = false;  // single: one sample per tile
    int uniform_info = -1;            // every tile has this (column tiles | board size << 8), or -1
    std::vector<int> tile_first;      // first sample of every tile, then the number of samples (ntiles + 1 entries)
};
static BoardPlan board_plan(const HostGeom& geom, const ConvOverride& ov) {
    BoardPlan bp;
    if (ov.no_board || geom.n <= 0) return bp;
    BoardPack pk;
    int max_pos = 0, info0 = -2;
    int tile_start = 0;
    auto close_tile = [&] {
        bp.tile_first.push_back(tile_start);
        max_pos = std::max(max_pos, pk.pos);
        const int info = ((pk.px + 15) / 16) | (pk.bs0 << 8);
        info0 = info0 == -2 ? info : (info0 == info ? info0 : -1);
        ++bp.ntiles;
    };
    for (int s = 0; s < geom.n; ++s) {
        const int bs = geom.bsz[s];
        if (!BoardPack{}.fits(bs)) return bp;  // a board that does not fit a tile on its own
        if (pk.cnt > 0 && !pk.fits(bs)) {
            close_tile();
            pk = BoardPack{};
            tile_start = s;
        }
        pk.add(bs);
    }
    close_tile();
    bp.tile_first.push_back(geom.n);
    bp.uniform_info = info0;
    bp.npos = round_up(max_pos, 64);
    bp.single = bp.ntiles == geom.n;
    bp.ok = true;
    return bp;
}
static const BoardEntry* pick_board(const BoardPlan& bp, int ko_pad, int* kot_tiles, int force = 0) {
    if (!bp.ok) return nullptr;
    // the channel tile that needs the fewest rounds of workgroups over the 256 CUs (time of a round ~ its channel count);
    // ties go to the larger tile (the halo is staged once per workgroup)
    const BoardEntry* best = nullptr;
    long best_cost = 0;
    for (const auto& e : kBoardEntries) {
        if (ko_pad % e.kot != 0 || e.lds(bp.npos) > kMaxLds) continue;
        if (force && force != e.kot) continue;
        const long kts = ko_pad / e.kot, rounds = (bp.ntiles * kts + kNumCU - 1) / kNumCU, cost = rounds * e.kot;
        if (!best || cost < best_cost) { best = &e; best_cost = cost; *kot_tiles = (int)kts; }
    }
    return best;
}
// Which kernel runs a k x k convolution with `ko_pad` weight rows on this geometry (`plan` = board_plan(geom, ov)): fp16 3x3
// layers one workgroup per board (`board`, `tiles` channel tiles per board tile) -- in a latency context many small workgroups
// (kConvSplit) --, else the LDS-DMA tiles across samples
// (`glds`, `tiles` pixel tiles), everything else the generic conv_mfma kernel (pick_tile).  The values are what
// sayuri_hip_test_last_conv_kind reports (kConvBoardSx: never a route -- a block's last convolution with its SE unit inside,
// Engine::conv_sx; the tap sayuri_hip_test_conv_sx reports it).
// kConvPw: a TOWER 1x1 layer of the fp16 engine (conv_pw.h), in a default and in a latency context alike.
// kConvDwLds: a depthwise layer of the fp16 engine on conv_dw.h (Engine::depthwise chooses; kConvDepthwise is depthwise_kernel).
enum ConvFamily { kConvGeneric = 0, kConvGlds = 1, kConvBoard = 2, kConvDepthwise = 3, kConvSplit = 4, kConvBoardSx = 5, kConvPw = 6,
                  kConvDwLds = 7 };

// What the three many-small-workgroups families share (conv_split.h, conv_pw.h, conv_dw.h): a sample's pixels are cut into items --
// strips of rows, pieces of column tiles --, an item times a channel tile (a slice) is one workgroup.  THE CUT RULE, where the
// caller forces no cut: as many items per sample as keep the launch near one round of the chip -- round / (samples x channel
// tiles), at least one; what a round is, and the family's own bounds, are stated at each plan.  The cut decides speed only.
// cut: the items a sample is cut into (a small board may have fewer); items: per sample in the grid, what the sample with the most
// has; tiles: channel tiles / slices; grid = samples x items x tiles; why: what refused a plan that is not ok.
struct CutPlan {
    bool ok = false;
    int cut = 0, items = 0, tiles = 0, grid = 0;
    size_t lds = 0;
    std::string why;
};
template <typename P> static P refused(P plan, const std::string& why) { plan.why = why; return plan; }
static int cut_for_round(int round, int ns, int tiles) { return std::max(1, round / std::max(1, ns * tiles)); }
// "This layer is the kernel's kind": whole 64-channel tiles of weight rows (conv_split.h); whole 32-channel chunks into whole
// 64-channel tiles (conv_pw.h).  route_conv, the plans, the taps and the plan queries ask here.
static bool split_covers(int ko_pad) { return ko_pad > 0 && ko_pad % kSplitKO == 0; }
static bool pw_covers(int cin, int cout, int ko_pad) { return cout % kPwKO == 0 && cin % kChunk == 0 && ko_pad % kPwKO == 0; }

// The many-small-workgroups plan of a tower 1x1 layer (conv_pw.h) for the samples [n0, n0 + ns): how many pieces a sample's
// pixels are cut into, the grid, the kernel variant and its LDS.  Host arithmetic only.
// The rule (pieces == 0): the cut rule (CutPlan) with a round of kPwRound -- kPwRound / (samples x channel
// tiles), at least one, a piece never smaller than one column tile (pw_cols) nor wider than the widest variant -- so a lone 19x19
// board on 128 output channels is cut into one piece per column tile and a batch of 256 gets one piece per sample.  A round is
// counted as three workgroups per CU: the thin variants (NJ <= 3, at most 48 KiB of LDS) are co-resident three to a CU.  The
// constant is a supposition -- no measurement compares this cut with 256 / (samples x channel tiles) -- in the direction the rows
// show: few wide pieces are what the kernel is bad at (DESIGN.md Kernel 1i: at 256 boards one piece per sample takes 1.15 to 1.30
// of the generic kernel's forward where four pieces take 0.78 to 0.81).  It decides the speed only: the
// results do not depend on the cut.  pieces == n forces n (SAYURI_PW_PIECES, the tap): a cut whose pieces
// would be wider than the widest variant holds is refused, not narrowed.
struct PwPlan : CutPlan { const PwEntry* e = nullptr; };  // cut: pieces
constexpr int kPwRound = 3 * kNumCU;
static int pw_auto(int ns, int kts) { return cut_for_round(kPwRound, ns, kts); }
static PwPlan pw_plan(const HostGeom& geom, int n0, int ns, int ko_pad, int cin_s, int pieces) {
    PwPlan pp;
    pp.why = "no pointwise plan for this layer or batch geometry";  // every refusal but the too-wide piece
    if (ns <= 0 || n0 < 0 || n0 + ns > geom.n || ko_pad <= 0 || ko_pad % kPwKO || cin_s <= 0 || cin_s % kChunk || pieces < 0) return pp;
    pp.tiles = ko_pad / kPwKO;
    pp.cut = pieces > 0 ? pieces : pw_auto(ns, pp.tiles);
    int max_cols = 0;
    for (int s = n0; s < n0 + ns; ++s) {
        const int bs = geom.bsz[s], ncol = (bs * bs + 15) / 16, cp = pw_cols(bs, pp.cut, /*cap=*/pieces == 0);
        if (cp > kPwMaxCols)
            return refused(pp, "a piece of " + std::to_string(cp) + " column tiles is wider than the kernel's " + std::to_string(kPwMaxCols) +
                                   " (SAYURI_PW_PIECES / pieces too small for this board)");
        pp.items = std::max(pp.items, (ncol + cp - 1) / cp);
        max_cols = std::max(max_cols, cp);
    }
    for (const auto& e : kPwEntries)
        if (!pp.e && 2 * e.nj >= max_cols) pp.e = &e;
    if (!pp.e) return pp;
    pp.lds = pw_lds_bytes(pp.e->nj);
    pp.grid = ns * pp.items * pp.tiles;
    pp.ok = pp.lds <= kMaxLds;
    if (pp.ok) pp.why.clear();
    return pp;
}
// The kernel's part of a launch (conv_params fills q.c before).  (The kernel caps a piece at the widest variant as the rule does;
// a forced cut that the cap would change was refused above.)
static void pw_params(PwParams& q, const PwPlan& pp, int n0) {
    q.c.npos = 0; q.c.num_pix_tiles = 0;
    q.pieces = pp.cut; q.pmax = pp.items; q.kts = pp.tiles; q.n0 = n0;
}
static void pw_launch(const PwPlan& pp, const PwParams& q, hipStream_t s) {
    hipLaunchKernelGGL(pp.e->fn, dim3(pp.grid), dim3(256), pp.lds, s, q);
}
// What route_conv needs to know of a 1x1 layer to give it conv_pw.h: null for every layer that is not a tower 1x1 (block slots
// PRE_BTL, POST_BTL, mixer CONV1 / CONV2) and under SAYURI_PW=0.
struct PwAsk { int cin, cout, cin_s, n0, ns, pieces; bool force; };  // force: SAYURI_PW=1, the taps -- the speed rule is not asked
// The speed rule of the route: the regimes where conv_pw.h is ahead of the generic kernel beyond the method's spread -- a launch
// whose samples get at least three pieces each, samples x channel tiles <= 256.  Measured (DESIGN.md Kernel 1i,
// profiles/r12_pw_conv.json): up to 64 boards of 19x19 every tower 1x1 of the 256 / 128 and 256-channel mixer networks qualifies
// and a forward takes 0.41 to 0.88 of its time on the generic kernel; with one or two pieces a sample (128 boards on three or more
// channel tiles, 256 boards) the kernel is level or 10 to 30 % of a forward behind.  Decides speed only.
static bool pw_pays(int ns, int kts) { return pw_auto(ns, kts) >= 3; }

// The plan of a depthwise k x k layer on LDS (conv_dw.h) for the samples [n0, n0 + ns): the channel slice, how many strips of
// rows a sample is cut into, the grid, the kernel variant (one per k) and its LDS.  Host arithmetic only.
// The slice is 64 channels where cs % 64 == 0 (a pixel's slice is one 128-byte line), 32 otherwise.
// The rule (strips == 0): the cut rule (CutPlan) with a round of kDwRound --
// kDwRound / (samples x slices), at least one, never more than a board has rows -- so a lone 19x19 board is cut into one strip per
// row and 256 boards are not cut at all (a strip re-reads its k - 1 halo rows: cutting a full batch only adds traffic).  A
// round is counted as two workgroups per CU, what kDwMaxLds leaves room for: a supposition, not A/B-measured.  A batch of boards
// so large that an uncut sample exceeds kDwMaxLds is cut until it fits.  strips == n forces n (SAYURI_DW_STRIPS, the tap): more
// strips than the largest board of the range has rows, or a cut whose item exceeds kDwMaxLds, is refused, not changed (a smaller
// board of a mixed batch has one strip per row at most: dw_rows).  The cut decides speed only.
struct DwPlan : CutPlan { int sp = 0, rows = 0; const DwEntry* e = nullptr; };  // cut: strips; tiles: slices; sp: 16-byte pieces of a pixel's slice; rows: the largest board's
// Where a follow-up should look (DESIGN.md Kernel 1j, profiles/r13_dw_conv.json): at small batches the constant cuts too FINELY --
// four forced strips beat the plan's eight at 16 boards (0.918 against 0.942 of the old kernel's forward) and its nineteen at 8
// boards in a latency context (0.904 against 0.923), one strip beats nine on a lone 9x9 board (0.883 against 0.903); from 32 boards
// on the plan's cut is the best measured.
constexpr int kDwRound = 2 * kNumCU;
static int dw_auto(int ns, int slices) { return cut_for_round(kDwRound, ns, slices); }
static size_t dw_plan_lds(const HostGeom& geom, int n0, int ns, int k, int sp, int strips) {
    size_t lds = 0;
    for (int s = n0; s < n0 + ns; ++s) {
        const int bs = geom.bsz[s], rp = dw_rows(bs, strips);
        for (int r0 = 0; r0 < bs; r0 += rp)  // the kernel's own arithmetic: a strip and the halo rows inside the board
            lds = std::max(lds, dw_lds_bytes(k, sp, (std::min(bs, std::min(bs, r0 + rp) + k / 2) - std::max(0, r0 - k / 2)) * bs));
    }
    return lds;
}
static DwPlan dw_plan(const HostGeom& geom, int n0, int ns, int cs, int k, int strips) {
    DwPlan dp;
    if (ns <= 0 || n0 < 0 || n0 + ns > geom.n || cs <= 0 || strips < 0) return refused(dp, "bad argument");
    for (const auto& e : kDwEntries)
        if (e.k == k) dp.e = &e;
    if (!dp.e) return refused(dp, "a depthwise layer of k = " + std::to_string(k) + " keeps depthwise_kernel (conv_dw.h has k = 3, 5, 7)");
    if (cs % 32) return refused(dp, "a channel stride of " + std::to_string(cs) + " is not whole 32-channel slices");
    dp.sp = cs % 64 == 0 ? 8 : 4;
    dp.tiles = cs / (8 * dp.sp);
    for (int s = n0; s < n0 + ns; ++s) dp.rows = std::max(dp.rows, geom.bsz[s]);
    if (strips > dp.rows)
        return refused(dp, std::to_string(strips) + " strips are more than the " + std::to_string(dp.rows) + " rows of the largest board (SAYURI_DW_STRIPS / strips)");
    dp.cut = strips > 0 ? strips : std::min(dp.rows, dw_auto(ns, dp.tiles));
    dp.lds = dw_plan_lds(geom, n0, ns, k, dp.sp, dp.cut);
    while (strips == 0 && dp.lds > kDwMaxLds && dp.cut < dp.rows) dp.lds = dw_plan_lds(geom, n0, ns, k, dp.sp, ++dp.cut);
    if (dp.lds > kDwMaxLds)
        return refused(dp, "an item of " + std::to_string(dp.lds) + " bytes of LDS is more than the kernel's " + std::to_string(kDwMaxLds) +
                               " (SAYURI_DW_STRIPS / strips too small for this board)");
    for (int s = n0; s < n0 + ns; ++s) {
        const int bs = geom.bsz[s], rp = dw_rows(bs, dp.cut);
        dp.items = std::max(dp.items, (bs + rp - 1) / rp);
    }
    dp.grid = ns * dp.items * dp.tiles;
    dp.ok = true;
    return dp;
}
static void dw_params(DwParams& q, const DwPlan& dp, int n0) {
    q.sp = dp.sp; q.slices = dp.tiles; q.strips = dp.cut; q.smax = dp.items; q.n0 = n0;
}
static void dw_launch(const DwPlan& dp, const DwParams& q, hipStream_t s) {
    hipLaunchKernelGGL(dp.e->fn, dim3(dp.grid), dim3(kDwThreads), dp.lds, s, q);
}
// The speed rule of Engine::depthwise.  Measured (DESIGN.md Kernel 1j, profiles/r13_dw_conv.json): on ten 7x7 mixer blocks at 256
// channels a forward under the plan's cut takes 0.73 to 0.94 of its time on depthwise_kernel at every point -- default contexts at 1,
// 16, 32, 64, 128, 256 boards of 19x19 (ratios 0.89, 0.94, 0.82, 0.78, 0.73, 0.74), latency contexts at 1, 8, 32 boards and one 9x9
// board (0.89, 0.92, 0.82, 0.90) -- each beyond the spread of the method (at most 0.008); a launch takes 21.6 us instead of 35.7 at
// 32 boards and 89.5 instead of 222.1 at 256; the RepLK head's one layer moves a residual network's forward by 0.2 to 1.8 %.  No regime loses, so the rule takes the kernel wherever its plan fits.  (What loses is
// a forced cut: one or two strips a sample at up to 32 boards, 1.10 to 1.47 -- SAYURI_DW_STRIPS, not the plan.)  Decides speed only.
static bool dw_pays() { return true; }

struct ConvRoute {
    ConvFamily family = kConvGeneric;
    const BoardEntry* board = nullptr;
    const GldsEntry* glds = nullptr;
    int tiles = 0;
    PwPlan pw;  // kConvPw
};
static ConvRoute route_conv(bool fp16, int k, int ko_pad, const HostGeom& geom, const BoardPlan& plan, const ConvOverride& ov, int force_kot = 0,
                            bool latency = false, const PwAsk* pw = nullptr) {
    ConvRoute r;
    // a tower 1x1 of whole 64-channel tiles over whole 32-channel chunks: many small workgroups (conv_pw.h) where the plan fits
    // and the rule says it pays
    if (fp16 && k == 1 && pw && pw_covers(pw->cin, pw->cout, ko_pad)) {
        r.pw = pw_plan(geom, pw->n0, pw->ns, ko_pad, pw->cin_s, pw->pieces);
        if (r.pw.ok && (pw->force || pw_pays(pw->ns, r.pw.tiles))) r.family = kConvPw;
        return r;
    }
    if (!fp16 || k != 3) return r;
    // a latency context: many small workgroups (`split`; the plan is split_plan's) for every batch; a layer whose weight rows
    // are not whole 64-channel tiles keeps the route below
    if (latency && split_covers(ko_pad)) { r.family = kConvSplit; return r; }
    if ((r.board = pick_board(plan, ko_pad, &r.tiles, force_kot))) r.family = kConvBoard;
    else if ((r.glds = pick_glds(geom, ko_pad, &r.tiles, ov))) r.family = kConvGlds;
    return r;
}

// The many-small-workgroups plan of a latency context (conv_split.h) for the samples [n0, n0 + ns) and a layer of `ko_pad`
// weight rows: how many strips a board is cut into, the grid, the kernel variant and its LDS.
// The split rule (strips == 0): the cut rule (CutPlan) with a round of the 256 CUs -- 256 / (samples x
// channel tiles), at least one, at most kSplitAutoMax and never more than a board has rows (split_rows) -- so a lone board is
// cut finely and a batch of 64 not at all.  It decides the speed only: the results do not depend on the split.
// The ring rule (ring == 0): the weight stages of the variant with `nj` column tiles per wave.  Like the split it decides the
// speed only, and it looks at nothing but nj -- which the batch geometry decides, as it decides the split.  Measured (DESIGN.md
// Kernel 1h, profiles/r11_latency_ring.json): the four-stage ring is 5 to 8 % of a forward ahead at nj = 1 (one or two 19x19
// boards, a lone small board, sixteen 9x9 boards on 256 channels) and level or up to 1.4 % behind at nj = 2 and 3, so only
// nj = 1 takes it; the wide variants have no deeper ring.  ring == n forces n stages: where the chosen variant has no such
// instantiation, or its LDS does not fit, the plan is not ok (why says so).
constexpr int kSplitAutoMax = 19;
struct SplitPlan : CutPlan { int npos = 0, stages = 0; const SplitEntry* e = nullptr; };  // cut: strips
static int split_auto(int ns, int kts) { return std::min(kSplitAutoMax, cut_for_round(kNumCU, ns, kts)); }
static int split_ring(int nj) { return nj == 1 ? kSplitDeepStages : kSplitStages; }
static SplitPlan split_plan(const HostGeom& geom, int n0, int ns, int ko_pad, int strips, int ring) {
    SplitPlan sp;
    sp.why = "no split fits this batch geometry";  // every refusal but the ring no variant has
    if (ns <= 0 || n0 < 0 || n0 + ns > geom.n || !split_covers(ko_pad)) return sp;
    sp.tiles = ko_pad / kSplitKO;
    sp.cut = strips > 0 ? strips : split_auto(ns, sp.tiles);
    int max_pos = 0, max_cols = 0;
    for (int s = n0; s < n0 + ns; ++s) {
        const int bs = geom.bsz[s], rp = split_rows(bs, sp.cut);
        sp.items = std::max(sp.items, (bs + rp - 1) / rp);
        max_pos = std::max(max_pos, (rp + 2) * (bs + 2));
        max_cols = std::max(max_cols, (rp * bs + 15) / 16);
    }
    sp.npos = round_up(max_pos, 64);
    if (sp.npos > kSplitMaxPos || max_cols > kSplitMaxCols) return sp;
    for (const auto& e : kSplitEntries)
        if (!sp.e && e.stages == kSplitStages && 2 * e.nj >= max_cols) sp.e = &e;
    if (!sp.e) return sp;
    const int want = ring ? ring : split_ring(sp.e->nj);
    if (want != kSplitStages) {  // the same width with the ring asked for; the rule keeps three stages where a deeper ring does not fit
        const SplitEntry* deep = nullptr;
        for (const auto& e : kSplitEntries)
            if (e.nj == sp.e->nj && e.stages == want && split_lds_bytes(sp.npos, want) <= kMaxLds) deep = &e;
        if (deep) sp.e = deep;
        else if (ring)
            return refused(sp, "no split kernel with a ring of " + std::to_string(ring) + " weight stages fits this batch geometry (SAYURI_LATENCY_RING)");
    }
    sp.stages = sp.e->stages;
    sp.lds = split_lds_bytes(sp.npos, sp.stages);
    sp.grid = ns * sp.items * sp.tiles;
    sp.ok = sp.lds <= kMaxLds;
    if (sp.ok) sp.why.clear();
    return sp;
}
// The split kernels' part of a launch (conv_params fills q.c before): the halo bound, the split and the first sample.
static void split_params(SplitParams& q, const SplitPlan& sp, int n0) {
    q.c.npos = sp.npos; q.c.num_pix_tiles = 0;
    q.strips = sp.cut; q.smax = sp.items; q.kts = sp.tiles; q.n0 = n0;
}
static void split_launch(const SplitPlan& sp, const SplitParams& q, hipStream_t s) {
    hipLaunchKernelGGL(sp.e->fn, dim3(sp.grid), dim3(256), sp.lds, s, q);
}

// ------------------------------------------------------------------ the parameters of one 3x3 / 1x1 convolution launch
// Shared by Engine<T> and the layer-level test taps.  conv_params fills every field but npos and num_pix_tiles (the kernel
// family decides them) member by member, so a struct the caller zeroed keeps zero padding.
static void conv_params(ConvParams& p, const void* in, const void* w, const float* bias, const void* res, void* out, const BatchGeom& g,
                        int cin_s, int cout_s, int ko_pad, int taps, int act) {
    p.in = in; p.w = w; p.bias = bias; p.res = res; p.out = out;
    p.g = g;
    p.cin_s = cin_s; p.cout_s = cout_s; p.ko_pad = ko_pad;
    p.taps = taps; p.act = act;
}
// The board kernels' part of a launch over the tiles of `plan` (conv_params fills bp.c afterwards).  Zeroed first: the tower
// table is compared bytewise with its cached copy (Engine::tower_flush).  The kernels compute their table entries (arith) when
// every tile is one sample of one size and the caller allows it (SAYURI_NO_ARITH).
static void board_params(BoardParams& bp, const BoardPlan& plan, const int* tab_src, const int2* tab_pix, const int* tab_cols, bool arith) {
    std::memset(&bp, 0, sizeof(bp));
    bp.tab_src = tab_src; bp.tab_pix = tab_pix; bp.tab_cols = tab_cols;
    bp.npos = plan.npos;
    bp.uniform_info = plan.uniform_info;
    bp.arith = plan.single && plan.uniform_info >= 0 && arith ? 1 : 0;
}
// Does a layer of the persistent launch get the generated epilogue (tower_seam.py epi_hook)?  Then its weights and bias go in
// board_row_channel order and BoardParams::row_order says so.  What the generated text covers (`gen_epi`: SAYURI_TOWER_GEN_EPI):
// Mish / ReLU / no activation, one sample per tile with computed table entries (arith), the layer's channels = the channel tile
// `kot`, an even number of row tiles per wave.  bp.c filled (conv_params).
static bool board_row_order_ok(const BoardParams& bp, int kot, bool gen_epi) {
    const ConvParams& p = bp.c;
    return gen_epi && !bp.dbg && board_uses_row_order(kot) && bp.arith && (p.act == kMish || p.act == kReLU || p.act == kIdentity) &&
           p.cout_s == kot && p.ko_pad == kot;
}
// A board convolution as an element of the persistent launch's table (conv_tower.h); tower_link fills self / last.  What the
// bodies never read (tile = workgroup id, the launch's grid is the batch) is left out of the table, so that a batch of 250
// positions finds the table of a batch of 256 in place and nothing is uploaded (Engine::tower_flush compares bytewise).
static TowerLayer tower_element(const BoardSeParams& sp, bool has_se) {
    TowerLayer t;
    std::memset(&t, 0, sizeof(t));
    t.sp = sp;
    t.has_se = has_se ? 1 : 0;
    ConvParams& c = t.sp.b.c;
    c.num_pix_tiles = 0;
    c.g.n_samples = 0;
    c.g.total_pix = 0;
    return t;
}
// Links the elements of one run, which will sit at dev_base[0 .. run.size()) on the device: every element's own address, the
// end of the run, and -- `chain` (SAYURI_TOWER_CHAIN) -- the weight hand-over (conv_board.h, CHAIN main loop): a plain layer
// without residual leaves the LDS alone after its K loop, so its last K group can bring in the next layer's first weight group.
// Needs the same weight geometry on both sides (the piece addresses are computed with this layer's strides) and an even number
// of 32-channel chunks (the last group then sits in ring slot 1 and slot 0 is free).  Returns the number of hand-overs.
static int tower_link(std::vector<TowerLayer>& run, const TowerLayer* dev_base, bool chain) {
    const int n = (int)run.size();
    for (int i = 0; i < n; ++i) {
        run[i].self = dev_base + i;
        run[i].last = i + 1 == n ? 1 : 0;
    }
    int links = 0;
    for (int i = 0; i + 1 < n && chain; ++i) {
        const ConvParams &a = run[i].sp.b.c, &b = run[i + 1].sp.b.c;
        if (run[i].has_se || a.res || a.cin_s != b.cin_s || a.ko_pad != b.ko_pad || (a.cin_s / kChunk) % 2) continue;
        run[i].sp.b.w_next = b.w;
        run[i + 1].sp.b.w_ready = 1;
        ++links;
    }
    return links;
}
// The across-sample kernel's part of a launch of `e` over `ntiles` pixel tiles (conv_params has filled gp.c); returns the grid.
static int glds_params(GldsParams& gp, const GldsEntry& e, const int* tab_src, const int2* tab_pix, const float* zeros, int ntiles) {
    gp.tab_src = tab_src; gp.tab_pix = tab_pix; gp.zeros = zeros;
    gp.c.npos = 0; gp.c.num_pix_tiles = ntiles;
    return ntiles * (gp.c.ko_pad / (e.wmt * 32));
}
// The convolution with the SE unit inside it (conv_board_se_kernel, the same stage in the persistent launch): the host's rule, for
// Engine::conv_se and the taps alike.  The board entry with an SE kernel whose channel tile is the WHOLE layer, whatever the batch
// size -- a position's result must not depend on how many others share its batch: a small batch would otherwise pick two half-width
// workgroups and the separate SE kernels, which round x to fp16 before pooling --; pick_board_se: ... and whose LDS fits `plan`.
static const BoardEntry* board_se_entry(int ko_pad) {
    for (const auto& e : kBoardEntries)
        if (e.fn_se && e.kot == ko_pad) return &e;
    return nullptr;
}
static const BoardEntry* pick_board_se(const BoardPlan& plan, int ko_pad) {
    const BoardEntry* e = plan.ok ? board_se_entry(ko_pad) : nullptr;
    return e && e->lds(plan.npos) <= kMaxLds ? e : nullptr;
}
// A unit whose images are not staged in LDS (make_se_images refused it) still runs inside the kernel with its FCs read from L2
// when the FC widths suit the kernel's loops: squeeze outputs and excite outputs in whole fours that divide 512 lanes' work.
static bool se_l2_form_ok(int sq_out, int ex_out) {
    if (sq_out <= 0 || ex_out <= 0 || sq_out % 4 || ex_out % 4) return false;  // (in front of the divisions)
    return sq_out <= 512 && ex_out <= 2048 && 512 % (sq_out / 4) == 0 && 512 % (ex_out / 4) == 0;
}
// The stage's own fields of a launch: the two FCs, the channels, and -- both or neither -- the staged images (null: the L2 form).
static void se_stage_params(BoardSeParams& sp, const FcDev& sq, const FcDev& ex, int C, const void* w1h, const void* w2h, int w1_bytes,
                            int w2_bytes) {
    sp.squeeze = sq; sp.excite = ex; sp.C = C;
    sp.w1h = w1h; sp.w2h = w2h; sp.w1_bytes = w1_bytes; sp.w2_bytes = w2_bytes;
}
// The split-channel SE convolution (conv_board_sx.h): which boards it takes, its board kernel entry, its part of a launch and
// its grid.  A board takes the form when at most kSxMaxSub samples of its size fit a tile (9x9 and larger): the kernel pools
// that many samples per tile.
static bool sx_board_fused(int bs) {
    BoardPack pk;
    int k = 0;
    while (pk.fits(bs)) { pk.add(bs); ++k; }
    return k <= kSxMaxSub;
}
// The 128-row board entry whose rings fit a tile of `npos` halo positions (the kernel's channel tile is 128), or nullptr.
static const BoardEntry* sx_board_entry(int npos) {
    const BoardEntry* be = nullptr;
    for (const auto& e : kBoardEntries)
        if (e.kot == 128 && e.lds(npos) <= kMaxLds) be = &e;
    return be;
}
// The kernel's own fields of a launch (board_params and conv_params fill sp.b; c.npos / c.num_pix_tiles = the launch's first tile
// and tile count): the per-channel-tile images of make_sx_images for boards 2..`board`, the exchange buffer
// [tile][kt][kSxMaxSub][kSxSlots], this launch's tag (never 0) and the host-visible error word.
static void sx_params(BoardSxParams& sp, const void* w1t, const void* w2t, int w1_bytes, int w2_bytes, int board, int se, int kts,
                      unsigned long long* xchg, unsigned epoch, unsigned* err, bool dbg_stall) {
    sp.w1t = w1t; sp.w2t = w2t; sp.w1_bytes = w1_bytes; sp.w2_bytes = w2_bytes;
    sp.nsizes = board - 1; sp.se = se; sp.kts = kts;
    sp.xchg = xchg; sp.epoch = epoch; sp.err = err;
    sp.dbg_stall = dbg_stall ? 1 : 0;
}
// Workgroups of a launch over `tiles` board tiles: whole groups of 8 tiles x kts siblings (the last group's empty places leave at once).
static int sx_grid(int tiles, int kts) { return (tiles + 7) / 8 * 8 * kts; }

// What a convolution over `px` pixels computes and moves (the flops / bytes of the profile rows and of bench.py's
// tower_conv_mfma_frac): the activations in, out (and the residual), the weights once.
struct ConvCost { double flops, bytes; };
static ConvCost conv_cost(double px, int cin, int cout, int taps, bool res, size_t elem_bytes) {
    return ConvCost{2.0 * px * cin * cout * taps, elem_bytes * (px * cin + px * cout * (res ? 2 : 1) + (double)cin * cout * taps)};
}

struct Stat {
    int launches = 0;
    float ms = 0.f;
    double flops = 0, bytes = 0;
};

// ------------------------------------------------------------------ layers
struct ConvLayerDev {
    int cin = 0, cout = 0, k = 0;
    bool depthwise = false;
    std::vector<float> hw, hb;  // host tensors as handed over the ABI
    int cin_s = 0, cout_s = 0, wmt = 0, ko_pad = 0;
    void* w = nullptr;      // MFMA image, or [k*k][cs] fp32 for depthwise
    void* w_board = nullptr;  // the same image in board_row_channel order (fp16 3x3 layers a board kernel may run) ...
    float* bias_board = nullptr;  // ... and the bias in the same order: what a layer gets whose epilogue is the generated one
    float* bias = nullptr;  // [ko_pad] / [cs]
    float* w32 = nullptr;   // plain fp32 copy [cout][cin] for the tiny head convs
};
struct FcLayerDev {
    int in = 0, out = 0;
    std::vector<float> hw, hb;
    float* wt = nullptr;  // [in][out]
    float* b = nullptr;
    void* img16 = nullptr;  // SE units of the fp16 engine: the LDS-staging image of conv_board.h (BoardSeParams::w1h / w2h)
    int img_bytes = 0;      // bytes of one image (whole 1 KiB pieces)
    void* sx_img = nullptr; // ... and the per-channel-tile images of conv_board_sx.h (BoardSxParams::w1t / w2t), layers of 2-4 tiles of 128
    int sx_bytes = 0;
    FcDev dev() const { return FcDev{wt, b, in, out}; }
};

// ------------------------------------------------------------------ host-side images shared by the engine and the test taps
// A 1x1 / 3x3 layer's output-channel tile (32 * wmt) and its weight rows padded to whole tiles.
static void conv_tile(int cout_s, bool fp16, int* wmt, int* ko_pad) {
    *wmt = pick_wmt(cout_s, fp16);
    *ko_pad = round_up(cout_s, *wmt * 32);
}
// Its MFMA image [tap][chunk of 32 input channels][k-group of 8][ko_pad][8] out of w [cout][cin][taps] (conv_mfma.h), ...
template <typename T> static std::vector<T> conv_image(const float* w, int cin, int cout, int taps, int ko_pad) {
    const int nch = round_up(cin, 32) / 32;
    std::vector<T> img((size_t)taps * nch * 4 * ko_pad * 8, (T)0.f);
    for (int t = 0; t < taps; ++t)
        for (int ko = 0; ko < cout; ++ko)
            for (int c = 0; c < cin; ++c)
                img[((((size_t)t * nch + c / 32) * 4 + (c % 32) / 8) * ko_pad + ko) * 8 + c % 8] = (T)w[((size_t)ko * cin + c) * taps + t];
    return img;
}
// ... and a layer's bias padded with zeros to `n_pad` entries (b == null: no bias).
static std::vector<float> padded_bias(const float* b, int n, int n_pad) {
    std::vector<float> out(n_pad, 0.f);
    if (b) std::copy(b, b + n, out.begin());
    return out;
}
// A depthwise layer's weights [c][taps] -> [tap][cout_s] (depthwise_kernel, small_ops.h).
static std::vector<float> depthwise_image(const float* w, int cout, int taps, int cout_s) {
    std::vector<float> wt((size_t)taps * cout_s, 0.f);
    for (int c = 0; c < cout; ++c)
        for (int t = 0; t < taps; ++t) wt[(size_t)t * cout_s + c] = w[(size_t)c * taps + t];
    return wt;
}
static std::vector<float> fc_transposed(const float* w, int in, int out) {  // [out][in] -> [in][out] (FcDev::wt)
    std::vector<float> t((size_t)in * out);
    for (int o = 0; o < out; ++o)
        for (int i = 0; i < in; ++i) t[(size_t)i * out + o] = w[(size_t)o * in + i];
    return t;
}

// fp16 images of an SE unit's two FCs for the LDS staging of board_se_stage (conv_board.h, BoardSeParams::w1h / w2h):
// the squeeze weights once per board size 2..board with the scaled-mean third of the pooled vector folded into the mean
// third (reference GlobalPooling<false>, se_unit.cc:9-40: pool = (mean, mean * (B-14)/10, max)), the excite weights with
// both bias vectors behind them.  sq_w [se][3C], ex_w [2C][se] as handed over the ABI.  false: the unit does not fit.
static bool make_se_images(int C, int se, int board, const float* sq_w, const float* sq_b, const float* ex_w, const float* ex_b,
                           std::vector<f16>* img1, std::vector<unsigned char>* img2, int* w1_bytes_out, int* w2_bytes_out) {
    if (se <= 0 || se % 4 || se > 512 || 2 * C > 512) return false;
    const int w1_bytes = round_up(2 * C * se * 2, 1024), w2_bytes = round_up(se * 2 * C * 2 + (2 * C + se) * 4, 1024);
    if ((size_t)w1_bytes + w2_bytes + 20 * 1024 > kMaxLds) return false;
    img1->assign((size_t)(board - 1) * (w1_bytes / 2), (f16)0.f);
    for (int bs = 2; bs <= board; ++bs) {
        const float sc = ((float)bs - 14.f) / 10.f;
        f16* d = img1->data() + (size_t)(bs - 2) * (w1_bytes / 2);
        for (int r = 0; r < 2 * C; ++r)
            for (int o = 0; o < se; ++o) {
                const float* w = sq_w + (size_t)o * 3 * C;
                d[(size_t)r * se + o] = (f16)(r < C ? w[r] + sc * w[C + r] : w[2 * C + (r - C)]);
            }
    }
    img2->assign(w2_bytes, 0);
    f16* h = (f16*)img2->data();
    for (int i = 0; i < se; ++i)
        for (int o = 0; o < 2 * C; ++o) h[((size_t)(i >> 2) * 2 * C + o) * 4 + (i & 3)] = (f16)ex_w[(size_t)o * se + i];
    float* bias = (float*)(img2->data() + (size_t)se * 2 * C * 2);
    std::copy(ex_b, ex_b + 2 * C, bias);
    std::copy(sq_b, sq_b + se, bias + 2 * C);
    *w1_bytes_out = w1_bytes;
    *w2_bytes_out = w2_bytes;
    return true;
}

// The same two FCs cut by 128-channel tile for conv_board_sx.h (a layer whose channels are split over kts workgroups): per tile kt
// the squeeze rows of its 128 channels (mean rows with the scaled-mean third folded in, once per board size; then the max rows),
// and the excite rows that produce its channels' gamma and beta, with their bias and the squeeze bias behind them.
static bool make_sx_images(int C, int se, int kts, int board, const float* sq_w, const float* sq_b, const float* ex_w, const float* ex_b,
                           std::vector<f16>* img1, std::vector<unsigned char>* img2, int* w1_bytes_out, int* w2_bytes_out) {
    if (se <= 0 || se % 4 || se > kSxSlots || kts < 2 || kts > 4 || C > kts * 128) return false;
    const int w1_bytes = round_up(256 * se * 2, 1024), w2_bytes = round_up(se * 256 * 2 + (256 + se) * 4, 1024);
    if (w1_bytes + w2_bytes > SxLds::stage_bytes) return false;
    img1->assign((size_t)kts * (board - 1) * (w1_bytes / 2), (f16)0.f);
    img2->assign((size_t)kts * w2_bytes, 0);
    for (int kt = 0; kt < kts; ++kt) {
        for (int bs = 2; bs <= board; ++bs) {
            const float sc = ((float)bs - 14.f) / 10.f;
            f16* d = img1->data() + ((size_t)kt * (board - 1) + (bs - 2)) * (w1_bytes / 2);
            for (int r = 0; r < 256; ++r) {
                const int c = kt * 128 + (r & 127);
                if (c >= C) continue;  // pad channels: x is 0 there, and their rows stay 0
                for (int o = 0; o < se; ++o) {
                    const float* w = sq_w + (size_t)o * 3 * C;
                    d[(size_t)r * se + o] = (f16)(r < 128 ? w[c] + sc * w[C + c] : w[2 * C + c]);
                }
            }
        }
        unsigned char* base = img2->data() + (size_t)kt * w2_bytes;
        f16* h = (f16*)base;
        float* bias = (float*)(base + (size_t)se * 256 * 2);
        for (int o = 0; o < 256; ++o) {
            const int c = kt * 128 + (o & 127);
            if (c >= C) continue;  // gamma = sigmoid(0), beta = 0 on x = 0
            const int row = o < 128 ? c : C + c;
            for (int i = 0; i < se; ++i) h[((size_t)(i >> 2) * 256 + o) * 4 + (i & 3)] = (f16)ex_w[(size_t)row * se + i];
            bias[o] = ex_b[row];
        }
        std::copy(sq_b, sq_b + se, bias + 256);
    }
    *w1_bytes_out = w1_bytes;
    *w2_bytes_out = w2_bytes;
    return true;
}

// Images of head_board_kernel (head_board.h): the stacked [policy | value] 1x1 head convolutions as one MFMA image
// (rows: policy channels rounded to a row tile of 16, then the value channels up to an even number of row tiles), the
// per-pixel weights (policy planes over the policy rows, ownership over the value rows) in the accumulator's channel
// order, the stacked bias.  Returns the kernel variant that fits, or nullptr (the separate head kernels run then).
struct HeadImages {
    std::vector<f16> img, img2;
    std::vector<float> bias;
    int PT = 0, VT = 0;
};
static HeadFn make_head_images(int C, int Cp, int Cv, int prob_ch, int board, const float* p_w, const float* p_b, const float* v_w,
                               const float* v_b, const float* prob_w, const float* own_w, HeadImages* out) {
    if (board * board > kHeadPix || prob_ch > 8) return nullptr;
    const int PT = round_up(Cp, 16), rows = round_up(PT + Cv, 32), VT = rows - PT, cs = round_up(C, 32), nch = cs / 32;
    HeadFn fn = nullptr;
    for (const auto& e : kHeadEntries)
        if (e.rt * 16 == rows && head_board_fits(rows, nch, e.depth)) { fn = e.fn; break; }
    if (!fn) return nullptr;
    // per-pixel weights in the accumulator's channel order: k-group kg of pair t holds stacked rows 32t + 4kg + s (s < 4)
    // and 32t + 16 + 4kg + (s - 4); row k < prob_ch = policy plane k over the policy rows, row prob_ch = ownership
    out->img2.assign((size_t)(rows / 32) * 4 * 16 * 8, (f16)0.f);
    for (int t = 0; t < rows / 32; ++t)
        for (int kg = 0; kg < 4; ++kg)
            for (int e = 0; e < 8; ++e) {
                const int ch = 32 * t + (e < 4 ? 4 * kg + e : 16 + 4 * kg + (e - 4));
                for (int k = 0; k < prob_ch; ++k)
                    if (ch < Cp) out->img2[(((size_t)t * 4 + kg) * 16 + k) * 8 + e] = (f16)prob_w[(size_t)k * Cp + ch];
                if (ch >= PT && ch - PT < Cv) out->img2[(((size_t)t * 4 + kg) * 16 + prob_ch) * 8 + e] = (f16)own_w[ch - PT];
            }
    out->img.assign((size_t)nch * 4 * rows * 8, (f16)0.f);
    out->bias.assign(rows, 0.f);
    for (int half = 0; half < 2; ++half) {
        const float* w = half ? v_w : p_w;
        const float* b = half ? v_b : p_b;
        const int cout = half ? Cv : Cp, r0 = half ? PT : 0;
        for (int ko = 0; ko < cout; ++ko) {
            out->bias[r0 + ko] = b[ko];
            for (int c = 0; c < C; ++c)
                out->img[(((size_t)(c / 32) * 4 + (c % 32) / 8) * rows + r0 + ko) * 8 + c % 8] = (f16)w[(size_t)ko * C + c];
        }
    }
    out->PT = PT;
    out->VT = VT;
    return fn;
}

// ------------------------------------------------------------------ launches shared by the engine and the test taps
// The parameters of the head kernels (head_tail_kernel, head_board_kernel): the device weights of the four FCs and of the two
// per-pixel convolutions, the dimensions, where the four outputs go (perm: device sample -> caller's slot, null = identity).
struct HeadWeights {
    FcDev p_inter, pass_fc, v_inter, v_misc;
    const float *prob_w, *prob_b, *own_w, *own_b;
};
static HeadParams head_params(const HeadWeights& w, int Cp, int Cv, int prob_ch, int act, int board, float* prob, float* pass, float* misc,
                              float* own, const int* perm) {
    HeadParams h{};
    h.p_inter = w.p_inter; h.pass_fc = w.pass_fc; h.v_inter = w.v_inter; h.v_misc = w.v_misc;
    h.prob_w = w.prob_w; h.prob_b = w.prob_b; h.own_w = w.own_w; h.own_b = w.own_b;
    h.Cp = Cp; h.cs_p = round_up(Cp, 32); h.Cv = Cv; h.cs_v = round_up(Cv, 32); h.prob_ch = prob_ch; h.act = act; h.board = board;
    h.prob = prob; h.pass = pass; h.misc = misc; h.own = own; h.perm = perm;
    return h;
}
// The SE unit as three kernels on the samples [n0, n0 + ns) (`px` pixels) of x, in place: se_pool -> se_fc -> se_scale.  Each
// launch goes through run(name, flops, bytes, launch): the engine's timed(), or a plain call (the test tap).
template <typename T, typename Run>
static int se_unit_launches(hipStream_t s, const BatchGeom& g, double px, T* x, const T* res, float* separt, float* gate, const FcDev& sq,
                            const FcDev& ex, int C, int cs, int act, int n0, int ns, Run&& run) {
    constexpr int EPP = ElemTraits<T>::kPieceElems;
    if (cs / EPP > 256) return fail("SE unit: more than 256*8 channels is not supported");
    const double fc = (double)sq.in * sq.out + (double)ex.in * ex.out;
    if (run("se_pool", 2.0 * px * C, sizeof(T) * px * C,
            [&] { hipLaunchKernelGGL(se_pool_kernel<T>, dim3(ns * kSeSplit), dim3(256), 0, s, (const T*)x, separt, g, cs, n0); }))
        return -1;
    const size_t smem = sizeof(float) * (3 * C + sq.out + kSeFcThreads);
    if (run("se_fc", 2.0 * ns * fc, 4.0 * ns * fc, [&] {
            hipLaunchKernelGGL(se_fc_kernel, dim3(ns), dim3(kSeFcThreads), smem, s, (const float*)separt, gate, g, C, cs, sq, ex, act, n0);
        }))
        return -1;
    const dim3 grid((g.slot_pix * (cs / EPP) + 256 * kScaleUnroll - 1) / (256 * kScaleUnroll), ns);
    return run("se_scale", 3.0 * px * C, sizeof(T) * px * C * 3,
               [&] { hipLaunchKernelGGL(se_scale_kernel<T>, grid, dim3(256), 0, s, (const T*)x, res, x, (const float*)gate, g, C, cs, act, n0); });
}
// The same unit as ONE launch (se_unit_kernel, small_ops.h: `parts` workgroups per sample, the three kernels as their phases,
// the same bits), same run() protocol; its row carries the flops and bytes of the three rows it replaces.  The result goes to
// `out`: x itself (in place) when parts == 1, else the residual's buffer -- never x, see the kernel.  Returns 1 when the form
// does not apply -- more than 256 pieces per pixel row, its LDS does not fit, or parts > 1 without such a buffer -- and the
// caller runs se_unit_launches.
template <typename T, typename Run>
static int se_unit_one_launch(hipStream_t s, const BatchGeom& g, double px, const T* x, const T* res, T* out, int parts, float* gate,
                              const FcDev& sq, const FcDev& ex, int C, int cs, int act, int n0, int ns, Run&& run) {
    constexpr int EPP = ElemTraits<T>::kPieceElems;
    const size_t smem = se_unit_lds(C, cs, sq.out, EPP);
    if (cs / EPP > 256 || smem > kMaxLds || parts < 1 || (parts > 1 && (out == x || out != res))) return 1;
    const double fc = (double)sq.in * sq.out + (double)ex.in * ex.out;
    return run("se_unit", 5.0 * px * C + 2.0 * ns * fc, sizeof(T) * px * C * 4 + 4.0 * ns * fc, [&] {
        hipLaunchKernelGGL(se_unit_kernel<T>, dim3(ns * parts), dim3(kSeFcThreads), smem, s, x, res, out, gate, g, C, cs, sq, ex, act, n0, parts);
    });
}

// ------------------------------------------------------------------ the input stage (small_ops.h), shared by the engine and its tap
// A packed batch whose device samples name their record and board symmetry (sayuri_hip_forward_packed_symm): `n_records`
// records in the caller's array, src[n] (null: sample i reads record i) and symm[n] in the caller's sample order.
struct SymmReq {
    int n_records = 0;
    const int* src = nullptr;
    const int* symm = nullptr;
};
// Packed records with `binary` bit planes for a network of `input_channels` planes on an NN grid of `board`: 0, or the refusal.
// A record holds at most kPackedMaxBinary bit planes -- the bit kernels' LDS copy and the record buffers are sized by it -- and
// 8 scalars behind them; a plane is 12 words of 32 cells.
static int packed_binary_check(int binary, int input_channels, int board) {
    if (binary > kPackedMaxBinary)
        return fail("packed planes: binary_planes = " + std::to_string(binary) + ": a record holds at most " + std::to_string(kPackedMaxBinary) +
                    " bit planes");
    if (binary <= 0 || binary > input_channels || input_channels - binary > kPackedScalars || board * board > kPackedWords * 32)
        return fail("packed planes: bad binary plane count for this network");
    return 0;
}
// A symmetry request's arguments, checked before anything is enqueued.  The record array is bounded by max_batch: the copy
// path moves it into the slot's record buffer, which holds that many.
static int check_symm_request(int n, int max_batch, const unsigned* packed, const SymmReq& sy) {
    if (!packed || !sy.symm) return fail("packed_symm: null argument");
    if (n <= 0 || n > max_batch) return fail("batch size out of range");
    if (sy.n_records <= 0 || sy.n_records > max_batch)
        return fail("packed_symm: n_records " + std::to_string(sy.n_records) + " out of range (1.." + std::to_string(max_batch) + ")");
    if (!sy.src && n > sy.n_records) return fail("packed_symm: the identity record map needs n <= n_records");
    for (int i = 0; i < n; ++i) {
        if (sy.symm[i] < 0 || sy.symm[i] > 7)
            return fail("packed_symm: symm[" + std::to_string(i) + "] = " + std::to_string(sy.symm[i]) + " is no board symmetry (0..7)");
        if (sy.src && (sy.src[i] < 0 || sy.src[i] >= sy.n_records))
            return fail("packed_symm: src[" + std::to_string(i) + "] = " + std::to_string(sy.src[i]) + " is outside the " +
                        std::to_string(sy.n_records) + " records");
    }
    return 0;
}
// Which kernel turns a batch's planes or records into the input convolution's image, and its launch.  fp32 planes: a sample
// that fits 64 KiB of LDS whole and whose planes are below 2^16 floats takes the flat kernel, one workgroup per sample; else
// the chunked one, kPackSplit workgroups per sample and `chunk` pixels per pass.  Records: kPackSplit workgroups per sample, or
// one when they are read in place across PCIe (a record then crosses once).  The values of `kernel` are what
// sayuri_hip_test_last_pack reports.
enum PackKernel { kPackChunked = 0, kPackFlat = 1, kPackBits = 2, kPackBitsSymm = 3 };
struct PackPlan {
    PackKernel kernel = kPackChunked;
    int split = kPackSplit;  // workgroups per sample
    int threads = kPackThreads;
    int chunk = 0;           // chunked: pixels per pass
    size_t lds = 0;          // dynamic LDS of the launch
    // passes a workgroup makes over its pixel range on a bs x bs sample (chunked); passes over a sample's planes (flat); else 1
    int passes(int bs, int cin, int board) const {
        if (kernel == kPackChunked) return ((bs * bs + kPackSplit - 1) / kPackSplit + chunk - 1) / chunk;
        if (kernel == kPackFlat) return (cin * board * board + kPackFlatThreads * kPackFlatLoads - 1) / (kPackFlatThreads * kPackFlatLoads);
        return 1;
    }
};
static PackPlan pack_plan(size_t elem, int cin, int cs, int board, bool records, bool symm, bool in_place) {
    PackPlan pl;
    if (records) {
        pl.kernel = symm ? kPackBitsSymm : kPackBits;
        pl.split = in_place ? 1 : kPackSplit;
        pl.threads = 256;
        return pl;
    }
    const int slot_pix = board * board;
    const size_t flat_lds = pack_input_flat_lds(slot_pix, cs, (int)elem);
    if (flat_lds <= 64 * 1024 && (size_t)cin * board * board < 65536) {
        pl.kernel = kPackFlat;
        pl.split = 1;
        pl.threads = kPackFlatThreads;
        pl.lds = flat_lds;
        return pl;
    }
    pl.chunk = pack_input_chunk(slot_pix, cs, (int)elem);
    pl.lds = (size_t)pl.chunk * (cs * elem + 16);
    return pl;
}
// The launch of `pl` over the samples [n0, n0 + ns): planes, or records of nbin bit planes (with the symmetry kernel the record
// map and the symmetries, in the caller's order) -> dst.  perm: device sample -> caller's slot.
struct PackSource {
    const float* planes = nullptr;
    const unsigned* records = nullptr;
    int nbin = 0;
    const int* src_map = nullptr;
    const int* symm_map = nullptr;
};
template <typename T>
static void pack_launch(const PackPlan& pl, hipStream_t s, const PackSource& in, T* dst, const BatchGeom& g, int cin, int cs, int board,
                        const int* perm, int n0, int ns) {
    const int words = in.nbin * kPackedWords + kPackedScalars;
    switch (pl.kernel) {
    case kPackBitsSymm:
        hipLaunchKernelGGL(pack_bits_symm_kernel<T>, dim3(ns * pl.split), dim3(pl.threads), 0, s, in.records, words, in.nbin, dst, g, cin, cs, perm,
                           in.src_map, in.symm_map, n0, pl.split);
        break;
    case kPackBits:
        hipLaunchKernelGGL(pack_bits_kernel<T>, dim3(ns * pl.split), dim3(pl.threads), 0, s, in.records, words, in.nbin, dst, g, cin, cs, perm, n0,
                           pl.split);
        break;
    case kPackFlat:
        hipLaunchKernelGGL(pack_input_flat_kernel<T>, dim3(ns), dim3(pl.threads), pl.lds, s, in.planes, dst, g, cin, cs, board, perm, n0);
        break;
    case kPackChunked:
        hipLaunchKernelGGL(pack_input_kernel<T>, dim3(ns * pl.split), dim3(pl.threads), pl.lds, s, in.planes, dst, g, cin, cs, board, perm, pl.chunk,
                           n0);
        break;
    }
}

// the persistent tower kernels (conv_tower.h) out of the embedded code object: [0] 256-channel tile, [1] 128-channel tile
}  // namespace sayuri
extern "C" const unsigned char sayuri_tower_hsaco[];
extern "C" const unsigned long long sayuri_tower_hsaco_size;
namespace sayuri {
static int load_tower_module(hipModule_t* mod, hipFunction_t fn[2]) {
    // an EMPTY blob: the build went on without the persistent kernel because tower_seam.py did not recognise the compiler's
    // assembly (sayuri_amd/_build.py tower_blob_from_asm); the caller reports the fallback and launches per layer
    if (sayuri_tower_hsaco_size == 0) return fail("this build carries no persistent tower kernel: tower_seam.py rejected the compiler's assembly at build time");
    HIP_OK(hipModuleLoadData(mod, sayuri_tower_hsaco));
    HIP_OK(hipModuleGetFunction(&fn[0], *mod, "_ZN6sayuri17conv_tower_kernelILi4EEEvPKNS_10TowerLayerE"));
    HIP_OK(hipModuleGetFunction(&fn[1], *mod, "_ZN6sayuri17conv_tower_kernelILi2EEEvPKNS_10TowerLayerE"));
    return 0;
}

}  // namespace sayuri
