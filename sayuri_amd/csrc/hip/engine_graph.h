// engine_graph.h -- EngineBase / Engine<T>: the per-GPU forward graph (weights, batch i/o on two tickets, the launches of one
// forward, the persistent tower run, chains) behind the C-ABI of engine.hip.  Counterpart of the reference's
// CudaForwardPipe::NNGraph (src/neural/cuda/cuda_forward_pipe.cc:133-1090).
#pragma once
#include "engine_plan.h"

namespace sayuri {

// The key of what an engine computes once per batch geometry (routes, plans, tile choices): what the entry is about (a, b, c) and
// the sample range [n0, n0 + ns) it was computed for (0, 0: the whole batch).  Nothing is packed: no value aliases another entry.
struct PlanKey {
    int a = 0, b = 0, c = 0, n0 = 0, ns = 0;
    bool operator<(const PlanKey& o) const { return std::tie(a, b, c, n0, ns) < std::tie(o.a, o.b, o.c, o.n0, o.ns); }
};
template <typename V, typename Make> static const V& cached(std::map<PlanKey, V>& m, const PlanKey& key, Make&& make) {
    auto it = m.find(key);
    if (it == m.end()) it = m.emplace(key, make()).first;
    return it->second;
}

class EngineBase {
public:
    virtual ~EngineBase() {}
    virtual int load_tensor(int layer, int kind, const float* host, size_t n) = 0;
    // `packed` != null: the inputs are packed records (packed_planes.h) with `binary` bit planes, `planes` is ignored
    // `sy` != null (packed only): the records are expanded under a per-sample record map and symmetry (pack_bits_symm_kernel)
    virtual int upload(int n, const float* planes, const int* board_sizes, const unsigned* packed = nullptr, int binary = 0,
                       const SymmReq* sy = nullptr) = 0;
    virtual int run() = 0;
    virtual int sync() = 0;
    virtual int download(float* prob, float* pass, float* misc, float* own) = 0;
    virtual int time_runs(int iters, float* ms) = 0;
    virtual int profile_run(sayuri_hip_kernel_stat* rows, int cap) = 0;
    virtual int submit(int n, const float* planes, const int* bsz, float* prob, float* pass, float* misc, float* own,
                       int* ticket, const unsigned* packed = nullptr, int binary = 0, const SymmReq* sy = nullptr) = 0;
    virtual int wait(int ticket) = 0;
    virtual int query(int ticket) = 0;
    virtual int mark_kernel(const char* name) = 0;
    virtual int timed_stat(sayuri_hip_kernel_stat* row) = 0;
    virtual size_t device_bytes() const = 0;
    virtual int last_chains() const = 0;
    virtual int last_pw_launches() const = 0;  // conv_pw.h launches of the last forward (0: none -- SAYURI_PW=0, or no such layer)
    virtual int last_dw_launches() const = 0;  // conv_dw.h launches of the last forward (0: none -- SAYURI_DW=0, or no depthwise layer)
    virtual int last_split_ring() const = 0;  // the deepest weight ring of the last forward's split convolutions (0: none ran)
    virtual int tower_state() const = 0;  // 1: the persistent tower kernel is loaded, 0: one launch per layer (fallback)
    virtual int latency_state() const = 0;  // 1: a latency context (conv_split.h), 0: the default engine
    virtual int debug_read(int buf, void* host, size_t bytes) = 0;  // debugging tap: activation buffer `buf` of ticket 0
    // live weight reload (sayuri_hip_reload_*): a second weight set is staged beside the live one and swapped in between two forwards
    virtual int reload_begin(const sayuri_hip_netdesc& d) = 0;
    virtual int reload_prepare() = 0;
    virtual int reload_commit() = 0;
    virtual int reload_abort() = 0;
    virtual int weights_generation() const = 0;
};

template <typename T> class Engine : public EngineBase {
public:
    struct TileTabs { int* src = nullptr; int2* pix = nullptr; bool fresh = false; };
    struct BoardTabs { int* src = nullptr; int2* pix = nullptr; int* cols = nullptr; int npos_built = 0; int ntiles_built = 0; bool fresh = false; };
    Engine(int device, const sayuri_hip_netdesc& d, int max_batch, int board, const EngineFlags& flags)
        : flags_(flags), device_(device), desc_(d), max_batch_(max_batch), board_(board) {
        blocks_.assign(d.blocks, d.blocks + d.residual_blocks);
        desc_.blocks = blocks_.data();
        live_ = std::make_unique<WeightSet>();
    }
    ~Engine() override { release(); }

    int init() {
        HIP_OK(hipSetDevice(device_));
        // The tickets' compute streams: one shared stream to begin with; the rule below gives ticket 1 a stream of its own.
        HIP_OK(hipStreamCreateWithFlags(&compute_[0], hipStreamNonBlocking));
        compute_[1] = compute_[0];
        HIP_OK(hipStreamCreateWithFlags(&h2d_stream_, hipStreamNonBlocking));
        HIP_OK(hipStreamCreateWithFlags(&d2h_stream_, hipStreamNonBlocking));
        for (int t = 0; t < 2; ++t) {
            HIP_OK(hipEventCreateWithFlags(&h2d_done_[t], hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&fwd_done_[t], hipEventDisableTiming));
        }
        HIP_OK(hipEventCreate(&ev0_));
        HIP_OK(hipEventCreate(&ev1_));
        enable_big_lds<T>();
        if (sizeof(T) == 2) enable_big_lds_glds();
        if (sizeof(T) == 2 && flags_.tower && tower_load()) {
            // the persistent launch is an optimisation: without its code object the per-layer launches (SAYURI_TOWER=0) run
            // the same kernels.  Say so once, loudly, and go on.
            std::fprintf(stderr, "[sayuri_hip] persistent tower kernel not loaded (%s): falling back to one launch per layer\n",
                         sayuri_hip_last_error());
            if (tower_mod_) (void)hipModuleUnload(tower_mod_);
            tower_mod_ = nullptr;
            tower_fn_[0] = tower_fn_[1] = nullptr;
        }
        // One stream per ticket (everything of a ticket in order on its own stream, no event between streams) whenever the
        // persistent kernel is loaded -- for every network, also one the launch does not cover (384 / 192 channels: the code
        // object is loaded and the layers are still launched one by one).  History of the rule: round 1 measured two tickets'
        // per-layer launches side by side as slower (48.0 k vs 54.0 k evals/s, the 482-workgroup kernel on the 256-channel
        // network evicting each other's L2 lines) and kept one compute stream; round 5 re-measured on the kernels of today --
        // 40b x 384 through submit / wait, two tickets in flight: a stream per ticket 26.3 k evals/s, one compute stream 23.7 k
        // (a layer is 450 workgroups, two rounds of the CUs, and the other ticket's launches fill the second; 200 batches
        // bit-identical to the solo result, profiles/r05_config5_pump_streams.json, tools/gpu/concurrent_ctx_dbg.py).  Without the code object
        // (SAYURI_TOWER=0, or a build whose seam was rejected) the older three-stream arrangement stays.
        if (describe_layers(*live_)) return -1;
        // A latency context has no persistent launch to keep small copies waiting, and a round trip of one position is what it
        // is for: a stream per ticket too, no event between streams.
        inorder_ = tower_fn_[0] != nullptr || flags_.latency;
        if (inorder_) HIP_OK(hipStreamCreateWithFlags(&compute_[1], hipStreamNonBlocking));
        return 0;
    }
    // every 3x3 convolution of the residual tower has 128 or 256 (padded) output channels and there is at least one
    bool tower_covers_net() const {
        int n3 = 0;
        for (const auto& kv : live_->convs) {
            const ConvLayerDev& L = kv.second;
            if (L.k != 3 || L.depthwise || kv.first == SAYURI_L_INPUT_CONV) continue;
            const int cs = round_up(L.cout, 32);
            if (cs != 256 && cs != 128) return false;
            ++n3;
        }
        const int c0 = round_up(desc_.residual_channels, 32);
        return n3 > 0 && (c0 == 256 || c0 == 128);
    }

    // -------------------------------------------------------------- chains (see forward())
    static constexpr int kMaxChains = 4;
    hipStream_t chain_stream_[kMaxChains] = {};
    hipEvent_t chain_fork_ = nullptr, chain_join_[kMaxChains] = {};
    int last_chains_ = 1;
    int last_split_ring_ = 0;
    int last_pw_launches_ = 0;
    int last_dw_launches_ = 0;
    bool dw_refusal_said_ = false;  // the one-time note of a forced SAYURI_DW_STRIPS that dw_plan refused
    int chain_setup(int G) {
        if (!chain_fork_) HIP_OK(hipEventCreateWithFlags(&chain_fork_, hipEventDisableTiming));
        for (int g = 0; g < G; ++g) {
            if (!chain_stream_[g]) HIP_OK(hipStreamCreateWithFlags(&chain_stream_[g], hipStreamNonBlocking));
            if (!chain_join_[g]) HIP_OK(hipEventCreateWithFlags(&chain_join_[g], hipEventDisableTiming));
        }
        return 0;
    }
    // How many chains the current batch is run as.  A layer of a network the persistent launch does not cover is one launch of
    // (tiles x channel tiles) workgroups of equal cost; at 450 of them (configs[4]: 150 tiles x three 128-channel tiles) the 256 CUs
    // run two rounds, the second 76 % full, whatever the item size.  The boards of a batch are independent: cut into G groups of
    // tiles, each a chain of per-layer launches on a stream of its own, a group's next layer starts on the CUs another group's
    // round leaves free -- the cross-layer pipelining of a persistent (layer, tile, channel tile) run, done by the dispatcher
    // instead of by dependency counters.  Measured from outside the engine (tools/gpu/c5_streams.py, G contexts): 24.4 k evals/s
    // as one chain, 25.8 / 25.9 / 25.6 k as 2 / 3 / 4, 21.4 k as 6.
    int chains_for_batch() {
        // The chains share the forward's activation buffers: a tile is whole samples, every layer of a network that qualifies has
        // ONE channel stride, and the packed input keeps a buffer of its own (forward_graph), so the chains' rows are disjoint
        // bytes in every buffer.  (The first version recycled the packed input's buffer, whose rows have another stride: a chain
        // that ran ahead overwrote a later chain's input -- a few dozen samples per batch off in two runs of three.)
        if (sizeof(T) != 2 || flags_.chains == 1 || profiling_ || light_ || !live_->head_img || !flags_.heads_fused) return 1;
        if (desc_.policy_head_type != 0 || tower_covers_net()) return 1;
        for (const auto& b : blocks_)
            if (b.type != SAYURI_BLOCK_RESIDUAL) return 1;  // every layer of the graph must be a board convolution or a per-sample kernel
        const ConvLayerDev& L = cv(SAYURI_L_BLOCK(0, SAYURI_S_CONV1));
        // (a network whose SE units could run inside the convolution keeps one chain: conv_se launches over the whole batch)
        // (board_se_entry, not pick_board_se: the answer is about the network, before any batch has a board plan whose LDS could be asked)
        if (board_se_entry(L.ko_pad))
            for (const auto& b : blocks_)
                if (b.apply_se) return 1;
        const ConvRoute& r = route(L);
        if (!r.board || !board_plan_.ok) return 1;
        const int wgs = board_plan_.ntiles * r.tiles;
        if (wgs <= kNumCU) return 1;  // one round already
        int G = flags_.chains > 1 ? flags_.chains : std::min(kMaxChains, std::max(2, (wgs + 159) / 160));
        G = std::min(G, board_plan_.ntiles / 8);
        return std::max(G, 1);
    }

    // -------------------------------------------------------------- weights
    int load_tensor(int layer, int kind, const float* host, size_t n) override {
        std::lock_guard<std::mutex> rl(reload_mu_);
        if (staged_ && staged_->built) return fail("load_tensor: the open reload is prepared already (commit or abort it)");
        if (!staged_ && finalized_) return fail("load_tensor after the first forward");
        WeightSet& ws = staged_ ? *staged_ : *live_;  // an open reload takes the tensors: the live set is never written in place
        auto& convs = ws.convs;
        auto& fcs = ws.fcs;
        auto ci = convs.find(layer);
        if (ci != convs.end()) {
            ConvLayerDev& L = ci->second;
            const size_t expect = kind == SAYURI_T_WEIGHTS
                                      ? (size_t)(L.depthwise ? 1 : L.cin) * L.cout * L.k * L.k
                                      : (size_t)L.cout;
            if (n != expect) return fail("conv tensor size mismatch for layer " + std::to_string(layer));
            (kind == SAYURI_T_WEIGHTS ? L.hw : L.hb).assign(host, host + n);
            return 0;
        }
        auto fi = fcs.find(layer);
        if (fi != fcs.end()) {
            FcLayerDev& L = fi->second;
            const size_t expect = kind == SAYURI_T_WEIGHTS ? (size_t)L.in * L.out : (size_t)L.out;
            if (n != expect) return fail("fc tensor size mismatch for layer " + std::to_string(layer));
            (kind == SAYURI_T_WEIGHTS ? L.hw : L.hb).assign(host, host + n);
            return 0;
        }
        return fail("unknown layer id " + std::to_string(layer));
    }

    // -------------------------------------------------------------- batch i/o
    // asynchronous: H2D, graph, D2H enqueued on the stream, an event marks the end
    int submit(int n, const float* planes, const int* board_sizes, float* prob, float* pass, float* misc, float* own,
               int* ticket, const unsigned* packed = nullptr, int binary = 0, const SymmReq* sy = nullptr) override {
        if (sy && check_symm(n, packed, *sy)) return -1;  // (before the ticket is taken: a refused call launches nothing)
        if (n_retired_.load(std::memory_order_relaxed)) retire_poll();  // (before mu_ is taken: the frees happen outside it)
        std::lock_guard<std::mutex> lk(mu_);  // (a reload's commit happens between two submits, never inside one)
        // The planes of batch k+1 cross PCIe while batch k computes, and the results of batch k while batch k+1 computes; each
        // of the two tickets owns its own device input / geometry / output buffers (and, by default, its own stream: below).
        const int t = next_ticket_;
        next_ticket_ ^= 1;
        HIP_OK(hipSetDevice(device_));
        if (finalize()) return -1;
        IoSlot& io = io_[t];
        const hipStream_t cs = compute_[t];
        // With the tower code object loaded (init()): everything of a ticket on the ticket's own stream, in
        // order -- no event between streams at all.  Each record / wait is a marker the runtime's signal thread handles; the
        // seven per batch of the three-stream arrangement kept that thread at a full host core during self-play (one of
        // eight busy; profiles/r04_host_profile.txt), for the same evals/s.  The other ticket's stream overlaps its copies
        // with this one's kernels as before; a ticket's slot is free when its stream gets to the next use.
        const bool inorder = inorder_;
        // One exception: fp32 planes (62 KB per sample, 16 MB per batch).  On the ticket's own stream, behind kernels, the runtime
        // moves them with a copy KERNEL, which cannot run beside the other ticket's persistent launch: the upload waited for that
        // launch to end (72.1 -> 65.0 k evals/s through submit / wait; packed planes are 0.5 MB and do not show it).  They keep the
        // upload stream and one event; the slot is free for them when the ticket's last completion event has fired, which the
        // caller has normally seen already.
        const bool big_upload = inorder && packed == nullptr;
        hipStream_t up = inorder && !big_upload ? cs : h2d_stream_, down = inorder ? cs : d2h_stream_;
        if (!inorder) HIP_OK(hipStreamWaitEvent(h2d_stream_, fwd_done_[t], 0));  // the forward that last read this slot's inputs
        else if (big_upload && tick_ev_[t]) HIP_OK(hipStreamWaitEvent(h2d_stream_, tick_ev_[t], 0));
        if (enqueue_inputs(t, n, planes, board_sizes, up, packed, binary, /*in_place=*/true, sy)) return -1;
        if (!inorder || big_upload) {
            HIP_OK(hipEventRecord(h2d_done_[t], h2d_stream_));
            HIP_OK(hipStreamWaitEvent(cs, h2d_done_[t], 0));
            if (!inorder && tick_ev_[t]) HIP_OK(hipStreamWaitEvent(cs, tick_ev_[t], 0));  // the download that last read this slot's outputs
        }
        have_batch_ = true;
        if (flags_.fwdstat) {  // SAYURI_HIP_FWDSTAT (measuring aid): device time of every submitted forward
            for (int k = 0; k < 2; ++k)
                if (!fs_ev_[t][k]) HIP_OK(hipEventCreate(&fs_ev_[t][k]));
            HIP_OK(hipEventRecord(fs_ev_[t][0], cs));
        }
        const int uploads_before = table_uploads_;
        // The persistent tower launch holds every CU (all registers, all LDS) for the whole forward.  A copy the runtime
        // does with a blit KERNEL (everything below 16 KB: pass, misc, the three geometry arrays, the tower table) can
        // therefore not run beside the OTHER ticket's tower launch: with two batches in flight a finished batch's small
        // downloads -- and with them its completion event -- waited for the next batch's 3.5 ms launch to end, the next
        // batch's geometry uploads likewise (driver line of round 3: 64.4 k evals/s in self-play against 70.5 k resident).
        // So nothing small is copied any more: the heads kernel stores pass / misc straight into the caller's pinned
        // buffers (20 KB of posted PCIe writes), a uniform batch uses geometry arrays that are resident (enqueue_inputs),
        // and the tower table does not depend on the batch size (tower_append).  The two large outputs keep their DMA copies.
        float* zc_pass = zc_device_pointer(pass);
        float* zc_misc = zc_pass ? zc_device_pointer(misc) : nullptr;
        if (!zc_misc) zc_pass = nullptr;  // both or neither: the heads kernel takes one path
        const bool small_direct = zc_pass != nullptr;
        if (forward(t, zc_pass, zc_misc)) return -1;
        if (flags_.fwdstat) {
            HIP_OK(hipEventRecord(fs_ev_[t][1], cs));
            fs_pending_[t] = true;
            fs_n_[t] = n;
            fs_uploads_ += table_uploads_ - uploads_before;
        }
        if (!inorder) {
            HIP_OK(hipEventRecord(fwd_done_[t], cs));
            HIP_OK(hipStreamWaitEvent(d2h_stream_, fwd_done_[t], 0));
        }
        const size_t B2 = (size_t)board_ * board_;
        HIP_OK(hipMemcpyAsync(prob, io.prob, sizeof(float) * n * desc_.probabilities_channels * B2, hipMemcpyDeviceToHost, down));
        if (!small_direct) {
            HIP_OK(hipMemcpyAsync(pass, io.pass, sizeof(float) * n * desc_.pass_probability_outputs, hipMemcpyDeviceToHost, down));
            HIP_OK(hipMemcpyAsync(misc, io.misc, sizeof(float) * n * desc_.value_misc_outputs, hipMemcpyDeviceToHost, down));
        }
        HIP_OK(hipMemcpyAsync(own, io.own, sizeof(float) * n * B2, hipMemcpyDeviceToHost, down));
        if (!tick_ev_[t]) HIP_OK(hipEventCreateWithFlags(&tick_ev_[t], hipEventDisableTiming));
        HIP_OK(hipEventRecord(tick_ev_[t], down));
        if (flags_.fwdstat) {
            if (!fs_ev_[t][2]) HIP_OK(hipEventCreate(&fs_ev_[t][2]));
            HIP_OK(hipEventRecord(fs_ev_[t][2], down));
        }
        *ticket = t;
        return 0;
    }
    int wait(int ticket) override {
        if (ticket < 0 || ticket > 1 || !tick_ev_[ticket]) return fail("wait: bad ticket");
        HIP_OK(hipSetDevice(device_));
        HIP_OK(hipEventSynchronize(tick_ev_[ticket]));
        if (n_retired_.load(std::memory_order_relaxed)) retire_poll();  // a replaced weight set whose last forwards have finished is given back
        if (sx_check(ticket)) return -1;
        if (flags_.fwdstat && fs_pending_[ticket]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, fs_ev_[ticket][0], fs_ev_[ticket][1]) == hipSuccess) {
                const int b = fs_n_[ticket] >= max_batch_ ? 2 : (fs_n_[ticket] * 2 > max_batch_ ? 1 : 0);
                fs_ms_[b] += ms;
                fs_cnt_[b] += 1;
            }
            if (fs_ev_[ticket][2] && hipEventElapsedTime(&ms, fs_ev_[ticket][1], fs_ev_[ticket][2]) == hipSuccess) {
                fs_d2h_ms_ += ms;
                fs_d2h_max_ = std::max(fs_d2h_max_, (double)ms);
                fs_d2h_slow_ += ms > 1.0f;
            }
            fs_pending_[ticket] = false;
        }
        return 0;
    }
    int query(int ticket) override {
        if (ticket < 0 || ticket > 1 || !tick_ev_[ticket]) return fail("query: bad ticket");
        const hipError_t e = hipEventQuery(tick_ev_[ticket]);
        if (e == hipSuccess) return 1;
        if (e == hipErrorNotReady) return 0;
        return fail(std::string("hipEventQuery: ") + hipGetErrorString(e));
    }

    int upload(int n, const float* planes, const int* board_sizes, const unsigned* packed = nullptr, int binary = 0,
               const SymmReq* sy = nullptr) override {
        if (sy && check_symm(n, packed, *sy)) return -1;
        std::lock_guard<std::mutex> lk(mu_);
        HIP_OK(hipSetDevice(device_));
        if (finalize()) return -1;
        HIP_OK(hipStreamSynchronize(h2d_stream_));
        HIP_OK(hipStreamSynchronize(d2h_stream_));
        for (hipStream_t cs : compute_)
            if (cs) HIP_OK(hipStreamSynchronize(cs));
        if (enqueue_inputs(0, n, planes, board_sizes, compute_[0], packed, binary, false, sy)) return -1;
        HIP_OK(hipStreamSynchronize(compute_[0]));
        have_batch_ = true;
        return 0;
    }

    // The heads kernel stores pass / misc straight into the caller's buffers when the device can address them: page-locked
    // memory that is MAPPED (sayuri_hip_host_alloc, hipHostMalloc, hipHostRegister with the mapped flag).  Anything else --
    // pinned but unmapped, pageable, another allocator's -- would fault the GPU inside the kernel with no error returned, so a
    // pointer is asked about once (hipHostGetDevicePointer) and the answer kept; a buffer that is not device-addressable gets
    // its results through the device-side copies and hipMemcpyAsync as before.
    float* zc_device_pointer(float* host) {
        if (!host) return nullptr;
        // (an address may be handed out again after sayuri_hip_host_free, to memory of another kind: answers do not outlive a free)
        const unsigned gen = g_host_free_gen.load(std::memory_order_acquire);
        if (gen != zc_gen_) {
            zc_known_.clear();
            zc_gen_ = gen;
        }
        auto it = zc_known_.find(host);
        if (it != zc_known_.end()) return it->second;
        void* dp = nullptr;
        float* ans = nullptr;
        if (hipHostGetDevicePointer(&dp, host, 0) == hipSuccess && dp) ans = (float*)dp;
        else (void)hipGetLastError();  // not an error of this engine: the fallback path is taken
        if (zc_known_.size() >= 64) zc_known_.clear();
        zc_known_[host] = ans;
        return ans;
    }
    std::map<float*, float*> zc_known_;
    unsigned zc_gen_ = 0;

    // resident geometry arrays of a uniform batch of `bs` x `bs` boards (valid for every n <= max_batch)
    struct IdentGeom { int *off = nullptr, *bsz = nullptr, *perm = nullptr; };
    const IdentGeom* ident_geom(int bs) {
        auto it = ident_.find(bs);
        if (it != ident_.end()) return &it->second;
        IdentGeom g;
        std::vector<int> off(max_batch_ + 1), bz(max_batch_, bs), pm(max_batch_);
        for (int i = 0; i <= max_batch_; ++i) off[i] = i * bs * bs;
        for (int i = 0; i < max_batch_; ++i) pm[i] = i;
        if (dev_upload(&g.off, off) || dev_upload(&g.bsz, bz) || dev_upload(&g.perm, pm)) return nullptr;
        return &ident_.emplace(bs, g).first->second;
    }
    std::map<int, IdentGeom> ident_;

    int check_symm(int n, const unsigned* packed, const SymmReq& sy) { return check_symm_request(n, max_batch_, packed, sy); }

    // geometry + planes of ticket t to the device (no sync): the planes or packed records H2D on `copy_stream`, the geometry
    // arrays of a mixed batch from a 2-deep pinned ring (a second batch can be enqueued while the first is still in flight) on
    // the ticket's compute stream.
    int enqueue_inputs(int t, int n, const float* planes, const int* board_sizes, hipStream_t copy_stream, const unsigned* packed = nullptr,
                       int binary = 0, bool in_place = false, const SymmReq* sy = nullptr) {
        HIP_OK(hipSetDevice(device_));
        if (n <= 0 || n > max_batch_) return fail("batch size out of range");
        if (packed && packed_binary_check(binary, desc_.input_channels, board_)) return -1;
        if (finalize()) return -1;
        prev_bsz_.swap(geom_.bsz);
        geom_.n = n;
        geom_.bsz.resize(n);
        geom_.off.resize(n + 1);
        geom_.off[0] = 0;
        // Device order = the batch's samples sorted by board size (largest first, stable): samples of one size become
        // neighbours, so the one-workgroup-per-board convolution packs them into full tiles (two 13x13 or four 9x9 boards
        // per tile) whatever order the queue collected them in.  perm[i] = the caller's slot of device sample i; only
        // pack_input (reads the planes) and head_tail (writes the outputs) see the caller's order.
        perm_.resize(n);
        bool mixed = false;
        for (int i = 0; i < n; ++i) {
            const int bs = board_sizes ? board_sizes[i] : board_;
            if (bs < 2 || bs > board_) return fail("sample board size out of range");
            perm_[i] = i;
            mixed |= board_sizes && bs != board_sizes[0];
        }
        if (mixed) std::stable_sort(perm_.begin(), perm_.end(), [&](int a, int b) { return board_sizes[a] > board_sizes[b]; });
        for (int i = 0; i < n; ++i) {
            geom_.bsz[i] = board_sizes ? board_sizes[perm_[i]] : board_;
            geom_.off[i + 1] = geom_.off[i] + geom_.bsz[i] * geom_.bsz[i];
        }
        geom_.total = geom_.off[n];
        if (geom_.bsz != prev_bsz_) forget_geometry();
        IoSlot& io = io_[t];
        const bool uniform = !mixed;
        // One sample per tile and one board size: the tables of a LONGER batch of the same size serve a shorter one (tile i
        // depends on sample i alone), so a queue that alternates between 256 and 250 positions keeps its tables.
        const bool one_per_tile = uniform && 2 * geom_.bsz[0] * geom_.bsz[0] > kBoardPT;
        const bool prefix = one_per_tile && io.tabs_single && io.tabs_bsz.size() >= (size_t)n &&
                            io.tabs_bsz[0] == geom_.bsz[0];
        if (!prefix && io.tabs_bsz != geom_.bsz) {  // this slot's tables were built for another geometry
            for (auto& kv : io.tabs) kv.second.fresh = false;
            io.board.fresh = false;
            io.tabs_bsz = geom_.bsz;
            io.tabs_single = one_per_tile;
        }
        // the tables of the across-sample tiles (conv_glds.h) know the pixel total: they serve exactly the batch size they were
        // built for (the board tables above serve every prefix)
        if (io.tabs_n != n) {
            for (auto& kv : io.tabs) kv.second.fresh = false;
            io.tabs_n = n;
        }
        // Geometry arrays on the device.  A uniform batch (the self-play queue: every position on the NN board) uses arrays
        // that are resident -- off[i] = i * bs^2, bsz[i] = bs, perm[i] = i hold for every n -- so nothing is copied.  A mixed
        // batch stages its arrays in a pinned ring and a one-workgroup kernel ON THE FORWARD'S OWN STREAM moves them: a
        // copy of a few KB is a blit kernel to the runtime, and on the copy stream it would wait for the other ticket's
        // persistent tower launch to give up a CU (see submit()).
        if (uniform) {
            const IdentGeom* id = ident_geom(geom_.bsz[0]);
            if (!id) return -1;
            io.g_off = id->off; io.g_bsz = id->bsz; io.g_perm = id->perm;
        } else {
            io.g_off = io.off; io.g_bsz = io.bsz; io.g_perm = io.perm;
            int* hg = h_geom_ + (size_t)geom_slot_ * (3 * max_batch_ + 1);
            geom_slot_ ^= 1;
            std::memcpy(hg, geom_.off.data(), sizeof(int) * (n + 1));
            std::memcpy(hg + max_batch_ + 1, geom_.bsz.data(), sizeof(int) * n);
            std::memcpy(hg + 2 * max_batch_ + 1, perm_.data(), sizeof(int) * n);
            hipLaunchKernelGGL(geom_stage_kernel, dim3(1), dim3(256), 0, compute_[t], (const int*)hg, max_batch_, n, io.off, io.bsz, io.perm);
            HIP_OK(hipGetLastError());
        }
        io.packed_binary = packed ? binary : 0;
        io.symm_on = packed && sy;
        if (io.symm_on) {
            // The record map and the symmetries (caller's order, a few hundred bytes): staged in a pinned ring like the geometry
            // arrays and moved by a one-workgroup kernel on the forward's own stream, for the reason given there.  Ring and
            // device arrays exist from the first such batch on: a ctx that never sees one holds what it always held.
            if (!h_symm_) HIP_OK(hipHostMalloc((void**)&h_symm_, sizeof(int) * 2 * 2 * max_batch_, hipHostMallocDefault));
            // (each pointer on its own: a second allocation that failed is tried again by the next batch.  Like every failure
            // inside enqueue_inputs this one leaves submit()'s ticket taken and nothing enqueued on it.)
            if (!io.sy_src && dev_alloc(&io.sy_src, max_batch_)) return -1;
            if (!io.sy_symm && dev_alloc(&io.sy_symm, max_batch_)) return -1;
            int* hs = h_symm_ + (size_t)symm_slot_ * 2 * max_batch_;
            symm_slot_ ^= 1;
            for (int i = 0; i < n; ++i) {
                hs[i] = sy->src ? sy->src[i] : i;
                hs[max_batch_ + i] = sy->symm[i];
            }
            hipLaunchKernelGGL(symm_stage_kernel, dim3(1), dim3(256), 0, compute_[t], (const int*)hs, max_batch_, n, io.sy_src, io.sy_symm);
            HIP_OK(hipGetLastError());
        }
        if (packed) {
            const size_t words = (size_t)binary * kPackedWords + kPackedScalars;
            const int nrec = sy ? sy->n_records : n;
            // Packed records in device-addressable host memory (sayuri_hip_host_alloc: the pump's buffers) are not copied at all:
            // pack_bits_kernel reads the 1.8 KB per sample across PCIe itself.  The copy was 14 us of DMA -- but the copy engine
            // takes its packets in the order they were submitted, and the OTHER ticket's two downloads, submitted earlier and
            // waiting for that ticket's heads kernel, were ahead of it: batch k+1's upload, and with it pack_bits and the tower
            // launch, started only after batch k's results had gone out (135 us between two tower launches against 54 us for
            // one forward after another on one stream; tools/pump_gaps.py, profiles/r05_pump_gaps.txt).  The caller keeps the
            // records untouched until wait(), as it must for the asynchronous copy.
            io.packed_src = nullptr;
            if (in_place) io.packed_src = (const unsigned*)zc_device_pointer((float*)const_cast<unsigned*>(packed));
            if (io.packed_src) return 0;
            if (!io.packed && dev_alloc(&io.packed, (size_t)max_batch_ * kPackedRecordWords)) return -1;
            HIP_OK(hipMemcpyAsync(io.packed, packed, sizeof(unsigned) * nrec * words, hipMemcpyHostToDevice, copy_stream));
            return 0;
        }
        HIP_OK(hipMemcpyAsync(io.planes, planes, sizeof(float) * (size_t)n * desc_.input_channels * board_ * board_,
                              hipMemcpyHostToDevice, copy_stream));
        return 0;
    }

    int run() override {
        std::lock_guard<std::mutex> lk(mu_);
        if (!have_batch_) return fail("run before upload");
        HIP_OK(hipSetDevice(device_));
        return forward(0);
    }

    // run() / sync() / download(), time_runs() and profile_run() work on ticket 0, the slot upload() fills
    int sync() override {
        HIP_OK(hipSetDevice(device_));
        HIP_OK(hipStreamSynchronize(compute_[0]));
        return sx_check(0);
    }

    int download(float* prob, float* pass, float* misc, float* own) override {
        HIP_OK(hipSetDevice(device_));
        const size_t n = geom_.n, B2 = (size_t)board_ * board_;
        const IoSlot& io = io_[0];
        const hipStream_t s = compute_[0];
        if (prob) HIP_OK(hipMemcpyAsync(prob, io.prob, sizeof(float) * n * desc_.probabilities_channels * B2, hipMemcpyDeviceToHost, s));
        if (pass) HIP_OK(hipMemcpyAsync(pass, io.pass, sizeof(float) * n * desc_.pass_probability_outputs, hipMemcpyDeviceToHost, s));
        if (misc) HIP_OK(hipMemcpyAsync(misc, io.misc, sizeof(float) * n * desc_.value_misc_outputs, hipMemcpyDeviceToHost, s));
        if (own) HIP_OK(hipMemcpyAsync(own, io.own, sizeof(float) * n * B2, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        return sx_check(0);
    }

    int time_runs(int iters, float* ms) override {
        std::lock_guard<std::mutex> lk(mu_);
        if (!have_batch_) return fail("time_runs before upload");
        HIP_OK(hipSetDevice(device_));
        const Measuring m{measuring_};
        pool_used_ = 0;
        group_counts_.clear();
        group_open_ = false;
        light_ = !light_name_.empty();
        HIP_OK(hipEventRecord(ev0_, compute_[0]));
        for (int i = 0; i < iters; ++i)
            if (forward(0)) { light_ = false; return -1; }
        if (group_open_ && close_group(compute_[0])) { light_ = false; return -1; }
        HIP_OK(hipEventRecord(ev1_, compute_[0]));
        light_ = false;
        HIP_OK(hipEventSynchronize(ev1_));
        HIP_OK(hipEventElapsedTime(ms, ev0_, ev1_));
        // fold the event pairs of the marked kernel class into one stat row (a pair brackets group_counts_[k] launches)
        timed_stat_ = Stat{};
        for (size_t k = 0; k < group_counts_.size() && 2 * k + 1 < pool_used_; ++k) {
            float t = 0.f;
            HIP_OK(hipEventElapsedTime(&t, pool_[2 * k], pool_[2 * k + 1]));
            timed_stat_.launches += group_counts_[k];
            timed_stat_.ms += t;
            timed_stat_.flops += light_flops_ * group_counts_[k];
            timed_stat_.bytes += light_bytes_ * group_counts_[k];
        }
        return 0;
    }

    // "class" brackets every launch of the class with its own event pair; "class/N" brackets RUNS of up to N consecutive
    // launches of the class with one pair (a launch of another class ends the run).  An event is a barrier packet on the
    // stream: the launch that follows it starts from an empty pipeline (~2-3 us), which a pair per launch both adds to
    // the step (34 tower launches: ~5 %) and counts into every measured duration; per run of five it is a fifth of that.
    int mark_kernel(const char* name) override {
        light_name_ = name ? name : "";
        light_group_ = 1;
        const size_t slash = light_name_.find('/');
        if (slash != std::string::npos) {
            light_group_ = std::max(1, atoi(light_name_.c_str() + slash + 1));
            light_name_.resize(slash);
        }
        return 0;
    }
    int timed_stat(sayuri_hip_kernel_stat* row) override {
        std::memset(row, 0, sizeof(*row));
        std::snprintf(row->name, sizeof(row->name), "%s", light_name_.c_str());
        row->launches = timed_stat_.launches;
        row->total_ms = timed_stat_.ms;
        row->flops = timed_stat_.flops;
        row->bytes = timed_stat_.bytes;
        return 0;
    }

    int profile_run(sayuri_hip_kernel_stat* rows, int cap) override {
        std::lock_guard<std::mutex> lk(mu_);
        if (!have_batch_) return fail("profile_run before upload");
        HIP_OK(hipSetDevice(device_));
        const Measuring m{measuring_};
        stats_.clear();
        profiling_ = true;
        const int rc = forward(0);
        profiling_ = false;
        if (rc) return -1;
        if (d_hdbg_) {
            std::vector<unsigned long long> h(4 * 8);
            HIP_OK(hipMemcpy(h.data(), d_hdbg_, h.size() * 8, hipMemcpyDeviceToHost));
            for (int wg = 0; wg < 4; ++wg) {
                const unsigned long long* d = &h[wg * 8];
                fprintf(stderr, "[heads timeline wg%d] DMA + K loop %llu | act, per-pixel MFMA, pooling partials %llu | pool fold %llu | FC 1 %llu | FC 2 + row bias %llu | stores %llu | total %llu\n",
                        wg, d[1] - d[0], d[2] - d[1], d[3] - d[2], d[4] - d[3], d[5] - d[4], d[6] - d[5], d[6] - d[0]);
            }
        }
        if (d_sxdbg_) {  // SAYURI_SX_DBG: the split SE convolution from inside (100 MHz ticks; blocks 0 / 8 / 16 = the siblings of a tile, 1)
            std::vector<unsigned long long> h(4 * 64);
            HIP_OK(hipMemcpy(h.data(), d_sxdbg_, h.size() * 8, hipMemcpyDeviceToHost));
            static const char* who[4] = {"block 0 (tile 0, kt 0)", "block 8 (tile 0, kt 1)", "block 16 (tile 0, kt 2)", "block 1 (tile 1, kt 0)"};
            for (int wg = 0; wg < 4; ++wg) {
                const unsigned long long* d = &h[(size_t)wg * 64];
                fprintf(stderr, "[split SE timeline %s] start +%llu | K loop %llu | pooling %llu | squeeze + publish %llu | siblings in %llu | mid + excite %llu | gate %llu | epilogue %llu | total %llu\n",
                        who[wg], d[0] - h[0], d[1] - d[0], d[2] - d[1], d[3] - d[2], d[4] - d[3], d[5] - d[4], d[6] - d[5], d[7] - d[6], d[7] - d[0]);
            }
        }
        if (d_dbg_) {  // SAYURI_BOARD_DBG: s_memtime timeline of the last tower convolution (workgroups 0-3, all waves)
            std::vector<unsigned long long> h(4 * 8 * 8);
            HIP_OK(hipMemcpy(h.data(), d_dbg_, h.size() * 8, hipMemcpyDeviceToHost));
            for (int wg = 0; wg < 4 && dbg_is_se_; ++wg)
                for (int w = 0; w < 8; w += 4) {
                    const unsigned long long* d = &h[((size_t)wg * 8 + w) * 8];
                    fprintf(stderr, "[board+SE timeline wg%d wave%d] prologue+K loop %llu | pooling %llu | squeeze FC %llu | excite FC %llu | gate applied %llu | epilogue %llu | total %llu\n",
                            wg, w, d[1] - d[0], d[2] - d[1], d[3] - d[2], d[4] - d[3], d[5] - d[4], d[6] - d[5], d[6] - d[0]);
                }
            for (int wg = 0; wg < 4 && !dbg_is_se_; ++wg)
                for (int w = 0; w < 8; ++w) {
                    const unsigned long long* d = &h[((size_t)wg * 8 + w) * 8];
                    fprintf(stderr, "[board timeline wg%d wave%d] tables+first DMA %llu | first barrier %llu | main loop %llu (sync %llu) | epilogue %llu | total %llu\n",
                            wg, w, d[1] - d[0], d[2] - d[1], d[3] - d[2], d[5], d[4] - d[3], d[4] - d[0]);
                }
        }
        int i = 0;
        for (auto& kv : stats_) {
            if (i >= cap) break;
            std::memset(&rows[i], 0, sizeof(rows[i]));
            std::snprintf(rows[i].name, sizeof(rows[i].name), "%s", kv.first.c_str());
            rows[i].launches = kv.second.launches;
            rows[i].total_ms = kv.second.ms;
            rows[i].flops = kv.second.flops;
            rows[i].bytes = kv.second.bytes;
            ++i;
        }
        return i;
    }

    // workspaces + the live weight set + a staged one + replaced ones whose last forwards have not finished yet
    size_t device_bytes() const override {
        Engine* self = const_cast<Engine*>(this);
        if (n_retired_.load(std::memory_order_relaxed)) (void)self->retire_poll();
        // (the staged set's count is a member of its own: a caller that watches the bytes does not wait for a prepare in progress)
        size_t b = staged_bytes_.load(std::memory_order_relaxed);
        std::lock_guard<std::mutex> lk(self->mu_);
        b += work_.bytes + live_->pool.bytes;
        for (const Retired& r : retired_) b += r.set->pool.bytes;
        return b;
    }

    // -------------------------------------------------------------- live weight reload
    // A reload stages a second WeightSet (begin, load_tensor), builds its images into device buffers of its own (prepare) and
    // swaps the one pointer the launch code reads the weights through (commit).  begin / load_tensor / prepare touch the staged
    // set only (reload_mu_); commit takes mu_, which submit() and every other call that enqueues a forward hold: it falls
    // between two forwards.  The replaced set is freed once an event recorded behind everything enqueued before the commit, on
    // each ticket's compute stream, has fired (retire_poll: looked at by submit, wait and device_bytes, freed outside mu_).
    int reload_begin(const sayuri_hip_netdesc& d) override {
        std::lock_guard<std::mutex> rl(reload_mu_);
        if (staged_) return fail("reload_begin: a reload is already open on this context (commit or abort it first)");
        if (measuring_.load(std::memory_order_acquire)) return fail("reload_begin: the context is profiling or timing");
        const std::string diff = desc_difference(d);
        if (!diff.empty()) return fail("reload_begin: the network differs from the context's: " + diff + " (a context is reloaded with the same architecture only)");
        auto ws = std::make_unique<WeightSet>();
        if (describe_layers(*ws)) return -1;
        staged_ = std::move(ws);
        return 0;
    }
    int reload_prepare() override {
        std::lock_guard<std::mutex> rl(reload_mu_);
        if (!staged_) return fail("reload_prepare: no reload is open");
        if (staged_->built) return fail("reload_prepare: the open reload is prepared already");
        if (hipSetDevice(device_) != hipSuccess) { drop_staged(); return fail("reload_prepare: hipSetDevice failed"); }
        int rc = build_set(*staged_);
        staged_bytes_.store(staged_->pool.bytes, std::memory_order_relaxed);
        if (!rc) {
            // What the workspaces were sized by must not move (same description: it cannot; checked, not assumed).  The live set is
            // the forwards' (mu_): the very first forward may be building it right now.
            std::lock_guard<std::mutex> lk(mu_);
            if (live_->built && (staged_->sx_kts != live_->sx_kts || (staged_->head_img != nullptr) != (live_->head_img != nullptr)))
                rc = fail("reload_prepare: the new weights take another kernel form than the context's workspaces were built for");
        }
        if (rc) {
            const std::string why = g_err;
            drop_staged();
            return fail("reload_prepare: " + why);
        }
        return 0;
    }
    int reload_commit() override {
        std::lock_guard<std::mutex> rl(reload_mu_);
        if (!staged_) return fail("reload_commit: no reload is open");
        if (!staged_->built) return fail("reload_commit: the open reload is not prepared (reload_prepare first)");
        std::lock_guard<std::mutex> lk(mu_);
        HIP_OK(hipSetDevice(device_));
        Retired r;
        for (int t = 0; t < 2; ++t) {
            if (t == 1 && compute_[1] == compute_[0]) break;
            hipError_t e = hipEventCreateWithFlags(&r.done[t], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(r.done[t], compute_[t]);
            if (e != hipSuccess) {
                for (hipEvent_t& ev : r.done) { if (ev) (void)hipEventDestroy(ev); ev = nullptr; }
                return fail(std::string("reload_commit: ") + hipGetErrorString(e));
            }
        }
        r.set = std::move(live_);
        live_ = std::move(staged_);
        staged_bytes_.store(0, std::memory_order_relaxed);
        retired_.push_back(std::move(r));
        n_retired_.store((int)retired_.size(), std::memory_order_relaxed);
        // Nothing else holds a weight address: routes, plans and index tables are keyed by the batch geometry and hold none, and
        // a tower slot's table is compared bytewise with what the device holds before every launch (tower_flush).
        return generation_.fetch_add(1, std::memory_order_acq_rel) + 1;
    }
    int reload_abort() override {
        std::lock_guard<std::mutex> rl(reload_mu_);
        if (!staged_) return fail("reload_abort: no reload is open");
        (void)hipSetDevice(device_);
        drop_staged();
        return 0;
    }
    int weights_generation() const override { return generation_.load(std::memory_order_acquire); }
    int last_chains() const override { return last_chains_; }
    int last_split_ring() const override { return last_split_ring_; }
    int last_pw_launches() const override { return last_pw_launches_; }
    int last_dw_launches() const override { return last_dw_launches_; }
    int tower_state() const override { return tower_fn_[0] != nullptr ? 1 : 0; }
    int latency_state() const override { return flags_.latency ? 1 : 0; }
    int debug_read(int buf, void* host, size_t bytes) override {
        if (buf < 0 || buf >= kNumBufs || !io_[0].bufs[buf]) return fail("debug_read: no such buffer");
        HIP_OK(hipSetDevice(device_));
        HIP_OK(hipDeviceSynchronize());
        const size_t have = (size_t)max_batch_ * slot_pix_ * cs_max_ * sizeof(T);
        HIP_OK(hipMemcpy(host, io_[0].bufs[buf], std::min(bytes, have), hipMemcpyDeviceToHost));
        return 0;
    }

private:
    // -------------------------------------------------------------- construction helpers
    // Device allocations with one owner and one byte count: the context's workspaces, or one weight set.
    struct DevPool {
        std::vector<void*> allocs;
        size_t bytes = 0;
    };
    // A WEIGHT SET: everything a forward reads that is derived from the weights -- the layers with their device images, the SE
    // images inside them, the head images -- in device allocations of its own.  The launch code reaches it through live_ alone.
    struct WeightSet {
        std::map<int, ConvLayerDev> convs;
        std::map<int, FcLayerDev> fcs;
        HeadFn head_fn = nullptr;
        void* head_img2 = nullptr;  // per-pixel weights (policy planes, ownership) as an MFMA image
        void* head_img = nullptr;   // stacked head-convolution image (head_board.h); null = separate head kernels
        float* head_bias = nullptr;
        int head_pt = 0, head_vt = 0;
        int sx_kts = 0;             // channel tiles per layer of the split SE images (0: the set has none)
        bool built = false;         // the images are on the device (build_set)
        DevPool pool;
    };
    // a replaced set and the events behind the last forwards that may read it, one per compute stream
    struct Retired {
        std::unique_ptr<WeightSet> set;
        hipEvent_t done[2] = {nullptr, nullptr};
    };
    struct Measuring {  // time_runs / profile_run in progress: no reload is opened meanwhile
        std::atomic<bool>& flag;
        explicit Measuring(std::atomic<bool>& f) : flag(f) { flag.store(true, std::memory_order_release); }
        ~Measuring() { flag.store(false, std::memory_order_release); }
    };
    void free_pool(DevPool& p) {
        for (void* q : p.allocs) (void)hipFree(q);
        p.allocs.clear();
        p.bytes = 0;
    }
    void drop_staged() {  // reload_mu_ held
        if (staged_) free_pool(staged_->pool);
        staged_.reset();
        staged_bytes_.store(0, std::memory_order_relaxed);
    }
    // Frees every replaced set whose events have all fired; a set whose forwards still run stays for the next look.  Called
    // WITHOUT mu_: the finished sets are taken off the list under it, and freed outside it -- hipFree synchronises the device, once
    // per allocation of the set, and a submit on another thread must not wait behind that for the mutex.
    int retire_poll() {
        std::vector<Retired> gone;
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t i = 0; i < retired_.size();) {
                bool done = true;
                for (hipEvent_t e : retired_[i].done)
                    if (e && hipEventQuery(e) != hipSuccess) done = false;
                if (!done) { (void)hipGetLastError(); ++i; continue; }
                gone.push_back(std::move(retired_[i]));
                retired_.erase(retired_.begin() + (long)i);
            }
            n_retired_.store((int)retired_.size(), std::memory_order_relaxed);
        }
        if (!gone.empty()) (void)hipSetDevice(device_);
        for (Retired& r : gone) {
            free_pool(r.set->pool);
            for (hipEvent_t e : r.done)
                if (e) (void)hipEventDestroy(e);
        }
        return 0;
    }
    // What of a description shapes buffers or kernels, against the context's own: "" when nothing differs.
    std::string desc_difference(const sayuri_hip_netdesc& d) const {
        const sayuri_hip_netdesc& c = desc_;
        auto ne = [](const char* what, int have, int got) { return std::string(what) + " " + std::to_string(got) + " (the context has " + std::to_string(have) + ")"; };
        if (d.residual_blocks != c.residual_blocks) return ne("residual_blocks", c.residual_blocks, d.residual_blocks);
        if (d.residual_channels != c.residual_channels) return ne("residual_channels", c.residual_channels, d.residual_channels);
        if (d.input_channels != c.input_channels) return ne("input_channels", c.input_channels, d.input_channels);
        if ((d.version <= 2) != (c.version <= 2)) return ne("version (encoder)", c.version, d.version);
        if (d.policy_head_type != c.policy_head_type) return ne("policy_head_type", c.policy_head_type, d.policy_head_type);
        if (d.policy_head_channels != c.policy_head_channels) return ne("policy_head_channels", c.policy_head_channels, d.policy_head_channels);
        if (d.value_head_channels != c.value_head_channels) return ne("value_head_channels", c.value_head_channels, d.value_head_channels);
        if (d.policy_dw_filter != c.policy_dw_filter) return ne("policy_dw_filter", c.policy_dw_filter, d.policy_dw_filter);
        if (d.probabilities_channels != c.probabilities_channels) return ne("probabilities_channels", c.probabilities_channels, d.probabilities_channels);
        if (d.pass_probability_outputs != c.pass_probability_outputs) return ne("pass_probability_outputs", c.pass_probability_outputs, d.pass_probability_outputs);
        if (d.ownership_channels != c.ownership_channels) return ne("ownership_channels", c.ownership_channels, d.ownership_channels);
        if (d.value_misc_outputs != c.value_misc_outputs) return ne("value_misc_outputs", c.value_misc_outputs, d.value_misc_outputs);
        if (d.default_act != c.default_act) return ne("default_act", c.default_act, d.default_act);
        if (!d.blocks) return "no block descriptions";
        for (int b = 0; b < c.residual_blocks; ++b) {
            const sayuri_hip_blockdesc &x = d.blocks[b], &y = blocks_[b];
            const std::string at = "block " + std::to_string(b) + ": ";
            if (x.type != y.type) return at + ne("type", y.type, x.type);
            if ((x.apply_se != 0) != (y.apply_se != 0)) return at + ne("apply_se", y.apply_se, x.apply_se);
            if (y.apply_se && x.se_size != y.se_size) return at + ne("se_size", y.se_size, x.se_size);
            if (x.bottleneck_channels != y.bottleneck_channels) return at + ne("bottleneck_channels", y.bottleneck_channels, x.bottleneck_channels);
            if (x.feedforward_channels != y.feedforward_channels) return at + ne("feedforward_channels", y.feedforward_channels, x.feedforward_channels);
            if (x.dw_filter != y.dw_filter) return at + ne("dw_filter", y.dw_filter, x.dw_filter);
        }
        return "";
    }

    // the layers of the context's description, without tensors, into `ws`
    int describe_layers(WeightSet& ws) {
        auto add_conv = [&ws](int id, int cin, int cout, int k, bool depthwise = false) {
            ConvLayerDev L;
            L.cin = cin; L.cout = cout; L.k = k; L.depthwise = depthwise;
            ws.convs[id] = L;
        };
        auto add_fc = [&ws](int id, int in, int out) {
            FcLayerDev L;
            L.in = in; L.out = out;
            ws.fcs[id] = L;
        };
        const auto& d = desc_;
        const int C = d.residual_channels;
        if (C <= 0 || d.input_channels <= 0) return fail("bad net description");
        add_conv(SAYURI_L_INPUT_CONV, d.input_channels, C, 3);
        int cs_max = std::max(round_up(C, 32), round_up(d.input_channels, 32));  // (a member for the context's own set only)
        for (int b = 0; b < d.residual_blocks; ++b) {
            const auto& bd = blocks_[b];
            const int I = bd.bottleneck_channels, F = bd.feedforward_channels;
            switch (bd.type) {
            case SAYURI_BLOCK_RESIDUAL:
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_CONV1), C, C, 3);
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2), C, C, 3);
                break;
            case SAYURI_BLOCK_BOTTLENECK:
            case SAYURI_BLOCK_NESTED_BOTTLENECK:
                if (I <= 0) return fail("bottleneck block without bottleneck_channels");
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_PRE_BTL), C, I, 1);
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_CONV1), I, I, 3);
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2), I, I, 3);
                if (bd.type == SAYURI_BLOCK_NESTED_BOTTLENECK) {
                    add_conv(SAYURI_L_BLOCK(b, SAYURI_S_CONV3), I, I, 3);
                    add_conv(SAYURI_L_BLOCK(b, SAYURI_S_CONV4), I, I, 3);
                }
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_POST_BTL), I, C, 1);
                cs_max = std::max(cs_max, round_up(I, 32));
                break;
            case SAYURI_BLOCK_MIXER:
                if (F <= 0 || bd.dw_filter <= 0) return fail("mixer block without ffn channels / dw filter");
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_DW_CONV), C, C, bd.dw_filter, true);
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_CONV1), C, F, 1);
                add_conv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2), F, C, 1);
                cs_max = std::max(cs_max, round_up(F, 32));
                break;
            default:
                return fail("unknown block type");
            }
            if (bd.apply_se) {
                if (bd.se_size <= 0) return fail("SE block without se_size");
                add_fc(SAYURI_L_BLOCK(b, SAYURI_S_SQUEEZE), 3 * C, bd.se_size);
                add_fc(SAYURI_L_BLOCK(b, SAYURI_S_EXCITE), bd.se_size, 2 * C);
            }
        }
        const int Cp = d.policy_head_channels, Cv = d.value_head_channels;
        if (Cp <= 0 || Cv <= 0) return fail("bad head channels");
        if (d.ownership_channels != 1) return fail("ownership_channels must be 1");
        if (d.probabilities_channels > 8) return fail("too many policy planes");
        add_conv(SAYURI_L_P_HD_CONV, C, Cp, 1);
        if (d.policy_head_type == 1) {
            if (d.policy_dw_filter <= 0) return fail("RepLK head without dw filter");
            add_conv(SAYURI_L_P_DW_CONV, Cp, Cp, d.policy_dw_filter, true);
            add_conv(SAYURI_L_P_PT_CONV, Cp, Cp, 1);
        }
        add_fc(SAYURI_L_P_INTER_FC, 3 * Cp, Cp);
        add_conv(SAYURI_L_PROB_CONV, Cp, d.probabilities_channels, 1);
        add_fc(SAYURI_L_PASS_FC, Cp, d.pass_probability_outputs);
        add_conv(SAYURI_L_V_HD_CONV, C, Cv, 1);
        add_fc(SAYURI_L_V_INTER_FC, 3 * Cv, 3 * Cv);
        add_conv(SAYURI_L_V_OWNERSHIP, Cv, 1, 1);
        add_fc(SAYURI_L_V_MISC, 3 * Cv, d.value_misc_outputs);
        cs_max = std::max(cs_max, std::max(round_up(Cp, 32), round_up(Cv, 32)));
        if (&ws == live_.get()) cs_max_ = cs_max;
        return 0;
    }

    template <typename U> int dev_alloc(U** p, size_t count) { return dev_alloc(work_, p, count); }
    template <typename U> int dev_upload(U** p, const std::vector<U>& h) { return dev_upload(work_, p, h); }
    template <typename U> int dev_alloc(DevPool& pool, U** p, size_t count) {
        void* q = nullptr;
        const size_t bytes = std::max<size_t>(count * sizeof(U), 256);
        HIP_OK(hipMalloc(&q, bytes));
        // The zero fill runs on the NULL stream and hipMemset returns before it has: this engine's streams are non-blocking, so
        // a copy or kernel they write into the new buffer right away could be overtaken by it (round 4: the first packed batch of
        // a staging slot lost the tail of its records to the fill of the buffer allocated for them one call earlier).
        HIP_OK(hipMemset(q, 0, bytes));
        HIP_OK(hipStreamSynchronize(nullptr));
        pool.allocs.push_back(q);
        pool.bytes += bytes;
        *p = (U*)q;
        return 0;
    }
    template <typename U> int dev_upload(DevPool& pool, U** p, const std::vector<U>& h) {
        if (dev_alloc(pool, p, h.size())) return -1;
        HIP_OK(hipMemcpy(*p, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice));
        return 0;
    }

    static bool is_tiny_head_conv(int id) { return id == SAYURI_L_PROB_CONV || id == SAYURI_L_V_OWNERSHIP; }

    // Stacked [policy | value] head-convolution image for head_board_kernel (fp16 engine, normal policy head).
    int build_head_image(WeightSet& ws) {
        const sayuri_hip_netdesc& d = desc_;
        if (sizeof(T) != 2 || d.policy_head_type != 0) return 0;
        const ConvLayerDev& P = ws.convs.at(SAYURI_L_P_HD_CONV);
        const ConvLayerDev& V = ws.convs.at(SAYURI_L_V_HD_CONV);
        const ConvLayerDev& PW = ws.convs.at(SAYURI_L_PROB_CONV);
        const ConvLayerDev& OW = ws.convs.at(SAYURI_L_V_OWNERSHIP);
        if (P.hw.empty() || V.hw.empty() || P.hb.empty() || V.hb.empty() || PW.hw.empty() || OW.hw.empty()) return 0;
        HeadImages hi;
        ws.head_fn = make_head_images(P.cin, P.cout, V.cout, d.probabilities_channels, board_, P.hw.data(), P.hb.data(), V.hw.data(),
                                      V.hb.data(), PW.hw.data(), OW.hw.data(), &hi);
        if (!ws.head_fn) return 0;
        f16 *w = nullptr, *w2 = nullptr;
        if (dev_upload(ws.pool, &w2, hi.img2) || dev_upload(ws.pool, &w, hi.img) || dev_upload(ws.pool, &ws.head_bias, hi.bias)) return -1;
        ws.head_img2 = w2;
        ws.head_img = w;
        ws.head_pt = hi.PT;
        ws.head_vt = hi.VT;
        return 0;
    }

    // Loaded tensors -> the device images of a weight set, in the set's own allocations.  The reusable half of what the first
    // forward does: finalize() builds the live set with it, reload_prepare() a staged one beside the running forwards (the
    // uploads go through the null stream into buffers nothing reads yet: they order against nothing, and need not).
    int build_set(WeightSet& ws) {
        DevPool& pool = ws.pool;
        if (build_head_image(ws)) return -1;
        for (auto& kv : ws.convs) {
            ConvLayerDev& L = kv.second;
            if (L.hw.empty() || L.hb.empty()) return fail("missing tensors for conv layer " + std::to_string(kv.first));
            L.cin_s = round_up(L.cin, 32);
            L.cout_s = round_up(L.cout, 32);
            if (is_tiny_head_conv(kv.first)) {  // consumed by head_tail_kernel in fp32
                if (dev_upload(pool, &L.w32, L.hw) || dev_upload(pool, &L.bias, L.hb)) return -1;
            } else if (L.depthwise) {
                float* w = nullptr;
                if (dev_upload(pool, &w, depthwise_image(L.hw.data(), L.cout, L.k * L.k, L.cout_s)) ||
                    dev_upload(pool, &L.bias, padded_bias(L.hb.data(), L.cout, L.cout_s)))
                    return -1;
                L.w = w;
            } else {
                conv_tile(L.cout_s, sizeof(T) == 2, &L.wmt, &L.ko_pad);
                const std::vector<T> img = conv_image<T>(L.hw.data(), L.cin, L.cout, L.k * L.k, L.ko_pad);
                const std::vector<float> b = padded_bias(L.hb.data(), L.cout, L.ko_pad);
                T* w = nullptr;
                if (dev_upload(pool, &w, img) || dev_upload(pool, &L.bias, b)) return -1;
                L.w = w;
                if (sizeof(T) == 2 && L.k == 3 && L.ko_pad % 128 == 0 && !flags_.latency) {  // (conv_split.h reads the natural order)
                    T* wb = nullptr;
                    if (dev_upload(pool, &wb, board_row_order(img, L.ko_pad)) || dev_upload(pool, &L.bias_board, board_row_order(b, L.ko_pad, 1))) return -1;
                    L.w_board = wb;
                }
            }
            std::vector<float>().swap(L.hw);
            std::vector<float>().swap(L.hb);
        }
        if (build_se_images(ws)) return -1;
        for (auto& kv : ws.fcs) {
            FcLayerDev& L = kv.second;
            if (L.hw.empty() || L.hb.empty()) return fail("missing tensors for fc layer " + std::to_string(kv.first));
            if (dev_upload(pool, &L.wt, fc_transposed(L.hw.data(), L.in, L.out)) || dev_upload(pool, &L.b, L.hb)) return -1;
            std::vector<float>().swap(L.hw);
            std::vector<float>().swap(L.hb);
        }
        ws.built = true;
        return 0;
    }

    // The once-only half: the live set (unless a reload committed before the first forward has brought one that is built), then
    // workspaces, pinned rings and tables.
    int finalize() {
        if (finalized_) return 0;
        if (!live_->built && build_set(*live_)) return -1;
        sx_kts_ = live_->sx_kts;
        // workspaces
        slot_pix_ = board_ * board_;
        const size_t act_elems = (size_t)max_batch_ * slot_pix_ * cs_max_;
        // the board kernels address an activation buffer with 24-bit row indices (__umul24) and 32-bit byte offsets from a
        // uniform base (conv_board.h epilogue): both must cover the largest batch this ctx can be handed
        if ((size_t)max_batch_ * slot_pix_ >= (size_t(1) << 24) || act_elems * sizeof(T) >= (size_t(1) << 32))
            return fail("max_batch " + std::to_string(max_batch_) + " is too large for this network on one ctx: max_batch * board^2 must stay below 2^24 rows and an activation buffer (" +
                        std::to_string(act_elems * sizeof(T) >> 20) + " MiB) below 4 GiB");
        for (IoSlot& io : io_)
            for (int i = 0; i < kNumBufs; ++i)
                // every activation buffer starts kZeroPrefix bytes into its (zero-filled) allocation: conv_board.h reads
                // its halo cells from that prefix
                if (dev_alloc(&io.bufs[i], act_elems + kZeroPrefix / sizeof(T))) return -1;
                else io.bufs[i] += kZeroPrefix / sizeof(T);
        const size_t B2 = (size_t)board_ * board_;
        for (IoSlot& io : io_) {
            if (dev_alloc(&io.planes, (size_t)max_batch_ * desc_.input_channels * B2)) return -1;
            if (dev_alloc(&io.packed, (size_t)max_batch_ * kPackedRecordWords)) return -1;  // the packed form of the same planes (packed_planes.h)
            if (dev_alloc(&io.off, max_batch_ + 1) || dev_alloc(&io.bsz, max_batch_) || dev_alloc(&io.perm, max_batch_)) return -1;
            if (dev_alloc(&io.prob, (size_t)max_batch_ * desc_.probabilities_channels * B2)) return -1;
            if (dev_alloc(&io.pass, (size_t)max_batch_ * desc_.pass_probability_outputs)) return -1;
            if (dev_alloc(&io.misc, (size_t)max_batch_ * desc_.value_misc_outputs)) return -1;
            if (dev_alloc(&io.own, (size_t)max_batch_ * B2)) return -1;
        }
        if (dev_alloc(&d_zeros_, 64)) return -1;
        HIP_OK(hipHostMalloc((void**)&h_geom_, sizeof(int) * 2 * (3 * max_batch_ + 1), hipHostMallocDefault));
        for (IoSlot& io : io_) {
            if (dev_alloc(&io.gate, (size_t)max_batch_ * 2 * round_up(desc_.residual_channels, 32))) return -1;
            if (dev_alloc(&io.separt, (size_t)max_batch_ * kSeSplit * 2 * round_up(desc_.residual_channels, 32))) return -1;
            // conv_board_sx.h: the granules the sibling channel tiles of a board tile exchange, [tile][kt][sample][slot]
            if (sx_kts_ && dev_alloc(&io.sx_xchg, (size_t)max_batch_ * sx_kts_ * kSxMaxSub * kSxSlots)) return -1;
            io.sx_epoch = flags_.dbg_sx_epoch0;
            if (sx_kts_) {
                HIP_OK(hipHostMalloc((void**)&io.sx_err_host, 64, hipHostMallocMapped));
                std::memset(io.sx_err_host, 0, 64);
                HIP_OK(hipHostGetDevicePointer((void**)&io.sx_err_dev, io.sx_err_host, 0));
            }
        }
        finalized_ = true;
        return 0;
    }

    // fp16 images of the SE units' two FCs, laid out for the LDS-DMA staging of board_se_stage (conv_board.h): the squeeze
    // weights once per board size 2..board with the scaled-mean third of the pooled vector folded into the mean third
    // (reference GlobalPooling<false>, se_unit.cc:9-40: pool = (mean, mean * (B-14)/10, max)), the excite weights with
    // both bias vectors behind them.  Units whose images do not fit the LDS keep reading fp32 weights from L2.
    int build_se_images(WeightSet& ws) {
        if (sizeof(T) != 2) return 0;
        auto& fcs = ws.fcs;
        DevPool& pool = ws.pool;
        const int C = desc_.residual_channels;
        for (int b = 0; b < desc_.residual_blocks; ++b) {
            if (!blocks_[b].apply_se) continue;
            FcLayerDev& sq = fcs.at(SAYURI_L_BLOCK(b, SAYURI_S_SQUEEZE));
            FcLayerDev& ex = fcs.at(SAYURI_L_BLOCK(b, SAYURI_S_EXCITE));
            const int se = sq.out;
            if (sq.hw.empty() || ex.hw.empty() || sq.hb.empty() || ex.hb.empty()) continue;  // finalize() reports it
            if (sq.in != 3 * C || ex.in != se || ex.out != 2 * C) continue;
            std::vector<f16> img1;
            std::vector<unsigned char> img2;
            int w1_bytes = 0, w2_bytes = 0;
            if (!make_se_images(C, se, board_, sq.hw.data(), sq.hb.data(), ex.hw.data(), ex.hb.data(), &img1, &img2, &w1_bytes, &w2_bytes)) {
                // a layer too wide for one workgroup: the per-channel-tile images of conv_board_sx.h
                const int kts = round_up(C, 128) / 128;
                if (flags_.se_split && round_up(C, 32) == kts * 128 &&
                    make_sx_images(C, se, kts, board_, sq.hw.data(), sq.hb.data(), ex.hw.data(), ex.hb.data(), &img1, &img2, &w1_bytes, &w2_bytes)) {
                    f16* d1 = nullptr;
                    unsigned char* d2 = nullptr;
                    if (dev_upload(pool, &d1, img1) || dev_upload(pool, &d2, img2)) return -1;
                    sq.sx_img = d1; sq.sx_bytes = w1_bytes;
                    ex.sx_img = d2; ex.sx_bytes = w2_bytes;
                    ws.sx_kts = kts;
                }
                continue;
            }
            f16* d1 = nullptr;
            unsigned char* d2 = nullptr;
            if (dev_upload(pool, &d1, img1) || dev_upload(pool, &d2, img2)) return -1;
            sq.img16 = d1; sq.img_bytes = w1_bytes;
            ex.img16 = d2; ex.img_bytes = w2_bytes;
        }
        return 0;
    }

    void release() {
        (void)hipSetDevice(device_);
        free_pool(work_);
        if (live_) free_pool(live_->pool);
        if (staged_) free_pool(staged_->pool);
        staged_.reset();
        for (Retired& r : retired_) {
            free_pool(r.set->pool);
            for (hipEvent_t e : r.done)
                if (e) (void)hipEventDestroy(e);
        }
        retired_.clear();
        n_retired_.store(0, std::memory_order_relaxed);
        ident_.clear();
        if (h_geom_) (void)hipHostFree(h_geom_);
        h_geom_ = nullptr;
        if (h_symm_) (void)hipHostFree(h_symm_);
        h_symm_ = nullptr;
        for (IoSlot& io : io_) {
            if (io.sx_err_host) (void)hipHostFree(io.sx_err_host);
            io.sx_err_host = nullptr;
            io.sx_err_dev = nullptr;
        }
        for (TowerSlot& ts : tower_)
            for (int i = 0; i < 2; ++i) {
                if (ts.stage[i]) (void)hipHostFree(ts.stage[i]);
                if (ts.staged[i]) (void)hipEventDestroy(ts.staged[i]);
                ts.stage[i] = nullptr; ts.staged[i] = nullptr;
            }
        if (tower_mod_) (void)hipModuleUnload(tower_mod_);
        tower_mod_ = nullptr;
        for (hipStream_t& cs : chain_stream_) { if (cs) (void)hipStreamDestroy(cs); cs = nullptr; }
        for (hipEvent_t& e : chain_join_) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        if (chain_fork_) (void)hipEventDestroy(chain_fork_);
        chain_fork_ = nullptr;
        if (flags_.fwdstat && fs_cnt_[0] + fs_cnt_[1] + fs_cnt_[2] > 0) {
            const long all = fs_cnt_[0] + fs_cnt_[1] + fs_cnt_[2];
            std::fprintf(stderr, "[hip fwdstat] forwards by batch size (<= half | partial | full): %ld / %ld / %ld, mean device ms %.4f / %.4f / %.4f, tower table uploads %ld; "
                         "forward end -> downloads done: mean %.3f ms, max %.3f, > 1 ms: %ld\n",
                         fs_cnt_[0], fs_cnt_[1], fs_cnt_[2], fs_cnt_[0] ? fs_ms_[0] / fs_cnt_[0] : 0.0, fs_cnt_[1] ? fs_ms_[1] / fs_cnt_[1] : 0.0,
                         fs_cnt_[2] ? fs_ms_[2] / fs_cnt_[2] : 0.0, fs_uploads_, fs_d2h_ms_ / all, fs_d2h_max_, fs_d2h_slow_);
            fs_cnt_[0] = fs_cnt_[1] = fs_cnt_[2] = 0;
        }
        for (auto& pr : fs_ev_) for (hipEvent_t& e : pr) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        for (hipEvent_t& e : tick_ev_) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        for (hipEvent_t e : pool_) (void)hipEventDestroy(e);
        pool_.clear();
        if (ev0_) (void)hipEventDestroy(ev0_);
        if (ev1_) (void)hipEventDestroy(ev1_);
        for (hipEvent_t& e : h2d_done_) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        for (hipEvent_t& e : fwd_done_) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        if (compute_[1] && compute_[1] != compute_[0]) (void)hipStreamDestroy(compute_[1]);
        if (compute_[0]) (void)hipStreamDestroy(compute_[0]);
        if (h2d_stream_) (void)hipStreamDestroy(h2d_stream_);
        if (d2h_stream_) (void)hipStreamDestroy(d2h_stream_);
        ev0_ = ev1_ = nullptr;
        compute_[0] = compute_[1] = h2d_stream_ = d2h_stream_ = nullptr;
    }

    // -------------------------------------------------------------- what one forward works on
    static constexpr int kNumBufs = 6;  // small pool of activation buffers
    // device-side batch i/o, one set per ticket
    struct IoSlot {
        float *planes = nullptr, *prob = nullptr, *pass = nullptr, *misc = nullptr, *own = nullptr;
        unsigned* packed = nullptr;  // packed records of the batch (allocated on first use)
        const unsigned* packed_src = nullptr;  // non-null: the batch's records are read where the caller has them (pinned host memory)
        int packed_binary = 0;       // > 0: the slot's current batch came as packed records with this many bit planes
        bool symm_on = false;        // the current packed batch has a record map and symmetries (SymmReq) in sy_src / sy_symm
        int *sy_src = nullptr, *sy_symm = nullptr;  // [max_batch], caller's order (allocated with the first such batch)
        int *off = nullptr, *bsz = nullptr, *perm = nullptr;  // a mixed batch's geometry arrays (enqueue_inputs)
        const int *g_off = nullptr, *g_bsz = nullptr, *g_perm = nullptr;  // the current batch's: off / bsz / perm, or resident ones
        T* bufs[kNumBufs] = {};
        float *gate = nullptr, *separt = nullptr;
        unsigned long long* sx_xchg = nullptr;
        unsigned sx_epoch = 0;  // the last tag used in sx_xchg
        unsigned *sx_err_host = nullptr, *sx_err_dev = nullptr;  // set by a split SE workgroup whose wait for its siblings ran out
        std::map<int, TileTabs> tabs;   // index tables of the geometry this slot last ran (keyed by tile variant)
        BoardTabs board;
        std::vector<int> tabs_bsz;
        bool tabs_single = false;  // tabs_bsz is one board size with one sample per tile
        int tabs_n = -1;           // batch size the across-sample tables (tabs) were last built for
    };
    // One forward of a ticket's batch, or one chain of it (forward()).  Every launch helper is handed the Fwd it works for:
    // the slot, the stream, the tiles and samples it covers and where the heads write are never read from engine members.
    struct Fwd {
        int t;                       // the ticket: i/o slot io_[t], tower table tower_[t]
        IoSlot& io;
        hipStream_t stream;
        bool chained = false;        // one of several chains: not ordered against the other chains' launches
        int tile0 = 0, ntiles = 0;   // the board tiles [tile0, tile0 + ntiles) ...
        int n0 = 0, ns = 0;          // ... = the samples [n0, n0 + ns)
        double px = 0;               // their pixels
        float *pass = nullptr, *misc = nullptr;  // where the heads put pass / misc: the slot's buffers or the caller's (submit())
        unsigned sx_epoch0 = 0;      // tags of the split SE launches: sx_epoch0 + 1 + index of the SE layer
        // what lives from one layer to the next
        bool busy[kNumBufs] = {};
        int sx_idx = 0, dbg_call = 0, dbg_se_call = 0;
        std::vector<TowerLayer> run;  // board convolutions waiting for the persistent launch (tower_append)
        int run_kot = 0, table_used = 0;
        double run_flops = 0, run_bytes = 0;
        int take() { for (int i = 0; i < kNumBufs; ++i) if (!busy[i]) { busy[i] = true; return i; } return -1; }
        void give(int i) { busy[i] = false; }
    };
    BatchGeom dgeom(const IoSlot& io) const { return BatchGeom{io.g_off, io.g_bsz, geom_.n, geom_.total, slot_pix_}; }

    // -------------------------------------------------------------- launch plumbing
    int close_group(hipStream_t s) {
        HIP_OK(hipEventRecord(pool_[pool_used_ + 1], s));
        pool_used_ += 2;
        group_open_ = false;
        return 0;
    }
    template <typename F> int timed(Fwd& f, const char* name, double flops, double bytes, F&& launch) {
        if (!f.run.empty() && tower_flush(f)) return -1;  // the pending run of board convolutions goes first (stream order)
        if (!profiling_) {
            // light mode: un-synchronised event pairs around runs of the dominant kernel class only
            const bool match = light_ && light_name_ == name;
            if (group_open_ && (!match || group_counts_.back() >= light_group_)) {
                if (close_group(f.stream)) return -1;
            }
            if (match && !group_open_) {
                if (pool_used_ + 2 > pool_.size()) {
                    for (int i = 0; i < 64; ++i) {
                        hipEvent_t e;
                        HIP_OK(hipEventCreate(&e));
                        pool_.push_back(e);
                    }
                }
                HIP_OK(hipEventRecord(pool_[pool_used_], f.stream));
                group_counts_.push_back(0);
                group_open_ = true;
            }
            launch();
            HIP_OK(hipGetLastError());
            if (!f.chained) rows_reset();  // a launch on the forward's one stream: ordered against everything behind it
            if (match) {
                group_counts_.back() += 1;
                light_flops_ = flops;
                light_bytes_ = bytes;
            }
            return 0;
        }
        HIP_OK(hipEventRecord(ev0_, f.stream));
        launch();
        HIP_OK(hipGetLastError());
        rows_reset();
        HIP_OK(hipEventRecord(ev1_, f.stream));
        HIP_OK(hipEventSynchronize(ev1_));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, ev0_, ev1_));
        Stat& s = stats_[name];
        s.launches += 1;
        s.ms += ms;
        s.flops += flops;
        s.bytes += bytes;
        return 0;
    }

    // the generic kernel's variant for the current batch geometry (cached: it depends on the geometry only)
    int choose_tile(int wmt, int kot_tiles, TileChoice<T>* out) {
        *out = cached(tile_cache_, PlanKey{wmt, kot_tiles}, [&] {
            TileChoice<T> tc{};  // (e stays null where none fits)
            return pick_tile<T>(geom_, wmt, kot_tiles, /*widest=*/false, &tc), tc;
        });
        return out->e ? 0 : fail("no conv tile configuration fits this batch geometry");
    }
    // Tile choices, routes, plans and the board tiles depend on the batch geometry alone.  The one place that forgets them.
    void forget_geometry() {
        tile_cache_.clear(); route_cache_.clear(); split_cache_.clear(); dw_cache_.clear();
        board_plan_valid_ = false;
    }

    // index tables of the current batch geometry for pixel-tile size 64*wnt (built on first use)
    int tile_tabs(Fwd& f, const GldsEntry& e, const TileTabs** out) {
        TileTabs& t = f.io.tabs[e.wnt];
        if (!t.src) {
            const size_t max_tiles = ((size_t)max_batch_ * slot_pix_ + e.pt - 1) / e.pt;
            if (dev_alloc(&t.src, max_tiles * e.npos) || dev_alloc(&t.pix, max_tiles * e.pt)) return -1;
        }
        if (!t.fresh) {
            const int ntiles = (geom_.total + e.pt - 1) / e.pt;
            hipLaunchKernelGGL(e.setup, dim3(ntiles), dim3(256), 0, f.stream, dgeom(f.io), t.src, t.pix);
            HIP_OK(hipGetLastError());
            t.fresh = true;
        }
        *out = &t;
        return 0;
    }
    // index tables of the current batch geometry for conv_board_kernel (built on first use)
    int board_tabs(Fwd& f, const BoardTabs** out) {
        BoardTabs& t = f.io.board;
        if (!t.src) {
            // a tile holds at least one sample
            if (dev_alloc(&t.src, (size_t)max_batch_ * kBoardMaxPos) || dev_alloc(&t.pix, (size_t)max_batch_ * kBoardPT) ||
                dev_alloc(&t.cols, max_batch_))
                return -1;
        }
        // (a slot's tables may be kept for a shorter batch of the same geometry -- enqueue_inputs' prefix rule trusts the
        // sizes recorded at enqueue time; what counts here is how many tiles the tables were BUILT for)
        if (!t.fresh || t.npos_built != board_plan_.npos || board_plan_.ntiles > t.ntiles_built) {
            hipLaunchKernelGGL(board_setup_kernel, dim3(board_plan_.ntiles), dim3(256), 0, f.stream, dgeom(f.io), board_plan_.npos, t.src,
                               t.pix, t.cols);
            HIP_OK(hipGetLastError());
            t.fresh = true;
            t.npos_built = board_plan_.npos;
            t.ntiles_built = board_plan_.ntiles;
        }
        *out = &t;
        return 0;
    }
    // the board tiles of the current batch geometry (computed on first use)
    const BoardPlan& plan() {
        if (!board_plan_valid_) { board_plan_ = board_plan(geom_, flags_.conv); board_plan_valid_ = true; }
        return board_plan_;
    }
    // Which kernel family runs layer L on the current batch geometry (route_conv; cached: it depends on the geometry only).
    // The one-workgroup-per-board kernel applies to fp16 3x3 layers whenever the batch's boards fit its tiles, however empty
    // the tiles are: which convolution kernel a sample meets must not depend on its batch mates (a lone 9x9 board fills a fifth
    // of its tile; with the across-sample kernel it came out ~1e-4 away from the same position inside a larger batch).
    // `tower_pw`: L is a tower 1x1 of forward f (block slots PRE_BTL / POST_BTL, mixer CONV1 / CONV2): the one kind of layer that
    // may take conv_pw.h.  Its plan is for f's samples, so their range is part of the cache key (today a network with such a layer
    // runs as one chain, chains_for_batch(): one range per geometry).
    const ConvRoute& route(const ConvLayerDev& L, const Fwd* f = nullptr, bool tower_pw = false) {
        const BoardPlan& bp = plan();
        const bool pw = tower_pw && f && L.k == 1 && flags_.pw != 0 && sizeof(T) == 2;
        const PlanKey key = pw ? PlanKey{-1, L.cin, L.cout, f->n0, f->ns} : PlanKey{L.k, L.ko_pad};  // (-1: no layer's k)
        return cached(route_cache_, key, [&] {
            const PwAsk ask{L.cin, L.cout, L.cin_s, pw ? f->n0 : 0, pw ? f->ns : 0, flags_.pw_pieces, flags_.pw == 1};
            return route_conv(sizeof(T) == 2, L.k, L.ko_pad, geom_, bp, flags_.conv, flags_.board_kot, flags_.latency, pw ? &ask : nullptr);
        });
    }

    // The last step of a board convolution (conv, conv_se) once its parameters are built: it joins the pending persistent run
    // (to_run), or ends that run and is launched now -- `fn` with sp.b, or be->fn_se with sp when has_se.  Outside a chained
    // forward the layer takes the row-order weights wherever the generated epilogue covers it (board_row_order_ok).
    int board_launch(Fwd& f, const char* name, const ConvLayerDev& L, const BoardEntry* be, BoardFn fn, BoardSeParams& sp, bool has_se,
                     bool to_run, int grid, double flops, double bytes) {
        BoardParams& bp = sp.b;
        ConvParams& p = bp.c;
        if (!f.chained && tower_ok(be->kot) && L.w_board && L.bias_board && board_row_order_ok(bp, be->kot, flags_.tower_gen_epi)) {
            p.w = L.w_board; p.bias = L.bias_board; bp.row_order = 1;
        }
        // a pending run this layer does not join ends here (a launch = an ordered point: the table starts afresh)
        if (!f.run.empty() && !(to_run && f.run_kot == be->kot) && tower_flush(f)) return -1;
        if (rows_use(f, p, name)) return -1;
        if (to_run) return tower_append(f, be->kot, sp, has_se, flops, bytes);
        const size_t lds = be->lds(board_plan_.npos);
        return timed(f, name, flops, bytes, [&] {
            if (has_se) hipLaunchKernelGGL(be->fn_se, dim3(grid), dim3(512), lds, f.stream, sp);
            else hipLaunchKernelGGL(fn, dim3(grid), dim3(512), lds, f.stream, bp);
        });
    }

    // An SE layer of a mixed batch (conv_se, conv_sx): WHICH samples take the fused form is a property of the sample alone, never
    // of its batch mates (a position's result must not depend on what else the queue collected: the fused forms pool the fp32
    // accumulators, the separate kernels pool x rounded to fp16).  `fused(bs)` holds for the larger boards, and the device order
    // is largest first, so the fused samples -- and their tiles -- lead the batch: of the forward's tiles, [f0, f1) are fused
    // and [r0, r1) are the plain tail.
    struct SeSplit { int f0, f1, r0, r1; };
    template <typename Rule> SeSplit se_split(const Fwd& f, Rule fused) const {
        int s = 0, tile = 0;
        while (s < geom_.n && fused(geom_.bsz[s])) ++s;
        while (tile < board_plan_.ntiles && board_plan_.tile_first[tile] < s) ++tile;  // the first tile that is not fused
        const int t1 = f.tile0 + f.ntiles;
        return SeSplit{f.tile0, std::min(t1, tile), std::max(f.tile0, tile), t1};
    }
    // ... and its plain tail, the tiles [r0, r1) behind: the board convolution of `bp` over kts channel tiles without activation,
    // residual or row order, then the SE unit's three kernels on those tiles' samples.
    int se_tail(Fwd& f, const ConvLayerDev& L, const FcLayerDev& sq, const FcLayerDev& ex, const BoardEntry* be, const BoardParams& bp,
                int kts, int r0, int r1, T* out, const T* res, int C, int act) {
        BoardParams rest = bp;
        rest.row_order = 0;
        rest.c.w = L.w; rest.c.bias = L.bias; rest.c.res = nullptr; rest.c.act = kIdentity;
        rest.c.npos = r0; rest.c.num_pix_tiles = r1 - r0;  // (npos: the launch's first tile, conv_board_kernel)
        const int s0 = board_plan_.tile_first[r0], s1 = board_plan_.tile_first[r1];
        const ConvCost cost = conv_cost(geom_.off[s1] - geom_.off[s0], L.cin, L.cout, 9, false, sizeof(T));
        const auto fn = be->fn;
        const size_t lds = be->lds(board_plan_.npos);
        const int grid = (r1 - r0) * kts;
        if (timed(f, "conv3x3_tower", cost.flops, cost.bytes, [&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(512), lds, f.stream, rest); }))
            return -1;
        return se_unit(f, sq, ex, out, res, C, round_up(C, 32), act, s0, s1 - s0);
    }

    // A block's last 3x3 convolution with the squeeze-and-excitation unit that follows it inside the kernel
    // (conv_board.h).  Returns 1 when the fused kernel does not apply (the caller then runs conv + se_unit), 0 / -1.
    int conv_se(Fwd& f, const ConvLayerDev& L, const FcLayerDev& sq, const FcLayerDev& ex, const T* in, T* out, const T* res, int C, int act) {
        const BoardEntry* be = flags_.se_fused && route(L).board ? pick_board_se(board_plan_, L.ko_pad) : nullptr;
        if (!be || C > be->kot) return 1;
        const bool staged = sq.img16 && ex.img16;
        if (!staged && !se_l2_form_ok(sq.out, ex.out)) return 1;
        if constexpr (sizeof(T) != 2) return 1;
        // fused: a board too large to share a tile with another of its size (2 bs^2 > 384 pixel slots, i.e. bs >= 14), alone in
        // its tile; a smaller board ALWAYS goes through the separate kernels, also when it happens to sit alone in a tile
        const auto [f0, f1, r0, r1] = se_split(f, [](int bs) { return 2 * bs * bs > kBoardPT; });
        if (f1 <= f0) return 1;
        // (conv_board_se_kernel's tile is its workgroup id: chains_for_batch() keeps a network with this form to one chain)
        if (f0 > 0) return fail("chained forward: conv_board_se_kernel starts at tile 0");
        const BoardTabs* tabs = nullptr;
        if (board_tabs(f, &tabs)) return -1;
        BoardSeParams sp;
        std::memset(&sp, 0, sizeof(sp));  // padding too: the tower table is compared bytewise with its cached copy
        BoardParams& bp = sp.b;
        board_params(bp, board_plan_, tabs->src, tabs->pix, tabs->cols, flags_.arith);
        ConvParams& p = bp.c;
        conv_params(p, in, L.w, L.bias, res, out, dgeom(f.io), L.cin_s, L.cout_s, L.ko_pad, 9, act);
        p.npos = 0; p.num_pix_tiles = f.ntiles;
        se_stage_params(sp, sq.dev(), ex.dev(), C, staged ? sq.img16 : nullptr, staged ? ex.img16 : nullptr, sq.img_bytes, ex.img_bytes);
#ifdef SAYURI_EXPERIMENTS
        if (flags_.board_dbg < 0) {  // negative n: timeline of the n-th SE convolution of the forward
            if (!d_dbg_ && dev_alloc(&d_dbg_, 4 * 8 * 8)) return -1;
            if (++f.dbg_se_call == -flags_.board_dbg) { bp.dbg = d_dbg_; dbg_is_se_ = true; }
        }
#endif
        const ConvCost cost = conv_cost(f.px, L.cin, L.cout, 9, res, sizeof(T));
        const double flops = cost.flops + 2.0 * f.ns * ((double)sq.in * sq.out + (double)ex.in * ex.out);
        const bool to_run = r1 <= r0 && !f.chained && tower_ok(be->kot) && !bp.dbg;
        if (board_launch(f, "conv3x3_tower_se", L, be, be->fn, sp, true, to_run, f1 - f0, flops, cost.bytes)) return -1;
        // the small boards behind: be->kot covers the layer, one channel tile
        if (r1 > r0 && se_tail(f, L, sq, ex, be, bp, 1, r0, r1, out, res, C, act)) return -1;
        return 0;
    }

    // A block's last 3x3 convolution with its SE unit when the layer's channels are split over kts = 2..4 workgroups of 128
    // (conv_board_sx.h: the siblings exchange their partial squeeze sums inside the launch).  Returns 1 when the form does not apply
    // (the caller runs conv + se_unit), 0 / -1.  Fused: a board of which at most kSxMaxSub fit a tile (9x9 and larger), never a
    // smaller one.  Honours the tile range of a chained forward.
    int conv_sx(Fwd& f, const ConvLayerDev& L, const FcLayerDev& sq, const FcLayerDev& ex, const T* in, T* out, const T* res, int C, int act) {
        if constexpr (sizeof(T) != 2) return 1;
        if (!flags_.se_split || sx_disabled_ || !sq.sx_img || !ex.sx_img || !sx_kts_ || L.ko_pad != sx_kts_ * 128 || L.cout_s != L.ko_pad) return 1;
        if (!route(L).board) return 1;
        const BoardEntry* be = sx_board_entry(board_plan_.npos);
        if (!be) return 1;
        const auto [f0, f1, r0, r1] = se_split(f, sx_board_fused);
        if (!f.run.empty() && tower_flush(f)) return -1;
        const BoardTabs* tabs = nullptr;
        if (board_tabs(f, &tabs)) return -1;
        const unsigned epoch = f.sx_epoch0 + 1u + (unsigned)f.sx_idx++;
        BoardSxParams sp;
        std::memset(&sp, 0, sizeof(sp));
        BoardParams& bp = sp.b;
        board_params(bp, board_plan_, tabs->src, tabs->pix, tabs->cols, flags_.arith);
        ConvParams& p = bp.c;
        conv_params(p, in, L.w, L.bias, res, out, dgeom(f.io), L.cin_s, L.cout_s, L.ko_pad, 9, act);
        if (rows_use(f, p, "conv3x3_tower_sx")) return -1;
        const size_t lds = be->lds(board_plan_.npos);
        const int kts = sx_kts_;
        if (f1 > f0) {
            p.npos = f0; p.num_pix_tiles = f1 - f0;
            sx_params(sp, sq.sx_img, ex.sx_img, sq.sx_bytes, ex.sx_bytes, board_, sq.out, kts, f.io.sx_xchg, epoch, f.io.sx_err_dev, flags_.dbg_sx_stall);
            if (flags_.sx_dbg > 0 && profiling_ && f.sx_idx == flags_.sx_dbg) {
                if (!d_sxdbg_ && dev_alloc(&d_sxdbg_, 4 * 64)) return -1;
                sp.b.dbg = d_sxdbg_;
            }
            const int s0 = board_plan_.tile_first[f0], s1 = board_plan_.tile_first[f1];
            const ConvCost cost = conv_cost(geom_.off[s1] - geom_.off[s0], L.cin, L.cout, 9, res, sizeof(T));
            const double flops = cost.flops + 2.0 * (s1 - s0) * ((double)sq.in * sq.out + (double)ex.in * ex.out);
            const int grid = sx_grid(f1 - f0, kts);
            if (timed(f, "conv3x3_tower_sx", flops, cost.bytes, [&] { hipLaunchKernelGGL(conv_board_sx_kernel<2>, dim3(grid), dim3(512), lds, f.stream, sp); }))
                return -1;
        }
        if (r1 > r0 && se_tail(f, L, sq, ex, be, bp, kts, r0, r1, out, res, C, act)) return -1;
        return 0;
    }

    // A 3x3 layer of a latency context as many small workgroups (conv_split.h): one launch over the forward's samples, the
    // split chosen from the batch geometry and the forward's samples (split_plan; cached like the routes).
    int conv_split(Fwd& f, const char* name, const ConvLayerDev& L, const T* in, T* out, const T* res, int act) {
        const SplitPlan& sp = cached(split_cache_, PlanKey{L.ko_pad, 0, 0, f.n0, f.ns},
                                     [&] { return split_plan(geom_, f.n0, f.ns, L.ko_pad, flags_.latency_split, flags_.latency_ring); });
        if (!sp.ok) return fail(std::string("latency context, layer ") + name + ": " + sp.why);
        last_split_ring_ = std::max(last_split_ring_, sp.stages);
        SplitParams q;
        std::memset(&q, 0, sizeof(q));
        conv_params(q.c, in, L.w, L.bias, res, out, dgeom(f.io), L.cin_s, L.cout_s, L.ko_pad, 9, act);
        split_params(q, sp, f.n0);
        const ConvCost cost = conv_cost(f.px, L.cin, L.cout, 9, res, sizeof(T));
        return timed(f, name, cost.flops, cost.bytes, [&] { split_launch(sp, q, f.stream); });
    }

    // A tower 1x1 layer as many small workgroups (conv_pw.h): one launch over the forward's samples, the cut chosen from the batch
    // geometry (the route's PwPlan).  The bits of the generic kernel.
    int conv_pw(Fwd& f, const char* name, const ConvLayerDev& L, const PwPlan& pp, const T* in, T* out, const T* res, int act) {
        PwParams q;
        std::memset(&q, 0, sizeof(q));
        conv_params(q.c, in, L.w, L.bias, res, out, dgeom(f.io), L.cin_s, L.cout_s, L.ko_pad, 1, act);
        pw_params(q, pp, f.n0);
        ++last_pw_launches_;
        const ConvCost cost = conv_cost(f.px, L.cin, L.cout, 1, res, sizeof(T));
        return timed(f, name, cost.flops, cost.bytes, [&] { pw_launch(pp, q, f.stream); });
    }

    int conv(Fwd& f, const char* name, const ConvLayerDev& L, const T* in, T* out, const T* res, int act, bool tower_pw = false) {
        const ConvRoute& r = route(L, &f, tower_pw);
        if (r.family == kConvPw) return conv_pw(f, name, L, r.pw, in, out, res, act);
        if (r.family == kConvSplit) return conv_split(f, name, L, in, out, res, act);
        if (const BoardEntry* be = r.board) {
            const int bkt = r.tiles;
            const BoardTabs* tabs = nullptr;
            if (board_tabs(f, &tabs)) return -1;
            BoardSeParams sp;
            std::memset(&sp, 0, sizeof(sp));  // (what the tower table holds of a layer without SE unit)
            BoardParams& bp = sp.b;
            board_params(bp, board_plan_, tabs->src, tabs->pix, tabs->cols, flags_.arith);
            auto fn = be->fn;
#ifdef SAYURI_EXPERIMENTS
            if (be->kot == 256 && flags_.board_dbg > 0 && !strcmp(name, "conv3x3_tower")) {
                // in-kernel timeline of the SAYURI_BOARD_DBG-th tower convolution of the forward (1 = first)
                if (!d_dbg_ && dev_alloc(&d_dbg_, 4 * 8 * 8)) return -1;
                if (++f.dbg_call == flags_.board_dbg) {
                    bp.dbg = d_dbg_;
                    fn = &conv_board_kernel<4, true>;
                }
            }
#endif
            ConvParams& p = bp.c;
            conv_params(p, in, L.w, L.bias, res, out, dgeom(f.io), L.cin_s, L.cout_s, L.ko_pad, 9, act);
            p.npos = f.tile0; p.num_pix_tiles = f.ntiles;  // (npos: the launch's first tile, conv_board_kernel)
#ifdef SAYURI_EXPERIMENTS
            if (flags_.act_override >= 0) p.act = flags_.act_override;  // timing experiments only
#endif
            const ConvCost cost = conv_cost(f.px, L.cin, L.cout, 9, res, sizeof(T));
            const bool to_run = bkt == 1 && !f.chained && tower_ok(be->kot) && !bp.dbg;
            return board_launch(f, name, L, be, fn, sp, false, to_run, f.ntiles * bkt, cost.flops, cost.bytes);
        }
        if (f.chained) return fail(std::string("chained forward: layer ") + name + " has no board kernel");
        if (const GldsEntry* ge = r.glds) {
            const TileTabs* tabs = nullptr;
            if (tile_tabs(f, *ge, &tabs)) return -1;
            GldsParams gp;
            conv_params(gp.c, in, L.w, L.bias, res, out, dgeom(f.io), L.cin_s, L.cout_s, L.ko_pad, 9, act);
            const int grid = glds_params(gp, *ge, tabs->src, tabs->pix, d_zeros_, r.tiles);
            const ConvCost cost = conv_cost(geom_.total, L.cin, L.cout, 9, res, sizeof(T));
            const auto fn = ge->fn;
            const size_t lds = ge->lds;
            return timed(f, name, cost.flops, cost.bytes, [&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(512), lds, f.stream, gp); });
        }
        const int kot = L.wmt * 32, kot_tiles = L.ko_pad / kot;
        TileChoice<T> tc;
        if (choose_tile(L.wmt, kot_tiles, &tc)) return -1;
        ConvParams p;
        conv_params(p, in, L.w, L.bias, res, out, dgeom(f.io), L.cin_s, L.cout_s, L.ko_pad, L.k * L.k, act);
        p.npos = tc.npos; p.num_pix_tiles = tc.ntiles;
        const ConvCost cost = conv_cost(geom_.total, L.cin, L.cout, p.taps, res, sizeof(T));
        const auto fn = tc.e->fn;
        const size_t lds = tc.e->lds(tc.npos);
        const int grid = tc.ntiles * kot_tiles;
        return timed(f, name, cost.flops, cost.bytes, [&] { hipLaunchKernelGGL(fn, dim3(grid), dim3(512), lds, f.stream, p); });
    }

    // A depthwise layer (a mixer block's DW_CONV, the RepLK head's P_DW_CONV).  The one place that chooses its kernel: conv_dw.h
    // (LDS staging, many small workgroups; the plan is dw_plan's for the forward's samples) in the fp16 engine for k = 3, 5, 7
    // where the plan fits and dw_pays says it pays, depthwise_kernel otherwise -- the fp32 engine, another k, a plan that does
    // not fit.  SAYURI_DW=0 / 1 force a kernel.  The rule decides speed only: the bits are the same either way.
    int depthwise(Fwd& f, const char* name, const ConvLayerDev& L, const T* in, T* out, const T* res, int act) {
        const double flops = 2.0 * f.px * L.cout * L.k * L.k, bytes = sizeof(T) * f.px * L.cout * (res ? 3 : 2);
        if constexpr (sizeof(T) == 2) {
            if (flags_.dw != 0) {
                const DwPlan& dp = cached(dw_cache_, PlanKey{L.cout_s, L.k, 0, f.n0, f.ns},
                                          [&] { return dw_plan(geom_, f.n0, f.ns, L.cout_s, L.k, flags_.dw_strips); });
                if (!dp.ok && flags_.dw_strips && !dw_refusal_said_) {  // a forced cut that is refused must not pass for a measurement of it
                    dw_refusal_said_ = true;
                    std::fprintf(stderr, "[sayuri_hip] SAYURI_DW_STRIPS=%d: %s: the layer keeps depthwise_kernel\n", flags_.dw_strips, dp.why.c_str());
                }
                if (dp.ok && (flags_.dw == 1 || dw_pays())) {
                    DwParams q;
                    std::memset(&q, 0, sizeof(q));
                    q.x = in; q.res = res; q.out = out; q.wt = (const float*)L.w; q.bias = L.bias;
                    q.g = dgeom(f.io); q.C = L.cout; q.cs = L.cout_s; q.act = act;
                    dw_params(q, dp, f.n0);
                    ++last_dw_launches_;
                    return timed(f, name, flops, bytes, [&] { dw_launch(dp, q, f.stream); });
                }
            }
        }
        const int EPP = ElemTraits<T>::kPieceElems;
        const size_t total = (size_t)geom_.total * (L.cout_s / EPP);
        const int grid = (int)((total + 255) / 256);
        const double px = geom_.total;
        const BatchGeom g = dgeom(f.io);
        return timed(f, name, 2.0 * px * L.cout * L.k * L.k, sizeof(T) * px * L.cout * (res ? 3 : 2), [&] {
            hipLaunchKernelGGL(depthwise_kernel<T>, dim3(grid), dim3(256), 0, f.stream, in, res, out,
                               (const float*)L.w, (const float*)L.bias, g, L.cout, L.cout_s, L.k, act);
        });
    }

    // The unit on the samples [n0, n0 + ns) of the batch.  The one place that chooses its form: se_pool / se_fc / se_scale, or
    // one launch (se_unit_kernel) of `parts` workgroups per sample (se_unit_parts: a piece per thread within one round of the
    // CUs).  The rule decides speed only: the bits are the same either way.  SAYURI_SE_ONE=1 / 0 force a form; unset, a latency
    // context takes the one launch when the scale phase of every workgroup is a single pass (kScaleUnroll x kSeFcThreads
    // pieces) -- measured in DESIGN.md Kernel 1g: with more passes on one CU the unit loses more than its two launches save.
    // For full 19x19 boards that is up to 85 boards on 256 channels (11552 pieces, parts >= 3) and up to 51 on 384 (17328
    // pieces, parts >= 5); a call that cannot split (parts == 1: no residual, a sample range) qualifies up to 11x11 / 9x9.
    // Several workgroups per sample cannot write x (a sibling still pools it): `into_res`, when the caller passes it, allows
    // the result in the residual's buffer `res_rw` instead and says whether it went there; the forward's whole batch only.
    int se_unit(Fwd& f, const FcLayerDev& sq, const FcLayerDev& ex, T* x, const T* res, int C, int cs, int act, int n0, int ns,
                T* res_rw = nullptr, bool* into_res = nullptr) {
        const double px = geom_.off[n0 + ns] - geom_.off[n0];
        if (into_res) *into_res = false;
        if (flags_.se_one < 0 ? flags_.latency : flags_.se_one != 0) {
            int max_pieces = 0;
            for (int i = n0; i < n0 + ns; ++i) max_pieces = std::max(max_pieces, geom_.bsz[i] * geom_.bsz[i] * (cs / ElemTraits<T>::kPieceElems));
            const bool may_split = into_res && res_rw && res_rw == res && n0 == 0 && ns == geom_.n;
            const int parts = may_split ? se_unit_parts(max_pieces, ns) : 1;
            const bool one_pass = (max_pieces + parts - 1) / parts <= kScaleUnroll * kSeFcThreads;
            if (flags_.se_one > 0 || one_pass) {
                const int rc = se_unit_one_launch<T>(f.stream, dgeom(f.io), px, (const T*)x, res, parts > 1 ? res_rw : x, parts, f.io.gate, sq.dev(),
                                                     ex.dev(), C, cs, act, n0, ns,
                                                     [&](const char* name, double flops, double bytes, auto&& launch) { return timed(f, name, flops, bytes, launch); });
                if (rc == 0 && parts > 1) *into_res = true;
                if (rc != 1) return rc;
            }
        }
        return se_unit_launches<T>(f.stream, dgeom(f.io), px, x, res, f.io.separt, f.io.gate, sq.dev(), ex.dev(), C, cs, act, n0, ns,
                                   [&](const char* name, double flops, double bytes, auto&& launch) { return timed(f, name, flops, bytes, launch); });
    }

    // -------------------------------------------------------------- who may write which bytes when (the buffer table)
    // Launches on one stream are ordered grid-wide; the layers INSIDE a persistent tower run are not (a workgroup walks the
    // whole run on its own clock), and neither are the chains of a chained forward (streams of their own).  In such an
    // UNORDERED SCOPE the only order is "this workgroup's / this chain's earlier layers", so a buffer may be written while
    // other workgroups still have to read it -- sound exactly when the bytes a tile touches in a buffer are the same in every
    // layer of the scope, i.e. when the buffer has ONE ROW STRIDE throughout it (a tile is whole samples, a sample's rows
    // start at sample * slot_pix * stride):
    //
    //   buffer                    written by                     row stride              may be recycled
    //   ------------------------  -----------------------------  ----------------------  ------------------------------------------
    //   `in` (packed input)       pack_bits / pack_input         input conv's cin_s (64) never inside the forward (kept to its end)
    //   pool buffers x, y, t0...  the convolution they are `out` the tower's cout_s      as soon as the layer that reads them is
    //                             of (epilogue, own tile's rows)  (256 / 384 / 128)        appended: give() -> take(), SAME stride only
    //   ... the block's skip      se_unit_kernel with parts > 1   the same                 never by the unit: it becomes the block's
    //                             (the unit's result, in place                             output (forward_graph's in_skip) and the
    //                             of the residual it has read)                             convolution's buffer y goes back instead
    //   io.separt, io.gate        se_pool / se_fc, per sample     per-sample records      per sample, inside its chain
    //                             (se_unit_kernel: io.gate only,
    //                             its partials stay in LDS)
    //   se_xchg (384-ch SE)       the sibling channel tiles       per (tile, channel tile) next SE layer (tagged with the layer's epoch)
    //   io.prob ... io.own        the heads kernel                per sample              by the ticket's next submit
    //
    // rounds 3-4 broke the first line (the input's buffer went back to the pool and came out again as a block's output with
    // stride 256: a late workgroup's input lay under an early workgroup's third layer).  The table below is that rule as a
    // run-time check: every use of a pool buffer inside an unordered scope names its stride, and a second stride is refused.
    // It spans every chain of a chained forward (forward() resets it once).
    int rows_stride_[kNumBufs] = {};          // 0: not used yet in the current scope
    const char* rows_first_[kNumBufs] = {};   // the layer that fixed it
    void rows_reset() {
        for (int i = 0; i < kNumBufs; ++i) rows_stride_[i] = 0;
    }
    // the buffers of one layer: `in` with its cin_s, `out` and `res` with its cout_s
    int rows_use(const Fwd& f, const ConvParams& p, const char* layer) {
        const void* use[3] = {p.in, p.out, p.res};
        for (int u = 0; u < 3 && flags_.dbg_recycle_input < 2; ++u)
            for (int i = 0; i < kNumBufs; ++i) {
                if (!use[u] || f.io.bufs[i] != use[u]) continue;
                const int stride = u ? p.cout_s : p.cin_s;
                if (rows_stride_[i] && rows_stride_[i] != stride)
                    return fail(std::string("activation buffer ") + std::to_string(i) + " is used with row stride " + std::to_string(stride) + " by " +
                                layer + " and with " + std::to_string(rows_stride_[i]) + " by " + (rows_first_[i] ? rows_first_[i] : "?") +
                                " inside one persistent run / chained forward: the rows of different tiles would overlap");
                rows_stride_[i] = stride;
                rows_first_[i] = layer;
            }
        return 0;
    }

    // the live weight set's layers: the one way the launch code reaches a weight
    const ConvLayerDev& cv(int id) const { return live_->convs.at(id); }
    const FcLayerDev& fc(int id) const { return live_->fcs.at(id); }

    // -------------------------------------------------------------- the graph
    // One forward of ticket t's batch: as ONE chain of launches on the ticket's compute stream, or -- chains_for_batch() -- as
    // G chains over G ranges of tiles on G streams, forked from and joined to that stream by events (the activations, tables
    // and outputs of the ranges are disjoint: a tile is whole samples).  zc_pass / zc_misc: see submit().
    int forward(int t, float* zc_pass = nullptr, float* zc_misc = nullptr) {
        const int G = chains_for_batch();
        last_chains_ = G;
        last_split_ring_ = 0;
        last_pw_launches_ = 0;
        last_dw_launches_ = 0;
        rows_reset();
        IoSlot& io = io_[t];
        Fwd f{t, io, compute_[t]};
        f.ntiles = plan().ntiles;
        f.ns = geom_.n;
        f.px = geom_.total;
        f.pass = zc_pass ? zc_pass : io.pass;
        f.misc = zc_misc ? zc_misc : io.misc;
        if (sx_kts_) {
            int nse = 0;
            for (const auto& b : blocks_) nse += b.apply_se ? 1 : 0;
            if (io.sx_epoch > 0xfff00000u) {  // tags about to wrap: start over on a clean buffer (stream order: behind the last readers)
                HIP_OK(hipMemsetAsync(io.sx_xchg, 0, sizeof(unsigned long long) * (size_t)max_batch_ * sx_kts_ * kSxMaxSub * kSxSlots, f.stream));
                io.sx_epoch = 0;
            }
            f.sx_epoch0 = io.sx_epoch;
            io.sx_epoch += (unsigned)nse;
        }
        if (G <= 1) return forward_graph(f);
        if (chain_setup(G)) return -1;
        const BoardTabs* tabs = nullptr;
        if (board_tabs(f, &tabs)) return -1;  // built on the ticket's stream, in front of the fork
        HIP_OK(hipEventRecord(chain_fork_, f.stream));
        const int nt = board_plan_.ntiles;
        for (int g = 0; g < G; ++g) {
            Fwd c = f;  // (nothing of f's layer-to-layer state is used yet)
            c.stream = chain_stream_[g];
            c.chained = true;
            c.tile0 = (int)((long)nt * g / G);
            c.ntiles = (int)((long)nt * (g + 1) / G) - c.tile0;
            c.n0 = board_plan_.tile_first[c.tile0];
            c.ns = board_plan_.tile_first[c.tile0 + c.ntiles] - c.n0;
            c.px = geom_.off[c.n0 + c.ns] - geom_.off[c.n0];
            hipError_t e = hipStreamWaitEvent(c.stream, chain_fork_, 0);
            if (flags_.chains_serial && g > 0 && e == hipSuccess) e = hipStreamWaitEvent(c.stream, chain_join_[g - 1], 0);
            if (e == hipSuccess && forward_graph(c)) return -1;
            if (e == hipSuccess) e = hipEventRecord(chain_join_[g], c.stream);
            if (e != hipSuccess) return fail(std::string("chained forward: ") + hipGetErrorString(e));
        }
        for (int g = 0; g < G; ++g) HIP_OK(hipStreamWaitEvent(f.stream, chain_join_[g], 0));
        return 0;
    }

    // The batch's planes or packed records -> the input convolution's layout in buffer `in`, for the samples of f.
    int pack_input(Fwd& f, T* dst) {
        const int cin = desc_.input_channels, cs = cv(SAYURI_L_INPUT_CONV).cin_s, board = board_;
        const int n0 = f.n0, ns = f.ns;
        const double px = f.px;
        const BatchGeom g = dgeom(f.io);
        const IoSlot& io = f.io;
        // (which kernel, its workgroups per sample -- one for records read across PCIe --, chunk and LDS: pack_plan, engine_plan.h)
        const bool records = io.packed_binary > 0;
        const PackPlan pl = pack_plan(sizeof(T), cin, cs, board, records, io.symm_on, io.packed_src != nullptr);
        PackSource in;
        in.planes = (const float*)io.planes;
        in.records = io.packed_src ? io.packed_src : io.packed;
        in.nbin = io.packed_binary;
        in.src_map = io.sy_src; in.symm_map = io.sy_symm;
        const double bytes_in = records ? (double)ns * (in.nbin * kPackedWords + kPackedScalars) * 4 : px * cin * 4;
        return timed(f, "pack_input", 0, bytes_in + px * cs * sizeof(T), [&] { pack_launch<T>(pl, f.stream, in, dst, g, cin, cs, board, io.g_perm, n0, ns); });
    }

    int forward_graph(Fwd& f) {
        const auto& d = desc_;
        const int C = d.residual_channels, csC = round_up(C, 32), act = d.default_act;
        T* const* buf = f.io.bufs;

        int x = f.take();
        const int in = f.take();
        if (pack_input(f, buf[in])) return -1;
        if (conv(f, "conv3x3_input", cv(SAYURI_L_INPUT_CONV), buf[in], buf[x], nullptr, act)) return -1;
        if (flags_.dbg_recycle_input) f.give(in);  // SAYURI_DEBUG_RECYCLE_INPUT: rounds 3-4's hand-back, to show what catches it
        // `in` is NOT handed back: it stays the packed input's buffer for the whole forward.  Its rows have the input
        // convolution's channel stride (64), every later buffer the tower's (256 / 384): recycled as a block's output, sample
        // m's rows would lie on top of sample n's packed input.  With a kernel boundary between every two layers and one
        // stream that is harmless.  Inside the persistent launch it is not -- a workgroup's layers follow one another with no
        // grid-wide order, and a workgroup that STARTS LATE (more tiles than CUs, or the chip shared with another ticket's
        // kernels) found its packed input overwritten by an early workgroup's third layer -- and across the chains of one
        // forward neither.  Rounds 3-4 recycled it: every full-chip launch won that race by a wide margin (all 256 workgroups
        // start together, the input is read within the first ~80 us and overwritten after ~170), which is why it took round
        // 5's bit-level harness to see it (tools/gpu/concurrent_ctx_dbg.py, chains_layers_dbg.py).

        for (int b = 0; b < d.residual_blocks; ++b) {
            const auto& bd = blocks_[b];
            const bool se = bd.apply_se != 0;
            const int last_act = se ? (int)kIdentity : act;
            const int y = f.take();
            int skip = x;  // buffer added back at the end of the block
            bool se_done = false;  // the SE unit already ran inside the block's last convolution
            if (bd.type == SAYURI_BLOCK_RESIDUAL) {
                const int t0 = f.take();
                if (conv(f, "conv3x3_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV1)), buf[x], buf[t0], nullptr, act)) return -1;
                int fused = 1;
                if (se) {
                    fused = conv_se(f, cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2)), fc(SAYURI_L_BLOCK(b, SAYURI_S_SQUEEZE)),
                                    fc(SAYURI_L_BLOCK(b, SAYURI_S_EXCITE)), buf[t0], buf[y], buf[x], C, act);
                    if (fused == 1)
                        fused = conv_sx(f, cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2)), fc(SAYURI_L_BLOCK(b, SAYURI_S_SQUEEZE)),
                                        fc(SAYURI_L_BLOCK(b, SAYURI_S_EXCITE)), buf[t0], buf[y], buf[x], C, act);
                    if (fused < 0) return -1;
                    se_done = fused == 0;
                }
                if (fused == 1 &&
                    conv(f, "conv3x3_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2)), buf[t0], buf[y], se ? nullptr : buf[x], last_act))
                    return -1;
                f.give(t0);
            } else if (bd.type == SAYURI_BLOCK_BOTTLENECK) {
                const int t0 = f.take(), t1 = f.take();
                if (conv(f, "conv1x1_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_PRE_BTL)), buf[x], buf[t0], nullptr, act, true)) return -1;
                if (conv(f, "conv3x3_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV1)), buf[t0], buf[t1], nullptr, act)) return -1;
                if (conv(f, "conv3x3_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2)), buf[t1], buf[t0], nullptr, act)) return -1;
                if (conv(f, "conv1x1_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_POST_BTL)), buf[t0], buf[y], se ? nullptr : buf[x], last_act, true)) return -1;
                f.give(t0); f.give(t1);
            } else if (bd.type == SAYURI_BLOCK_NESTED_BOTTLENECK) {
                const int r1 = f.take(), t0 = f.take(), t1 = f.take();
                if (conv(f, "conv1x1_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_PRE_BTL)), buf[x], buf[r1], nullptr, act, true)) return -1;
                if (conv(f, "conv3x3_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV1)), buf[r1], buf[t0], nullptr, act)) return -1;
                if (conv(f, "conv3x3_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2)), buf[t0], buf[t1], buf[r1], act)) return -1;
                if (conv(f, "conv3x3_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV3)), buf[t1], buf[t0], nullptr, act)) return -1;
                if (conv(f, "conv3x3_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV4)), buf[t0], buf[r1], buf[t1], act)) return -1;
                if (conv(f, "conv1x1_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_POST_BTL)), buf[r1], buf[y], se ? nullptr : buf[x], last_act, true)) return -1;
                f.give(r1); f.give(t0); f.give(t1);
            } else {  // mixer: x' = act(dw(x)+b) + x is the new skip
                const int s2 = f.take(), t1 = f.take();
                if (depthwise(f, "depthwise", cv(SAYURI_L_BLOCK(b, SAYURI_S_DW_CONV)), buf[x], buf[s2], buf[x], act)) return -1;
                if (conv(f, "conv1x1_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV1)), buf[s2], buf[t1], nullptr, act, true)) return -1;
                if (conv(f, "conv1x1_tower", cv(SAYURI_L_BLOCK(b, SAYURI_S_CONV2)), buf[t1], buf[y], se ? nullptr : buf[s2], last_act, true)) return -1;
                f.give(t1);
                f.give(x);
                x = s2;
                skip = s2;
            }
            // skip == x in every block type here (the mixer sets both to s2), so a result left in the skip's buffer is a result in x
            bool in_skip = false;  // the one-launch SE unit left the block's output in the skip's buffer (se_unit)
            if (se && !se_done) {
                if (se_unit(f, fc(SAYURI_L_BLOCK(b, SAYURI_S_SQUEEZE)), fc(SAYURI_L_BLOCK(b, SAYURI_S_EXCITE)), buf[y], buf[skip], C, csC,
                            act, f.n0, f.ns, buf[skip], &in_skip))
                    return -1;
            }
            if (in_skip) {
                f.give(y);
            } else {
                f.give(x);
                x = y;
            }
        }
        return heads(f, x);
    }

    // Both heads on the trunk in buffer x: head_board_kernel, one workgroup per sample, or the separate head kernels.
    int heads(Fwd& f, int x) {
        const auto& d = desc_;
        const int C = d.residual_channels, csC = round_up(C, 32), act = d.default_act;
        const int Cp = d.policy_head_channels, Cv = d.value_head_channels;
        T* const* buf = f.io.bufs;
        const BatchGeom g = dgeom(f.io);
        const ConvLayerDev &pw = cv(SAYURI_L_PROB_CONV), &ow = cv(SAYURI_L_V_OWNERSHIP);
        const HeadWeights hw{fc(SAYURI_L_P_INTER_FC).dev(), fc(SAYURI_L_PASS_FC).dev(), fc(SAYURI_L_V_INTER_FC).dev(), fc(SAYURI_L_V_MISC).dev(),
                             pw.w32, pw.bias, ow.w32, ow.bias};
        const HeadParams h = head_params(hw, Cp, Cv, d.probabilities_channels, act, board_, f.io.prob, f.pass, f.misc, f.io.own, f.io.g_perm);
        if (live_->head_img && flags_.heads_fused) {
            // both heads of a sample in one workgroup: trunk -> LDS -> stacked 1x1 convolution on the matrix cores -> pooling,
            // FCs and the per-pixel planes (head_board.h)
            HeadBoardParams hp;
            hp.dbg = nullptr;
#ifdef SAYURI_EXPERIMENTS
            if (flags_.heads_dbg) {
                if (!d_hdbg_ && dev_alloc(&d_hdbg_, 4 * 8)) return -1;
                hp.dbg = d_hdbg_;
            }
#endif
            hp.trunk = buf[x]; hp.w = live_->head_img; hp.w2 = live_->head_img2; hp.bias = live_->head_bias; hp.g = g; hp.cs = csC; hp.PT = live_->head_pt; hp.VT = live_->head_vt; hp.h = h;
            hp.n0 = f.n0;
            const auto fn = live_->head_fn;
            const int ns = f.ns;
            return timed(f, "heads_fused", 2.0 * f.px * C * (Cp + Cv), f.px * csC * 2, [&] {
                hipLaunchKernelGGL(fn, dim3(ns), dim3(512), kMaxLds, f.stream, hp);
            });
        }
        if (f.chained) return fail("chained forward reached the separate head kernels");
        int pb = f.take();
        const int vb = f.take();
        if (conv(f, "conv1x1_head", cv(SAYURI_L_P_HD_CONV), buf[x], buf[pb], nullptr, act)) return -1;
        if (d.policy_head_type == 1) {
            const int p2 = f.take();
            if (depthwise(f, "depthwise", cv(SAYURI_L_P_DW_CONV), buf[pb], buf[p2], nullptr, act)) return -1;
            if (conv(f, "conv1x1_head", cv(SAYURI_L_P_PT_CONV), buf[p2], buf[pb], nullptr, act)) return -1;
            f.give(p2);
        }
        if (conv(f, "conv1x1_head", cv(SAYURI_L_V_HD_CONV), buf[x], buf[vb], nullptr, act)) return -1;
        const int maxc = std::max(Cp, Cv);
        const size_t smem = sizeof(float) * (7 * maxc + 512);
        const T* pc = buf[pb];
        const T* vc = buf[vb];
        return timed(f, "head_tail", 0, 0, [&] {
            hipLaunchKernelGGL(head_tail_kernel<T>, dim3(2 * geom_.n), dim3(256), smem, f.stream, pc, vc, g, h);
        });
    }

    // -------------------------------------------------------------- the persistent tower launch (conv_tower.h)
    // Consecutive board convolutions whose channel tile covers the layer are not launched one by one: conv() / conv_se()
    // append them to f.run, and the first launch of anything else (timed()) -- in practice the heads -- sends the whole run
    // as ONE launch that walks a table of TowerLayer in device memory.  The table of a slot is re-uploaded only when its
    // contents change (another batch geometry; the buffers and weights of a slot never move).
    static constexpr int kTowerCap = 512;  // table elements per slot
    struct TowerSlot {
        TowerLayer* dev = nullptr;
        TowerLayer* stage[2] = {nullptr, nullptr};  // pinned staging, alternating
        hipEvent_t staged[2] = {nullptr, nullptr};   // the last copy out of stage[i]
        int next_stage = 0;
        std::vector<TowerLayer> cache;               // what dev holds
    };
    int tower_load() { return load_tower_module(&tower_mod_, tower_fn_); }
    bool tower_ok(int kot) const { return tower_mod_ && !profiling_ && (kot == 256 || kot == 128); }
    int tower_append(Fwd& f, int kot, const BoardSeParams& sp, bool has_se, double flops, double bytes) {
        if (!f.run.empty() && (f.run_kot != kot || (int)f.run.size() + f.table_used >= kTowerCap) && tower_flush(f)) return -1;
        if (f.run.empty()) { f.run_kot = kot; f.run_flops = f.run_bytes = 0; }
        f.run.push_back(tower_element(sp, has_se));
        f.run_flops += flops;
        f.run_bytes += bytes;
        return 0;
    }
    int tower_flush(Fwd& f) {
        std::vector<TowerLayer> run;
        run.swap(f.run);  // timed() below must not see a pending run
        TowerSlot& ts = tower_[f.t];
        if (!ts.dev) {
            if (dev_alloc(&ts.dev, kTowerCap)) return -1;
            for (int i = 0; i < 2; ++i) {
                HIP_OK(hipHostMalloc((void**)&ts.stage[i], sizeof(TowerLayer) * kTowerCap, hipHostMallocDefault));
                HIP_OK(hipEventCreateWithFlags(&ts.staged[i], hipEventDisableTiming));
            }
            ts.cache.assign(kTowerCap, TowerLayer{});
        }
        const int n = (int)run.size(), first = f.table_used;
        if (first + n > kTowerCap) return fail("tower table overflow");
        if (flags_.tower_noepi_after >= 0 && tower_launches_++ >= flags_.tower_noepi_after)
            for (auto& t : run)
                if (t.sp.b.row_order == 1 && !t.has_se) t.sp.b.row_order = 3;  // MEASURING: no epilogue (tower_seam.py epi_hook)
        (void)tower_link(run, ts.dev + first, flags_.tower_chain);  // self, last, the weight hand-over (engine_plan.h)
        if (std::memcmp(run.data(), ts.cache.data() + first, sizeof(TowerLayer) * n) != 0) {
            const int st = ts.next_stage;
            ts.next_stage ^= 1;
            HIP_OK(hipEventSynchronize(ts.staged[st]));  // the copy that last read this staging area (never recorded: returns at once)
            std::memcpy(ts.stage[st], run.data(), sizeof(TowerLayer) * n);
            HIP_OK(hipMemcpyAsync(ts.dev + first, ts.stage[st], sizeof(TowerLayer) * n, hipMemcpyHostToDevice, f.stream));
            ++table_uploads_;
            HIP_OK(hipEventRecord(ts.staged[st], f.stream));
            std::memcpy(ts.cache.data() + first, run.data(), sizeof(TowerLayer) * n);
        }
        f.table_used += n;
        const hipFunction_t fn = tower_fn_[f.run_kot == 256 ? 0 : 1];
        const TowerLayer* arg = ts.dev + first;
        const int grid = board_plan_.ntiles;
        hipError_t lrc = hipSuccess;
        if (flags_.tower_sync) HIP_OK(hipStreamSynchronize(f.stream));
        const int rc = timed(f, "tower_run", f.run_flops, f.run_bytes, [&] {
            void* params[] = {(void*)&arg};
            lrc = hipModuleLaunchKernel(fn, grid, 1, 1, 512, 1, 1, 0, f.stream, params, nullptr);
        });
        if (flags_.tower_sync && lrc == hipSuccess) HIP_OK(hipStreamSynchronize(f.stream));
        if (lrc != hipSuccess) return fail(std::string("hipModuleLaunchKernel(conv_tower_kernel): ") + hipGetErrorString(lrc));
        return rc;
    }
    // conv_board_sx.h (SE units of layers split over channel tiles)
    int sx_kts_ = 0;                      // channel tiles per layer (0: the network has no such unit)
    bool sx_disabled_ = false;            // set by sx_check(): the exchange timed out once on this ctx
    // ticket t's forwards: did a split SE workgroup's wait for its siblings run out (IoSlot::sx_err_host)?
    int sx_check(int t) {
        unsigned* err = io_[t].sx_err_host;
        if (err && *(volatile unsigned*)err) {
            const unsigned e = *(volatile unsigned*)err;
            *(volatile unsigned*)err = 0;
            sx_disabled_ = true;  // this ctx goes on with the separate kernels: a wait that ran out once is not tried again
            return fail("SE exchange between the channel tiles of a board tile timed out (epoch " + std::to_string(e) +
                        "): the results of this forward are invalid; from here on this context runs the unit as separate kernels (SAYURI_SE_SPLIT=0)");
        }
        return 0;
    }
    EngineFlags flags_;
    hipModule_t tower_mod_ = nullptr;
    hipFunction_t tower_fn_[2] = {nullptr, nullptr};
    TowerSlot tower_[2];
    long tower_launches_ = 0;
    int table_uploads_ = 0;
    // SAYURI_HIP_FWDSTAT: device time of the forwards sent through submit(), by batch-size class
    hipEvent_t fs_ev_[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    double fs_d2h_ms_ = 0, fs_d2h_max_ = 0;
    long fs_d2h_slow_ = 0;
    bool fs_pending_[2] = {false, false};
    int fs_n_[2] = {0, 0};
    double fs_ms_[3] = {0, 0, 0};
    long fs_cnt_[3] = {0, 0, 0}, fs_uploads_ = 0;

    int device_;
    sayuri_hip_netdesc desc_;
    std::vector<sayuri_hip_blockdesc> blocks_;
    int max_batch_, board_;
    int cs_max_ = 32, slot_pix_ = 0;
    std::unique_ptr<WeightSet> live_;    // what forwards read (mu_)
    std::unique_ptr<WeightSet> staged_;  // an open reload's set (reload_mu_)
    std::vector<Retired> retired_;       // replaced sets whose last forwards may still run (mu_)
    std::atomic<int> n_retired_{0}, generation_{0};
    std::atomic<size_t> staged_bytes_{0};  // device bytes of the staged set (updated when a prepare ends, a reload closes)
    std::atomic<bool> measuring_{false};
    std::mutex mu_;         // everything that enqueues a forward, and a reload's commit
    std::mutex reload_mu_;  // the staged set; taken before mu_ where both are
    bool finalized_ = false, have_batch_ = false, profiling_ = false;
    hipStream_t h2d_stream_ = nullptr, d2h_stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    hipEvent_t h2d_done_[2] = {nullptr, nullptr}, fwd_done_[2] = {nullptr, nullptr};
    IoSlot io_[2];
    hipStream_t compute_[2] = {nullptr, nullptr};  // each ticket's forwards (init())
    bool inorder_ = false;  // a ticket's copies on the ticket's compute stream (init(), submit())
    DevPool work_;  // workspaces, tables, i/o buffers: everything that is not a weight
    std::vector<int> perm_;  // device sample -> caller's slot (enqueue_inputs)
    float* d_zeros_ = nullptr;
    int* h_symm_ = nullptr;  // pinned 2-slot ring: [slot][src(max_batch) | symm(max_batch)] (allocated with the first SymmReq batch)
    int symm_slot_ = 0;
    int* h_geom_ = nullptr;  // pinned 2-slot ring: [slot][off(max_batch+1) | bsz(max_batch) | perm(max_batch)]
    int geom_slot_ = 0, next_ticket_ = 0;
    hipEvent_t tick_ev_[2] = {nullptr, nullptr};
    HostGeom geom_;
    std::vector<int> prev_bsz_;
    // for the current batch geometry (forget_geometry); a plan for a sample range has the range in its key
    std::map<PlanKey, ConvRoute> route_cache_;  // by (k, ko_pad) -- a tower 1x1 that may take conv_pw.h: by (-1, cin, cout) and the range
    std::map<PlanKey, DwPlan> dw_cache_;        // by (cs, k) and the range
    std::map<PlanKey, SplitPlan> split_cache_;  // latency context: by ko_pad and the range
    BoardPlan board_plan_;
    unsigned long long* d_hdbg_ = nullptr;  // SAYURI_HEADS_DBG timeline of head_board_kernel
    unsigned long long* d_dbg_ = nullptr;  // SAYURI_BOARD_DBG timeline of one tower convolution
    unsigned long long* d_sxdbg_ = nullptr;  // SAYURI_SX_DBG timeline of one split SE convolution
    bool dbg_is_se_ = false;
    bool board_plan_valid_ = false;
    std::map<PlanKey, TileChoice<T>> tile_cache_;  // by (wmt, channel tiles)
    std::map<std::string, Stat> stats_;
    // light per-launch timing of one kernel class inside time_runs()
    bool light_ = false;
    std::string light_name_;
    int light_group_ = 1;            // launches of the marked class bracketed by one event pair
    std::vector<int> group_counts_;  // launches inside each pair of the last time_runs
    bool group_open_ = false;
    std::vector<hipEvent_t> pool_;
    size_t pool_used_ = 0;
    double light_flops_ = 0, light_bytes_ = 0;
    Stat timed_stat_;

};

}  // namespace sayuri
