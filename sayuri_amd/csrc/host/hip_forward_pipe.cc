// hip_forward_pipe.cc -- see hip_forward_pipe.h.
#include "hip_forward_pipe.h"
#include "fiber.h"

#include <dlfcn.h>
#include <pthread.h>
#include <algorithm>
#include <chrono>
#include <cstring>
#include <exception>
#include <stdexcept>

#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <climits>

#include "../../../include/sayuri_hip.h"

SAYURI_HOST_BEGIN

#ifndef SAYURI_IN_TREE
std::string NetworkForwardPipe::GetName() const { return Valid() ? weights_->name : "random"; }
int NetworkForwardPipe::GetVersion() const { return Valid() ? weights_->version : -1; }
#endif

namespace {

// Completion is a per-request 32-bit flag; blocked callers sleep in the kernel on that word
// (futex) instead of polling, so hundreds of waiting search threads leave the host cores to
// the pump thread and the encoder.  (The reference parks each caller on its own heap-allocated
// mutex + condition variable, batch_forward_pipe.cc:35-46.)
static_assert(sizeof(std::atomic<int>) == sizeof(int), "futex needs a plain 32-bit word");
inline void FutexWait(std::atomic<int>* w, int expected) {
    syscall(SYS_futex, reinterpret_cast<int*>(w), FUTEX_WAIT_PRIVATE, expected, nullptr, nullptr, 0);
}
inline void FutexWakeAll(std::atomic<int>* w) {
    syscall(SYS_futex, reinterpret_cast<int*>(w), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}

[[noreturn]] void ThrowHip(const char* what) {
    throw std::runtime_error(std::string(what) + ": " + sayuri_hip_last_error());
}
[[noreturn]] void ThrowBatchFailed() { throw std::runtime_error("HIP forward pipe failed while evaluating a batch"); }

using Clock = std::chrono::steady_clock;
inline long long Ns(Clock::duration d) { return std::chrono::duration_cast<std::chrono::nanoseconds>(d).count(); }

void LoadConv(sayuri_hip_ctx* ctx, int id, ConvLayer& c) {
    if (sayuri_hip_load_tensor(ctx, id, SAYURI_T_WEIGHTS, c.GetWeights().data(), c.GetWeights().size()) ||
        sayuri_hip_load_tensor(ctx, id, SAYURI_T_BIASES, c.GetBiases().data(), c.GetBiases().size()))
        ThrowHip("sayuri_hip_load_tensor");
}
void LoadFc(sayuri_hip_ctx* ctx, int id, LinearLayer& f) {
    if (sayuri_hip_load_tensor(ctx, id, SAYURI_T_WEIGHTS, f.GetWeights().data(), f.GetWeights().size()) ||
        sayuri_hip_load_tensor(ctx, id, SAYURI_T_BIASES, f.GetBiases().data(), f.GetBiases().size()))
        ThrowHip("sayuri_hip_load_tensor");
}

int BlockTypeCode(BlockBasic& b) {  // the reference's Is*Block() are non-const
    if (b.IsResidualBlock()) return SAYURI_BLOCK_RESIDUAL;
    if (b.IsBottleneckBlock()) return SAYURI_BLOCK_BOTTLENECK;
    if (b.IsNestedBottleneckBlock()) return SAYURI_BLOCK_NESTED_BOTTLENECK;
    if (b.IsMixerBlock()) return SAYURI_BLOCK_MIXER;
    throw std::runtime_error("unknown block type in DNNWeights");
}

// Network description + tensors -> one device graph (NNGraph::ConstructGraph,
// cuda_forward_pipe.cc:133-613).
// sayuri_hip_create_ex of the device library IN USE -- the one whose sayuri_hip_create this library calls -- or null when that
// library has none (an older build, or the serial stand-in of the host tests).  Looked up by name, and only when a flag is set: a
// device library without the entry point keeps serving every pipe that asks for nothing new.
typedef sayuri_hip_ctx* (*CreateExFn)(int, const sayuri_hip_netdesc*, int, int, int, unsigned);
void* FindInDeviceLibrary(const char* name) {
    Dl_info info;
    if (!dladdr(reinterpret_cast<void*>(&sayuri_hip_create), &info) || !info.dli_fname) return nullptr;
    void* lib = dlopen(info.dli_fname, RTLD_NOW | RTLD_NOLOAD);
    if (!lib) return nullptr;
    void* sym = dlsym(lib, name);
    Dl_info where;  // (a handle's lookup also searches the library's dependencies: the entry point must be the library's own)
    if (sym && (!dladdr(sym, &where) || !where.dli_fname || std::strcmp(where.dli_fname, info.dli_fname) != 0)) sym = nullptr;
    dlclose(lib);  // drops the extra reference only: the library stays loaded
    return sym;
}
CreateExFn FindCreateEx() { return reinterpret_cast<CreateExFn>(FindInDeviceLibrary("sayuri_hip_create_ex")); }
// sayuri_hip_submit_packed_symm, looked up the same way (ensemble requests): a library without it serves everything else
typedef int (*SubmitSymmFn)(sayuri_hip_ctx*, int, const unsigned*, int, int, const int*, const int*, const int*, float*, float*, float*,
                            float*, int*);

// The live-reload entry points of the device library in use, looked up like create_ex: a library without them (an older build, the
// plain stand-in of the host tests) serves everything else, and the pipe says AcceptsReload() == false.
struct ReloadFns {
    int (*begin)(sayuri_hip_ctx*, const sayuri_hip_netdesc*) = nullptr;
    int (*prepare)(sayuri_hip_ctx*) = nullptr;
    int (*commit)(sayuri_hip_ctx*) = nullptr;
    int (*abort)(sayuri_hip_ctx*) = nullptr;
    int (*generation)(const sayuri_hip_ctx*) = nullptr;
    bool all() const { return begin && prepare && commit && abort && generation; }
};
ReloadFns FindReload() {
    ReloadFns f;
    f.begin = reinterpret_cast<decltype(f.begin)>(FindInDeviceLibrary("sayuri_hip_reload_begin"));
    f.prepare = reinterpret_cast<decltype(f.prepare)>(FindInDeviceLibrary("sayuri_hip_reload_prepare"));
    f.commit = reinterpret_cast<decltype(f.commit)>(FindInDeviceLibrary("sayuri_hip_reload_commit"));
    f.abort = reinterpret_cast<decltype(f.abort)>(FindInDeviceLibrary("sayuri_hip_reload_abort"));
    f.generation = reinterpret_cast<decltype(f.generation)>(FindInDeviceLibrary("sayuri_hip_weights_generation"));
    return f;
}

// The architecture of a DNNWeights as the device library takes it.
struct NetDesc {
    std::vector<sayuri_hip_blockdesc> blocks;
    sayuri_hip_netdesc d{};
};
void DescribeNet(DNNWeights& w, NetDesc* nd) {
    std::vector<sayuri_hip_blockdesc>& blocks = nd->blocks;
    sayuri_hip_netdesc& d = nd->d;
    blocks.assign(w.residual_blocks, sayuri_hip_blockdesc{});
    for (int i = 0; i < w.residual_blocks; ++i) {
        BlockBasic& b = *w.tower[i];
        blocks[i].type = BlockTypeCode(b);
        blocks[i].apply_se = b.apply_se;
        blocks[i].se_size = b.se_size;
        blocks[i].bottleneck_channels = b.bottleneck_channels;
        blocks[i].feedforward_channels = b.feedforward_channels;
        blocks[i].dw_filter = b.IsMixerBlock() ? b.dw_conv.GetFilter() : 0;
    }
    d = sayuri_hip_netdesc{};
    d.version = w.version;
    d.input_channels = w.input_channels;
    d.residual_channels = w.residual_channels;
    d.residual_blocks = w.residual_blocks;
    d.policy_head_channels = w.policy_head_channels;
    d.value_head_channels = w.value_head_channels;
    d.probabilities_channels = w.probabilities_channels;
    d.pass_probability_outputs = w.pass_probability_outputs;
    d.ownership_channels = w.ownership_channels;
    d.value_misc_outputs = w.value_misc_outputs;
    d.default_act = static_cast<int>(w.default_act);
    d.policy_head_type = w.policy_head_type == PolicyHeadType::kRepLK ? 1 : 0;
    d.policy_dw_filter = d.policy_head_type ? w.p_dw_conv.GetFilter() : 0;
    d.blocks = blocks.data();
}

// Every tensor of the network into the context: a new one's own set, or the staged set of an open reload.  Throws on a refusal.
void LoadTensors(sayuri_hip_ctx* ctx, DNNWeights& w) {
    LoadConv(ctx, SAYURI_L_INPUT_CONV, w.input_conv);
    for (int i = 0; i < w.residual_blocks; ++i) {
        BlockBasic& b = *w.tower[i];
        if (b.IsResidualBlock()) {
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_CONV1), b.conv1);
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_CONV2), b.conv2);
        } else if (b.IsBottleneckBlock() || b.IsNestedBottleneckBlock()) {
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_PRE_BTL), b.pre_btl_conv);
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_CONV1), b.conv1);
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_CONV2), b.conv2);
            if (b.IsNestedBottleneckBlock()) {
                LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_CONV3), b.conv3);
                LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_CONV4), b.conv4);
            }
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_POST_BTL), b.post_btl_conv);
        } else {
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_DW_CONV), b.dw_conv);
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_CONV1), b.conv1);
            LoadConv(ctx, SAYURI_L_BLOCK(i, SAYURI_S_CONV2), b.conv2);
        }
        if (b.apply_se) {
            LoadFc(ctx, SAYURI_L_BLOCK(i, SAYURI_S_SQUEEZE), b.squeeze);
            LoadFc(ctx, SAYURI_L_BLOCK(i, SAYURI_S_EXCITE), b.excite);
        }
    }
    LoadConv(ctx, SAYURI_L_P_HD_CONV, w.p_hd_conv);
    if (w.policy_head_type == PolicyHeadType::kRepLK) {
        LoadConv(ctx, SAYURI_L_P_DW_CONV, w.p_dw_conv);
        LoadConv(ctx, SAYURI_L_P_PT_CONV, w.p_pt_conv);
    }
    LoadFc(ctx, SAYURI_L_P_INTER_FC, w.p_inter_fc);
    LoadConv(ctx, SAYURI_L_PROB_CONV, w.prob_conv);
    LoadFc(ctx, SAYURI_L_PASS_FC, w.pass_fc);
    LoadConv(ctx, SAYURI_L_V_HD_CONV, w.v_hd_conv);
    LoadFc(ctx, SAYURI_L_V_INTER_FC, w.v_inter_fc);
    LoadConv(ctx, SAYURI_L_V_OWNERSHIP, w.v_ownership);
    LoadFc(ctx, SAYURI_L_V_MISC, w.v_misc);
}

sayuri_hip_ctx* BuildCtx(int device, DNNWeights& w, int max_batch, int board, bool fp16, unsigned hip_flags) {
    NetDesc nd;
    DescribeNet(w, &nd);
    const sayuri_hip_netdesc& d = nd.d;

    sayuri_hip_ctx* ctx = nullptr;
    if (hip_flags) {
        const CreateExFn create_ex = FindCreateEx();
        if (!create_ex)
            throw std::runtime_error("the device library has no entry point sayuri_hip_create_ex: it cannot make a context with flags " +
                                     std::to_string(hip_flags) + " (latency mode needs a current libsayuri_hip.so)");
        ctx = create_ex(device, &d, max_batch, board, fp16 ? 1 : 0, hip_flags);
        if (!ctx) ThrowHip("sayuri_hip_create_ex");
    } else {
        ctx = sayuri_hip_create(device, &d, max_batch, board, fp16 ? 1 : 0);
        if (!ctx) ThrowHip("sayuri_hip_create");
    }
    try {
        LoadTensors(ctx, w);
    } catch (...) {
        sayuri_hip_destroy(ctx);
        throw;
    }
    return ctx;
}

}  // namespace

struct HipForwardPipe::PumpTimer {
    const HipForwardPipe* pipe;
    PumpCounter slot;
    Clock::time_point t0 = Clock::now();
    ~PumpTimer() { pipe->pump_stat_[slot] += Ns(Clock::now() - t0); }
};

HipForwardPipe::HipForwardPipe(HipPipeConfig cfg) : cfg_(std::move(cfg)) {}

HipForwardPipe::~HipForwardPipe() {
    try {
        Destroy();
    } catch (...) {
    }
}

bool HipForwardPipe::Valid() const { return valid_.load(std::memory_order_acquire); }

sayuri_hip_ctx* HipForwardPipe::ctx(int gpu) const {
    return gpu >= 0 && gpu < static_cast<int>(graphs_.size()) ? graphs_[gpu]->ctx : nullptr;
}

void HipForwardPipe::Initialize(std::shared_ptr<DNNWeights> weights) {
    // cuda_forward_pipe.cc:14-25
    Construct(ForwardPipeOption::Get().SetBoardSize(cfg_.default_boardsize).SetBatchSize(cfg_.batch_size), weights);
}

void HipForwardPipe::Construct(ForwardPipeOption option, std::shared_ptr<DNNWeights> weights) {
    // cuda_forward_pipe.cc:44-119: rebuild only when the board changes or the batch grows.
    if (weights) weights_ = weights;
    valid_.store(weights_ != nullptr, std::memory_order_release);
    if (weights_ == nullptr) return;  // Network falls back to its dummy backend
    int board = option.IsValidBoardSize() ? option.board_size : board_size_;
    int batch = option.IsValidBatchSize() ? option.batch_size : max_batch_;
    board = std::max(board, cfg_.fixed_nn_boardsize);
    if (board <= 0 || batch <= 0) return;
    if (board > kBoardSize) throw std::runtime_error("NN board size exceeds MAX_BOARD_SIZE");
    cfg_.batch_size = batch;  // forwarding size of the collector (SetForwardingSize)
    forward_size_.store(batch, std::memory_order_release);  // the pump and Reserve() read this one (the pump may be running)
    if (board_size_ == board && batch <= max_batch_ && !graphs_.empty() && !weights) return;
    Release();
    board_size_ = board;
    max_batch_ = batch;
    BuildGraphs();
}

void HipForwardPipe::BuildGraphs() {
    const int ndev = sayuri_hip_device_count();
    std::vector<int> devices;
    for (int g : cfg_.gpus)
        if (g >= 0 && g < ndev) devices.push_back(g);
    if (devices.empty())
        for (int i = 0; i < ndev; ++i) devices.push_back(i);
    if (devices.empty()) throw std::runtime_error("No executable GPU device!");

    const size_t B2 = static_cast<size_t>(board_size_) * board_size_;
    DNNWeights& w = *weights_;
    shape_ = NetShape{w.version, w.input_channels, w.probabilities_channels, w.pass_probability_outputs, w.value_misc_outputs};
    weights_version_.store(w.version, std::memory_order_release);
    accepts_reload_ = FindReload().all();
    // Ensemble requests: the contexts and the output / fp32 staging take the 7 extra samples of each of the E requests a batch
    // can expand; with E = 0 (or a device library without the entry point) every size below is what it was.
    submit_symm_ = cfg_.ensemble_slots > 0 ? FindInDeviceLibrary("sayuri_hip_submit_packed_symm") : nullptr;
    const size_t dev_batch = static_cast<size_t>(AcceptsEnsemble() ? DeviceBatch() : max_batch_);
    for (int dev : devices) {
        auto g = std::make_unique<Graph>();
        g->device = dev;
        g->ctx = BuildCtx(dev, w, static_cast<int>(dev_batch), board_size_, cfg_.fp16, cfg_.hip_flags);
        auto pinned = [&](size_t count) {
            float* p = static_cast<float*>(sayuri_hip_host_alloc(sizeof(float) * count));
            if (!p) ThrowHip("sayuri_hip_host_alloc");
            return p;
        };
        for (Staging& s : g->st) {
            s.planes = pinned(dev_batch * w.input_channels * B2);
            s.packed = reinterpret_cast<std::uint32_t*>(pinned(static_cast<size_t>(max_batch_) * PackedPlanes::RecordWords(BinaryPlanes())));
            s.is_packed.assign(max_batch_, 0);
            s.is_ens.assign(max_batch_, 0);
            s.ens_base.assign(max_batch_, -1);
            s.fin_ens_base.assign(max_batch_, -1);
            s.dev_src.assign(dev_batch, 0);
            s.dev_symm.assign(dev_batch, 0);
            s.prob = pinned(dev_batch * w.probabilities_channels * B2);
            s.pass = pinned(dev_batch * w.pass_probability_outputs);
            s.misc = pinned(dev_batch * w.value_misc_outputs);
            s.own = pinned(dev_batch * B2);
            s.bsz.assign(dev_batch, board_size_);
            s.reqs.resize(max_batch_);
            s.fin_reqs.resize(max_batch_);
            s.fin_list.resize(max_batch_);
            s.fin_pos.resize(max_batch_);
        }
        graphs_.push_back(std::move(g));
    }
    trace_.on = std::getenv("SAYURI_PIPE_TRACE") != nullptr;
    if (const char* e = std::getenv("SAYURI_PIPE_TAIL")) tail_frac_ = std::atof(e);
    running_.store(true);
    for (auto& g : graphs_) g->pump = std::thread([this, gp = g.get()] { PumpLoop(gp); });
}

long long HipForwardPipe::Trace::now_ns() { return Ns(Clock::now().time_since_epoch()); }

void HipForwardPipe::Trace::Dump() const {
    auto row = [](const char* title, const auto& bins) {
        std::fprintf(stderr, "%s", title);
        for (const auto& a : bins) std::fprintf(stderr, " %ld", a.load());
    };
    row("[pipe trace] arrivals after the last finished batch, 250 us bins:", arrival);
    row("\n[pipe trace] fibers, last finished batch -> the game runs again:", resume);
    row("\n[pipe trace] fibers, the game runs again -> its next request:", think);
    row("\n[pipe trace] tail rule (SAYURI_PIPE_TAIL), age of the running batch at the close:", tail);
    row("\n[pipe trace] batch sizes /16:", size);
    std::fprintf(stderr, "\n[pipe trace] closed: full %ld, idle-wait %ld, 85%%-rule %ld, stray %ld, group flush %ld\n", reason[kCloseFull].load(),
                 reason[kCloseIdleWait].load(), reason[kCloseTail].load(), reason[kCloseStray].load(), reason[kCloseFlush].load());
}

void HipForwardPipe::DestroyGraphs() {
    if (trace_.on && !graphs_.empty()) trace_.Dump();
    running_.store(false);
    for (auto& g : graphs_) {
        {
            std::lock_guard<std::mutex> lk(g->mu);
        }
        g->cv.notify_all();
        g->epoch.fetch_add(1, std::memory_order_release);
        FutexWakeAll(&g->epoch);  // callers parked for a free staging set see running_ == false
    }
    for (auto& g : graphs_)
        if (g->pump.joinable()) g->pump.join();
    for (auto& g : graphs_) {
        for (Staging& s : g->st) {
            sayuri_hip_host_free(s.planes);
            sayuri_hip_host_free(s.packed);
            sayuri_hip_host_free(s.prob);
            sayuri_hip_host_free(s.pass);
            sayuri_hip_host_free(s.misc);
            sayuri_hip_host_free(s.own);
        }
        if (g->ctx) sayuri_hip_destroy(g->ctx);
    }
    graphs_.clear();
}

void HipForwardPipe::Release() { DestroyGraphs(); }

// For each graph: begin -> tensors -> prepare on the caller's thread, beside the pump's batches (the device library lets these
// three run next to submit / wait), then the commits.  Nothing is committed before every graph is prepared: a refusal leaves all
// of them on the old network.
void HipForwardPipe::Reload(std::shared_ptr<DNNWeights> weights) {
    if (!weights) throw std::runtime_error("HipForwardPipe::Reload: no weights");
    std::lock_guard<std::mutex> one(reload_mu_);  // one reload at a time; Construct / Release are the owner's, as ever
    if (graphs_.empty()) throw std::runtime_error("HipForwardPipe::Reload: the pipe is not constructed");
    const ReloadFns fn = FindReload();
    if (!fn.all()) throw std::runtime_error("HipForwardPipe::Reload: the device library has no live-reload entry points (sayuri_hip_reload_*)");
    NetDesc nd;
    DescribeNet(*weights, &nd);
    size_t opened = 0;
    try {
        for (auto& g : graphs_) {
            if (fn.begin(g->ctx, &nd.d)) ThrowHip("sayuri_hip_reload_begin");
            ++opened;
            LoadTensors(g->ctx, *weights);
            if (fn.prepare(g->ctx)) {  // (a failed prepare has closed its reload itself)
                --opened;
                ThrowHip("sayuri_hip_reload_prepare");
            }
        }
    } catch (...) {
        for (size_t i = 0; i < opened; ++i) (void)fn.abort(graphs_[i]->ctx);
        throw;
    }
    // the light step: a pointer flip per graph, serialised with the pump's submit by the context itself
    for (size_t i = 0; i < graphs_.size(); ++i)
        if (fn.commit(graphs_[i]->ctx) < 0) {
            // (cannot happen after a successful prepare short of a device error; graphs before i serve the new network already)
            const std::string why = sayuri_hip_last_error();
            for (size_t k = i; k < graphs_.size(); ++k) (void)fn.abort(graphs_[k]->ctx);
            throw std::runtime_error("sayuri_hip_reload_commit: " + why);
        }
    weights_version_.store(weights->version, std::memory_order_release);
    weights_ = std::move(weights);
}

int HipForwardPipe::WeightsGeneration() const {
    const ReloadFns fn = FindReload();
    if (!fn.generation || graphs_.empty()) return 0;
    int g = fn.generation(graphs_[0]->ctx);
    for (auto& gr : graphs_) g = std::min(g, fn.generation(gr->ctx));
    return g;
}

void HipForwardPipe::Destroy() { DestroyGraphs(); }

// Copy one request into staging slot `slot`, re-padding a smaller board top-left into the NN
// grid (what SendQueryAndWait does with a temporary InputData, batch_forward_pipe.cc:15-33).
void HipForwardPipe::StageInput(Staging* st, int slot, const InputData& in, bool already_padded) {
    const int B = board_size_, bs = in.board_size, C = shape_.input_channels;
    if (bs < 2 || bs > B) throw std::runtime_error("InputData board size does not fit the NN board");
    float* dst = st->planes + static_cast<size_t>(slot) * C * B * B;
    st->bsz[slot] = bs;
    if (bs == B || already_padded) {
        std::memcpy(dst, in.planes.data(), sizeof(float) * C * B * B);
        return;
    }
    std::memset(dst, 0, sizeof(float) * C * B * B);
    for (int c = 0; c < C; ++c)
        for (int y = 0; y < bs; ++y)
            std::memcpy(dst + (static_cast<size_t>(c) * B + y) * B, in.planes.data() + (static_cast<size_t>(c) * bs + y) * bs,
                        sizeof(float) * bs);
}

int HipForwardPipe::BinaryPlanes() const { return PackedPlanes::BinaryPlanes(shape_.input_channels); }

// The packed flavour: the record goes into the pinned packed buffer as it is -- the bits are in the sample's own cell
// order, the device kernel knows the sample's board size, nothing is re-padded.
void HipForwardPipe::StagePacked(Staging* st, int slot, const PackedPlanes& in) {
    if (in.board_size < 2 || in.board_size > board_size_) throw std::runtime_error("PackedPlanes board size does not fit the NN board");
    if (in.binary_planes != BinaryPlanes()) throw std::runtime_error("PackedPlanes: binary plane count does not match the network");
    st->bsz[slot] = in.board_size;
    in.Store(st->packed + static_cast<size_t>(slot) * PackedPlanes::RecordWords(in.binary_planes));
}

// A packed slot of a batch that also holds fp32 requests: expand it into the fp32 staging (NN grid), pump thread.  An ensemble
// slot's symmetries 1..7 go to their device samples the same way, each cell taken through PackedPlanes::SymmetryIndex.
void HipForwardPipe::ExpandPacked(Staging* st, int slot, int dst_slot, int symmetry) {
    const int B = board_size_, bs = st->bsz[slot], C = shape_.input_channels, nbin = BinaryPlanes();
    const std::uint32_t* rec = st->packed + static_cast<size_t>(slot) * PackedPlanes::RecordWords(nbin);
    float* dst = st->planes + static_cast<size_t>(dst_slot) * C * B * B;
    std::memset(dst, 0, sizeof(float) * C * B * B);
    for (int c = 0; c < C; ++c) {
        float scalar = 0.f;
        if (c >= nbin) std::memcpy(&scalar, rec + nbin * PackedPlanes::kWords + (c - nbin), sizeof scalar);
        for (int y = 0; y < bs; ++y)
            for (int x = 0; x < bs; ++x) {
                const int cell = symmetry ? PackedPlanes::SymmetryIndex(bs, symmetry, y * bs + x) : y * bs + x;
                dst[(static_cast<size_t>(c) * B + y) * B + x] =
                    c < nbin ? static_cast<float>((rec[c * PackedPlanes::kWords + (cell >> 5)] >> (cell & 31)) & 1u) : scalar;
            }
    }
}

// FillOutputs of the CPU pipe (blas_forward_pipe.cc:565-619 -- the oracle; the CUDA pipe's
// pass[0] for every offset, cuda_forward_pipe.cc:1074, is a known discrepancy) fused with the
// un-padding of SendQueryAndWait (batch_forward_pipe.cc:48-68).
void HipForwardPipe::FillOutput(const Staging* g, int slot, const Echo& in, bool unpad, OutputResult* out) const {
    const NetShape& w = shape_;  // (not weights_: Reload replaces that pointer while callers fill their outputs)
    const int B = board_size_, B2 = B * B, bs = in.board_size;
    const bool v1 = w.version <= 2;  // Encoder::GetEncoderVersion, encoder.h:64-77
    int offset = v1 ? 0 : static_cast<int>(in.offset);
    if (offset < 0 || offset >= w.probabilities_channels) offset = 0;
    const float* prob = g->prob + (static_cast<size_t>(slot) * w.probabilities_channels + offset) * B2;
    const float* own = g->own + static_cast<size_t>(slot) * B2;
    const float* misc = g->misc + static_cast<size_t>(slot) * w.value_misc_outputs;
    const float* pass = g->pass + static_cast<size_t>(slot) * w.pass_probability_outputs;
    if (unpad && bs != B) {
        for (int y = 0; y < bs; ++y)
            for (int x = 0; x < bs; ++x) {
                out->probabilities[y * bs + x] = prob[y * B + x];
                out->ownership[y * bs + x] = own[y * B + x];
            }
    } else {
        std::copy(prob, prob + B2, out->probabilities.begin());
        std::copy(own, own + B2, out->ownership.begin());
    }
    out->pass_probability = pass[offset];
    out->wdl[0] = misc[0];
    out->wdl[1] = misc[1];
    out->wdl[2] = misc[2];
    out->stm_winrate = misc[3];
    if (v1) {
        out->final_score = misc[4];
        out->q_error = 0.f;
        out->score_error = 0.f;
        out->offset = PolicyBufferOffset::kNormal;
    } else {
        out->final_score = misc[8];
        out->q_error = misc[13];
        out->score_error = misc[14];
        out->offset = in.offset;
    }
    out->board_size = bs;
    out->komi = in.komi;
    out->fp16 = cfg_.fp16;
}

void HipForwardPipe::SubmitBatch(Graph* g, Staging* s, int n) {
    const auto t0 = Clock::now();
    int npacked = 0, nens = 0;
    for (int i = 0; i < n; ++i) npacked += s->is_packed[i];
    // The device batch: the set's slots as they are, then symmetries 1..7 of every ensemble slot behind them.
    for (int i = 0; i < n; ++i) {
        s->ens_base[i] = -1;
        if (!s->is_ens[i]) continue;
        const int base = s->ens_base[i] = n + 7 * nens++;
        for (int k = 0; k < 7; ++k) {
            s->dev_src[base + k] = i;
            s->dev_symm[base + k] = k + 1;
            s->bsz[base + k] = s->bsz[i];
        }
    }
    s->dev_n = n + 7 * nens;
    if (npacked > 0 && npacked < n)  // a mixed batch travels as fp32 planes
        for (int i = 0; i < n; ++i) {
            if (!s->is_packed[i]) continue;
            ExpandPacked(s, i, i, 0);
            for (int k = 0; k < 7 && s->ens_base[i] >= 0; ++k) ExpandPacked(s, i, s->ens_base[i] + k, k + 1);
        }
    std::lock_guard<std::mutex> dev(g->dev_mu);
    if (nens > 0) {
        if (npacked == n) {
            for (int i = 0; i < n; ++i) { s->dev_src[i] = i; s->dev_symm[i] = 0; }
            if (reinterpret_cast<SubmitSymmFn>(submit_symm_)(g->ctx, s->dev_n, s->packed, n, BinaryPlanes(), s->bsz.data(), s->dev_src.data(),
                                                             s->dev_symm.data(), s->prob, s->pass, s->misc, s->own, &s->ticket))
                ThrowHip("sayuri_hip_submit_packed_symm");
        } else if (sayuri_hip_submit(g->ctx, s->dev_n, s->planes, s->bsz.data(), s->prob, s->pass, s->misc, s->own, &s->ticket)) {
            ThrowHip("sayuri_hip_submit");
        }
        pump_stat_[kSubmitCall] += Ns(Clock::now() - t0);
        return;
    }
    if (npacked == n ? sayuri_hip_submit_packed(g->ctx, n, s->packed, BinaryPlanes(), s->bsz.data(), s->prob, s->pass, s->misc, s->own, &s->ticket)
                     : sayuri_hip_submit(g->ctx, n, s->planes, s->bsz.data(), s->prob, s->pass, s->misc, s->own, &s->ticket))
        ThrowHip(npacked == n ? "sayuri_hip_submit_packed" : "sayuri_hip_submit");
    // (a submit that failed has thrown: its time is not counted)
    pump_stat_[kSubmitCall] += Ns(Clock::now() - t0);
}

void HipForwardPipe::FinishBatch(Graph* g, Staging* s, int n) {
    int rc;
    {
        const PumpTimer t{this, kDeviceWait};
        std::lock_guard<std::mutex> dev(g->dev_mu);
        rc = sayuri_hip_wait(g->ctx, s->ticket);
    }
    const PumpTimer t{this, kHandOut};
    // the previous batch of this set was handed out at least one batch time ago
    while (s->wakes_done.load(std::memory_order_acquire) < s->fin_count) std::this_thread::yield();
    // (counted before anybody is told: a caller that has its result sees the batch in the counters)
    batches_.fetch_add(1, std::memory_order_relaxed);
    evals_.fetch_add(static_cast<size_t>(std::max(n, s->dev_n)), std::memory_order_relaxed);
    int count = 0, fibers = 0;
    for (int i = 0; i < n; ++i) {
        const Request& r = s->reqs[i];
        s->fin_reqs[i] = r;
        s->fin_ens_base[i] = s->ens_base[i];
        if (r.fiber) {
            ++fibers;  // flagged below, once fin_status is in place
        } else if (r.self_serve) {
            s->fin_pos[i] = count;
            s->fin_list[count++] = i;
        } else {  // asynchronous Submit(): filled and signalled here
            if (rc == 0) FillOutput(s, i, r.echo, true, r.output);
            r.done->store(rc == 0 ? 1 : -1, std::memory_order_release);
            FutexWakeAll(r.done);
        }
    }
    s->fin_count = count;
    s->fin_fibers = fibers;
    s->wakes_done.store(0, std::memory_order_relaxed);
    s->consumed.store(0, std::memory_order_relaxed);
    s->fin_status.store(rc == 0 ? 1 : -1, std::memory_order_relaxed);
    if (fibers > 0) {  // games scheduled as fibers: one flag store each, one wake word for their scheduler threads
        for (int i = 0; i < n; ++i)
            if (s->fin_reqs[i].fiber) s->fin_reqs[i].done->store(rc == 0 ? 1 : -1, std::memory_order_release);
        sayuri_fiber::NotifyAll();
    }
    if (count > 0) {  // root of the wake tree
        std::atomic<int>* root = s->fin_reqs[s->fin_list[0]].done;
        root->store(1, std::memory_order_release);
        FutexWakeAll(root);
    }
    // The set takes new requests at once: its inputs are on the GPU already, the snapshot above keeps the hand-out
    // independent of new reservations, and the pinned OUTPUT buffers are not written again before the set's next
    // batch is submitted -- SubmitBatch waits for `consumed` there (callers need microseconds, that is a batch away).
    Reopen(g, s);
}

// A set re-opened or the fill index moved: wake the callers parked for a free staging set.  Threads sleep on the epoch word;
// fibers parked on it in Reserve() are woken by their scheduler threads, which may be asleep themselves -- only when a fiber IS
// parked there (rare with four sets): a NotifyAll wakes every scheduler thread, one per rotation was half of a rank's wake-ups.
void HipForwardPipe::AnnounceEpoch(Graph* g) {
    g->epoch.fetch_add(1, std::memory_order_seq_cst);
    FutexWakeAll(&g->epoch);
    if (epoch_parked_.load(std::memory_order_seq_cst) > 0) sayuri_fiber::NotifyAll();
}

void HipForwardPipe::Reopen(Graph* g, Staging* s) {
    s->ready.store(0, std::memory_order_relaxed);
    s->ens_taken.store(0, std::memory_order_relaxed);
    s->dev_n = 0;
    s->reserved.store(0, std::memory_order_release);  // re-open for callers
    AnnounceEpoch(g);
}

// The pump thread's own state: nobody else reads or writes it.
struct HipForwardPipe::Pump {
    struct Batch { int set, n; };
    struct Fifo {  // of closed sets and their sizes; the ring has kSets sets, so it never holds more
        Batch b[Graph::kSets];
        int size{0};
        void push(Batch x) { b[size++] = x; }
        Batch pop() { const Batch x = b[0]; std::copy(b + 1, b + size--, b); return x; }
    };
    Graph* const g;
    int cur{0};                          // set currently filling
    Fifo pending{}, inflight{};           // closed sets waiting for a GPU slot; sets on the GPU, at most two
    bool timing{false};                  // idle-wait rule: a partial fill set was first seen at first_seen
    Clock::time_point first_seen{};
    Clock::time_point gpu_busy_since{};  // when the batch at the head of the GPU queue started executing (estimate)
    double gpu_batch_us{1000.0};         // running mean of a batch's time on the GPU
    Clock::time_point gpu_idle_since{};
    bool ever_busy{false};
};

// Close an open set and queue its requests as a batch; false when it was empty (it is open again then).
bool HipForwardPipe::CloseSet(Pump& p, int set, CloseReason reason) {
    Staging& s = p.g->st[set];
    const unsigned prev = s.reserved.fetch_or(Staging::kClosed, std::memory_order_acq_rel);
    const int n = static_cast<int>(std::min<unsigned>(prev & ~Staging::kClosed, static_cast<unsigned>(max_batch_)));
    if (n == 0) { s.reserved.store(0, std::memory_order_release); return false; }
    const bool stray = reason == kCloseStray;  // counts as partial whatever its size, and is not in the size histogram
    if (stray || static_cast<unsigned>(n) < WantNow()) pump_stat_[kPartialBatches] += 1;
    if (trace_.on) {
        if (!stray) Trace::Count(trace_.size[std::min(n / 16, 16)]);
        Trace::Count(trace_.reason[reason]);
    }
    p.pending.push({set, n});
    return true;
}

// close the fill set and point callers at the next one of the ring
void HipForwardPipe::CloseFillSet(Pump& p, CloseReason reason) {
    p.timing = false;
    if (!CloseSet(p, p.cur, reason)) return;
    p.cur = (p.cur + 1) % Graph::kSets;
    p.g->fill.store(p.cur, std::memory_order_release);
    const PumpTimer t{this, kWakeParked};
    AnnounceEpoch(p.g);
}

// A caller that read `fill`, was preempted, and resumed after that set had been closed, evaluated and re-opened
// finds `reserved` == 0 there and takes a slot in a set that is no longer the fill set.  Such a set is open, not
// `cur`, and holds requests: close it where it stands and queue it like any other batch (the fill index does not
// move).  Without this the request would wait until the ring wraps around to its set -- forever once traffic stops.
bool HipForwardPipe::CloseStrays(Pump& p) {
    bool any = false;
    for (int k = 0; k < Graph::kSets && p.pending.size < Graph::kSets; ++k) {
        if (k == p.cur) continue;
        const unsigned seen = p.g->st[k].reserved.load(std::memory_order_acquire);
        if ((seen & Staging::kClosed) || seen == 0) continue;
        any |= CloseSet(p, k, kCloseStray);
    }
    return any;
}

// wait for the callers' plane copies of the oldest pending set, then enqueue it
void HipForwardPipe::SubmitOldestPending(Pump& p) {
    const Pump::Batch b = p.pending.pop();
    Staging& s = p.g->st[b.set];
    {
        const PumpTimer t{this, kWaitCallers};
        while (s.ready.load(std::memory_order_acquire) < static_cast<unsigned>(b.n)) std::this_thread::yield();
        // every blocking caller of this set's previous batch has copied its result out of the pinned outputs
        while (s.consumed.load(std::memory_order_acquire) < s.fin_count + s.fin_fibers) std::this_thread::yield();
    }
    try {
        SubmitBatch(p.g, &s, b.n);
    } catch (const std::exception&) {
        // nothing was evaluated: every caller gets the failure directly (no tree: nothing to copy out)
        for (int k = 0; k < b.n; ++k) {
            s.reqs[k].done->store(-1, std::memory_order_release);
            FutexWakeAll(s.reqs[k].done);
        }
        sayuri_fiber::NotifyAll();
        Reopen(p.g, &s);
        return;
    }
    if (p.inflight.size == 0) {
        p.gpu_busy_since = Clock::now();
        if (p.ever_busy) pump_stat_[kGpuQueueEmpty] += Ns(p.gpu_busy_since - p.gpu_idle_since);
        p.ever_busy = true;
    }
    p.inflight.push(b);
}

bool HipForwardPipe::OldestIsDone(Pump& p) {
    std::lock_guard<std::mutex> dev(p.g->dev_mu);
    return sayuri_hip_query(p.g->ctx, p.g->st[p.inflight.b[0].set].ticket) != 0;
}

// wait for the batch at the head of the GPU queue and hand it out
void HipForwardPipe::FinishOldest(Pump& p) {
    const Pump::Batch b = p.inflight.b[0];
    if (trace_.on) trace_.last_done_ns.store(Trace::now_ns(), std::memory_order_relaxed);
    FinishBatch(p.g, &p.g->st[b.set], b.n);
    const auto now = Clock::now();
    const double us = std::chrono::duration<double, std::micro>(now - p.gpu_busy_since).count();
    p.gpu_batch_us = 0.8 * p.gpu_batch_us + 0.2 * us;
    p.gpu_busy_since = now;  // the next queued batch (if any) has the GPU from here
    p.inflight.pop();
    if (p.inflight.size == 0) p.gpu_idle_since = now;
}

// One persistent pump per GPU over a ring of staging sets.  Callers fill the set `fill` points at; when it holds
// batch_size requests (or its wait expired) the pump closes it and points callers at the next set of the ring.
// Closed sets are ENQUEUED on the GPU in order, at most two at a time (H2D, graph, D2H are stream-ordered, so
// the second runs back to back with the first); the pump hands out a batch's results when its event fires and
// re-opens the set.  With more leaves in flight than two batches the remaining sets hold full batches that are
// ready the moment the GPU frees a slot.  A set that is not full is sent after gpu_waittime_ms, and once that
// happened the pump stops waiting until the fill set runs dry again (the adaptive 0 <-> base wait of
// batch_forward_pipe.cc:99-193).
void HipForwardPipe::PumpLoop(Graph* g) {
    pthread_setname_np(pthread_self(), "sayuri-pump");
    Pump p{g};
    while (true) {
        if (CloseStrays(p)) continue;
        if (!running_.load() && p.inflight.size == 0 && p.pending.size == 0 &&
            std::all_of(g->st, g->st + Graph::kSets, [](const Staging& s) { return s.count() == 0; }))
            return;
        // keep the GPU fed: closed sets go out while it has a free slot
        if (p.pending.size > 0 && p.inflight.size < 2) { SubmitOldestPending(p); continue; }
        const Staging& s = g->st[p.cur];
        if (s.closed()) {  // the ring is full: wait for the oldest batch, its set is the one callers are parked on
            if (p.inflight.size > 0) FinishOldest(p);
            p.timing = false;
            continue;
        }
        const unsigned c = s.count();
        if (c >= WantNow()) { CloseFillSet(p, kCloseFull); continue; }
        if (c > 0 && group_filling_.load(std::memory_order_acquire) > 0) {
            // a ForwardGroup caller is writing its requests (microseconds): the set stays open for them, whatever the rules below say
            if (p.inflight.size > 0 && OldestIsDone(p)) FinishOldest(p);
            else std::this_thread::yield();
            continue;
        }
        if (c > 0 && group_flush_.load(std::memory_order_acquire) > 0) { CloseFillSet(p, kCloseFlush); continue; }
        if (c > 0 && (cfg_.gpu_waittime_ms <= 0 || !running_.load())) { CloseFillSet(p, kCloseFull); continue; }
        if (c == 0 || p.inflight.size > 0) p.timing = false;  // the idle-wait clock runs for a partial set and an idle GPU only
        if (c > 0 && p.inflight.size == 0) {
            // partial batch and an idle GPU: give stragglers gpu_waittime_ms, then send what is there
            if (!p.timing) { p.timing = true; p.first_seen = Clock::now(); }
            if (Clock::now() - p.first_seen >= std::chrono::milliseconds(cfg_.gpu_waittime_ms)) { CloseFillSet(p, kCloseIdleWait); continue; }
        } else if (c > 0 && p.inflight.size == 1) {
            // one batch is running and nothing is queued behind it: let the partial set keep filling, but enqueue it
            // shortly before that batch is expected to finish, so its upload hides under the running batch's tail
            const auto run = Clock::now() - p.gpu_busy_since;
            if (std::chrono::duration<double, std::micro>(run).count() >= tail_frac_ * p.gpu_batch_us) {
                if (trace_.on) Trace::Count(trace_.tail[Trace::bin250us(Ns(run))]);
                CloseFillSet(p, kCloseTail);
                continue;
            }
        }
        // nothing to send yet: retire a finished batch if there is one, else nap
        if (p.inflight.size > 0 && OldestIsDone(p)) { FinishOldest(p); continue; }
        const PumpTimer nap{this, kNap};
        std::unique_lock<std::mutex> lk(g->mu);
        // (a flush raised since the look above: its caller takes `mu` before it notifies, so it is seen here or it wakes the wait)
        if (group_flush_.load(std::memory_order_acquire) > 0 && s.count() > 0) continue;
        g->cv.wait_for(lk, std::chrono::microseconds(p.inflight.size > 0 ? 50 : 200));
    }
}

HipForwardPipe::Ticket HipForwardPipe::Reserve(const InputData* input, const PackedPlanes* packed, OutputResult* out,
                                               std::atomic<int>* done, bool self_serve, bool fiber, bool ensemble) {
    if (graphs_.empty()) throw std::runtime_error("HipForwardPipe is not constructed");
    const Echo echo = EchoOf(input, packed);
    if (echo.board_size < 2 || echo.board_size > board_size_)
        throw std::runtime_error("InputData board size does not fit the NN board");
    done->store(0, std::memory_order_relaxed);
    if (trace_.on) {
        const long long now = Trace::now_ns();
        Trace::Count(trace_.arrival[Trace::bin250us(now - trace_.last_done_ns.load(std::memory_order_relaxed))]);
        if (long long* st = sayuri_fiber::FiberStamp()) {
            if (*st) Trace::Count(trace_.think[Trace::bin250us(now - *st)]);
        }
    }
    Graph* g = graphs_[next_graph_.fetch_add(1, std::memory_order_relaxed) % graphs_.size()].get();
    const unsigned cap = static_cast<unsigned>(max_batch_);
    const unsigned want = WantNow();
    for (;;) {
        const int epoch = g->epoch.load(std::memory_order_acquire);
        Staging& s = g->st[g->fill.load(std::memory_order_acquire)];
        const unsigned seen = s.reserved.load(std::memory_order_acquire);
        if (!(seen & Staging::kClosed) && seen < cap) {
            const unsigned r = s.reserved.fetch_add(1, std::memory_order_acq_rel);
            if (!(r & Staging::kClosed) && r < cap) {
                const int slot = static_cast<int>(r);
                // the one copy of the planes, by the calling thread
                if (input) StageInput(&s, slot, *input, false);
                else StagePacked(&s, slot, *packed);
                s.is_packed[slot] = input ? 0 : 1;
                // an ensemble request expands while the set has capacity left; past it the slot is a plain identity request
                s.is_ens[slot] = ensemble && s.ens_taken.fetch_add(1, std::memory_order_relaxed) < cfg_.ensemble_slots ? 1 : 0;
                s.reqs[slot] = Request{echo, out, done, self_serve, fiber};
                s.ready.fetch_add(1, std::memory_order_release);
                if (r == 0 || r + 1 >= want) g->cv.notify_one();
                return Ticket{g, &s, slot};
            }
        }
        // both sets are taken (one on the GPU, one full or being rotated): sleep until the pump re-opens one
        if (!running_.load()) throw std::runtime_error("HipForwardPipe is shutting down");
        if (fiber) {
            // let the thread's other games run meanwhile.  The count is raised BEFORE the word is looked at again (inside
            // WaitWhileEqual) and the pump looks at the count AFTER it changed the word: one of the two sees the other.
            epoch_parked_.fetch_add(1, std::memory_order_seq_cst);
            sayuri_fiber::WaitWhileEqual(&g->epoch, epoch);
            epoch_parked_.fetch_sub(1, std::memory_order_seq_cst);
        } else {
            FutexWait(&g->epoch, epoch);
        }
    }
}

void HipForwardPipe::Submit(const InputData& input, OutputResult* out, std::atomic<int>* done) {
    Reserve(&input, nullptr, out, done, false);
}

OutputResult HipForwardPipe::Forward(const InputData& input) {
    OutputResult out;
    ForwardAny(&input, nullptr, &out);
    return out;
}

OutputResult HipForwardPipe::ForwardPacked(const PackedPlanes& input) {
    OutputResult out;
    ForwardAny(nullptr, &input, &out);
    return out;
}

bool HipForwardPipe::ForwardEnsemble(const PackedPlanes& identity, OutputResult out[8]) {
    if (!AcceptsEnsemble()) throw std::runtime_error("HipForwardPipe: ensemble requests are off (ensemble_slots = 0, or a device library without sayuri_hip_submit_packed_symm)");
    const bool all = ForwardAny(nullptr, &identity, &out[0], out);
    if (!all) ens_fallbacks_.fetch_add(1, std::memory_order_relaxed);
    return all;
}

void HipForwardPipe::WakePumps() {
    for (auto& g : graphs_) {
        { std::lock_guard<std::mutex> lk(g->mu); }
        g->cv.notify_one();
    }
}

void HipForwardPipe::ForwardGroup(const PackedPlanes* in, int n, OutputResult* out) {
    if (sayuri_fiber::InFiber())
        throw std::runtime_error("HipForwardPipe::ForwardGroup is for OS-thread callers: a fiber sends its requests one by one (ForwardPacked)");
    if (n <= 0) return;
    if (graphs_.empty()) throw std::runtime_error("HipForwardPipe is not constructed");
    // everything Reserve and StagePacked would refuse, BEFORE the first slot is taken: a group is sent whole or not at all
    for (int i = 0; i < n; ++i) {
        if (in[i].board_size < 2 || in[i].board_size > board_size_) throw std::runtime_error("PackedPlanes board size does not fit the NN board");
        if (in[i].binary_planes != BinaryPlanes()) throw std::runtime_error("PackedPlanes: binary plane count does not match the network");
    }
    bool failed = false;
    for (int base = 0; base < n;) {
        const int m = std::min(n - base, std::max(1, static_cast<int>(WantNow())));
        std::vector<std::atomic<int>> done(static_cast<size_t>(m));
        int reserved = 0;
        std::exception_ptr error;
        group_filling_.fetch_add(1, std::memory_order_acq_rel);
        try {
            for (; reserved < m; ++reserved) Reserve(nullptr, &in[base + reserved], &out[base + reserved], &done[static_cast<size_t>(reserved)], false);
        } catch (...) {  // (the pipe is shutting down) what was reserved is still waited for: the pump writes through these pointers
            error = std::current_exception();
        }
        // the flush goes up before the hold comes down: the pumps see one of the two, never a gap in which the other rules apply
        group_flush_.fetch_add(1, std::memory_order_acq_rel);
        group_filling_.fetch_sub(1, std::memory_order_acq_rel);
        WakePumps();
        // the pump fills out[] and flips the flags in slot order: the last one first, the others are set by then
        for (int i = reserved - 1; i >= 0; --i) {
            std::atomic<int>& d = done[static_cast<size_t>(i)];
            int st;
            while ((st = d.load(std::memory_order_acquire)) == 0) FutexWait(&d, 0);
            failed |= st < 0;
        }
        group_flush_.fetch_sub(1, std::memory_order_acq_rel);
        if (error) std::rethrow_exception(error);
        if (failed) ThrowBatchFailed();
        base += m;
    }
}

HipForwardPipe::Echo HipForwardPipe::EchoOf(const InputData* input, const PackedPlanes* packed) {
    return input ? Echo{input->board_size, input->offset, input->komi}
                 : Echo{packed->board_size, static_cast<PolicyBufferOffset>(packed->offset), packed->komi};
}

// A Forward() caller copies its own result out of its set's pinned outputs, and says so: the set's next batch waits for that.
// An ensemble request's symmetries 1..7 lie at the device samples FinishBatch's snapshot names; true when they were taken.
bool HipForwardPipe::TakeResult(Staging* s, int slot, const Echo& echo, int status, OutputResult* out, OutputResult* ens_out) const {
    const int base = ens_out ? s->fin_ens_base[slot] : -1;
    if (status > 0) {
        FillOutput(s, slot, echo, true, out);
        for (int k = 0; k < 7 && base >= 0; ++k) FillOutput(s, base + k, echo, true, &ens_out[k + 1]);
    }
    s->consumed.fetch_add(1, std::memory_order_release);
    if (status < 0) ThrowBatchFailed();
    return base >= 0;
}

bool HipForwardPipe::ForwardAny(const InputData* in, const PackedPlanes* pk, OutputResult* outp, OutputResult* ens_out) {
    OutputResult& out = *outp;
    std::atomic<int> done{0};
    const Echo echo = EchoOf(in, pk);
    if (sayuri_fiber::InFiber()) {
        // M:N game scheduling (fiber.h): hand the request over and run this thread's other games until the batch is back
        const Ticket t = Reserve(in, pk, nullptr, &done, false, true, ens_out != nullptr);
        sayuri_fiber::WaitWhileEqual(&done, 0);
        if (trace_.on) {
            const long long now = Trace::now_ns();
            Trace::Count(trace_.resume[Trace::bin250us(now - trace_.last_done_ns.load(std::memory_order_relaxed))]);
            if (long long* st = sayuri_fiber::FiberStamp()) *st = now;
        }
        return TakeResult(t.s, t.slot, echo, done.load(std::memory_order_acquire), &out, ens_out);
    }
    const Ticket t = Reserve(in, pk, nullptr, &done, true, false, ens_out != nullptr);
    int st;
    while ((st = done.load(std::memory_order_acquire)) == 0) FutexWait(&done, 0);
    if (st < 0) ThrowBatchFailed();  // the batch was never submitted: no tree, nothing to take
    // woken through the batch's tree: pass the wake-up on to this node's children first, then take the result
    Staging& s = *t.s;
    const int count = s.fin_count, pos = s.fin_pos[t.slot];
    for (int c = Staging::kFanout * pos + 1; c <= Staging::kFanout * pos + Staging::kFanout && c < count; ++c) {
        std::atomic<int>* child = s.fin_reqs[s.fin_list[c]].done;
        child->store(1, std::memory_order_release);
        FutexWakeAll(child);
    }
    s.wakes_done.fetch_add(1, std::memory_order_release);
    return TakeResult(&s, t.slot, echo, s.fin_status.load(std::memory_order_relaxed), &out, ens_out);
}

std::vector<OutputResult> HipForwardPipe::BatchForward(int gpu, const std::vector<InputData>& inputs) {
    if (gpu < 0 || gpu >= static_cast<int>(graphs_.size())) throw std::runtime_error("BatchForward: bad gpu index");
    const int n = static_cast<int>(inputs.size());
    if (n > max_batch_) throw std::runtime_error("BatchForward: batch exceeds the constructed maximum");
    std::vector<OutputResult> outs(inputs.size());
    if (n == 0) return outs;
    Graph* g = graphs_[gpu].get();
    // pageable scratch staging of its own: the pinned sets belong to the queue path
    const NetShape& w = shape_;
    const size_t B2 = static_cast<size_t>(board_size_) * board_size_;
    Staging s;
    std::vector<float> planes(static_cast<size_t>(n) * w.input_channels * B2), prob(static_cast<size_t>(n) * w.probabilities_channels * B2),
        pass(static_cast<size_t>(n) * w.pass_probability_outputs), misc(static_cast<size_t>(n) * w.value_misc_outputs), own(static_cast<size_t>(n) * B2);
    s.planes = planes.data(); s.prob = prob.data(); s.pass = pass.data(); s.misc = misc.data(); s.own = own.data();
    s.bsz.assign(n, board_size_);
    for (int i = 0; i < n; ++i) StageInput(&s, i, inputs[i], true);
    {
        std::lock_guard<std::mutex> dev(g->dev_mu);  // keep the pump's batches out while we use the ctx
        if (sayuri_hip_forward(g->ctx, n, s.planes, s.bsz.data(), s.prob, s.pass, s.misc, s.own))
            ThrowHip("sayuri_hip_forward");
    }
    for (int i = 0; i < n; ++i) FillOutput(&s, i, Echo{inputs[i].board_size, inputs[i].offset, inputs[i].komi}, false, &outs[i]);
    batches_.fetch_add(1, std::memory_order_relaxed);
    evals_.fetch_add(static_cast<size_t>(n), std::memory_order_relaxed);
    return outs;
}

SAYURI_HOST_END
