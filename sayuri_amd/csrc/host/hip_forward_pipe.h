// hip_forward_pipe.h -- the MI355X backend behind Sayuri's NetworkForwardPipe plugin interface.
//
// Counterpart of CudaForwardPipe (reference src/neural/cuda/cuda_forward_pipe.{h,cc}) +
// BatchForwardPipe (reference src/neural/batch_forward_pipe.{h,cc}):
//   * same seven entry points (Initialize / Forward / Construct / Release / Destroy / Valid /
//     GetNumWorkers) plus BatchForward(gpu, inputs), same argument meaning, same error
//     behaviour (device/API failures surface as std::runtime_error, cuda_common.cc:46-62);
//   * the device side is reached only through the C-ABI of include/sayuri_hip.h;
//   * the leaf-batch collector is rewritten: callers write their planes ONCE, straight into a
//     pinned staging slot of the batch being assembled (the reference copies the 62 KB
//     InputData three times per evaluation: batch_forward_pipe.cc:9, :178,
//     cuda_forward_pipe.cc:696-701), one persistent pump thread per GPU owns its ctx and its
//     own queue shard, and completion is a per-request flag instead of a heap-allocated
//     mutex+condvar pair per leaf.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#ifdef SAYURI_IN_TREE
// Built inside the reference tree: the reference's own plugin types (global namespace).
#include "neural/description.h"
#include "neural/network_basic.h"
#include "packed_planes.h"
using sayuri_host::PackedPlanes;
#define SAYURI_HOST_BEGIN
#define SAYURI_HOST_END
#define SAYURI_EXT_OVERRIDE  // the reference's NetworkForwardPipe has no packed entry points: plain members there
#else
#include "packed_planes.h"
#include "pipe_api.h"
#include "weights_model.h"
#define SAYURI_HOST_BEGIN namespace sayuri_host {
#define SAYURI_HOST_END }
#define SAYURI_EXT_OVERRIDE override
#endif

struct sayuri_hip_ctx;

SAYURI_HOST_BEGIN

// What the reference reads from its global option map (config.cc:21-133): "batch_size",
// "gpus", "fp16", "gpu_waittime", "defualt_boardsize", "fixed_nn_boardsize".
struct HipPipeConfig {
    int batch_size{256};
    std::vector<int> gpus;       // empty = every visible device
    bool fp16{true};
    int gpu_waittime_ms{2};
    int default_boardsize{kBoardSize};
    int fixed_nn_boardsize{0};
    unsigned hip_flags{0};       // sayuri_hip_create_ex flags of every GPU's context (SAYURI_HIP_LATENCY); 0 = sayuri_hip_create
    int ensemble_slots{0};       // E: ensemble requests (ForwardEnsemble) a batch can expand on the device; every context gets
                                 // batch_size + 7 * E device samples.  0 = off: the pipe and its contexts are as without it
};

// What the pump thread keeps count of, in the order pump_times() reports it: time spent ...
enum PumpCounter {
    kSubmitCall,      // ... in SubmitBatch: expanding a mixed batch, sayuri_hip_submit / sayuri_hip_submit_packed
    kHandOut,         // ... handing a finished batch out: snapshot, flags, root of the wake tree, re-opening the set
    kNap,             // ... asleep with nothing to send and nothing to retire
    kDeviceWait,      // ... inside sayuri_hip_wait
    kWakeParked,      // ... announcing a rotation of the fill set to callers parked for a free staging set
    kPartialBatches,  // NOT a time: batches sent with fewer than batch_size requests
    kGpuQueueEmpty,   // ... with nothing enqueued on the GPU between two batches
    kWaitCallers,     // ... waiting for a closed set's plane copies and for the consumers of the set's previous batch
    kPumpCounters
};

class HipForwardPipe : public NetworkForwardPipe {
public:
    explicit HipForwardPipe(HipPipeConfig cfg = {});
    ~HipForwardPipe() override;

    void Initialize(std::shared_ptr<DNNWeights> weights) override;
    OutputResult Forward(const InputData& input) override;
    void Construct(ForwardPipeOption option, std::shared_ptr<DNNWeights> weights) override;
    void Release() override;
    void Destroy() override;
    bool Valid() const override;
    int GetNumWorkers() const override { return static_cast<int>(graphs_.size()); }

    // The compact-input flavour of Forward (packed_planes.h): same collector, same result
    // bit for bit, 1.8 KB of bit planes per request through staging and PCIe instead of 62 KB of fp32 planes.  A batch
    // made of packed requests only goes to the GPU packed (sayuri_hip_submit_packed); in a mixed batch the pump expands
    // the packed ones into the fp32 staging first.
    OutputResult ForwardPacked(const PackedPlanes& input) SAYURI_EXT_OVERRIDE;
    bool AcceptsPacked() const SAYURI_EXT_OVERRIDE { return true; }

    // The eight board symmetries of one position as ONE request (one slot of the batch, one record over PCIe): the device
    // expands the record under symmetries 1..7 into extra samples behind the batch's own (sayuri_hip_submit_packed_symm).
    // A batch expands at most ensemble_slots requests; one that comes after them is served as a plain identity request --
    // false, out[0] filled, the caller evaluates symmetries 1..7 through ForwardPacked (counted in num_ensemble_fallbacks).
    bool AcceptsEnsemble() const SAYURI_EXT_OVERRIDE { return cfg_.ensemble_slots > 0 && submit_symm_ != nullptr; }
    bool ForwardEnsemble(const PackedPlanes& identity, OutputResult out[8]) SAYURI_EXT_OVERRIDE;
    size_t num_ensemble_fallbacks() const { return ens_fallbacks_.load(std::memory_order_relaxed); }

    // n >= 1 packed requests of ONE caller (an OS thread: a tree search with several playouts in flight) as one call: out[i] is
    // what ForwardPacked(in[i]) returns, bit for bit.  The requests take slots like everybody's (other callers may share the
    // set); the pump leaves the set alone while they are being written and closes it the moment they all are -- a group does
    // not wait for gpu_waittime_ms or the tail rule, whatever else is going on.  A group larger than the forwarding size goes
    // out in chunks of that size, one after the other.  Throws when a batch failed (the pipe stays usable), and from a fiber.
    bool AcceptsGroup() const SAYURI_EXT_OVERRIDE { return true; }
    void ForwardGroup(const PackedPlanes* in, int n, OutputResult* out) SAYURI_EXT_OVERRIDE;

    // A new network of the same architecture into the running pipe (pipe_api.h).  Each device context stages and builds the new
    // weight set on the CALLER's thread while the pump keeps sending batches, then all contexts commit; batches submitted before
    // a context's commit finish on the old set.  Throws with the device's message when a step is refused -- nothing was committed
    // then, the pipe serves the old network.  AcceptsReload() is false on a device library without sayuri_hip_reload_*.
    // Construct(option, weights) keeps its meaning: it rebuilds the graphs.
    bool AcceptsReload() const SAYURI_EXT_OVERRIDE { return accepts_reload_; }
    void Reload(std::shared_ptr<DNNWeights> weights) SAYURI_EXT_OVERRIDE;
    // With several GPUs the graphs commit one after the other (microseconds apart) while requests keep being routed round robin:
    // until Reload has returned, one caller may get the new network from one graph and then the old one from the next.  "Old
    // answers, then new ones" holds per graph, and for every request that begins after Reload has returned.
    int WeightsGeneration() const;  // commits every graph has seen: 0 = never reloaded
    int WeightsVersion() const { return weights_version_.load(std::memory_order_acquire); }  // DNNWeights::version of the network in use

    // batch_forward_pipe.h:27-28.  `inputs` are already re-padded into the NN grid.
    std::vector<OutputResult> BatchForward(int gpu, const std::vector<InputData>& inputs);

    // Non-blocking flavour for M:N self-play schedulers: the result lands in *out and
    // *done flips to 1 (release) once the batch containing it has been evaluated.
    void Submit(const InputData& input, OutputResult* out, std::atomic<int>* done);
    // (Submit: the pump fills *out and flips *done.  Forward: the caller is woken through the batch's wake tree and
    // copies its own result.)

    int board_size() const { return board_size_; }
    int max_batch() const { return max_batch_; }
    bool fp16() const { return cfg_.fp16; }
    sayuri_hip_ctx* ctx(int gpu) const;
    size_t num_batches() const { return batches_.load(std::memory_order_relaxed); }
    size_t num_evals() const { return evals_.load(std::memory_order_relaxed); }
    // the PumpCounters since construction: microseconds, and the count of partial batches as it is
    void pump_times(double out[kPumpCounters]) const {
        for (int i = 0; i < kPumpCounters; ++i)
            out[i] = static_cast<double>(pump_stat_[i].load(std::memory_order_relaxed)) * (i == kPartialBatches ? 1.0 : 1e-3);
    }

private:
    struct Echo {  // what FillOutput needs of the request once its planes are staged
        int board_size;
        PolicyBufferOffset offset;
        float komi;
    };
    struct Request {
        Echo echo;
        OutputResult* output;
        std::atomic<int>* done;
        bool self_serve;  // a blocking Forward() caller: woken through the tree, takes its result itself
        bool fiber;       // a Forward() caller that is a fiber (fiber.h): takes its result itself, no futex: the pump only
                          // flips `done`, the fiber's scheduler thread sees it
    };
    // One batch being assembled or evaluated.  Callers reserve a slot with one atomic add and copy
    // their planes straight into the pinned buffer the GPU will read (one copy per evaluation,
    // done in parallel by the calling threads); `ready` counts finished copies.
    struct Staging {
        static constexpr unsigned kClosed = 1u << 31;
        float* planes{nullptr};
        std::uint32_t* packed{nullptr};      // packed records of the slots filled through ForwardPacked (pinned)
        std::vector<std::uint8_t> is_packed;  // per slot: its planes are in `packed`, not in `planes`
        std::vector<std::uint8_t> is_ens;     // per slot: an ensemble request this batch expands (ForwardEnsemble)
        std::atomic<int> ens_taken{0};        // ensemble requests of the set, counted AFTER the slot is taken: the first E expand
        // pump-private, SubmitBatch: the batch's device samples [0, n) are its slots; expanded slot i has symmetries 1..7 at
        // ens_base[i] .. ens_base[i] + 6, behind n.  fin_ens_base is FinishBatch's snapshot of it (-1: not expanded)
        std::vector<int> ens_base, fin_ens_base, dev_src, dev_symm;
        int dev_n{0};                         // device samples of the submitted batch: n + 7 * expanded slots
        float *prob{nullptr}, *pass{nullptr}, *misc{nullptr}, *own{nullptr};
        std::vector<int> bsz;
        std::vector<Request> reqs;
        std::atomic<unsigned> reserved{0};  // slot counter | kClosed
        std::atomic<unsigned> ready{0};
        unsigned count() const { return reserved.load(std::memory_order_acquire) & ~kClosed; }
        bool closed() const { return (reserved.load(std::memory_order_acquire) & kClosed) != 0; }
        int ticket{-1};      // pump-private: sayuri_hip_submit ticket
        // ---- hand-out of a finished batch to blocking Forward() callers.  The pump wakes ONE of them; every woken
        // caller wakes up to kFanout others (a tree over the batch, log depth), then copies its own result out of the
        // pinned output buffers.  Waking a sleeping thread costs microseconds of kernel time: done serially by the pump
        // it is 0.5 ms for 256 requests and 8 ms for 1024; spread over the callers it is a few wake-ups each, in
        // parallel.  The fin_* arrays are a snapshot of the batch, so the set can take new requests at once.
        static constexpr int kFanout = 8;
        std::vector<Request> fin_reqs;      // requests of the finished batch, blocking callers first come in fin_list order
        std::vector<int> fin_list;          // slots of the blocking callers
        std::vector<int> fin_pos;           // slot -> position in fin_list
        int fin_count{0};
        int fin_fibers{0};                  // fiber callers of the finished batch (they also count in `consumed`)
        std::atomic<int> fin_status{0};     // 1 ok, -1 failed
        std::atomic<int> wakes_done{0};     // callers that have woken their children
        std::atomic<int> consumed{0};       // callers that have taken their result
    };
    struct Graph {  // one per GPU (NNGraph in the reference)
        int device{-1};
        sayuri_hip_ctx* ctx{nullptr};
        static constexpr int kSets = 4;  // ring of staging sets: one fills, up to two are on the GPU, the rest are
                                         // full and queued -- with more leaves in flight than two batches the next
                                         // batch is always ready when the GPU finishes one
        Staging st[kSets];
        std::atomic<int> fill{0};    // index of the staging set new requests go to
        std::atomic<int> epoch{0};   // bumped whenever a set re-opens or the fill index moves: callers that found
                                     // both sets taken sleep on it (futex) instead of polling
        std::thread pump;
        std::mutex dev_mu;  // owner of ctx (pump batch or a direct BatchForward)
        std::mutex mu;      // pump sleep / wake-up only
        std::condition_variable cv;
    };

    struct Pump;  // the pump thread's own state and its two FIFOs (hip_forward_pipe.cc)
    enum CloseReason { kCloseFull, kCloseIdleWait, kCloseTail, kCloseStray, kCloseFlush, kCloseReasons };
    // SAYURI_PIPE_TRACE=1 (read once at construction; a measuring aid, printed to stderr when the graphs are destroyed):
    // when do requests arrive relative to the last finished batch, how full are the batches and why were they closed
    struct Trace {
        bool on{false};
        std::atomic<long long> last_done_ns{0};
        std::atomic<long> arrival[32] = {};  // 250 us bins since the last finished batch
        std::atomic<long> size[17] = {};     // batch size / 16
        std::atomic<long> resume[32] = {};   // fibers: batch finished -> the game runs again
        std::atomic<long> think[32] = {};    // fibers: the game runs again -> its next request
        std::atomic<long> tail[32] = {};     // tail rule: how long the running batch had been running when the set was closed
        std::atomic<long> reason[kCloseReasons] = {};
        static long long now_ns();
        static int bin250us(long long ns) { return static_cast<int>(ns < 0 ? 0 : ns / 250000 > 31 ? 31 : ns / 250000); }
        static void Count(std::atomic<long>& bin) { bin.fetch_add(1, std::memory_order_relaxed); }
        void Dump() const;
    };

    struct Ticket { Graph* g; Staging* s; int slot; };
    static Echo EchoOf(const InputData* input, const PackedPlanes* packed);
    // exactly one of input / packed is non-null
    Ticket Reserve(const InputData* input, const PackedPlanes* packed, OutputResult* out, std::atomic<int>* done, bool self_serve,
                   bool fiber = false, bool ensemble = false);
    // ens_out: null, or the eight results of an ensemble request (out = ens_out[0]); returns whether all eight were filled
    bool ForwardAny(const InputData* input, const PackedPlanes* packed, OutputResult* out, OutputResult* ens_out = nullptr);
    bool TakeResult(Staging* s, int slot, const Echo& echo, int status, OutputResult* out, OutputResult* ens_out = nullptr) const;
    int DeviceBatch() const { return max_batch_ + 7 * std::max(cfg_.ensemble_slots, 0); }
    int BinaryPlanes() const;
    // forwarding size, read live: Construct() may lower it while the pump runs (no rebuild)
    unsigned WantNow() const { return static_cast<unsigned>(std::min(forward_size_.load(std::memory_order_acquire), max_batch_)); }
    void AnnounceEpoch(Graph* g);
    void Reopen(Graph* g, Staging* s);
    void BuildGraphs();
    void DestroyGraphs();
    void PumpLoop(Graph* g);
    bool CloseSet(Pump& p, int set, CloseReason reason);
    bool CloseStrays(Pump& p);
    void CloseFillSet(Pump& p, CloseReason reason);
    void SubmitOldestPending(Pump& p);
    bool OldestIsDone(Pump& p);
    void FinishOldest(Pump& p);
    void SubmitBatch(Graph* g, Staging* s, int n);
    void FinishBatch(Graph* g, Staging* s, int n);
    void StageInput(Staging* s, int slot, const InputData& in, bool already_padded);
    void StagePacked(Staging* s, int slot, const PackedPlanes& in);
    void ExpandPacked(Staging* s, int slot, int dst_slot, int symmetry);
    void FillOutput(const Staging* s, int slot, const Echo& in, bool unpad, OutputResult* out) const;

    // what the callers' own code reads of the network (staging, outputs): fixed by the architecture, so a reload does not move it
    struct NetShape { int version, input_channels, probabilities_channels, pass_probability_outputs, value_misc_outputs; };
    NetShape shape_{};
    bool accepts_reload_{false};
    std::atomic<int> weights_version_{-1};
    std::atomic<bool> valid_{false};  // weights_ != nullptr, for callers that ask while Reload replaces the pointer
    std::mutex reload_mu_;
    HipPipeConfig cfg_;
    int board_size_{0};
    int max_batch_{0};
    std::atomic<int> forward_size_{0};  // batch size the collector forwards at (<= max_batch_); Construct() may lower it live
    std::vector<std::unique_ptr<Graph>> graphs_;
    std::atomic<bool> running_{false};
    std::atomic<unsigned> next_graph_{0};
    std::atomic<size_t> batches_{0}, evals_{0}, ens_fallbacks_{0};
    void* submit_symm_{nullptr};  // sayuri_hip_submit_packed_symm of the device library in use, null when it has none
    mutable std::atomic<long long> pump_stat_[kPumpCounters] = {};  // nanoseconds, but kPartialBatches: a count
    struct PumpTimer;  // adds its own lifetime to one of them
    std::atomic<int> epoch_parked_{0};  // fibers suspended in Reserve() until a staging set re-opens
    // ForwardGroup callers that are writing their requests into the fill set (the pumps leave a partial set open meanwhile) and
    // callers that wait for a group's results (the FLUSH: the pumps close a non-empty fill set at once while it is raised)
    std::atomic<int> group_filling_{0}, group_flush_{0};
    void WakePumps();
    Trace trace_;
    // SAYURI_PIPE_TAIL (measuring aid): the fraction of a batch's time after which a partial set is enqueued behind it
    double tail_frac_{0.93};
};

SAYURI_HOST_END
