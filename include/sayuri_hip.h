/* include/sayuri_hip.h -- C-ABI of the MI355X (gfx950) forward-pipe engine.
 *
 * This is the drop-in boundary for Sayuri's NN hot path.  In the reference the path sits
 * behind `class NetworkForwardPipe` (reference src/neural/network_basic.h:132-161) and, for
 * GPU backends, `BatchForwardPipe::BatchForward(int gpu, const std::vector<InputData>&)`
 * (reference src/neural/batch_forward_pipe.h:27-28), implemented for CUDA by
 * `CudaForwardPipe::NNGraph` (reference src/neural/cuda/cuda_forward_pipe.cc:133-1090).
 * A `HipForwardPipe` (sayuri_amd/csrc/host/hip_forward_pipe.h, or the stub shown in
 * INTEGRATION.md inside the reference tree) owns one `sayuri_hip_ctx` per GPU and calls the
 * entry points below; no HIP or torch type crosses this header.
 *
 * Conventions: plain C, pointers + sizes, return 0 on success / -1 on failure with the
 * message in sayuri_hip_last_error() (thread-local); no exception crosses the ABI
 * (the C++ pipe turns -1 into std::runtime_error like reference cuda_common.cc:46-62).
 * One ctx per GPU; a ctx is driven by ONE caller thread at a time (the pump thread).
 */
#ifndef SAYURI_HIP_H
#define SAYURI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sayuri_hip_ctx sayuri_hip_ctx;

/* reference src/neural/activation.h:8-17 (enum class Activation) */
enum {
    SAYURI_ACT_IDENTITY = 0, SAYURI_ACT_RELU = 1, SAYURI_ACT_ELU = 2, SAYURI_ACT_SELU = 3,
    SAYURI_ACT_GELU = 4, SAYURI_ACT_MISH = 5, SAYURI_ACT_SWISH = 6, SAYURI_ACT_HARDSWISH = 7
};

/* reference src/neural/description.h:92-93 (BlockBasic::Type) */
enum {
    SAYURI_BLOCK_RESIDUAL = 1, SAYURI_BLOCK_BOTTLENECK = 2, SAYURI_BLOCK_NESTED_BOTTLENECK = 3,
    SAYURI_BLOCK_MIXER = 4
};

/* One tower block: mirrors the shape fields of reference description.h:90-137 (BlockBasic). */
typedef struct {
    int32_t type;                 /* SAYURI_BLOCK_* */
    int32_t apply_se;             /* BlockBasic::apply_se */
    int32_t se_size;              /* BlockBasic::se_size */
    int32_t bottleneck_channels;  /* BlockBasic::bottleneck_channels (0 if n/a) */
    int32_t feedforward_channels; /* BlockBasic::feedforward_channels (0 if n/a) */
    int32_t dw_filter;            /* dw_conv.GetFilter() for mixer blocks (0 if n/a) */
} sayuri_hip_blockdesc;

/* The architecture part of reference description.h:164-215 (DNNWeights). */
typedef struct {
    int32_t version;                  /* DNNWeights::version (1..5) */
    int32_t input_channels;           /* 43 (v3+) or 38 */
    int32_t residual_channels;
    int32_t residual_blocks;
    int32_t policy_head_channels;
    int32_t value_head_channels;
    int32_t probabilities_channels;   /* 5 (v3+) or 1 */
    int32_t pass_probability_outputs; /* 5 (v3+) or 1 */
    int32_t ownership_channels;       /* 1 */
    int32_t value_misc_outputs;       /* 15 (v3+) or 5 */
    int32_t default_act;              /* SAYURI_ACT_* */
    int32_t policy_head_type;         /* 0 = kNormal, 1 = kRepLK */
    int32_t policy_dw_filter;         /* p_dw_conv.GetFilter() when RepLK, else 0 */
    const sayuri_hip_blockdesc* blocks; /* [residual_blocks] */
} sayuri_hip_netdesc;

/* Layer ids for sayuri_hip_load_tensor: the named members of DNNWeights / BlockBasic. */
enum {
    SAYURI_L_INPUT_CONV = 0, SAYURI_L_P_HD_CONV = 1, SAYURI_L_P_DW_CONV = 2, SAYURI_L_P_PT_CONV = 3,
    SAYURI_L_P_INTER_FC = 4, SAYURI_L_PROB_CONV = 5, SAYURI_L_PASS_FC = 6, SAYURI_L_V_HD_CONV = 7,
    SAYURI_L_V_INTER_FC = 8, SAYURI_L_V_OWNERSHIP = 9, SAYURI_L_V_MISC = 10,
    SAYURI_L_BLOCK_BASE = 16 /* block b, slot s -> 16 + 16*b + s */
};
enum { /* slots inside a block */
    SAYURI_S_CONV1 = 0, SAYURI_S_CONV2 = 1, SAYURI_S_CONV3 = 2, SAYURI_S_CONV4 = 3,
    SAYURI_S_PRE_BTL = 4, SAYURI_S_POST_BTL = 5, SAYURI_S_DW_CONV = 6, SAYURI_S_SQUEEZE = 7,
    SAYURI_S_EXCITE = 8
};
#define SAYURI_L_BLOCK(b, slot) (SAYURI_L_BLOCK_BASE + 16 * (b) + (slot))
enum { SAYURI_T_WEIGHTS = 0, SAYURI_T_BIASES = 1 };

/* Number of visible gfx950 devices (replaces reference src/utils/probe_gpu.h:10-27 GetGpuCount). */
int sayuri_hip_device_count(void);

/* Build the per-GPU graph: replaces NNGraph::ConstructGraph (cuda_forward_pipe.cc:133-613).
 * `board` is the NN board size (ForwardPipeOption::board_size), `max_batch` the largest batch
 * BatchForward will be handed, `use_fp16` mirrors option "fp16" (1: fp16 storage + MFMA with
 * fp32 accumulation; 0: fp32 storage + fp32 MFMA, the strict-parity mode). NULL on failure. */
sayuri_hip_ctx* sayuri_hip_create(int device, const sayuri_hip_netdesc* desc, int max_batch,
                                  int board, int use_fp16);

/* The same with option flags.  SAYURI_HIP_LATENCY makes a LATENCY CONTEXT for the small batches of a playing or analysing engine
 * (1 to 16 positions): every fp16 3x3 tower convolution whose padded output channels are a multiple of 64 is cut into many
 * small workgroups (csrc/hip/conv_split.h: 64 channels x a strip of board rows each), so that a lone board's layer runs on tens
 * of CUs instead of one to three.  Such a context takes that route for EVERY batch, whatever its size (a position's result
 * does not depend on its batch), has no persistent tower launch (sayuri_hip_tower_state = 0), runs no chains and runs every SE
 * unit as ONE launch behind its convolution (se_unit_kernel, csrc/hip/small_ops.h: the bits of se_pool / se_fc / se_scale, which
 * SAYURI_SE_ONE=0 runs instead, as do batches of more than 85 full 19x19 boards on 256 channels and 51 on 384); its outputs are
 * those of a default context created under SAYURI_TOWER=0 SAYURI_SE_FUSED=0 SAYURI_SE_SPLIT=0, bit for bit.  Full batches are what
 * the default context is for (INTEGRATION.md says where they cross).
 * fp16 engine only: flags != 0 with use_fp16 == 0 returns NULL with a message.  sayuri_hip_create is create_ex(..., 0) --
 * unless SAYURI_LATENCY=1 is set in the environment, which gives an fp16 context the flag (for callers that cannot pass one).
 * SAYURI_LATENCY_SPLIT=n forces n strips per board instead of the engine's choice (measurements, tests). */
enum { SAYURI_HIP_LATENCY = 1 };
sayuri_hip_ctx* sayuri_hip_create_ex(int device, const sayuri_hip_netdesc* desc, int max_batch,
                                     int board, int use_fp16, unsigned flags);

/* Hand one host tensor of DNNWeights to the device (replaces the LoadWeights calls of
 * cuda_layers.cc:621-716).  Tensors are the BN-folded fp32 arrays the reference loader
 * produces: conv weights [K][C][k][k] (depthwise [C][1][k][k]), fc weights [out][in],
 * biases [K].  `n` must equal the element count implied by the netdesc. */
int sayuri_hip_load_tensor(sayuri_hip_ctx* ctx, int layer_id, int kind, const float* host, size_t n);

/* LIVE WEIGHT RELOAD: a new network of the SAME architecture into a context that keeps serving forwards (the reference
 * rebuilds its graph: CudaForwardPipe::Construct with weights, cuda_forward_pipe.cc:44-119).  Everything a forward reads that
 * is derived from the weights is one WEIGHT SET with device buffers of its own; a reload builds a second set beside the live
 * one and swaps them between two forwards.  No forward sees a mixture; a context that is never reloaded does what it always did.
 *   sayuri_hip_reload_begin    opens a reload.  -1 with a message that names the difference, the context unchanged, when
 *                              `desc` differs from the context's in anything that shapes buffers or kernels (block count,
 *                              types and widths, SE placement and widths, head type and widths, input / output channels,
 *                              activation, version as far as it selects the encoder); when a reload is already open; while
 *                              the context is inside sayuri_hip_time_runs / sayuri_hip_profile_run.
 *   sayuri_hip_load_tensor     while a reload is open: fills the STAGED set, same layer ids and kinds.  (Outside a reload it
 *                              stays refused after the first forward.)
 *   sayuri_hip_reload_prepare  the heavy step: checks that every tensor is there, builds all images, uploads them into NEW
 *                              device buffers (the live set is never written in place).  On failure -1, the staged set is
 *                              freed, the reload is closed and the context is unchanged.
 *   sayuri_hip_reload_commit   the light step, a pointer flip: forwards enqueued after it returns use the new set, forwards
 *                              enqueued before it finish on the old one.  Returns the new generation (>= 1); -1 without a
 *                              prepared reload.  The old set's memory is given back once every forward enqueued before the
 *                              commit has finished ON THE DEVICE (events behind them on the tickets' streams; nobody needs to
 *                              have waited for those tickets): submit, wait and device_bytes look, and
 *                              sayuri_hip_device_bytes is then what it was before the reload.
 *   sayuri_hip_reload_abort    drops an open reload, prepared or not.
 *   sayuri_hip_weights_generation   0 for a context that was never reloaded, +1 per commit.
 * Threads: begin / load_tensor / prepare may run on one thread while another calls submit / wait / query on the same context:
 * they touch the staged set only (prepare's uploads slow the forwards beside it, nothing more).  commit is serialised with
 * submit by the context itself: any thread may call it.  The fp32 engine, latency contexts and contexts that run chains or
 * ensemble batches take reloads the same way. */
int sayuri_hip_reload_begin(sayuri_hip_ctx* ctx, const sayuri_hip_netdesc* desc);
int sayuri_hip_reload_prepare(sayuri_hip_ctx* ctx);
int sayuri_hip_reload_commit(sayuri_hip_ctx* ctx);
int sayuri_hip_reload_abort(sayuri_hip_ctx* ctx);
int sayuri_hip_weights_generation(const sayuri_hip_ctx* ctx);

/* One batch through the net: replaces NNGraph::BatchForward (cuda_forward_pipe.cc:684-1018)
 * up to, not including, FillOutputs.
 *   planes      [n][input_channels][board*board]  each sample already re-padded top-left into
 *               the NN grid as BatchForwardPipe::SendQueryAndWait does (batch_forward_pipe.cc:15-33)
 *   board_sizes [n]  the sample's own board size (InputData::board_size), NULL = all `board`
 *   prob [n][probabilities_channels][board*board], pass [n][pass_probability_outputs],
 *   misc [n][value_misc_outputs], own [n][board*board]   raw (pre-softmax/tanh) outputs in the
 *               NN grid; off-board entries of smaller samples are 0.
 * Blocking; host pointers. */
int sayuri_hip_forward(sayuri_hip_ctx* ctx, int n, const float* planes, const int* board_sizes,
                       float* prob, float* pass, float* misc, float* own);

/* The three phases of sayuri_hip_forward, for callers that keep inputs resident in HBM
 * (bench.py times `run` only) or overlap copies with compute. upload/download block. */
int sayuri_hip_upload(sayuri_hip_ctx* ctx, int n, const float* planes, const int* board_sizes);
int sayuri_hip_run(sayuri_hip_ctx* ctx);   /* asynchronous on the ctx stream */
int sayuri_hip_sync(sayuri_hip_ctx* ctx);
int sayuri_hip_download(sayuri_hip_ctx* ctx, float* prob, float* pass, float* misc, float* own);

/* Pipelined form for the pump thread: enqueue H2D + the whole graph + D2H on the ctx stream and
 * return at once; `ticket` (0 or 1, two batches may be in flight) is waited for / polled later.
 * All host buffers must be page-locked and stay valid until the wait.  `pass` and `misc` are written by the heads kernel
 * itself when the device can address them -- memory from sayuri_hip_host_alloc (or any other page-locked memory that is
 * MAPPED into the device's address space); a buffer that is page-locked but not mapped is detected once per pointer
 * (hipHostGetDevicePointer) and served through copies.  Packed records (sayuri_hip_submit_packed) in such memory are likewise
 * read by the first kernel where they lie, with no copy: they must stay UNCHANGED until the wait, not merely valid. */
int sayuri_hip_submit(sayuri_hip_ctx* ctx, int n, const float* planes, const int* board_sizes, float* prob,
                      float* pass, float* misc, float* own, int* ticket);
/* The same two entry points for PACKED planes (sayuri_amd/csrc/host/packed_planes.h; SURVEY.md section 8 row f1, the
 * encoder on the critical path -- reference src/neural/encoder.cc:101-368 fills 43 fp32 planes per evaluation).
 *   records  [n][binary_planes*12 + 8] 32-bit words: bits[binary_planes][12] (bit y*bs+x of a 0/1 plane, in the
 *            SAMPLE's own cell order -- no re-padding into the NN grid), then 8 floats (the value of each broadcast
 *            plane: rule, wave, komi/20, -komi/20, N/361, 1 for 43-plane nets)
 *   binary_planes = input_channels - 6 (37) for v3+ nets, 34 for the 38-plane v1/v2 encoder
 *            A record holds at most 40 bit planes and 8 scalars: any other count returns -1 with a message, nothing is launched.
 * 1.8 KB per sample instead of 62 KB; the first kernel expands the bits into the fp16 activations, the network sees the
 * same values as through sayuri_hip_forward and returns bit-identical outputs. */
int sayuri_hip_forward_packed(sayuri_hip_ctx* ctx, int n, const unsigned* records, int binary_planes, const int* board_sizes,
                              float* prob, float* pass, float* misc, float* own);
int sayuri_hip_submit_packed(sayuri_hip_ctx* ctx, int n, const unsigned* records, int binary_planes, const int* board_sizes,
                             float* prob, float* pass, float* misc, float* own, int* ticket);
/* The same two entry points with a RECORD MAP and a BOARD SYMMETRY per device sample: the eight symmetries of a position
 * (reference Network::kAverage, src/neural/network.cc:258) travel as ONE record and are expanded on the device.
 *   n          device samples (<= max_batch); outputs are per device sample, in the caller's order, as above
 *   records    [n_records] records as above (1 <= n_records <= max_batch)
 *   src   [n]  the record of sample i, 0..n_records-1; several samples may name one record.  NULL = the identity map
 *              (sample i reads record i; needs n <= n_records)
 *   symm  [n]  the symmetry of sample i, 0..7: cell d = y*bs + x of the sample shows record cell Index(bs, symm, d) of
 *              reference src/game/symmetry.cc:97-123 -- tx = x, ty = y; symm & 4: swap tx and ty; symm & 2: tx = bs-1-tx;
 *              symm & 1: ty = bs-1-ty; source cell ty*bs + tx.  The broadcast planes are unaffected.  Sample i's outputs are
 *              those of sayuri_hip_forward_packed on the record so permuted (the record Encoder::Packed builds for that
 *              symmetry), bit for bit; the caller maps them back with its own tables.
 *   board_sizes [n]  board_sizes[i] is the board size of record src[i]: the CALLER's contract, a record does not carry its
 *              size.  NULL = all `board`.
 * With symm all 0 and src the identity map the results are those of sayuri_hip_forward_packed.  A symm outside 0..7, a src
 * outside the record array, n_records outside 1..max_batch or n outside 1..max_batch returns -1 with a message before
 * anything is launched.  The two small tables are copied by the call (they need not outlive it, nor be page-locked). */
int sayuri_hip_forward_packed_symm(sayuri_hip_ctx* ctx, int n, const unsigned* records, int n_records, int binary_planes,
                                   const int* board_sizes, const int* src, const int* symm, float* prob, float* pass,
                                   float* misc, float* own);
int sayuri_hip_submit_packed_symm(sayuri_hip_ctx* ctx, int n, const unsigned* records, int n_records, int binary_planes,
                                  const int* board_sizes, const int* src, const int* symm, float* prob, float* pass,
                                  float* misc, float* own, int* ticket);
int sayuri_hip_wait(sayuri_hip_ctx* ctx, int ticket);
int sayuri_hip_query(sayuri_hip_ctx* ctx, int ticket); /* 1 = finished, 0 = still running, -1 = error */

/* Time `iters` back-to-back runs of the uploaded batch with HIP events on the ctx stream
 * (torch.cuda.Event cannot see this stream). total_ms = wall of all iters on the device. */
int sayuri_hip_time_runs(sayuri_hip_ctx* ctx, int iters, float* total_ms);

/* Per-kernel-class device time of ONE run of the uploaded batch (events around every launch).
 * Fills up to `cap` rows; returns the row count, -1 on error. */
typedef struct {
    char name[48];
    int32_t launches;
    float total_ms;
    double flops;  /* algorithmic FLOPs (2*MAC of the direct convolution) of those launches */
    double bytes;  /* algorithmic HBM bytes (inputs + outputs + weights once) of those launches */
} sayuri_hip_kernel_stat;
int sayuri_hip_profile_run(sayuri_hip_ctx* ctx, sayuri_hip_kernel_stat* rows, int cap);

/* Per-launch timing INSIDE the timed region: after sayuri_hip_mark_kernel(ctx, "conv3x3_tower"),
 * every launch of that kernel class during sayuri_hip_time_runs is bracketed by an
 * un-synchronised HIP event pair on the ctx stream; sayuri_hip_timed_stat returns their sum
 * (launch count, total ms, algorithmic FLOPs/bytes).  NULL / "" disables marking. */
int sayuri_hip_mark_kernel(sayuri_hip_ctx* ctx, const char* name);
int sayuri_hip_timed_stat(sayuri_hip_ctx* ctx, sayuri_hip_kernel_stat* row);

/* Page-locked host memory for the staging buffers handed to upload/download/forward
 * (replaces the cudaHostAlloc staging of reference cuda_common.cc:312-403); the host side
 * never includes a HIP header. */
void* sayuri_hip_host_alloc(size_t bytes);
void sayuri_hip_host_free(void* p);

/* Bytes of device memory held by the ctx. */
size_t sayuri_hip_device_bytes(const sayuri_hip_ctx* ctx);

/* How many chains the last forward of the ctx was run as (measurement / tests).  A batch whose layers are more than one
 * round of workgroups on a network without the persistent launch (configs[4]: 40b x 384) is cut into groups of board tiles,
 * each a chain of per-layer launches on a stream of its own -- the reference has one stream per GPU and one launch per
 * kernel (cuda_forward_pipe.cc:713-981).  SAYURI_CHAINS=1 turns it off, =N forces N. */
int sayuri_hip_last_chains(const sayuri_hip_ctx* ctx);

/* 1 when the ctx runs its residual tower as ONE persistent launch (the code object of csrc/hip/conv_tower.h is in the library
 * and loaded), 0 when it falls back to one launch per layer -- a build whose assembly post-processor (tower_seam.py, validated
 * on ROCm 7.2's hipcc) rejected the compiler's output, SAYURI_TOWER=0, or the fp32 engine.  bench.py prints it on its line.
 * The reference always launches per layer (cuda_forward_pipe.cc:713-981). */
int sayuri_hip_tower_state(const sayuri_hip_ctx* ctx);

/* 1 when the ctx is a latency context (sayuri_hip_create_ex with SAYURI_HIP_LATENCY, or SAYURI_LATENCY=1): its fp16 3x3 layers
 * take the split route; 0 for a default context. */
int sayuri_hip_latency_state(const sayuri_hip_ctx* ctx);

/* The weight ring of a latency context's split convolutions (csrc/hip/conv_split.h: conv_split_kernel<NJ, ST>).  A strip's K
 * loop takes its weights through a ring of ST groups in LDS; the thin strips of a small batch (NJ = 1, 2, 3 column tiles per
 * wave) have a deep ring beside the three-stage one, and the engine's rule (csrc/hip/engine_plan.h: split_ring) picks by NJ.
 * The ring decides speed only: the K order, and so every bit of the output, is the same.  SAYURI_LATENCY_RING=n forces n stages
 * (3: the three-stage kernel everywhere); a depth that the chosen variant does not have, or whose LDS does not fit, is an error
 * of the forward.
 * sayuri_hip_split_ring_plan is host arithmetic (no device is touched): the stages a latency context gives a batch of n boards
 * and a 3x3 layer of `cout` output channels under `strips` strips per board and `ring` stages, 0 meaning the engine's choice
 * for either; -1 with a message where no split applies -- weight rows that are not whole 64-channel tiles, a forced ring that
 * does not exist or does not fit.
 * sayuri_hip_last_split_ring is the deepest ring any split convolution of the ctx's last forward ran with, 0 if none ran (a
 * default context); with ctx == NULL, the ring of the calling thread's last sayuri_hip_test_conv_split launch. */
int sayuri_hip_split_ring_plan(int n, const int* board_sizes, int max_board, int cout, int strips, int ring);
int sayuri_hip_last_split_ring(const sayuri_hip_ctx* ctx);

/* The tower's 1x1 convolutions of bottleneck-family networks (csrc/hip/conv_pw.h: conv_pw_kernel<NJ>).  In the fp16 engine a
 * block's PRE_BTL / POST_BTL layer and a mixer block's CONV1 / CONV2, when they map whole 32-channel chunks onto whole 64-channel
 * tiles, run as many small independent workgroups -- one per (sample, piece of that sample's pixels, 64 output channels) -- in a
 * default and in a latency context alike -- where the engine's speed rule says it pays --, with the bits of the generic kernel.
 * SAYURI_PW=0 keeps the generic kernel everywhere, SAYURI_PW=1 takes conv_pw.h wherever it applies;
 * SAYURI_PW_PIECES=n forces n pieces per sample.  The cut decides speed only.
 * sayuri_hip_pw_plan is host arithmetic (no device is touched): out = {pieces asked for per sample, grid, NJ (column tiles per
 * wave of the variant), LDS bytes} of a batch of n boards and a cin -> cout layer under `pieces` pieces per sample, 0 meaning the
 * engine's choice; -1 with a message where no plan applies -- cout % 64, cin % 32, a forced cut whose pieces are wider than the
 * kernel holds.  (Whether a context takes the plan is the speed rule's business: csrc/hip/engine_plan.h, pw_pays; SAYURI_PW=1
 * takes it wherever it applies.)
 * sayuri_hip_last_pw_launches counts the conv_pw launches of the ctx's last forward: 0 under SAYURI_PW=0 and for every network
 * without such layers. */
int sayuri_hip_pw_plan(int n, const int* board_sizes, int max_board, int cin, int cout, int pieces, int out[4]);
int sayuri_hip_last_pw_launches(const sayuri_hip_ctx* ctx);

/* The depthwise k x k convolutions (a mixer block's DW_CONV, the RepLK policy head's P_DW_CONV) on LDS (csrc/hip/conv_dw.h:
 * conv_dw_kernel<k>, k = 3, 5, 7).  In the fp16 engine such a layer runs as many small independent workgroups -- one per (sample,
 * slice of 64 or 32 channels, strip of rows) that stages its rows, the halo rows inside the board and the slice's weights into LDS
 * once -- where the engine's speed rule says it pays (csrc/hip/engine_plan.h, dw_pays), with the bits of depthwise_kernel.
 * SAYURI_DW=0 keeps depthwise_kernel everywhere, SAYURI_DW=1 takes conv_dw.h wherever it applies; SAYURI_DW_STRIPS=n forces n strips
 * per sample.  The cut decides speed only.
 * sayuri_hip_dw_plan is host arithmetic (no device is touched): out = {channels of a slice, strips asked for per sample (a board
 * with fewer rows has one strip per row), grid, LDS bytes} of a batch of n boards and a layer of `channels` channels (stride: the
 * next multiple of 32) under `strips` strips per sample, 0 meaning the engine's choice; -1 with a message where no plan applies --
 * k other than 3, 5, 7, more strips than the largest board has rows, an item beyond the kernel's 64 KiB of LDS.
 * sayuri_hip_last_dw_launches counts the conv_dw launches of the ctx's last forward: 0 under SAYURI_DW=0 and for every network
 * without a depthwise layer. */
int sayuri_hip_dw_plan(int n, const int* board_sizes, int max_board, int channels, int k, int strips, int out[4]);
int sayuri_hip_last_dw_launches(const sayuri_hip_ctx* ctx);

/* Release everything (replaces NNGraph::DestroyGraph, cuda_forward_pipe.cc:1092-1130). */
void sayuri_hip_destroy(sayuri_hip_ctx* ctx);

const char* sayuri_hip_last_error(void);

/* ---- layer-level taps for the parity tests (not used by the pipe) ---------------------- */
/* One convolution layer on host NCHW fp32 tensors, through the same device kernels:
 * x [n][cin][bs*bs] with per-sample board sizes (compact, stride bs*bs per channel),
 * w [cout][cin][k][k], bias [cout] or NULL, res like the output or NULL,
 * y [n][cout][bs*bs].  k = 1 or 3 (MFMA implicit GEMM) or depthwise (cin == 1 in w). */
int sayuri_hip_test_conv(int device, int use_fp16, int n, const int* board_sizes, int max_board,
                         int cin, int cout, int k, int depthwise, int act, int post_residual,
                         const float* x, const float* w, const float* bias, const float* res,
                         float* y);
/* The fp16 3x3 case of sayuri_hip_test_conv through the latency context's kernel (conv_split.h), with a forced split:
 * strips = strips per board (0: the engine's choice for this batch; a board gets at most one strip per row),
 * channel_tiles = 0 or the layer's number of 64-channel tiles (the kernel has one channel tile size; another count is an
 * error, as is a layer whose padded output channels are not a multiple of 64).  Same results as sayuri_hip_test_conv's
 * board kernel, bit for bit. */
int sayuri_hip_test_conv_split(int device, int n, const int* board_sizes, int max_board, int cin, int cout, int act,
                               const float* x, const float* w, const float* bias, const float* res, float* y,
                               int channel_tiles, int strips);
/* The fp16 1x1 case of sayuri_hip_test_conv through conv_pw.h, the route of a tower 1x1 layer: pieces = pieces per sample (0: the
 * engine's choice for this batch).  -1 with a message for a layer outside the route (cout % 64, cin % 32) and for a forced cut
 * that does not fit (a piece wider than 24 column tiles).  y's device buffer is pre-set to NaN.  Same results as
 * sayuri_hip_test_conv's generic kernel, bit for bit; sayuri_hip_test_last_conv_kind reports 6. */
int sayuri_hip_test_conv_pw(int device, int n, const int* board_sizes, int max_board, int cin, int cout, int act, const float* x,
                            const float* w, const float* bias, const float* res, float* y, int pieces);
/* One fp16 depthwise k x k layer through conv_dw.h: x, res (or NULL: no residual; given, it is added BEHIND the activation, as
 * sayuri_hip_test_conv's post_residual = 1 does), y are [n][channels][bs*bs]; w [channels][k*k]; strips = strips per sample (0:
 * the engine's choice for this batch).  use_fp16 must be 1: the fp32 engine keeps depthwise_kernel.  -1 with a message for what
 * the route does not cover (k other than 3, 5, 7, fp32, a forced cut that does not fit).  y's device buffer is pre-set to NaN.
 * Same results as sayuri_hip_test_conv(depthwise = 1), bit for bit; sayuri_hip_test_last_conv_kind reports 7. */
int sayuri_hip_test_conv_dw(int device, int use_fp16, int n, const int* board_sizes, int max_board, int channels, int k, int act,
                            const float* x, const float* w, const float* bias, const float* res, int strips, float* y);
/* The pad channels [channels, stride) of every board pixel after the calling thread's last sayuri_hip_test_conv_dw, as raw fp16
 * bits in sample-major, pixel-major order: which = 0 what conv_dw_kernel stored into its NaN-pre-set buffer, which = 1 what
 * depthwise_kernel stores on the same operands (the tap runs it into a NaN-pre-set buffer of its own).  Copies up to cap values;
 * returns how many there are (0: channels is a multiple of 32), -1 on a bad argument. */
int sayuri_hip_test_last_dw_pad(int which, unsigned short* bits, int cap);
/* Kernel family the calling thread's last sayuri_hip_test_conv / sayuri_hip_test_conv_split / sayuri_hip_test_conv_sx ran:
 * 0 generic implicit GEMM (conv_mfma.h), 1 LDS-DMA tiles across samples (conv_glds.h), 2 one workgroup per board
 * (conv_board.h), 3 depthwise, 4 many small workgroups (conv_split.h), 5 the split-channel SE convolution (conv_board_sx.h),
 * 6 the pointwise tower kernel (conv_pw.h; sayuri_hip_test_conv_pw only), 7 the depthwise kernel on LDS (conv_dw.h;
 * sayuri_hip_test_conv_dw only). */
int sayuri_hip_test_last_conv_kind(void);
/* One squeeze-and-excitation unit through the se_pool / se_fc / se_scale kernels (reference SEUnit::Forward,
 * src/neural/blas/se_unit.cc:70-128): x, res (or NULL), y are [n][channels][bs*bs] like sayuri_hip_test_conv's tensors,
 * w1 [se_size][3*channels], b1 [se_size], w2 [2*channels][se_size], b2 [2*channels];
 * gate (or NULL) receives [n][2*channels] = sigmoid(gamma) | beta, i.e. GlobalPooling<false> + both FullyConnects.
 * Honours SAYURI_SE_ONE, read per call: =1 runs the unit as one launch (se_unit_kernel), same bits. */
int sayuri_hip_test_se_unit(int device, int use_fp16, int n, const int* board_sizes, int max_board, int channels,
                            int se_size, int act, const float* x, const float* res, const float* w1, const float* b1,
                            const float* w2, const float* b2, float* y, float* gate);
/* Everything after the two head convolutions in one launch (head_tail_kernel; reference blas_forward_pipe.cc:496-580):
 * pconv [n][policy_channels][bs*bs], vconv [n][value_channels][bs*bs] (activated head convolutions),
 * weights12 = { p_inter w [Cp][3Cp], b; pass_fc w [pass_outs][Cp], b; v_inter w [3Cv][3Cv], b; v_misc w [misc_outs][3Cv], b;
 * prob_conv w [prob_channels][Cp], b; ownership w [Cv], b[1] };  outputs in the NN grid as sayuri_hip_forward's. */
int sayuri_hip_test_head_tail(int device, int use_fp16, int n, const int* board_sizes, int max_board, int policy_channels,
                              int value_channels, int prob_channels, int pass_outs, int misc_outs, int act,
                              const float* pconv, const float* vconv, const float* const* weights12, float* prob,
                              float* pass, float* misc, float* own);

/* The two fused kernels of the fp16 engine at kernel level (round 3):
 * sayuri_hip_test_conv_se   a channels -> channels 3x3 convolution (w [C][C][3][3], bias [C]) with the SE unit that follows
 *   it INSIDE the kernel (conv_board_se_kernel; via_tower != 0: the same stage inside a one-layer run of the persistent
 *   tower kernel): y = act(sigmoid(gamma) * conv(x) + beta + res), reference SEUnit::Forward on the convolution's output
 *   (se_unit.cc:70-128).  Tensors as in sayuri_hip_test_conv / sayuri_hip_test_se_unit.
 * sayuri_hip_test_head_board   both heads of a sample in one workgroup (head_board_kernel): trunk [n][channels][bs*bs],
 *   p_w [Cp][channels], p_b [Cp], v_w [Cv][channels], v_b [Cv] (the two 1x1 head convolutions, reference
 *   blas_forward_pipe.cc:449-495), weights12 and outputs as in sayuri_hip_test_head_tail.
 * Both return 1 (not an error) when the fused kernel does not apply to the arguments: the engine then runs the separate
 * kernels (several samples per tile / channel counts without a kernel variant). */
int sayuri_hip_test_conv_se(int device, int n, const int* board_sizes, int max_board, int channels, int se_size, int act,
                            int via_tower, const float* x, const float* w, const float* bias, const float* res, const float* w1,
                            const float* b1, const float* w2, const float* b2, float* y);
/* Form of the SE stage the calling thread's last sayuri_hip_test_conv_se launched (either kernel): 0 it launched nothing,
 * 1 both FC images staged into LDS as fp16 (make_se_images fits), 2 the FCs read their fp32 weights from L2. */
int sayuri_hip_test_last_se_form(void);
/* A RUN of nlayers = 1..8 board convolutions as ONE launch of the persistent tower kernel (conv_tower.h), every layer built and
 * the run linked by the engine's own host code: layer 0 is cin0 -> channels, every later layer channels -> channels, channels =
 * 128 or 256 (the two widths of the kernel).  act [nlayers]; res_from [nlayers]: -1 no residual, 0 the run's input (cin0 ==
 * channels), k the output of layer k - 1; w = [channels][cin0][3][3], then [channels][channels][3][3] per later layer; bias
 * [nlayers][channels].  se_layer >= 0: that layer carries the SE unit (se_size, w1, b1, w2, b2 as in sayuri_hip_test_conv_se,
 * which also states when the stage applies; sayuri_hip_test_last_se_form reports its form), < 0: none.  chain = 1: the weight
 * hand-over between layers where the engine's rule allows it, 0: none.  x [n][cin0][bs*bs]; y [nlayers][n][channels][bs*bs]
 * receives EVERY layer's output (each layer writes a buffer of its own, pre-set to NaN).  Returns 1 when the batch has no
 * board plan, -1 on bad arguments.
 * sayuri_hip_test_last_tower_run: out = {layers, layers that took the generated epilogue (row order), hand-over links} of the
 * calling thread's last sayuri_hip_test_tower_run launch (zeros: that call launched nothing). */
int sayuri_hip_test_tower_run(int device, int n, const int* board_sizes, int max_board, int channels, int cin0, int nlayers,
                              const int* act, const int* res_from, const float* w, const float* bias, int se_layer, int se_size,
                              const float* w1, const float* b1, const float* w2, const float* b2, int chain, const float* x,
                              float* y);
int sayuri_hip_test_last_tower_run(int out[3]);
/* sayuri_hip_test_conv_se's layer when its channels are split over 2..4 workgroups of 128 per board tile, which exchange their
 * partial squeeze sums inside the launch (conv_board_sx_kernel, conv_board_sx.h; the 40b x 384 network): same tensors, same
 * y = act(sigmoid(gamma) * conv(x) + beta + res).  The images, the board plan and the launch are the engine's own host code;
 * the exchange buffer is fresh and zeroed, the tag fixed.  Returns 1 (not an error) when the form does not apply: channels
 * (padded to 32) that are not 2..4 whole tiles of 128, an SE width the images do not fit (se_size % 4, se_size > 128, or
 * the two images larger than the kernel's LDS stage), or a board of the batch of which more than 4 fit a tile (8x8 and
 * smaller).  -1 when a workgroup's wait for its siblings ran out.
 * sayuri_hip_test_last_sx_kts: channel tiles per board tile of the calling thread's last sayuri_hip_test_conv_sx launch
 * (0: that call launched nothing). */
int sayuri_hip_test_conv_sx(int device, int n, const int* board_sizes, int max_board, int channels, int se_size, int act,
                            const float* x, const float* w, const float* bias, const float* res, const float* w1,
                            const float* b1, const float* w2, const float* b2, float* y);
int sayuri_hip_test_last_sx_kts(void);
int sayuri_hip_test_head_board(int device, int n, const int* board_sizes, int max_board, int channels, int policy_channels,
                               int value_channels, int prob_channels, int pass_outs, int misc_outs, int act, const float* trunk,
                               const float* p_w, const float* p_b, const float* v_w, const float* v_b,
                               const float* const* weights12, float* prob, float* pass, float* misc, float* own);

/* The input stage, the first kernel of every forward: planes or packed records -> the input convolution's NHWC image.  ONE of
 * pack_input_kernel (chunked), pack_input_flat_kernel, pack_bits_kernel, pack_bits_symm_kernel (csrc/hip/small_ops.h) on host
 * data, the kernel, its chunk, LDS and workgroups per sample chosen by the engine's own code (pack_plan, engine_plan.h).
 *   board_sizes [n]  the board of every DEVICE sample; perm [n] the caller's slot each shows, NULL = no table (sample i shows
 *                    slot i); the launch covers the device samples [n0, n0 + ns) as one chain of a chained forward does
 *   planes != NULL   fp32 planes [n][cin][max_board^2] on the NN grid, by slot
 *   else records     [n_records][binary_planes*12 + 8] as sayuri_hip_forward_packed takes them, read by slot (n_records >= n);
 *                    symm != NULL: read through the record map src [n] (NULL = the identity) under the symmetries symm [n], both by
 *                    slot, as sayuri_hip_forward_packed_symm takes them
 *   stage_batch > 0  off | bsz | perm and src | symm travel through geom_stage_kernel / symm_stage_kernel from a pinned ring laid
 *                    out for stage_batch >= n samples (a mixed batch's path; a missing perm is staged as the identity); 0: copied
 *   in_place != 0    the records stay in pinned host memory of sayuri_hip_host_alloc's allocator and one workgroup per sample
 *                    reads them there (sayuri_hip_submit_packed's path)
 *   image            float [n*max_board^2 + guard_rows][cs], cs = cin rounded up to 32: the whole device image and guard_rows rows
 *                    behind its last slot, all set to `sentinel` (converted to the engine's type) before the launch, returned
 *                    as stored: every row of every slot, every pad channel
 * Refused (-1, the engine's messages) like a forward with max_batch = stage_batch (or n): board sizes outside 2..max_board, a
 * binary plane count the network or a record cannot have (more than 40 bit planes, more than 8 scalars), a symm outside 0..7, a src
 * outside the records; and a perm outside the batch or a sample range outside it.
 * sayuri_hip_test_last_pack: out = {kernel: 0 chunked, 1 flat, 2 bits, 3 bits + symmetry (-1: the call launched nothing), cs,
 * workgroups per sample, passes: the chunked kernel's passes per workgroup on the largest board of the launch, the flat
 * kernel's passes over a sample's planes, else 1} of the calling thread's last sayuri_hip_test_pack_input. */
int sayuri_hip_test_pack_input(int device, int use_fp16, int n, const int* board_sizes, int max_board, int cin, const float* planes,
                               const unsigned* records, int n_records, int binary_planes, const int* src, const int* symm,
                               const int* perm, int n0, int ns, int stage_batch, int in_place, float sentinel, int guard_rows,
                               float* image);
int sayuri_hip_test_last_pack(int out[4]);

#ifdef __cplusplus
}
#endif
#endif
