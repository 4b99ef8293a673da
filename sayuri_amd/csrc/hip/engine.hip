// engine.hip -- the C-ABI of include/sayuri_hip.h: one translation unit in three parts
//   (conv_split.h: the many-small-workgroups convolution of a latency context, sayuri_hip_create_ex;
//    conv_pw.h: the tower's 1x1 convolutions of bottleneck-family networks as many small workgroups;
//    conv_dw.h: the depthwise convolutions of mixer blocks and the RepLK head on LDS)
//   engine_plan.h   kernel registries, environment switches, batch geometry, tile plans and the routing of a convolution to its
//                   kernel family, the device images of the layers and the launch parameters the engine and the taps share
//   engine_graph.h  Engine<T>: the per-GPU forward graph -- counterpart of the reference's CudaForwardPipe::NNGraph
//                   (src/neural/cuda/cuda_forward_pipe.cc:133-1090) and its layer objects (src/neural/cuda/cuda_layers.cc),
//                   re-designed for MI355X: compact NHWC activations (common.h), one workgroup per board with the whole residual
//                   tower as ONE persistent launch (conv_board.h, conv_tower.h), SE units inside the convolutions (conv_board.h,
//                   conv_board_sx.h), both heads in one kernel (head_board.h), mixed board sizes without masked work
//   engine_taps.h   layer-level test taps (sayuri_hip_test_*): host layout conversion around ONE launch built by engine_plan.h's code
// and, in this file, the entry points themselves.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../../include/sayuri_hip.h"
#include "common.h"
#include "conv_mfma.h"
#include "conv_glds.h"
#include "conv_board.h"
#include "conv_board_sx.h"
#include "conv_split.h"
#include "conv_pw.h"
#include "conv_dw.h"
#include "conv_tower.h"
#include "head_board.h"
#include "small_ops.h"

#include "engine_plan.h"
#include "engine_graph.h"

// ====================================================================== C ABI
using namespace sayuri;

struct sayuri_hip_ctx {
    std::unique_ptr<EngineBase> eng;
};

extern "C" {

const char* sayuri_hip_last_error(void) { return g_err.c_str(); }

int sayuri_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

sayuri_hip_ctx* sayuri_hip_create_ex(int device, const sayuri_hip_netdesc* desc, int max_batch, int board, int use_fp16, unsigned flags) {
    if (!desc || !desc->blocks || max_batch <= 0 || board < 2 || board > 25) {
        fail("sayuri_hip_create: bad arguments");
        return nullptr;
    }
    if (flags & ~(unsigned)SAYURI_HIP_LATENCY) {
        fail("sayuri_hip_create_ex: unknown flag bits " + std::to_string(flags & ~(unsigned)SAYURI_HIP_LATENCY));
        return nullptr;
    }
    if (flags && !use_fp16) {
        fail("sayuri_hip_create_ex: SAYURI_HIP_LATENCY needs the fp16 engine (use_fp16 = 1): the fp32 engine is the strict-parity mode and has no split kernels");
        return nullptr;
    }
    int ndev = sayuri_hip_device_count();
    if (device < 0 || device >= ndev) {
        fail("sayuri_hip_create: no such HIP device (found " + std::to_string(ndev) + ")");
        return nullptr;
    }
    auto ctx = std::make_unique<sayuri_hip_ctx>();
    int rc;
    const EngineFlags env = EngineFlags::from_env();
    const EngineFlags eflags = (flags & SAYURI_HIP_LATENCY) ? env.for_latency() : env;
    if (use_fp16) {
        auto e = std::make_unique<Engine<f16>>(device, *desc, max_batch, board, eflags);
        rc = e->init();
        ctx->eng = std::move(e);
    } else {
        auto e = std::make_unique<Engine<float>>(device, *desc, max_batch, board, eflags);
        rc = e->init();
        ctx->eng = std::move(e);
    }
    if (rc) return nullptr;
    return ctx.release();
}

sayuri_hip_ctx* sayuri_hip_create(int device, const sayuri_hip_netdesc* desc, int max_batch, int board, int use_fp16) {
    // SAYURI_LATENCY=1: the flag for callers that cannot pass one (a reference tree with the pipe compiled in).  It asks for the
    // fp16 engine's latency mode; an fp32 context is created as ever.
    const char* e = getenv("SAYURI_LATENCY");
    const unsigned flags = use_fp16 && e && atoi(e) != 0 ? (unsigned)SAYURI_HIP_LATENCY : 0u;
    return sayuri_hip_create_ex(device, desc, max_batch, board, use_fp16, flags);
}

int sayuri_hip_load_tensor(sayuri_hip_ctx* ctx, int layer_id, int kind, const float* host, size_t n) {
    if (!ctx || !host) return fail("load_tensor: null argument");
    return ctx->eng->load_tensor(layer_id, kind, host, n);
}

int sayuri_hip_reload_begin(sayuri_hip_ctx* ctx, const sayuri_hip_netdesc* desc) {
    if (!ctx || !desc) return fail("reload_begin: null argument");
    return ctx->eng->reload_begin(*desc);
}
int sayuri_hip_reload_prepare(sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->reload_prepare() : fail("reload_prepare: null ctx"); }
int sayuri_hip_reload_commit(sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->reload_commit() : fail("reload_commit: null ctx"); }
int sayuri_hip_reload_abort(sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->reload_abort() : fail("reload_abort: null ctx"); }
int sayuri_hip_weights_generation(const sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->weights_generation() : -1; }

int sayuri_hip_upload(sayuri_hip_ctx* ctx, int n, const float* planes, const int* board_sizes) {
    if (!ctx || !planes) return fail("upload: null argument");
    return ctx->eng->upload(n, planes, board_sizes);
}
int sayuri_hip_run(sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->run() : fail("run: null ctx"); }
int sayuri_hip_sync(sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->sync() : fail("sync: null ctx"); }
int sayuri_hip_download(sayuri_hip_ctx* ctx, float* prob, float* pass, float* misc, float* own) {
    return ctx ? ctx->eng->download(prob, pass, misc, own) : fail("download: null ctx");
}

int sayuri_hip_forward(sayuri_hip_ctx* ctx, int n, const float* planes, const int* board_sizes, float* prob,
                       float* pass, float* misc, float* own) {
    if (!ctx) return fail("forward: null ctx");
    if (ctx->eng->upload(n, planes, board_sizes)) return -1;
    if (ctx->eng->run()) return -1;
    return ctx->eng->download(prob, pass, misc, own);
}

int sayuri_hip_forward_packed(sayuri_hip_ctx* ctx, int n, const unsigned* records, int binary_planes, const int* board_sizes,
                              float* prob, float* pass, float* misc, float* own) {
    if (!ctx || !records) return fail("forward_packed: null argument");
    if (ctx->eng->upload(n, nullptr, board_sizes, records, binary_planes)) return -1;
    if (ctx->eng->run()) return -1;
    return ctx->eng->download(prob, pass, misc, own);
}
int sayuri_hip_submit_packed(sayuri_hip_ctx* ctx, int n, const unsigned* records, int binary_planes, const int* board_sizes,
                             float* prob, float* pass, float* misc, float* own, int* ticket) {
    if (!ctx || !records || !ticket) return fail("submit_packed: null argument");
    return ctx->eng->submit(n, nullptr, board_sizes, prob, pass, misc, own, ticket, records, binary_planes);
}
int sayuri_hip_forward_packed_symm(sayuri_hip_ctx* ctx, int n, const unsigned* records, int n_records, int binary_planes,
                                   const int* board_sizes, const int* src, const int* symm, float* prob, float* pass, float* misc,
                                   float* own) {
    if (!ctx || !records || !symm) return fail("forward_packed_symm: null argument");
    const SymmReq sy{n_records, src, symm};
    if (ctx->eng->upload(n, nullptr, board_sizes, records, binary_planes, &sy)) return -1;
    if (ctx->eng->run()) return -1;
    return ctx->eng->download(prob, pass, misc, own);
}
int sayuri_hip_submit_packed_symm(sayuri_hip_ctx* ctx, int n, const unsigned* records, int n_records, int binary_planes,
                                  const int* board_sizes, const int* src, const int* symm, float* prob, float* pass, float* misc,
                                  float* own, int* ticket) {
    if (!ctx || !records || !symm || !ticket) return fail("submit_packed_symm: null argument");
    const SymmReq sy{n_records, src, symm};
    return ctx->eng->submit(n, nullptr, board_sizes, prob, pass, misc, own, ticket, records, binary_planes, &sy);
}
int sayuri_hip_submit(sayuri_hip_ctx* ctx, int n, const float* planes, const int* board_sizes, float* prob,
                      float* pass, float* misc, float* own, int* ticket) {
    if (!ctx || !planes || !prob || !pass || !misc || !own || !ticket) return fail("submit: null argument");
    return ctx->eng->submit(n, planes, board_sizes, prob, pass, misc, own, ticket);
}
int sayuri_hip_wait(sayuri_hip_ctx* ctx, int ticket) { return ctx ? ctx->eng->wait(ticket) : fail("wait: null ctx"); }
int sayuri_hip_query(sayuri_hip_ctx* ctx, int ticket) { return ctx ? ctx->eng->query(ticket) : fail("query: null ctx"); }

int sayuri_hip_time_runs(sayuri_hip_ctx* ctx, int iters, float* total_ms) {
    if (!ctx || !total_ms || iters <= 0) return fail("time_runs: bad argument");
    return ctx->eng->time_runs(iters, total_ms);
}

int sayuri_hip_mark_kernel(sayuri_hip_ctx* ctx, const char* name) {
    return ctx ? ctx->eng->mark_kernel(name) : fail("mark_kernel: null ctx");
}
int sayuri_hip_timed_stat(sayuri_hip_ctx* ctx, sayuri_hip_kernel_stat* row) {
    if (!ctx || !row) return fail("timed_stat: bad argument");
    return ctx->eng->timed_stat(row);
}

int sayuri_hip_profile_run(sayuri_hip_ctx* ctx, sayuri_hip_kernel_stat* rows, int cap) {
    if (!ctx || !rows) return fail("profile_run: bad argument");
    return ctx->eng->profile_run(rows, cap);
}

void* sayuri_hip_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail("hipHostMalloc failed");
        return nullptr;
    }
    return p;
}
void sayuri_hip_host_free(void* p) {
    if (!p) return;
    g_host_free_gen.fetch_add(1, std::memory_order_release);
    (void)hipHostFree(p);
}

size_t sayuri_hip_device_bytes(const sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->device_bytes() : 0; }
int sayuri_hip_last_chains(const sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->last_chains() : 0; }
int sayuri_hip_tower_state(const sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->tower_state() : -1; }
int sayuri_hip_latency_state(const sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->latency_state() : -1; }
int sayuri_hip_last_split_ring(const sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->last_split_ring() : sayuri::g_test_split_ring; }
// host arithmetic only: the geometry, the layer's weight rows and split_plan, as a latency context and the conv_split tap run them
int sayuri_hip_split_ring_plan(int n, const int* board_sizes, int max_board, int cout, int strips, int ring) {
    HostGeom hg;
    if (cout <= 0 || strips < 0) return fail("split_ring_plan: bad argument");
    if (host_geom(n, board_sizes, max_board, "split_ring_plan", &hg)) return -1;
    int wmt, ko_pad;
    conv_tile(round_up(cout, 32), true, &wmt, &ko_pad);
    if (!split_covers(ko_pad))
        return fail("split_ring_plan: a layer of " + std::to_string(ko_pad) + " weight rows is not whole 64-channel tiles: it keeps the default route");
    const SplitPlan sp = split_plan(hg, 0, n, ko_pad, strips, ring);
    if (!sp.ok) return fail("split_ring_plan: " + sp.why);
    return sp.stages;
}
int sayuri_hip_last_pw_launches(const sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->last_pw_launches() : 0; }
// host arithmetic only: the geometry, the layer's weight rows and route_conv's plan, as a context and the conv_pw tap run them
int sayuri_hip_pw_plan(int n, const int* board_sizes, int max_board, int cin, int cout, int pieces, int out[4]) {
    HostGeom hg;
    if (cin <= 0 || cout <= 0 || pieces < 0 || !out) return fail("pw_plan: bad argument");
    if (host_geom(n, board_sizes, max_board, "pw_plan", &hg)) return -1;
    int wmt, ko_pad;
    conv_tile(round_up(cout, 32), true, &wmt, &ko_pad);
    if (!pw_covers(cin, cout, ko_pad))
        return fail("pw_plan: a layer of " + std::to_string(cin) + " -> " + std::to_string(cout) +
                    " channels is not whole 32-channel chunks into whole 64-channel tiles: it keeps the generic kernel");
    const PwAsk ask{cin, cout, round_up(cin, 32), 0, n, pieces, /*force=*/true};  // the plan itself: whether a context takes it is the speed rule's business (pw_pays)
    const ConvRoute r = route_conv(true, 1, ko_pad, hg, BoardPlan{}, ConvOverride{}, 0, false, &ask);
    if (!r.pw.ok) return fail("pw_plan: " + r.pw.why);
    out[0] = r.pw.cut; out[1] = r.pw.grid; out[2] = r.pw.e->nj; out[3] = (int)r.pw.lds;
    return 0;
}
int sayuri_hip_last_dw_launches(const sayuri_hip_ctx* ctx) { return ctx ? ctx->eng->last_dw_launches() : 0; }
// host arithmetic only: the geometry and dw_plan, as a context and the conv_dw tap run them
int sayuri_hip_dw_plan(int n, const int* board_sizes, int max_board, int channels, int k, int strips, int out[4]) {
    HostGeom hg;
    if (channels <= 0 || strips < 0 || !out) return fail("dw_plan: bad argument");
    if (host_geom(n, board_sizes, max_board, "dw_plan", &hg)) return -1;
    const DwPlan dp = dw_plan(hg, 0, n, round_up(channels, 32), k, strips);
    if (!dp.ok) return fail("dw_plan: " + dp.why);
    out[0] = dp.sp * 8; out[1] = dp.cut; out[2] = dp.grid; out[3] = (int)dp.lds;
    return 0;
}
// debugging tap (not part of the ABI, not in the header): activation buffer `buf` (0..5) of ticket 0 as it stands after the last forward
extern "C" int sayuri_hip_debug_read_activations(sayuri_hip_ctx* ctx, int buf, void* host, size_t bytes) {
    return ctx ? ctx->eng->debug_read(buf, host, bytes) : -1;
}

void sayuri_hip_destroy(sayuri_hip_ctx* ctx) { delete ctx; }

}

#include "engine_taps.h"
