// engine_taps.h -- layer-level test taps of the C-ABI (sayuri_hip_test_*): one kernel family at a time on host tensors, for the
// parity tests (tests/test_gpu_layers.py, test_gpu_smallops.py, test_gpu_input.py).  Not used by the pipe.  A tap converts the layouts on the host,
// in and out, and launches ONE layer -- sayuri_hip_test_tower_run one RUN of layers, as one persistent launch; the device images,
// the routing of a convolution to its kernel family, the plans, the rule and the parameters of the fused SE stage, the launch
// parameters and the linking of a run are the engine's own code (engine_plan.h), so the tests check the host code the engine runs.
// The taps' own: the staging of host tensors and, where a comment says so, a deliberately different choice of variant.
#pragma once
#include "engine_graph.h"

namespace sayuri {

struct TestGeom {
    HostGeom hg;
    int slot = 0;
    int* d_off = nullptr;
    int* d_bsz = nullptr;
    BatchGeom g{};
};

class TestArena {  // device allocations of one tap call, freed at scope exit
public:
    ~TestArena() { for (void* p : ptrs_) (void)hipFree(p); }
    void* alloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 256)) != hipSuccess) return nullptr;
        (void)hipMemset(p, 0, std::max<size_t>(bytes, 256));
        ptrs_.push_back(p);
        return p;
    }
    template <typename U> U* upload(const std::vector<U>& h) {
        U* d = (U*)alloc(h.size() * sizeof(U));
        if (d && hipMemcpy(d, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
        return d;
    }
    // activations with the kZeroPrefix zero bytes in front that the board kernels read their halo cells from (conv_board.h)
    template <typename U> U* upload_prefixed(const std::vector<U>& h) {
        U* d = (U*)alloc(h.size() * sizeof(U) + kZeroPrefix);
        if (!d) return nullptr;
        d += kZeroPrefix / sizeof(U);
        return hipMemcpy(d, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice) == hipSuccess ? d : nullptr;
    }
private:
    std::vector<void*> ptrs_;
};

static int make_test_geom(TestArena& A, int n, const int* board_sizes, int max_board, TestGeom* tg) {
    if (host_geom(n, board_sizes, max_board, "test tap", &tg->hg)) return -1;
    tg->slot = max_board * max_board;
    tg->d_off = A.upload(tg->hg.off);
    tg->d_bsz = A.upload(tg->hg.bsz);
    if (!tg->d_off || !tg->d_bsz) return fail("test tap: hipMalloc failed");
    tg->g = BatchGeom{tg->d_off, tg->d_bsz, n, tg->hg.total, tg->slot};
    return 0;
}
// host NCHW (compact per sample) -> compact NHWC with channel stride cs ...
template <typename T> static std::vector<T> nchw_to_nhwc(const TestGeom& tg, const float* src, int C, int cs) {
    std::vector<T> h((size_t)tg.hg.n * tg.slot * cs, (T)0.f);
    size_t so = 0;
    for (int i = 0; i < tg.hg.n; ++i) {
        const int S = tg.hg.bsz[i] * tg.hg.bsz[i];
        for (int c = 0; c < C; ++c)
            for (int p = 0; p < S; ++p) h[((size_t)i * tg.slot + p) * cs + c] = (T)src[so + (size_t)c * S + p];
        so += (size_t)C * S;
    }
    return h;
}
// ... and a device tensor of that layout back into host NCHW
template <typename T> static int nhwc_to_nchw(const TestGeom& tg, const T* dev, int C, int cs, float* dst) {
    std::vector<T> h((size_t)tg.hg.n * tg.slot * cs);
    HIP_OK(hipMemcpy(h.data(), dev, h.size() * sizeof(T), hipMemcpyDeviceToHost));
    size_t so = 0;
    for (int i = 0; i < tg.hg.n; ++i) {
        const int S = tg.hg.bsz[i] * tg.hg.bsz[i];
        for (int c = 0; c < C; ++c)
            for (int p = 0; p < S; ++p) dst[so + (size_t)c * S + p] = (float)h[((size_t)i * tg.slot + p) * cs + c];
        so += (size_t)C * S;
    }
    return 0;
}
// The device side of a convolution tap: x [n][cx][bs*bs] behind the zero prefix, the residual (null: none) and y with `cy` channels
// -- y starts as fp16 NaN (0xffff: what comes back finite was written) or as zero --, the layer's weight image and bias (empty:
// the tap uploads its own).  0, or the tap's "...: hipMalloc failed".
template <typename T> struct TapBufs {
    const T *x = nullptr, *res = nullptr;
    T* y = nullptr;
    const void* w = nullptr;
    const float* bias = nullptr;
};
template <typename T, typename W>
static int stage_conv_tap(TestArena& A, const TestGeom& tg, const char* tap, const float* x, int cx, int cx_s, const float* res, int cy,
                          int cy_s, bool y_nan, const std::vector<W>& w_img, const std::vector<float>& bias_img, TapBufs<T>* b) {
    const size_t y_bytes = (size_t)tg.hg.n * tg.slot * cy_s * sizeof(T);
    b->x = A.upload_prefixed(nchw_to_nhwc<T>(tg, x, cx, cx_s));
    b->res = res ? A.upload(nchw_to_nhwc<T>(tg, res, cy, cy_s)) : nullptr;
    b->y = (T*)A.alloc(y_bytes);
    if (!w_img.empty()) b->w = A.upload(w_img);
    if (!bias_img.empty()) b->bias = A.upload(bias_img);
    if (!b->x || (res && !b->res) || !b->y || (!w_img.empty() && !b->w) || (!bias_img.empty() && !b->bias))
        return fail(std::string(tap) + ": hipMalloc failed");
    if (y_nan) HIP_OK(hipMemset(b->y, 0xff, y_bytes));
    return 0;
}
// ... and its end: the launch's status, the device's, y back in host NCHW.
template <typename T> static int finish(const TestGeom& tg, const T* dy, int C, int cs, float* y) {
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    return nhwc_to_nchw(tg, dy, C, cs, y);
}
// The index tables of the board kernels for `plan` (board_setup_kernel), as board_params takes them.  false: out of memory.
struct TestBoardTabs { int* src; int2* pix; int* cols; };
static bool make_board_tabs(TestArena& A, const TestGeom& tg, const BoardPlan& plan, TestBoardTabs* t) {
    t->src = (int*)A.alloc(sizeof(int) * (size_t)plan.ntiles * plan.npos);
    t->pix = (int2*)A.alloc(sizeof(int2) * (size_t)plan.ntiles * kBoardPT);
    t->cols = (int*)A.alloc(sizeof(int) * (size_t)plan.ntiles);
    if (!t->src || !t->pix || !t->cols) return false;
    hipLaunchKernelGGL(board_setup_kernel, dim3(plan.ntiles), dim3(256), 0, 0, tg.g, plan.npos, t->src, t->pix, t->cols);
    return true;
}

// Drives ONE convolution kernel directly, so the parity tests can localise a defect to a layer kind.
template <typename T>
static int test_conv_impl(int device, int n, const int* board_sizes, int max_board, int cin, int cout, int k,
                          int depthwise, int act, int post_residual, const float* x, const float* w, const float* bias,
                          const float* res, float* y) {
    HIP_OK(hipSetDevice(device));
    enable_big_lds<T>();
    if (sizeof(T) == 2 && k == 3) enable_big_lds_glds();
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    const HostGeom& hg = tg.hg;
    const int cin_s = round_up(depthwise ? cout : cin, 32), cout_s = round_up(cout, 32);
    int wmt, ko_pad;
    conv_tile(cout_s, sizeof(T) == 2, &wmt, &ko_pad);
    TapBufs<T> b;
    if (depthwise ? stage_conv_tap(A, tg, "test_conv", x, cout, cin_s, res, cout, cout_s, false, depthwise_image(w, cout, k * k, cout_s),
                                   padded_bias(bias, cout, cout_s), &b)
                  : stage_conv_tap(A, tg, "test_conv", x, cin, cin_s, res, cout, cout_s, false, conv_image<T>(w, cin, cout, k * k, ko_pad),
                                   padded_bias(bias, cout, ko_pad), &b))
        return -1;
    if (depthwise) {
        g_test_conv_kind = kConvDepthwise;
        const size_t total = (size_t)hg.total * (cout_s / ElemTraits<T>::kPieceElems);
        hipLaunchKernelGGL(depthwise_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, b.x, post_residual ? b.res : (const T*)nullptr,
                           b.y, (const float*)b.w, b.bias, tg.g, cout, cout_s, k, act);
    } else {
        const ConvOverride ov = EngineFlags::from_env().conv;
        const BoardPlan plan = board_plan(hg, ov);
        const ConvRoute r = route_conv(sizeof(T) == 2, k, ko_pad, hg, plan, ov);
        g_test_conv_kind = r.family;
        if (r.board) {
            TestBoardTabs tabs;
            if (!make_board_tabs(A, tg, plan, &tabs)) return fail("test_conv: hipMalloc failed");
            BoardParams bp;
            board_params(bp, plan, tabs.src, tabs.pix, tabs.cols, true);
            conv_params(bp.c, b.x, b.w, b.bias, b.res, b.y, tg.g, cin_s, cout_s, ko_pad, 9, act);
            bp.c.npos = 0; bp.c.num_pix_tiles = plan.ntiles;
            hipLaunchKernelGGL(r.board->fn, dim3(plan.ntiles * r.tiles), dim3(512), r.board->lds(plan.npos), 0, bp);
        } else if (r.glds) {
            const float* dz = (const float*)A.alloc(256);
            int* tsrc = (int*)A.alloc(sizeof(int) * (size_t)r.tiles * r.glds->npos);
            int2* tpix = (int2*)A.alloc(sizeof(int2) * (size_t)r.tiles * r.glds->pt);
            if (!dz || !tsrc || !tpix) return fail("test_conv: hipMalloc failed");
            hipLaunchKernelGGL(r.glds->setup, dim3(r.tiles), dim3(256), 0, 0, tg.g, tsrc, tpix);
            GldsParams gp;
            conv_params(gp.c, b.x, b.w, b.bias, b.res, b.y, tg.g, cin_s, cout_s, ko_pad, 9, act);
            const int grid = glds_params(gp, *r.glds, tsrc, tpix, dz, r.tiles);
            hipLaunchKernelGGL(r.glds->fn, dim3(grid), dim3(512), r.glds->lds, 0, gp);
        } else {
            // (deliberately not the engine's choice by cost: the widest pixel tile that fits, which is what the test cases were written to cover)
            TileChoice<T> tc;
            if (!pick_tile<T>(hg, wmt, ko_pad / (wmt * 32), /*widest=*/true, &tc)) return fail("test_conv: no tile configuration fits");
            ConvParams p;
            conv_params(p, b.x, b.w, b.bias, b.res, b.y, tg.g, cin_s, cout_s, ko_pad, k * k, act);
            p.npos = tc.npos; p.num_pix_tiles = tc.ntiles;
            hipLaunchKernelGGL(tc.e->fn, dim3(tc.ntiles * (ko_pad / (wmt * 32))), dim3(512), tc.e->lds(tc.npos), 0, p);
        }
    }
    return finish(tg, b.y, cout, cout_s, y);
}

// The same fp16 3x3 layer as many small workgroups (conv_split.h, the latency context's route): the engine's image in natural
// row order, split_plan's launch.  strips: strips per board (0: the engine's choice for this batch); channel_tiles: 0, or
// the number of 64-channel tiles the layer has -- the kernel has one channel tile size, any other count is refused.
// SAYURI_LATENCY_RING=n (read per call, as SAYURI_CONV is) forces the weight ring; sayuri_hip_last_split_ring(NULL) says what ran.
static int test_conv_split_impl(int device, int n, const int* board_sizes, int max_board, int cin, int cout, int act, const float* x,
                                const float* w, const float* bias, const float* res, float* y, int channel_tiles, int strips) {
    typedef f16 T;
    HIP_OK(hipSetDevice(device));
    enable_big_lds_glds();
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    const int cin_s = round_up(cin, 32), cout_s = round_up(cout, 32);
    int wmt, ko_pad;
    conv_tile(cout_s, true, &wmt, &ko_pad);
    if (!split_covers(ko_pad)) return fail("test_conv_split: a layer of " + std::to_string(ko_pad) + " weight rows is not whole 64-channel tiles: it keeps the default route");
    if (channel_tiles && channel_tiles != ko_pad / kSplitKO)
        return fail("test_conv_split: the split kernel's channel tile is 64: this layer has " + std::to_string(ko_pad / kSplitKO) + " channel tiles");
    if (strips < 0) return fail("test_conv_split: bad strip count");
    const SplitPlan sp = split_plan(tg.hg, 0, n, ko_pad, strips, EngineFlags::from_env().latency_ring);
    if (!sp.ok) return fail("test_conv_split: " + sp.why);
    TapBufs<T> b;
    if (stage_conv_tap(A, tg, "test_conv_split", x, cin, cin_s, res, cout, cout_s, false, conv_image<T>(w, cin, cout, 9, ko_pad),
                       padded_bias(bias, cout, ko_pad), &b))
        return -1;
    g_test_conv_kind = kConvSplit;
    g_test_split_ring = sp.stages;
    SplitParams q;
    std::memset(&q, 0, sizeof(q));
    conv_params(q.c, b.x, b.w, b.bias, b.res, b.y, tg.g, cin_s, cout_s, ko_pad, 9, act);
    split_params(q, sp, 0);
    split_launch(sp, q, nullptr);
    return finish(tg, b.y, cout, cout_s, y);
}

// The fp16 1x1 case of test_conv_impl through conv_pw.h (the route of a tower 1x1 layer): the engine's image, route_conv's plan.
// pieces: pieces per sample (0: the engine's choice for this batch).  y's device buffer starts as NaN: what comes back finite was
// written.
static int test_conv_pw_impl(int device, int n, const int* board_sizes, int max_board, int cin, int cout, int act, const float* x,
                             const float* w, const float* bias, const float* res, float* y, int pieces) {
    typedef f16 T;
    HIP_OK(hipSetDevice(device));
    enable_big_lds_glds();
    if (cin <= 0 || cout <= 0 || pieces < 0) return fail("test_conv_pw: bad argument");
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    const int cin_s = round_up(cin, 32), cout_s = round_up(cout, 32);
    int wmt, ko_pad;
    conv_tile(cout_s, true, &wmt, &ko_pad);
    if (!pw_covers(cin, cout, ko_pad))
        return fail("test_conv_pw: a layer of " + std::to_string(cin) + " -> " + std::to_string(cout) +
                    " channels is not whole 32-channel chunks into whole 64-channel tiles: it keeps the generic kernel");
    const PwAsk ask{cin, cout, cin_s, 0, n, pieces, /*force=*/true};
    const ConvRoute r = route_conv(true, 1, ko_pad, tg.hg, BoardPlan{}, ConvOverride{}, 0, false, &ask);
    if (!r.pw.ok) return fail("test_conv_pw: " + r.pw.why);
    TapBufs<T> b;
    if (stage_conv_tap(A, tg, "test_conv_pw", x, cin, cin_s, res, cout, cout_s, /*y_nan=*/true, conv_image<T>(w, cin, cout, 1, ko_pad),
                       padded_bias(bias, cout, ko_pad), &b))
        return -1;
    g_test_conv_kind = kConvPw;
    PwParams q;
    std::memset(&q, 0, sizeof(q));
    conv_params(q.c, b.x, b.w, b.bias, b.res, b.y, tg.g, cin_s, cout_s, ko_pad, 1, act);
    pw_params(q, r.pw, 0);
    pw_launch(r.pw, q, nullptr);
    return finish(tg, b.y, cout, cout_s, y);
}

// The pad channels [C, cs) of every board pixel (sample-major, pixel-major) as the last sayuri_hip_test_conv_dw call found them, raw
// fp16 bits: [0] conv_dw_kernel's output, [1] depthwise_kernel's on the same operands (sayuri_hip_test_last_dw_pad).
static thread_local std::vector<uint16_t> g_test_dw_pad[2];
static int read_dw_pad(const TestGeom& tg, const f16* dev, int C, int cs, std::vector<uint16_t>* pad) {
    std::vector<uint16_t> h((size_t)tg.hg.n * tg.slot * cs);
    HIP_OK(hipMemcpy(h.data(), dev, h.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    pad->clear();
    for (int i = 0; i < tg.hg.n; ++i)
        for (int p = 0; p < tg.hg.bsz[i] * tg.hg.bsz[i]; ++p)
            for (int c = C; c < cs; ++c) pad->push_back(h[((size_t)i * tg.slot + p) * cs + c]);
    return 0;
}

// One fp16 depthwise layer through conv_dw.h: the engine's [tap][cs] image and bias, dw_plan's launch.  strips: strips per sample
// (0: the engine's choice for this batch).  res, when given, is added behind the activation.  y's device buffer starts as NaN.
static int test_conv_dw_impl(int device, int n, const int* board_sizes, int max_board, int C, int k, int act, const float* x,
                             const float* w, const float* bias, const float* res, int strips, float* y) {
    typedef f16 T;
    HIP_OK(hipSetDevice(device));
    if (C <= 0 || strips < 0) return fail("test_conv_dw: bad argument");
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    const int cs = round_up(C, 32);
    const DwPlan dp = dw_plan(tg.hg, 0, n, cs, k, strips);
    if (!dp.ok) return fail("test_conv_dw: " + dp.why);
    TapBufs<T> b;
    if (stage_conv_tap(A, tg, "test_conv_dw", x, C, cs, res, C, cs, /*y_nan=*/true, depthwise_image(w, C, k * k, cs), padded_bias(bias, C, cs), &b))
        return -1;
    const float* dw = (const float*)b.w;
    const size_t y_bytes = (size_t)n * tg.slot * cs * sizeof(T);
    g_test_conv_kind = kConvDwLds;
    DwParams q;
    std::memset(&q, 0, sizeof(q));
    q.x = b.x; q.res = b.res; q.out = b.y; q.wt = dw; q.bias = b.bias;
    q.g = tg.g; q.C = C; q.cs = cs; q.act = act;
    dw_params(q, dp, 0);
    dw_launch(dp, q, nullptr);
    g_test_dw_pad[0].clear();
    g_test_dw_pad[1].clear();
    if (cs > C) {  // what both kernels leave in the pad channels: depthwise_kernel into a NaN buffer of its own, same operands
        T* dold = (T*)A.alloc(y_bytes);
        if (!dold) return fail("test_conv_dw: hipMalloc failed");
        HIP_OK(hipMemset(dold, 0xff, y_bytes));
        const size_t total = (size_t)tg.hg.total * (cs / ElemTraits<T>::kPieceElems);
        hipLaunchKernelGGL(depthwise_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, b.x, b.res, dold, dw, b.bias, tg.g, C, cs, k, act);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        if (read_dw_pad(tg, b.y, C, cs, &g_test_dw_pad[0]) || read_dw_pad(tg, dold, C, cs, &g_test_dw_pad[1])) return -1;
    }
    return finish(tg, b.y, C, cs, y);
}

template <typename T>
static int test_se_unit_impl(int device, int n, const int* board_sizes, int max_board, int C, int se, int act, const float* x,
                             const float* res, const float* w1, const float* b1, const float* w2, const float* b2, float* y,
                             float* gate_out) {
    HIP_OK(hipSetDevice(device));
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    const int cs = round_up(C, 32);
    T* dx = A.upload(nchw_to_nhwc<T>(tg, x, C, cs));
    T* dres = res ? A.upload(nchw_to_nhwc<T>(tg, res, C, cs)) : nullptr;
    float* dw1 = A.upload(fc_transposed(w1, 3 * C, se));
    float* dw2 = A.upload(fc_transposed(w2, se, 2 * C));
    float* db1 = A.upload(std::vector<float>(b1, b1 + se));
    float* db2 = A.upload(std::vector<float>(b2, b2 + 2 * C));
    float* separt = (float*)A.alloc(sizeof(float) * (size_t)n * kSeSplit * 2 * cs);
    float* gate = (float*)A.alloc(sizeof(float) * (size_t)n * 2 * cs);
    if (!dx || (res && !dres) || !dw1 || !dw2 || !db1 || !db2 || !separt || !gate) return fail("test_se_unit: hipMalloc failed");
    const FcDev sq{dw1, db1, 3 * C, se}, ex{dw2, db2, se, 2 * C};
    const auto run = [](const char*, double, double, auto&& launch) { launch(); return 0; };
    int rc = 1;  // SAYURI_SE_ONE=1 (read per call, as SAYURI_CONV is): the one-launch form where it applies
    T* dy = dx;  // where the result is: with several workgroups per sample the one launch leaves it in the residual's buffer
    if (EngineFlags::from_env().se_one == 1) {
        se_unit_enable_lds<T>();
        int max_pieces = 0;
        for (int i = 0; i < n; ++i) max_pieces = std::max(max_pieces, board_sizes[i] * board_sizes[i] * (cs / ElemTraits<T>::kPieceElems));
        const int parts = dres ? se_unit_parts(max_pieces, n) : 1;
        rc = se_unit_one_launch<T>(nullptr, tg.g, tg.hg.total, (const T*)dx, (const T*)dres, parts > 1 ? dres : dx, parts, gate, sq, ex, C, cs, act, 0, n,
                                   run);
        if (rc == 0 && parts > 1) dy = dres;
    }
    if (rc == 1) rc = se_unit_launches<T>(nullptr, tg.g, tg.hg.total, dx, dres, separt, gate, sq, ex, C, cs, act, 0, n, run);
    if (rc) return -1;
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    if (nhwc_to_nchw(tg, dy, C, cs, y)) return -1;
    if (gate_out) {
        std::vector<float> hg((size_t)n * 2 * cs);
        HIP_OK(hipMemcpy(hg.data(), gate, hg.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < C; ++c) {
                gate_out[(size_t)i * 2 * C + c] = hg[(size_t)i * 2 * cs + c];
                gate_out[(size_t)i * 2 * C + C + c] = hg[(size_t)i * 2 * cs + cs + c];
            }
    }
    return 0;
}

// The twelve head weight tensors of a head tap (`w`: p_inter_w, p_inter_b, pass_w, pass_b, v_inter_w, v_inter_b, v_misc_w, v_misc_b,
// prob_w, prob_b, own_w, own_b) on the device, as head_params takes them.  false: out of memory.
static bool upload_head_weights(TestArena& A, const float* const* w, int Cp, int Cv, int prob_ch, int pass_outs, int misc_outs, HeadWeights* hw) {
    const int in[4] = {3 * Cp, Cp, 3 * Cv, 3 * Cv}, out[4] = {Cp, pass_outs, 3 * Cv, misc_outs};
    FcDev* fcs[4] = {&hw->p_inter, &hw->pass_fc, &hw->v_inter, &hw->v_misc};
    for (int i = 0; i < 4; ++i) {
        *fcs[i] = FcDev{A.upload(fc_transposed(w[2 * i], in[i], out[i])), A.upload(std::vector<float>(w[2 * i + 1], w[2 * i + 1] + out[i])), in[i], out[i]};
        if (!fcs[i]->wt || !fcs[i]->b) return false;
    }
    hw->prob_w = A.upload(std::vector<float>(w[8], w[8] + (size_t)prob_ch * Cp));
    hw->prob_b = A.upload(std::vector<float>(w[9], w[9] + prob_ch));
    hw->own_w = A.upload(std::vector<float>(w[10], w[10] + Cv));
    hw->own_b = A.upload(std::vector<float>(w[11], w[11] + 1));
    return hw->prob_w && hw->prob_b && hw->own_w && hw->own_b;
}
// The four output tensors of a head tap on the device, and their way back to the caller.
struct TestHeadOut {
    float *prob = nullptr, *pass = nullptr, *misc = nullptr, *own = nullptr;
    size_t n_prob, n_pass, n_misc, n_own;
    bool alloc(TestArena& A, int n, int prob_ch, int pass_outs, int misc_outs, int B2) {
        n_prob = (size_t)n * prob_ch * B2; n_pass = (size_t)n * pass_outs; n_misc = (size_t)n * misc_outs; n_own = (size_t)n * B2;
        prob = (float*)A.alloc(sizeof(float) * n_prob);
        pass = (float*)A.alloc(sizeof(float) * n_pass);
        misc = (float*)A.alloc(sizeof(float) * n_misc);
        own = (float*)A.alloc(sizeof(float) * n_own);
        return prob && pass && misc && own;
    }
    int download(float* h_prob, float* h_pass, float* h_misc, float* h_own) const {
        HIP_OK(hipMemcpy(h_prob, prob, sizeof(float) * n_prob, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(h_pass, pass, sizeof(float) * n_pass, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(h_misc, misc, sizeof(float) * n_misc, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(h_own, own, sizeof(float) * n_own, hipMemcpyDeviceToHost));
        return 0;
    }
};

template <typename T>
static int test_head_tail_impl(int device, int n, const int* board_sizes, int max_board, int Cp, int Cv, int prob_ch, int pass_outs,
                               int misc_outs, int act, const float* pconv, const float* vconv, const float* const* w, float* prob,
                               float* pass, float* misc, float* own) {
    HIP_OK(hipSetDevice(device));
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    if (prob_ch > 8) return fail("test_head_tail: too many policy planes");
    const int cs_p = round_up(Cp, 32), cs_v = round_up(Cv, 32);
    const T* dp = A.upload(nchw_to_nhwc<T>(tg, pconv, Cp, cs_p));
    const T* dv = A.upload(nchw_to_nhwc<T>(tg, vconv, Cv, cs_v));
    HeadWeights hw;
    TestHeadOut o;
    if (!dp || !dv || !upload_head_weights(A, w, Cp, Cv, prob_ch, pass_outs, misc_outs, &hw) ||
        !o.alloc(A, n, prob_ch, pass_outs, misc_outs, max_board * max_board))
        return fail("test_head_tail: hipMalloc failed");
    const HeadParams h = head_params(hw, Cp, Cv, prob_ch, act, max_board, o.prob, o.pass, o.misc, o.own, nullptr);
    const int maxc = std::max(Cp, Cv);
    hipLaunchKernelGGL(head_tail_kernel<T>, dim3(2 * n), dim3(256), sizeof(float) * (7 * maxc + 512), 0, dp, dv, tg.g, h);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    return o.download(prob, pass, misc, own);
}

// An SE unit's two FCs as handed over the ABI and -- img1 != null -- its staged images on the device, as se_stage_params takes
// them.  false: out of memory.
static bool upload_se_stage(TestArena& A, BoardSeParams& sp, int C, int se, const float* w1, const float* b1, const float* w2, const float* b2,
                            const std::vector<f16>* img1, const std::vector<unsigned char>* img2, int w1_bytes, int w2_bytes) {
    const FcDev sq{A.upload(fc_transposed(w1, 3 * C, se)), A.upload(std::vector<float>(b1, b1 + se)), 3 * C, se};
    const FcDev ex{A.upload(fc_transposed(w2, se, 2 * C)), A.upload(std::vector<float>(b2, b2 + 2 * C)), se, 2 * C};
    se_stage_params(sp, sq, ex, C, img1 ? A.upload(*img1) : nullptr, img1 ? A.upload(*img2) : nullptr, w1_bytes, w2_bytes);
    return sq.wt && sq.b && ex.wt && ex.b && (!img1 || (sp.w1h && sp.w2h));
}

// The convolution with the SE unit inside it (conv_board_se_kernel, or the same stage inside the persistent tower kernel
// when via_tower != 0): C -> C 3x3 convolution + bias, then the unit's pool -> FC -> FC -> act(sigmoid(g) x + b + res).
// Returns 1 when the fused kernel does not apply to this batch (several samples per tile, channel tile not 128 / 256).
static thread_local int g_test_se_form = 0;  // form of the SE stage the last sayuri_hip_test_conv_se launched: 0 nothing, 1 staged images, 2 FCs from L2
static int test_conv_se_impl(int device, int n, const int* board_sizes, int max_board, int C, int se, int act, int via_tower,
                             const float* x, const float* w, const float* bias, const float* res, const float* w1, const float* b1,
                             const float* w2, const float* b2, float* y) {
    typedef f16 T;
    g_test_se_form = 0;
    HIP_OK(hipSetDevice(device));
    enable_big_lds_glds();
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    const int cs = round_up(C, 32);
    int wmt, ko_pad;
    conv_tile(cs, true, &wmt, &ko_pad);
    const BoardPlan plan = board_plan(tg.hg, ConvOverride{});
    const BoardEntry* be = pick_board_se(plan, ko_pad);
    // (deliberately the kernel's own rule, one sample per tile -- not Engine::conv_se's, which fuses only boards too large to share a tile)
    if (!be || !plan.single || C > be->kot) return 1;
    std::vector<f16> img1;
    std::vector<unsigned char> img2;
    int w1_bytes = 0, w2_bytes = 0;
    const bool staged = make_se_images(C, se, max_board, w1, b1, w2, b2, &img1, &img2, &w1_bytes, &w2_bytes);
    if (!staged && !se_l2_form_ok(se, 2 * C)) return 1;  // (nothing of the layer is uploaded or launched yet)
    TapBufs<T> b;
    TestBoardTabs tabs;
    if (stage_conv_tap(A, tg, "test_conv_se", x, C, cs, res, C, cs, false, std::vector<T>(), std::vector<float>(), &b)) return -1;
    if (!make_board_tabs(A, tg, plan, &tabs)) return fail("test_conv_se: hipMalloc failed");
    BoardSeParams sp;
    std::memset(&sp, 0, sizeof(sp));
    BoardParams& bp = sp.b;
    board_params(bp, plan, tabs.src, tabs.pix, tabs.cols, true);
    ConvParams& p = bp.c;
    conv_params(p, b.x, nullptr, nullptr, b.res, b.y, tg.g, cs, cs, ko_pad, 9, act);
    p.num_pix_tiles = plan.ntiles;
    // through the tower a layer the generated epilogue covers takes its weights and bias in board_row_channel order, as in Engine::board_launch
    bp.row_order = via_tower && board_row_order_ok(bp, be->kot, !EngineFlags::off("SAYURI_TOWER_GEN_EPI")) ? 1 : 0;
    const std::vector<T> img = conv_image<T>(w, C, C, 9, ko_pad);
    const std::vector<float> hb = padded_bias(bias, C, ko_pad);
    p.w = A.upload(bp.row_order ? board_row_order(img, ko_pad) : img);
    p.bias = A.upload(bp.row_order ? board_row_order(hb, ko_pad, 1) : hb);
    if (!p.w || !p.bias || !upload_se_stage(A, sp, C, se, w1, b1, w2, b2, staged ? &img1 : nullptr, &img2, w1_bytes, w2_bytes))
        return fail("test_conv_se: hipMalloc failed");
    hipModule_t mod = nullptr;
    g_test_se_form = sp.w1h ? 1 : 2;  // what both kernels branch on (board_se_pool / board_se_fc, the seam's image staging)
    if (via_tower) {
        hipFunction_t fn[2] = {nullptr, nullptr};
        if (load_tower_module(&mod, fn)) return -1;
        TowerLayer t;
        std::memset(&t, 0, sizeof(t));
        TowerLayer* dt = (TowerLayer*)A.alloc(sizeof(TowerLayer));
        if (!dt) return fail("test_conv_se: hipMalloc failed");
        t.self = dt; t.last = 1; t.has_se = 1; t.sp = sp;
        HIP_OK(hipMemcpy(dt, &t, sizeof(t), hipMemcpyHostToDevice));
        const TowerLayer* arg = dt;
        void* params[] = {(void*)&arg};
        HIP_OK(hipModuleLaunchKernel(fn[be->kot == 256 ? 0 : 1], plan.ntiles, 1, 1, 512, 1, 1, 0, nullptr, params, nullptr));
    } else {
        hipLaunchKernelGGL(be->fn_se, dim3(plan.ntiles), dim3(512), be->lds(plan.npos), 0, sp);
    }
    const int rc = finish(tg, b.y, C, cs, y);
    if (mod) (void)hipModuleUnload(mod);
    return rc;
}

// A RUN of 1..8 board convolutions as ONE launch of the persistent tower kernel (conv_tower.h): layer 0 is cin0 -> C, every later
// layer C -> C, C = the channel tile (128 / 256); at most one layer carries the SE unit.  Each layer's parameters are built the
// way Engine::conv / conv_se / board_launch build them (board_plan, board_params, conv_params, the row order wherever
// board_row_order_ok allows it), the table is tower_element + tower_link's, the launch is Engine::tower_flush's.  Every layer
// writes a buffer of its own that starts as fp16 NaN, and reads the previous layer's; y receives all of them.
// res_from[l]: -1 no residual, 0 the run's input, k the output of layer k - 1.  Returns 1 when the batch has no board plan.
static thread_local int g_test_tower_run[3] = {0, 0, 0};  // the last run launched: layers, layers in row order, hand-over links
struct TestSeUnit { int layer, se; const float *w1, *b1, *w2, *b2; };
static int test_tower_run_impl(int device, int n, const int* board_sizes, int max_board, int C, int cin0, int nlayers, const int* act,
                               const int* res_from, const float* w, const float* bias, const TestSeUnit& se, int chain, const float* x, float* y) {
    typedef f16 T;
    g_test_tower_run[0] = g_test_tower_run[1] = g_test_tower_run[2] = 0;
    g_test_se_form = 0;
    if (C != 128 && C != 256) return fail("test_tower_run: the run's channels are a channel tile of the tower kernel, 128 or 256");
    if (nlayers < 1 || nlayers > 8) return fail("test_tower_run: 1 to 8 layers");
    if (cin0 < 1 || cin0 > 512) return fail("test_tower_run: bad input channel count");
    if (se.layer >= nlayers) return fail("test_tower_run: the SE layer is not a layer of the run");
    for (int l = 0; l < nlayers; ++l) {
        if (act[l] < 0 || act[l] > 7) return fail("test_tower_run: bad activation");
        if (res_from[l] < -1 || res_from[l] > l) return fail("test_tower_run: a layer's residual is the run's input or an earlier layer's output");
        if (res_from[l] == 0 && cin0 != C) return fail("test_tower_run: the run's input has " + std::to_string(cin0) + " channels, a residual has " + std::to_string(C));
    }
    HIP_OK(hipSetDevice(device));
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    const EngineFlags flags = EngineFlags::from_env();
    const int cin0_s = round_up(cin0, 32);
    int wmt, ko_pad;
    conv_tile(C, true, &wmt, &ko_pad);
    const BoardPlan plan = board_plan(tg.hg, ConvOverride{});
    const BoardEntry* be = pick_board_se(plan, ko_pad);  // (both channel tiles of the tower kernel have the SE stage)
    if (!be) return 1;
    // the SE layer: the rule of sayuri_hip_test_conv_se (one sample per tile; the images staged, or FC widths the L2 form takes)
    const bool has_unit = se.layer >= 0;
    std::vector<f16> img1;
    std::vector<unsigned char> img2;
    int w1_bytes = 0, w2_bytes = 0;
    bool staged = false;
    if (has_unit) {
        if (!se.w1 || !se.b1 || !se.w2 || !se.b2) return fail("test_tower_run: the SE layer's weights are missing");
        if (!plan.single) return fail("test_tower_run: the SE stage needs one sample per tile");
        staged = make_se_images(C, se.se, max_board, se.w1, se.b1, se.w2, se.b2, &img1, &img2, &w1_bytes, &w2_bytes);
        if (!staged && !se_l2_form_ok(se.se, 2 * C))
            return fail("test_tower_run: no form of the SE stage takes this SE width");
    }
    const size_t act_bytes = (size_t)n * tg.slot * C * sizeof(T);
    const T* dx = A.upload_prefixed(nchw_to_nhwc<T>(tg, x, cin0, cin0_s));
    TestBoardTabs tabs;
    if (!dx || !make_board_tabs(A, tg, plan, &tabs)) return fail("test_tower_run: hipMalloc failed");
    T* out[8];
    for (int l = 0; l < nlayers; ++l) {
        // a buffer of its own behind the zero prefix; fp16 NaN (0xffff) wherever no layer wrote
        unsigned char* raw = (unsigned char*)A.alloc(act_bytes + kZeroPrefix);
        if (!raw) return fail("test_tower_run: hipMalloc failed");
        out[l] = (T*)(raw + kZeroPrefix);
        HIP_OK(hipMemset(out[l], 0xff, act_bytes));
    }
    std::vector<TowerLayer> run;
    size_t w_off = 0;
    int row_ordered = 0;
    for (int l = 0; l < nlayers; ++l) {
        const int cin = l ? C : cin0, cin_s = l ? C : cin0_s;
        const bool unit = l == se.layer;
        BoardSeParams sp;
        std::memset(&sp, 0, sizeof(sp));
        BoardParams& bp = sp.b;
        board_params(bp, plan, tabs.src, tabs.pix, tabs.cols, flags.arith);
        ConvParams& p = bp.c;
        const T* res = res_from[l] < 0 ? nullptr : res_from[l] == 0 ? dx : out[res_from[l] - 1];
        conv_params(p, l ? out[l - 1] : dx, nullptr, nullptr, res, out[l], tg.g, cin_s, C, ko_pad, 9, act[l]);
        p.npos = 0; p.num_pix_tiles = plan.ntiles;
        bp.row_order = board_row_order_ok(bp, be->kot, flags.tower_gen_epi) ? 1 : 0;  // Engine::board_launch
        row_ordered += bp.row_order;
        const std::vector<T> img = conv_image<T>(w + w_off, cin, C, 9, ko_pad);
        const std::vector<float> hb = padded_bias(bias + (size_t)l * C, C, ko_pad);
        w_off += (size_t)C * cin * 9;
        p.w = A.upload(bp.row_order ? board_row_order(img, ko_pad) : img);
        p.bias = A.upload(bp.row_order ? board_row_order(hb, ko_pad, 1) : hb);
        if (!p.w || !p.bias) return fail("test_tower_run: hipMalloc failed");
        if (unit && !upload_se_stage(A, sp, C, se.se, se.w1, se.b1, se.w2, se.b2, staged ? &img1 : nullptr, &img2, w1_bytes, w2_bytes))
            return fail("test_tower_run: hipMalloc failed");
        run.push_back(tower_element(sp, unit));
    }
    TowerLayer* dt = (TowerLayer*)A.alloc(sizeof(TowerLayer) * nlayers);
    if (!dt) return fail("test_tower_run: hipMalloc failed");
    const int links = tower_link(run, dt, chain != 0);
    HIP_OK(hipMemcpy(dt, run.data(), sizeof(TowerLayer) * nlayers, hipMemcpyHostToDevice));
    hipModule_t mod = nullptr;
    hipFunction_t fn[2] = {nullptr, nullptr};
    if (load_tower_module(&mod, fn)) return -1;
    if (has_unit) g_test_se_form = staged ? 1 : 2;
    g_test_tower_run[0] = nlayers; g_test_tower_run[1] = row_ordered; g_test_tower_run[2] = links;
    const TowerLayer* arg = dt;
    void* params[] = {(void*)&arg};
    hipError_t rc = hipModuleLaunchKernel(fn[be->kot == 256 ? 0 : 1], plan.ntiles, 1, 1, 512, 1, 1, 0, nullptr, params, nullptr);
    if (rc == hipSuccess) rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipDeviceSynchronize();
    (void)hipModuleUnload(mod);
    if (rc != hipSuccess) return fail(std::string("test_tower_run: ") + hipGetErrorString(rc));
    const size_t per_layer = (size_t)C * tg.hg.total;
    for (int l = 0; l < nlayers; ++l)
        if (nhwc_to_nchw(tg, out[l], C, C, y + l * per_layer)) return -1;
    return 0;
}

// The same layer when its channels are split over kts = 2..4 workgroups of 128 (conv_board_sx_kernel, conv_board_sx.h): the
// images of make_sx_images, the launch of Engine::conv_sx (sx_board_entry / sx_params / sx_grid) over every tile of the batch,
// on a zeroed exchange buffer with a fixed tag.  Returns 1 when the form does not apply: the channels are not 2..4 whole tiles
// of 128 (after padding to 32), the unit's images do not fit, no 128-row board entry fits, or a board of the batch is too small
// (sx_board_fused: the engine runs such samples through se_tail).  -1 when a workgroup's wait for its siblings ran out.
struct TestHostWord {  // a zeroed host-visible word the device can write (BoardSxParams::err)
    unsigned *host = nullptr, *dev = nullptr;
    ~TestHostWord() { if (host) (void)hipHostFree(host); }
    bool alloc() {
        if (hipHostMalloc((void**)&host, 64, hipHostMallocMapped) != hipSuccess) { host = nullptr; return false; }
        std::memset(host, 0, 64);
        return hipHostGetDevicePointer((void**)&dev, host, 0) == hipSuccess;
    }
};
static thread_local int g_test_sx_kts = 0;  // channel tiles per board tile of the last sayuri_hip_test_conv_sx launch (0: it launched nothing)
static int test_conv_sx_impl(int device, int n, const int* board_sizes, int max_board, int C, int se, int act, const float* x,
                             const float* w, const float* bias, const float* res, const float* w1, const float* b1, const float* w2,
                             const float* b2, float* y) {
    typedef f16 T;
    constexpr unsigned kEpoch = 0x5e17u;
    g_test_sx_kts = 0;
    HIP_OK(hipSetDevice(device));
    enable_big_lds_glds();
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    const int cs = round_up(C, 32), kts = round_up(C, 128) / 128;
    int wmt, ko_pad;
    conv_tile(cs, true, &wmt, &ko_pad);
    if (cs != kts * 128 || ko_pad != kts * 128) return 1;  // Engine::build_se_images / conv_sx: the layer is whole 128-channel tiles
    std::vector<f16> img1;
    std::vector<unsigned char> img2;
    int w1_bytes = 0, w2_bytes = 0;
    if (!make_sx_images(C, se, kts, max_board, w1, b1, w2, b2, &img1, &img2, &w1_bytes, &w2_bytes)) return 1;
    const BoardPlan plan = board_plan(tg.hg, ConvOverride{});
    const BoardEntry* be = plan.ok ? sx_board_entry(plan.npos) : nullptr;
    if (!be) return 1;
    for (int i = 0; i < n; ++i)
        if (!sx_board_fused(tg.hg.bsz[i])) return 1;
    TapBufs<T> b;  // y starts as fp16 NaN (0xffff): an output no workgroup wrote comes back as NaN, not as a plausible 0
    if (stage_conv_tap(A, tg, "test_conv_sx", x, C, cs, res, C, cs, /*y_nan=*/true, conv_image<T>(w, C, C, 9, ko_pad), padded_bias(bias, C, ko_pad), &b))
        return -1;
    const f16* d1 = A.upload(img1);
    const unsigned char* d2 = A.upload(img2);
    unsigned long long* xchg = (unsigned long long*)A.alloc(sizeof(unsigned long long) * (size_t)plan.ntiles * kts * kSxMaxSub * kSxSlots);
    TestBoardTabs tabs;
    TestHostWord err;
    if (!d1 || !d2 || !xchg || !make_board_tabs(A, tg, plan, &tabs) || !err.alloc())
        return fail("test_conv_sx: hipMalloc failed");
    BoardSxParams sp;
    std::memset(&sp, 0, sizeof(sp));
    board_params(sp.b, plan, tabs.src, tabs.pix, tabs.cols, true);
    conv_params(sp.b.c, b.x, b.w, b.bias, b.res, b.y, tg.g, cs, cs, ko_pad, 9, act);
    sp.b.c.npos = 0; sp.b.c.num_pix_tiles = plan.ntiles;
    sx_params(sp, d1, d2, w1_bytes, w2_bytes, max_board, se, kts, xchg, kEpoch, err.dev, /*dbg_stall=*/false);
    g_test_conv_kind = kConvBoardSx;
    g_test_sx_kts = kts;
    hipLaunchKernelGGL(conv_board_sx_kernel<2>, dim3(sx_grid(plan.ntiles, kts)), dim3(512), be->lds(plan.npos), 0, sp);
    const int rc = finish(tg, b.y, C, cs, y);
    if (rc == 0 && *(volatile unsigned*)err.host) return fail("test_conv_sx: a workgroup's wait for its sibling channel tiles ran out");
    return rc;
}

// Both heads of a sample in one workgroup (head_board_kernel): trunk [n][C][bs*bs] -> the four output tensors.
// Returns 1 when no head_board_kernel variant fits these channel counts (the engine then runs conv1x1 x2 + head_tail).
static int test_head_board_impl(int device, int n, const int* board_sizes, int max_board, int C, int Cp, int Cv, int prob_ch,
                                int pass_outs, int misc_outs, int act, const float* trunk, const float* p_w, const float* p_b,
                                const float* v_w, const float* v_b, const float* const* w, float* prob, float* pass, float* misc,
                                float* own) {
    typedef f16 T;
    HIP_OK(hipSetDevice(device));
    enable_big_lds_glds();
    TestArena A;
    TestGeom tg;
    if (make_test_geom(A, n, board_sizes, max_board, &tg)) return -1;
    HeadImages hi;
    const HeadFn fn = make_head_images(C, Cp, Cv, prob_ch, max_board, p_w, p_b, v_w, v_b, w[8], w[10], &hi);
    if (!fn) return 1;
    const int cs = round_up(C, 32);
    const T* dt = A.upload(nchw_to_nhwc<T>(tg, trunk, C, cs));
    const f16* d_img = A.upload(hi.img);
    const f16* d_img2 = A.upload(hi.img2);
    const float* d_bias = A.upload(hi.bias);
    HeadWeights hw;
    TestHeadOut o;
    if (!dt || !d_img || !d_img2 || !d_bias || !upload_head_weights(A, w, Cp, Cv, prob_ch, pass_outs, misc_outs, &hw) ||
        !o.alloc(A, n, prob_ch, pass_outs, misc_outs, max_board * max_board))
        return fail("test_head_board: hipMalloc failed");
    HeadBoardParams hp;
    std::memset(&hp, 0, sizeof(hp));
    hp.h = head_params(hw, Cp, Cv, prob_ch, act, max_board, o.prob, o.pass, o.misc, o.own, nullptr);
    hp.trunk = dt; hp.w = d_img; hp.w2 = d_img2; hp.bias = d_bias; hp.g = tg.g; hp.cs = cs; hp.PT = hi.PT; hp.VT = hi.VT;
    hipLaunchKernelGGL(fn, dim3(n), dim3(512), kMaxLds, 0, hp);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    return o.download(prob, pass, misc, own);
}

// The input stage: ONE of pack_input_kernel / pack_input_flat_kernel / pack_bits_kernel / pack_bits_symm_kernel on host data,
// chosen and launched by the engine's own pack_plan / pack_launch (engine_plan.h), into an image that starts as a sentinel and
// comes back whole.  The arguments are refused as Engine::enqueue_inputs / check_symm refuse them (max_batch = stage_batch, or n).
// Geometry and maps reach the device as the engine's do: copied (the resident arrays of a uniform batch), or -- stage_batch > 0
// -- from a pinned ring laid out for stage_batch samples through geom_stage_kernel / symm_stage_kernel.  What the staging
// kernels left is read back and compared BEFORE the pack kernel runs on it: a board size that is not the batch's would send a
// pack kernel past the image.  (The unused entries of the ring and of the device arrays hold harmless values for the same reason.)
static thread_local int g_test_pack[4] = {-1, 0, 0, 0};  // the last sayuri_hip_test_pack_input launch: kernel (-1: none), cs, workgroups per sample, passes
struct TestPinned {  // host memory from the allocator behind sayuri_hip_host_alloc, freed at scope exit
    ~TestPinned() { for (void* p : ptrs_) sayuri_hip_host_free(p); }
    void* alloc(size_t bytes) {
        void* p = sayuri_hip_host_alloc(bytes);
        if (p) ptrs_.push_back(p);
        return p;
    }
private:
    std::vector<void*> ptrs_;
};
struct TestPackArgs {
    int n, max_board, cin;
    const int* board_sizes;  // [n] the board of every DEVICE sample
    const float* planes;
    const unsigned* records;
    int n_records, binary;
    const int *src, *symm, *perm;
    int n0, ns, stage_batch, in_place;
    float sentinel;
    int guard_rows;
};
static bool test_staged_equal(const int* dev, const std::vector<int>& want) {
    std::vector<int> got(want.size());
    return hipMemcpy(got.data(), dev, sizeof(int) * want.size(), hipMemcpyDeviceToHost) == hipSuccess && got == want;
}
template <typename T> static int test_pack_input_impl(int device, const TestPackArgs& a, float* image) {
    g_test_pack[0] = -1; g_test_pack[1] = g_test_pack[2] = g_test_pack[3] = 0;
    const int n = a.n, board = a.max_board, cin = a.cin;
    const int max_batch = a.stage_batch > 0 ? a.stage_batch : n;
    if (n <= 0 || n > max_batch) return fail("batch size out of range");
    if (board < 2 || board > 25 || cin < 1 || cin > 512 || a.guard_rows < 0) return fail("test_pack_input: bad argument");
    const bool records = a.planes == nullptr, symm = records && a.symm != nullptr;
    if (records && !a.records) return fail("test_pack_input: neither planes nor records");
    if (records && packed_binary_check(a.binary, cin, board)) return -1;
    const SymmReq sy{a.n_records, a.src, a.symm};
    if (symm && check_symm_request(n, max_batch, a.records, sy)) return -1;
    if (records && !symm && a.n_records < n) return fail("test_pack_input: records are read by slot: n_records >= n");
    if (a.in_place && !records) return fail("test_pack_input: only records are read in place");
    if (a.n0 < 0 || a.ns <= 0 || a.n0 + a.ns > n) return fail("test_pack_input: the sample range [n0, n0 + ns) is not inside the batch");
    for (int i = 0; i < n; ++i)
        if (a.perm && (a.perm[i] < 0 || a.perm[i] >= n)) return fail("test_pack_input: perm[" + std::to_string(i) + "] is no slot of the batch");
    HIP_OK(hipSetDevice(device));
    TestArena A;
    TestPinned P;
    const int B2 = board * board, cs = round_up(cin, 32);
    // the geometry arrays: off[n + 1], bsz[n], perm[n]
    std::vector<int> off(n + 1, 0), bsz(a.board_sizes, a.board_sizes + n), perm(n);
    for (int i = 0; i < n; ++i) {
        if (bsz[i] < 2 || bsz[i] > board) return fail("sample board size out of range");
        off[i + 1] = off[i] + bsz[i] * bsz[i];
        perm[i] = a.perm ? a.perm[i] : i;
    }
    int* d_off = A.upload(std::vector<int>(max_batch + 1, 0));
    int* d_bsz = A.upload(std::vector<int>(max_batch, 2));
    int* d_perm = A.upload(std::vector<int>(max_batch, 0));
    int *d_src = nullptr, *d_symm = nullptr;
    if (!d_off || !d_bsz || !d_perm) return fail("test_pack_input: hipMalloc failed");
    std::vector<int> src(n, 0), sym(n, 0);
    if (symm) {
        for (int i = 0; i < n; ++i) { src[i] = a.src ? a.src[i] : i; sym[i] = a.symm[i]; }
        d_src = A.upload(std::vector<int>(max_batch, 0));
        d_symm = A.upload(std::vector<int>(max_batch, 0));
        if (!d_src || !d_symm) return fail("test_pack_input: hipMalloc failed");
    }
    if (a.stage_batch > 0) {
        // Engine::enqueue_inputs' rings: off | bsz | perm at strides of max_batch + 1 / max_batch, src | symm at max_batch
        int* hg = (int*)P.alloc(sizeof(int) * (3 * max_batch + 1));
        if (!hg) return fail("test_pack_input: hipHostMalloc failed");
        for (int i = 0; i < 3 * max_batch + 1; ++i) hg[i] = i > max_batch && i <= 2 * max_batch ? 2 : 0;
        std::memcpy(hg, off.data(), sizeof(int) * (n + 1));
        std::memcpy(hg + max_batch + 1, bsz.data(), sizeof(int) * n);
        std::memcpy(hg + 2 * max_batch + 1, perm.data(), sizeof(int) * n);
        hipLaunchKernelGGL(geom_stage_kernel, dim3(1), dim3(256), 0, 0, (const int*)hg, max_batch, n, d_off, d_bsz, d_perm);
        HIP_OK(hipGetLastError());
        if (symm) {
            int* hs = (int*)P.alloc(sizeof(int) * 2 * max_batch);
            if (!hs) return fail("test_pack_input: hipHostMalloc failed");
            std::memset(hs, 0, sizeof(int) * 2 * max_batch);
            std::memcpy(hs, src.data(), sizeof(int) * n);
            std::memcpy(hs + max_batch, sym.data(), sizeof(int) * n);
            hipLaunchKernelGGL(symm_stage_kernel, dim3(1), dim3(256), 0, 0, (const int*)hs, max_batch, n, d_src, d_symm);
            HIP_OK(hipGetLastError());
        }
        HIP_OK(hipDeviceSynchronize());
        if (!test_staged_equal(d_off, off) || !test_staged_equal(d_bsz, bsz) || !test_staged_equal(d_perm, perm))
            return fail("test_pack_input: geom_stage_kernel left other geometry arrays than the ring holds");
        if (symm && (!test_staged_equal(d_src, src) || !test_staged_equal(d_symm, sym)))
            return fail("test_pack_input: symm_stage_kernel left another record map or other symmetries than the ring holds");
    } else {
        HIP_OK(hipMemcpy(d_off, off.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_bsz, bsz.data(), sizeof(int) * n, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(d_perm, perm.data(), sizeof(int) * n, hipMemcpyHostToDevice));
        if (symm) {
            HIP_OK(hipMemcpy(d_src, src.data(), sizeof(int) * n, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(d_symm, sym.data(), sizeof(int) * n, hipMemcpyHostToDevice));
        }
    }
    // the planes, or the records: copied, or where they lie in pinned memory (submit_packed's in-place path)
    PackSource in;
    if (records) {
        const size_t words = (size_t)(symm ? a.n_records : n) * (a.binary * kPackedWords + kPackedScalars);
        if (a.in_place) {
            unsigned* h = (unsigned*)P.alloc(sizeof(unsigned) * words);
            if (!h) return fail("test_pack_input: hipHostMalloc failed");
            std::memcpy(h, a.records, sizeof(unsigned) * words);
            HIP_OK(hipHostGetDevicePointer((void**)&in.records, h, 0));
        } else {
            in.records = A.upload(std::vector<unsigned>(a.records, a.records + words));
        }
        in.nbin = a.binary;
        in.src_map = d_src; in.symm_map = d_symm;
        if (!in.records) return fail("test_pack_input: hipMalloc failed");
    } else {
        in.planes = A.upload(std::vector<float>(a.planes, a.planes + (size_t)n * cin * B2));
        if (!in.planes) return fail("test_pack_input: hipMalloc failed");
    }
    // the image and the guard behind its last slot: the sentinel everywhere
    const size_t elems = ((size_t)n * B2 + a.guard_rows) * cs;
    T* dimg = A.upload(std::vector<T>(elems, (T)a.sentinel));
    if (!dimg) return fail("test_pack_input: hipMalloc failed");
    const PackPlan pl = pack_plan(sizeof(T), cin, cs, board, records, symm, a.in_place != 0);
    const BatchGeom g{d_off, d_bsz, n, off[n], B2};
    pack_launch<T>(pl, 0, in, dimg, g, cin, cs, board, a.perm || a.stage_batch > 0 ? d_perm : nullptr, a.n0, a.ns);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    g_test_pack[0] = pl.kernel; g_test_pack[1] = cs; g_test_pack[2] = pl.split;
    g_test_pack[3] = pl.passes(*std::max_element(bsz.begin() + a.n0, bsz.begin() + a.n0 + a.ns), cin, board);
    std::vector<T> h(elems);
    HIP_OK(hipMemcpy(h.data(), dimg, elems * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < elems; ++i) image[i] = (float)h[i];
    return 0;
}

}  // namespace sayuri

extern "C" int sayuri_hip_test_conv_se(int device, int n, const int* board_sizes, int max_board, int channels, int se_size, int act,
                                       int via_tower, const float* x, const float* w, const float* bias, const float* res,
                                       const float* w1, const float* b1, const float* w2, const float* b2, float* y) {
    if (!board_sizes || !x || !w || !w1 || !b1 || !w2 || !b2 || !y || n <= 0) return fail("test_conv_se: bad argument");
    return test_conv_se_impl(device, n, board_sizes, max_board, channels, se_size, act, via_tower, x, w, bias, res, w1, b1, w2, b2, y);
}

extern "C" int sayuri_hip_test_conv_sx(int device, int n, const int* board_sizes, int max_board, int channels, int se_size, int act,
                                       const float* x, const float* w, const float* bias, const float* res, const float* w1,
                                       const float* b1, const float* w2, const float* b2, float* y) {
    if (!board_sizes || !x || !w || !w1 || !b1 || !w2 || !b2 || !y || n <= 0) return fail("test_conv_sx: bad argument");
    return test_conv_sx_impl(device, n, board_sizes, max_board, channels, se_size, act, x, w, bias, res, w1, b1, w2, b2, y);
}

extern "C" int sayuri_hip_test_last_se_form(void) { return sayuri::g_test_se_form; }

extern "C" int sayuri_hip_test_tower_run(int device, int n, const int* board_sizes, int max_board, int channels, int cin0, int nlayers,
                                         const int* act, const int* res_from, const float* w, const float* bias, int se_layer, int se_size,
                                         const float* w1, const float* b1, const float* w2, const float* b2, int chain, const float* x,
                                         float* y) {
    if (!board_sizes || !act || !res_from || !w || !bias || !x || !y || n <= 0 || (chain != 0 && chain != 1))
        return fail("test_tower_run: bad argument");
    return test_tower_run_impl(device, n, board_sizes, max_board, channels, cin0, nlayers, act, res_from, w, bias,
                               TestSeUnit{se_layer < 0 ? -1 : se_layer, se_size, w1, b1, w2, b2}, chain, x, y);
}
extern "C" int sayuri_hip_test_last_tower_run(int out[3]) {
    if (!out) return fail("test_last_tower_run: bad argument");
    std::copy(sayuri::g_test_tower_run, sayuri::g_test_tower_run + 3, out);
    return 0;
}

extern "C" int sayuri_hip_test_last_sx_kts(void) { return sayuri::g_test_sx_kts; }

extern "C" int sayuri_hip_test_head_board(int device, int n, const int* board_sizes, int max_board, int channels, int policy_channels,
                                          int value_channels, int prob_channels, int pass_outs, int misc_outs, int act, const float* trunk,
                                          const float* p_w, const float* p_b, const float* v_w, const float* v_b,
                                          const float* const* weights12, float* prob, float* pass, float* misc, float* own) {
    if (!board_sizes || !trunk || !p_w || !p_b || !v_w || !v_b || !weights12 || !prob || !pass || !misc || !own || n <= 0)
        return fail("test_head_board: bad argument");
    return test_head_board_impl(device, n, board_sizes, max_board, channels, policy_channels, value_channels, prob_channels, pass_outs,
                                misc_outs, act, trunk, p_w, p_b, v_w, v_b, weights12, prob, pass, misc, own);
}

extern "C" int sayuri_hip_test_se_unit(int device, int use_fp16, int n, const int* board_sizes, int max_board, int channels, int se_size,
                                       int act, const float* x, const float* res, const float* w1, const float* b1, const float* w2,
                                       const float* b2, float* y, float* gate) {
    if (!board_sizes || !x || !w1 || !b1 || !w2 || !b2 || !y || n <= 0) return fail("test_se_unit: bad argument");
    if (use_fp16) return test_se_unit_impl<f16>(device, n, board_sizes, max_board, channels, se_size, act, x, res, w1, b1, w2, b2, y, gate);
    return test_se_unit_impl<float>(device, n, board_sizes, max_board, channels, se_size, act, x, res, w1, b1, w2, b2, y, gate);
}

extern "C" int sayuri_hip_test_head_tail(int device, int use_fp16, int n, const int* board_sizes, int max_board, int policy_channels,
                                         int value_channels, int prob_channels, int pass_outs, int misc_outs, int act, const float* pconv,
                                         const float* vconv, const float* const* weights12, float* prob, float* pass, float* misc,
                                         float* own) {
    if (!board_sizes || !pconv || !vconv || !weights12 || !prob || !pass || !misc || !own || n <= 0) return fail("test_head_tail: bad argument");
    if (use_fp16)
        return test_head_tail_impl<f16>(device, n, board_sizes, max_board, policy_channels, value_channels, prob_channels, pass_outs,
                                        misc_outs, act, pconv, vconv, weights12, prob, pass, misc, own);
    return test_head_tail_impl<float>(device, n, board_sizes, max_board, policy_channels, value_channels, prob_channels, pass_outs,
                                      misc_outs, act, pconv, vconv, weights12, prob, pass, misc, own);
}

extern "C" int sayuri_hip_test_conv_split(int device, int n, const int* board_sizes, int max_board, int cin, int cout, int act, const float* x,
                                          const float* w, const float* bias, const float* res, float* y, int channel_tiles, int strips) {
    if (!board_sizes || !x || !w || !y || n <= 0) return fail("test_conv_split: bad argument");
    return test_conv_split_impl(device, n, board_sizes, max_board, cin, cout, act, x, w, bias, res, y, channel_tiles, strips);
}

extern "C" int sayuri_hip_test_conv_pw(int device, int n, const int* board_sizes, int max_board, int cin, int cout, int act, const float* x,
                                       const float* w, const float* bias, const float* res, float* y, int pieces) {
    if (!board_sizes || !x || !w || !y || n <= 0) return fail("test_conv_pw: bad argument");
    return test_conv_pw_impl(device, n, board_sizes, max_board, cin, cout, act, x, w, bias, res, y, pieces);
}

extern "C" int sayuri_hip_test_conv_dw(int device, int use_fp16, int n, const int* board_sizes, int max_board, int channels, int k, int act,
                                       const float* x, const float* w, const float* bias, const float* res, int strips, float* y) {
    if (!board_sizes || !x || !w || !y || n <= 0) return fail("test_conv_dw: bad argument");
    if (!use_fp16) return fail("test_conv_dw: conv_dw.h is an fp16 kernel: the fp32 engine keeps depthwise_kernel");
    return test_conv_dw_impl(device, n, board_sizes, max_board, channels, k, act, x, w, bias, res, strips, y);
}

extern "C" int sayuri_hip_test_last_dw_pad(int which, unsigned short* bits, int cap) {
    if (which < 0 || which > 1 || cap < 0 || (cap > 0 && !bits)) return fail("test_last_dw_pad: bad argument");
    const std::vector<uint16_t>& v = sayuri::g_test_dw_pad[which];
    std::copy(v.begin(), v.begin() + std::min<size_t>(v.size(), (size_t)cap), bits);
    return (int)v.size();
}

extern "C" int sayuri_hip_test_last_conv_kind(void) { return sayuri::g_test_conv_kind; }

extern "C" int sayuri_hip_test_conv(int device, int use_fp16, int n, const int* board_sizes, int max_board, int cin,
                                    int cout, int k, int depthwise, int act, int post_residual, const float* x,
                                    const float* w, const float* bias, const float* res, float* y) {
    if (!board_sizes || !x || !w || !y || n <= 0) return fail("test_conv: bad argument");
    if (use_fp16)
        return test_conv_impl<f16>(device, n, board_sizes, max_board, cin, cout, k, depthwise, act, post_residual, x, w,
                                   bias, res, y);
    return test_conv_impl<float>(device, n, board_sizes, max_board, cin, cout, k, depthwise, act, post_residual, x, w,
                                 bias, res, y);
}

extern "C" int sayuri_hip_test_pack_input(int device, int use_fp16, int n, const int* board_sizes, int max_board, int cin, const float* planes,
                                          const unsigned* records, int n_records, int binary_planes, const int* src, const int* symm,
                                          const int* perm, int n0, int ns, int stage_batch, int in_place, float sentinel, int guard_rows,
                                          float* image) {
    if (!board_sizes || !image) return fail("test_pack_input: bad argument");
    const sayuri::TestPackArgs a{n, max_board, cin, board_sizes, planes, records, n_records, binary_planes, src, symm, perm, n0, ns, stage_batch,
                                 in_place, sentinel, guard_rows};
    return use_fp16 ? sayuri::test_pack_input_impl<f16>(device, a, image) : sayuri::test_pack_input_impl<float>(device, a, image);
}
extern "C" int sayuri_hip_test_last_pack(int out[4]) {
    if (!out) return fail("test_last_pack: bad argument");
    std::copy(sayuri::g_test_pack, sayuri::g_test_pack + 4, out);
    return 0;
}
