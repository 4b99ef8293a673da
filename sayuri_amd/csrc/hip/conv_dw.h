// conv_dw.h -- the fp16 depthwise k x k convolution (k = 3, 5, 7) of a mixer block (DW_CONV) and of the RepLK policy head
// (P_DW_CONV) on LDS: depthwise_kernel's layer (small_ops.h), bit for bit, as MANY SMALL INDEPENDENT WORKGROUPS.
//
// One workgroup (256 threads) is one item
//     (sample, slice of channels, strip of rows of that sample).
// A slice is `sp` 16-byte pieces of 8 channels: 64 channels where cs is a multiple of 64 (a pixel's slice is then one whole
// 128-byte line), 32 channels otherwise -- cs is a multiple of 32 everywhere.  A strip is whole rows of ONE sample.  No workgroup
// waits for another: the launch boundary is the only synchronisation.
//
// STAGING is LDS-DMA (glds16_s, the idiom of conv_pw.h / conv_split.h), all of it issued before the first wait:
//   * the slice's weights, as they lie in the engine's [tap][cs] fp32 image: a tap's slice is 2 sp contiguous 16-byte pieces;
//   * the strip's rows and the k/2 halo rows above and below that lie INSIDE the board -- consecutive rows of one sample are
//     consecutive pixels of its slot, so the LDS image [pixel][piece] is the global run itself with the channel stride taken
//     out.  One wave instruction writes 64 consecutive 16-byte slots; lane l of block b brings slot 64 b + l, i.e. piece
//     (slot mod sp) of pixel (slot / sp).  Slots beyond the image (the last block's tail) re-read the image's last slot into
//     the slack the allocation is rounded up by.
// Every input element and every weight is read from global memory once per item.  There is no zero frame: a tap outside the
// board is SKIPPED, as in depthwise_kernel, so nothing outside the board is staged.
//
// THREAD MAPPING.  A thread owns one piece (8 channels) and computes kDwW = 4 neighbouring outputs of a row from LDS.  Per
// tap row it reads the row's k weights of its piece once (2 k ds_read_b128, the same address in every lane of that piece: a
// broadcast) and the kDwW + k - 1 input pixels its outputs touch once each; every input pixel feeds up to kDwW outputs and
// every weight kDwW outputs from registers.  Lanes: the piece fastest, then the ROW, then the group of four columns.  A
// ds_read_b128 is served in groups of 16 lanes that must hit 16 distinct 16-byte slots mod 16 (one 256-byte bank row): lanes
// that differ in the piece hit neighbouring slots, lanes that differ by one row are bs x sp slots apart -- 152 = 8 mod 16 for
// a 19-wide board on 64-channel slices (two rows x eight pieces cover the bank row), 76 = 12 mod 16 on 32-channel slices
// (four rows x four pieces do); every odd board width does the same, an even width leaves a two-way conflict on the input reads
// (speed only).
//
// ARITHMETIC: depthwise_kernel<f16>'s per output element -- the accumulator starts at +0; kr ascending, then kc ascending, a
// tap outside the board skipped, every other tap one fused multiply-add of float(x) and the fp32 weight; + bias as one fp32
// add; activate() (common.h); + float(res) behind the activation; one conversion.  The register blocking walks a tap row's
// INPUT columns in ascending order and gives each to the outputs it belongs to: for one output that is kc ascending.
// Channels [C, cs) are stored as 0.
#pragma once
#include "conv_split.h"

namespace sayuri {

constexpr int kDwThreads = 256;
constexpr int kDwW = 4;                     // outputs of one row a thread computes
constexpr size_t kDwMaxLds = 64 * 1024;     // an item's LDS: at least two items are resident on a CU

struct DwParams {
    const f16* x;
    const f16* res;  // or null
    f16* out;
    const float* wt;    // [k*k][cs]
    const float* bias;  // [cs]
    BatchGeom g;
    int C, cs, act;
    int sp;      // 16-byte pieces of a channel slice: 8 or 4
    int slices;  // cs / (8 sp)
    int strips;  // strips asked for per sample; dw_rows() makes it rows per strip for every board size
    int smax;    // strips per sample in the grid (a board with fewer leaves the rest of its workgroups idle)
    int n0;      // first sample of the launch
};

// Rows per strip of a bs x bs board cut into `strips` (no more strips than rows).  One rule for the host and the kernel.
__host__ __device__ inline int dw_rows(int bs, int strips) {
    const int s = strips < 1 ? 1 : (strips > bs ? bs : strips);
    return (bs + s - 1) / s;
}
// LDS bytes: the weights, then the image of `pix` staged pixels, each rounded up to whole DMA blocks of 64 slots.
__host__ __device__ inline size_t dw_lds_bytes(int k, int sp, int pix) {
    return (size_t)((k * k * 2 * sp + 63) / 64 + (pix * sp + 63) / 64) * 1024;
}

template <int K>
__global__ __launch_bounds__(kDwThreads) void conv_dw_kernel(const DwParams p) {
    constexpr int PAD = K / 2, W = kDwW, NI = W + K - 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // slice fastest: neighbouring workgroup ids share a strip's pixels
    const int sl = blockIdx.x % p.slices, item = blockIdx.x / p.slices;
    const int strip = item % p.smax, sample = p.n0 + item / p.smax;
    const int bs = p.g.bsz[sample];
    const int rp = dw_rows(bs, p.strips), r0 = strip * rp;
    if (r0 >= bs) return;  // this board has fewer strips than the grid: the whole workgroup leaves, in front of the barrier
    const int r1 = min(bs, r0 + rp);
    const int h0 = max(0, r0 - PAD), h1 = min(bs, r1 + PAD);  // the staged rows
    const int sp = p.sp, spl = sp == 8 ? 3 : 2, cs = p.cs;
    const int xslots = (h1 - h0) * bs * sp, xblocks = (xslots + 63) >> 6;
    const int wslots = K * K * 2 * sp, wblocks = (wslots + 63) >> 6;
    const uint32_t lds0 = (uint32_t)(uintptr_t)smem, xoff = (uint32_t)wblocks * 1024u;
    const size_t row0 = (size_t)sample * p.g.slot_pix;  // activation row of the sample's first pixel

    // ---- DMA: block b of a region goes to wave b mod 4
    const unsigned char* gw = (const unsigned char*)(p.wt + sl * sp * 8);
    const unsigned char* gx = (const unsigned char*)(p.x + (row0 + (size_t)h0 * bs) * cs + sl * sp * 8);
    for (int b = wave; b < wblocks; b += 4) {
        const int s = min(b * 64 + lane, wslots - 1);
        const int tap = s >> (spl + 1), part = s & (2 * sp - 1);
        glds16_s((uint32_t)(tap * cs * 4 + part * 16), gw, lds0 + b * 1024);
    }
    for (int b = wave; b < xblocks; b += 4) {
        const int s = min(b * 64 + lane, xslots - 1);
        const int pix = s >> spl, piece = s & (sp - 1);
        glds16_s((uint32_t)(pix * cs * 2 + piece * 16), gx, lds0 + xoff + b * 1024);
    }

    const int piece = tid & (sp - 1), c0 = (sl * sp + piece) * 8;  // the thread's 8 channels
    float b8[8];
    *(f32x4*)b8 = *(const f32x4*)(p.bias + c0);
    *(f32x4*)(b8 + 4) = *(const f32x4*)(p.bias + c0 + 4);

    wait_vmcnt<0>();
    __syncthreads();

    const float* wl = (const float*)smem + piece * 8;   // a tap is sp * 8 floats
    const unsigned char* xl = smem + xoff + piece * 16;  // a pixel is sp * 16 bytes
    const int XG = (bs + W - 1) / W, R = r1 - r0, units = R * XG;
    const f16* __restrict__ gres = p.res;
    f16* __restrict__ gout = p.out;
    const int act = p.act, C = p.C;
    for (int u = tid >> spl; u < units; u += kDwThreads >> spl) {
        const int xg = u / R, row = r0 + (u - xg * R), x0 = xg * W;
        const size_t o = (row0 + (size_t)(row * bs + x0)) * cs + c0;
        f16x8 rr[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            rr[j] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (gres && x0 + j < bs) rr[j] = *(const f16x8*)(gres + o + (size_t)j * cs);
        }
        float acc[W][8];
#pragma unroll
        for (int j = 0; j < W; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
#pragma unroll 1
        for (int kr = 0; kr < K; ++kr) {
            const int iy = row + kr - PAD;
            if (iy < 0 || iy >= bs) continue;
            float w[K][8];
#pragma unroll
            for (int kc = 0; kc < K; ++kc) {
                const float* wp = wl + (kr * K + kc) * (sp * 8);
                *(f32x4*)w[kc] = *(const f32x4*)wp;
                *(f32x4*)(w[kc] + 4) = *(const f32x4*)(wp + 4);
            }
            const unsigned char* xr = xl + (size_t)((iy - h0) * bs) * (sp * 16);
#pragma unroll
            for (int ii = 0; ii < NI; ++ii) {
                const int ix = x0 + ii - PAD;
                if (ix < 0 || ix >= bs) continue;
                const f16x8 v = *(const f16x8*)(xr + ix * (sp * 16));
                float xf[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) xf[e] = to_float(v[e]);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const int kc = ii - j;  // output x0 + j reads input x0 + j + kc - PAD
                    if (kc < 0 || kc >= K) continue;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[j][e] += xf[e] * w[kc][e];  // (depthwise_kernel's statement: contracted as it is there)
                }
            }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            if (x0 + j >= bs) continue;
            f16x8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = 0.f;
                if (c0 + e < C) {
                    v = activate(acc[j][e] + b8[e], act);
                    if (gres) v += to_float(rr[j][e]);
                }
                h[e] = from_float<f16>(v);
            }
            *(f16x8*)(gout + o + (size_t)j * cs) = h;
        }
    }
}

}  // namespace sayuri
