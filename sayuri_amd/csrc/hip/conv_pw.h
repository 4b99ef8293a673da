// conv_pw.h -- the tower's 1x1 (pointwise) convolutions of bottleneck-family networks (fp16: PRE_BTL / POST_BTL of a bottleneck
// or nested-bottleneck block, CONV1 / CONV2 of a mixer block) as MANY SMALL INDEPENDENT WORKGROUPS on LDS-DMA: conv_split.h's
// make, without a halo.
//
// One workgroup (256 threads, one wave per SIMD, waves 2 along M x 2 along N) is one item
//     (sample, piece of that sample's pixels, 64 output channels).
// A piece is a run of consecutive pixels of ONE sample -- whole column tiles of 16 pixels, up to 2 NJ of them; a 1x1 layer has no
// halo, so a piece is not rows -- and never spans two samples.  No workgroup waits for another: no spin, no exchange, no item
// queue; the launch boundary is the only synchronisation.
//
// What it shares with conv_split.h: glds16_s / wait_vmcnt<>, ConvParams / BatchGeom, the k-group-plane LDS layout (every
// ds_read_b128 of a fragment touches 16 distinct 16-byte slots) and the engine's EXISTING weight image of a 1x1 layer,
// [chunk][k-group][ko_pad][8]: the 64 rows of a channel tile are one 1 KiB DMA piece per (chunk, k-group).  There is no second
// weight image.
//
// LDS: a RING of kPwStages stages; a stage is one 32-channel chunk of the item's operands -- 4 KiB of weights (4 k-group planes
// x 64 rows x 16 bytes) and the pixel chunk behind them (4 planes x npos positions x 16 bytes, npos = the piece's pixel slots
// rounded up to DMA blocks of 64).  The item's whole weight slab (64 x cin x 2 bytes: 32 KiB at 256 input channels, 48 KiB at
// 384) is NOT kept in LDS: next to four 24 KiB pixel chunks of the widest piece it would take 144 KiB of kMaxLds = 160, a wider
// layer would not fit at all, and a weight chunk is needed exactly when its pixel chunk is -- so both travel through the same
// ring, 32 KiB (NJ = 1, 2) to 112 KiB (NJ = 12) whatever cin is, and one counted wait covers both.
//
// ARITHMETIC: conv_mfma_kernel's for T = f16, taps = 1 (conv_mfma.h), so that the bits are its bits.  Accumulators start at
// zero; v_mfma_f32_16x16x32_f16 with A = weight rows, B = pixels; the 32-channel chunks ascending, one MFMA per chunk and tile;
// then, per element in fp32: + bias, + residual, activate() (common.h), one conversion to fp16.  A lane stores the 4 channels
// x 1 pixel it holds (8 bytes) exactly as the generic kernel does -- no lane exchange, no value moves.  Only rows that are board
// pixels of the item's sample are stored, and only channels below cout_s.
#pragma once
#include "conv_split.h"

namespace sayuri {

constexpr int kPwKO = 64;          // output channels per workgroup
constexpr int kPwMaxCols = 24;     // column tiles a piece may have (12 per wave in the widest variant)
constexpr int kPwStages = 4;       // chunks in the ring
constexpr int kPwABytes = 4 * kPwKO * 16;  // one chunk of weights: 4 k-group planes x 64 rows x 8 channels

struct PwParams {
    ConvParams c;  // npos, num_pix_tiles unused
    int pieces;    // pieces asked for per sample; pw_cols() makes it column tiles per piece for every board size
    int pmax;      // pieces per sample in the grid (a board with fewer leaves the rest of its workgroups idle)
    int kts;       // channel tiles: ko_pad / 64
    int n0;        // first sample of the launch
};

// DMA blocks (64 positions) of a pixel chunk of the variant with NJ column tiles per wave, and the ring's bytes.
constexpr int pw_blocks(int nj) { return (2 * nj * 16 + 63) / 64; }
constexpr size_t pw_lds_bytes(int nj) { return (size_t)kPwStages * (kPwABytes + (size_t)pw_blocks(nj) * 64 * 64); }
// Column tiles per piece of a bs x bs board cut into `pieces` (no more pieces than column tiles; `cap`: no more tiles than the
// widest variant holds).  One rule for the host (grid, kernel variant) and the kernel.
__host__ __device__ inline int pw_cols(int bs, int pieces, bool cap = true) {
    const int ncol = (bs * bs + 15) >> 4;
    const int s = pieces < 1 ? 1 : (pieces > ncol ? ncol : pieces);
    const int cp = (ncol + s - 1) / s;
    return cap && cp > kPwMaxCols ? kPwMaxCols : cp;
}

// NJ: column tiles per wave (a piece has up to 2 NJ).
template <int NJ>
__global__ __launch_bounds__(256) void conv_pw_kernel(const PwParams pp) {
    constexpr int ST = kPwStages, NPB = pw_blocks(NJ), NPOS = NPB * 64;
    constexpr int STAGE = kPwABytes + NPOS * 64;  // bytes of a stage: the weights, then the pixel planes
    constexpr int PIECES = 1 + NPB;               // DMA pieces per wave and stage
    static_assert((ST - 2) * PIECES < 64, "the counted wait is a 6-bit vmcnt");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ConvParams& p = pp.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // channel tile fastest: neighbouring workgroup ids share a piece's pixels
    const int kt = blockIdx.x % pp.kts, item = blockIdx.x / pp.kts;
    const int piece = item % pp.pmax, sample = pp.n0 + item / pp.pmax;
    const int bs = p.g.bsz[sample];
    const int spix = bs * bs, cp = pw_cols(bs, pp.pieces), c0 = piece * cp;
    if (c0 * 16 >= spix) return;  // this board has fewer pieces than the grid: the whole workgroup leaves, in front of every barrier
    const int pix0 = c0 * 16, npix = min(cp * 16, spix - pix0), ncols = (npix + 15) >> 4;
    const int wave_m = wave & 1, wave_n = wave >> 1;
    const int nj0 = (ncols + 1) >> 1, col0 = wave_n ? nj0 : 0, nj = wave_n ? ncols - nj0 : nj0;
    const int kg = lane >> 4, px = lane & 15;
    const uint32_t ring = (uint32_t)(uintptr_t)smem;
    const int first_row = sample * p.g.slot_pix + pix0;  // activation row of the piece's first pixel

    // ---- the ordinary loads: bias and residual rows.  Asked for first, ahead of every DMA in the memory queue, and CONSUMED IN
    // FRONT OF THE K LOOP (below): hipcc waits for a load of its own with a vmcnt that knows nothing of the DMA pieces -- left to
    // where the epilogue first uses them, or worse inside the loop, that wait would drain the ring (conv_split.h, Kernel 1h).
    const int ko0 = kt * kPwKO + wave_m * 32 + 4 * kg;  // D rows 4 * (lane >> 4) + r of row tile i: channels ko0 + 16 i + r
    f32x4 b4[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) b4[i] = *(const f32x4*)(p.bias + ko0 + 16 * i);  // (bias has ko_pad entries)
    int orow[NJ], lp[NJ];
    f16x4 rr[2][NJ];
    const f16* __restrict__ gres = (const f16*)p.res;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = (col0 + j) * 16 + px;
        const bool in = j < nj && q < npix;
        orow[j] = in ? first_row + q : -1;
        lp[j] = in ? q : 0;  // an unused slot multiplies the piece's first pixel and is never stored
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            rr[i][j] = f16x4{0, 0, 0, 0};
            if (gres && in && ko0 + 16 * i < p.cout_s) rr[i][j] = *(const f16x4*)(gres + (size_t)orow[j] * p.cout_s + ko0 + 16 * i);
        }
    }

    // ---- DMA.  A stage's pieces of wave w: k-group plane w of the weights (64 rows x 16 bytes = 1 KiB, contiguous in the image)
    // and k-group plane w of every position block (64 positions; a position beyond the piece reads the piece's first pixel --
    // always a row of this sample -- and feeds a column nobody stores).  Every wave issues PIECES pieces per stage: the counted
    // waits below rely on it.
    const unsigned char* gin = (const unsigned char*)p.in;
    const unsigned char* gw = (const unsigned char*)p.w;
    const int nchunks = p.cin_s / kChunk;
    const uint32_t lane16 = lane * 16;
    const unsigned char* wbase = gw + ((size_t)wave * p.ko_pad + (size_t)kt * kPwKO) * 16;
    const size_t chunk_stride = (size_t)4 * p.ko_pad * 16;
    uint32_t boff[NPB];
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
        const int pos = i * 64 + lane;
        boff[i] = (uint32_t)(first_row + (pos < npix ? pos : 0)) * (uint32_t)(p.cin_s * 2) + wave * 16;
    }
    auto issue = [&](int chunk, int stage) {
        const uint32_t dst = ring + stage * STAGE;
        glds16_s(lane16, wbase + chunk * chunk_stride, dst + wave * 1024);
#pragma unroll
        for (int i = 0; i < NPB; ++i) glds16_s(boff[i], gin + chunk * (kChunk * 2), dst + kPwABytes + (wave * NPOS + i * 64) * 16);
    };
    // The prologue: the chunks 0 .. ST - 2, never beyond the layer.
    issue(0, 0);
#pragma unroll
    for (int c = 1; c <= ST - 2; ++c)
        if (c < nchunks) issue(c, c);

    // the bias and the residual rows have arrived (this wait is hipcc's own and also covers the prologue's DMA: chunk 0 is needed
    // at once anyway, the others were asked for a few instructions ago)
    asm volatile("" : "+v"(b4[0]), "+v"(b4[1]));
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(rr[0][j]), "+v"(rr[1][j]));

    f32x4 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // per-lane fragment offsets within a stage: A = (k-group plane, this wave's rows), B = (k-group plane, the pixel)
    const uint32_t a_off = (uint32_t)((kg * kPwKO + wave_m * 32 + px) * 16);
    uint32_t b_off[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) b_off[j] = (uint32_t)kPwABytes + (uint32_t)(kg * NPOS + lp[j]) * 16u;

    // ---- K loop.  Chunk c issues, behind its barrier, chunk c + ST - 1 into the stage of chunk c - 1, so every wave's memory
    // queue is, oldest first,
    //     ... chunk c | chunk c + 1 ... chunk c + ST - 2,
    // PIECES pieces per wave and chunk, the same number from every wave, and nothing else: the ordinary loads were consumed above.
    // The wait at the head of chunk c lets the (ST - 2) PIECES youngest pieces be outstanding: chunk c is older than all of them,
    // so its weights and pixels have landed -- for this wave.  In a layer's last ST - 2 chunks fewer chunks are behind c than the
    // count assumes; vmcnt is an immediate, so there the wait is for everything (what it asks for in excess was issued at least
    // one chunk earlier).  The barrier then says the same for all four waves -- each brought one k-group plane of the stage --
    // and that all of them are done with chunk c - 1, whose stage, (c - 1) mod ST, is where chunk c + ST - 1 goes.
    int stage = 0;
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (chunk + ST - 2 < nchunks) wait_vmcnt<(ST - 2) * PIECES>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");  // no fragment read of this chunk moves above the barrier
        const int refill = stage >= 1 ? stage - 1 : ST - 1;
        if (__builtin_expect(chunk + ST - 1 < nchunks, 1)) issue(chunk + ST - 1, refill);
        const unsigned char* st = smem + stage * STAGE;
        const f16x8 a0 = *(const f16x8*)(st + a_off);
        const f16x8 a1 = *(const f16x8*)(st + a_off + 256);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            // (no test for j < nj: a chunk stays one straight run of reads and MFMAs)
            const f16x8 b = *(const f16x8*)(st + b_off[j]);
            acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b, acc[0][j], 0, 0, 0);
            acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b, acc[1][j], 0, 0, 0);
        }
        stage = stage + 1 == ST ? 0 : stage + 1;
    }

    // ---- epilogue: conv_mfma_kernel's, statement by statement
    f16* __restrict__ gout = (f16*)p.out;
    const int act = p.act;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int ko = ko0 + 16 * i;
        if (ko >= p.cout_s) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (orow[j] < 0) continue;
            const size_t o = (size_t)orow[j] * p.cout_s + ko;
            f32x4 v = acc[i][j] + b4[i];
            if (gres) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += to_float(rr[i][j][r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = activate(v[r], act);
            f16x4 h;
#pragma unroll
            for (int r = 0; r < 4; ++r) h[r] = (f16)v[r];
            *(f16x4*)(gout + o) = h;
        }
    }
}

}  // namespace sayuri
