// conv_split.h -- the tower convolution (fp16 3x3 implicit GEMM) cut into MANY SMALL WORKGROUPS, for small batches.
//
// conv_board.h gives a board to one workgroup: right for 256 boards on 256 CUs, and one to three busy CUs for the lone board
// of a playing engine.  Here one workgroup (256 threads, one wave per SIMD) is one item
//     (sample, strip of whole board rows, 64 output channels),
// so that a 256-channel layer of one 19x19 board is 4 channel tiles x up to 19 strips.  A strip carries its own one-row
// halo above and below (rows of the neighbouring strips, or the zero prefix outside the board); it never spans two samples,
// and no workgroup waits for another: the launch boundary is the only synchronisation.
//
// What it shares with conv_board.h: the engine's weight image in natural row order ([tap][chunk][k-group][ko_pad][8], the
// 64 rows of a channel tile are one 1 KiB DMA piece per (tap, chunk, k-group)) and its zero-prefixed activation buffers;
// weights and halo reach LDS by global_load_lds_dwordx4 only; one s_barrier per K group (3 taps x 32 channels); the same
// ConvParams / BatchGeom.  And the ARITHMETIC: per output element the K order is 32-channel chunk, kernel row, tap in the
// row, with the bias in the accumulator first (board_mainloop), and the epilogue is board_store_pair (residual added in
// fp32, board_act8, one rounding to fp16) -- the outputs are the board kernel's bit for bit, whatever the split.
//
// Waves: 2 along M x 2 along N.  Wave (m, n) owns the row tiles 2m, 2m + 1 of the channel tile (32 channels: one pair for the
// epilogue's lane exchange) and half of the strip's column tiles.  LDS: a ring of three weight groups (12 KiB each, fetched
// two groups ahead and waited for with a counted vmcnt) and two halo chunks (64 bytes per halo position); ~60 KiB for a
// strip of five rows of a 19x19 board.  The fragment reads are plain LDS loads that hipcc schedules and counts; only the
// DMA is inline asm (glds16_s), so only vmcnt is counted by hand.
// The thin variants (a strip of at most six column tiles) also exist with a ring of four weight groups (+12 KiB) whose K loop
// holds no wait but the counted ones (see the bias below); engine_plan.h's split_ring says who runs which.
#pragma once
#include "conv_board.h"

namespace sayuri {

constexpr int kSplitKO = 64;        // output channels per workgroup
constexpr int kSplitMaxCols = 24;   // column tiles a strip may have (12 per wave in the widest variant)
constexpr int kSplitMaxPos = 512;   // halo positions a strip may have (DMA blocks of 64)
constexpr int kSplitStages = 3;     // weight groups in the ring: every variant has this form
constexpr int kSplitDeepStages = 4; // ... and the thin variants (NJ = 1, 2, 3: a K group of 6 to 18 MFMAs per wave) a deeper one.  Measured
                                    // (DESIGN.md Kernel 1h): every stage beyond four costs more at the start than it hides later
constexpr int kSplitABytes = 3 * kSplitKO * 64;  // one K group of weights: 3 taps x 64 rows x 32 channels
// Halo chunks a ring of `stages` weight groups keeps in LDS: the chunk in use and the ceil((stages - 2) / 3) chunks asked for
// ahead of it (the K loop's comment derives the lead).  Two up to five stages; the rings of six and eight stages that Kernel 1h
// measured ran with three.
constexpr int split_halo_slots(int stages) { return 1 + (stages - 2 + 2) / 3; }

struct SplitParams {
    ConvParams c;  // npos = halo positions per strip of this launch (multiple of 64: the largest strip's), num_pix_tiles unused
    int strips;    // strips asked for per board; split_rows() makes it rows per strip for every board size
    int smax;      // strips per sample in the grid (a board with fewer leaves the rest of its workgroups idle)
    int kts;       // channel tiles: ko_pad / 64
    int n0;        // first sample of the launch
};

// Rows per strip of a bs x bs board cut into `strips` (no more strips than rows; no more rows than fit the pixel slots).
// One rule for the host (grid, LDS size, kernel variant) and the kernel.
__host__ __device__ inline int split_rows(int bs, int strips) {
    const int s = strips < 1 ? 1 : (strips > bs ? bs : strips);
    const int rp = (bs + s - 1) / s, cap = kSplitMaxCols * 16 / bs;
    return rp < cap ? rp : cap;
}
constexpr size_t split_lds_bytes(int npos, int stages = kSplitStages) {
    return (size_t)stages * kSplitABytes + (size_t)split_halo_slots(stages) * (size_t)npos * 64;
}

template <int NJ, int ACT>
__device__ __forceinline__ void split_epilogue(const ConvParams& p, f32x4 (&acc)[2][NJ], const f16x8 (&rr)[NJ], const int (&orow)[NJ], int nj,
                                               int cb) {
    const bool with_res = p.res != nullptr, cok = cb < p.cout_s;
    const uint32_t row_bytes = (uint32_t)p.cout_s * 2u;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j < nj) {  // wave-uniform
            // the tile's last MFMA has left the pipeline before the lane exchange (inline asm) reads its result
            asm volatile("s_nop 15" : "+v"(acc[0][j]), "+v"(acc[1][j]));
            const bool ok = orow[j] >= 0 && cok;
            board_store_pair<ACT>(acc[0][j], acc[1][j], with_res, rr[j], (unsigned char*)p.out,
                                  (uint32_t)(ok ? orow[j] : 0) * row_bytes + (uint32_t)cb * 2u, ok);
        }
    }
}

// NJ: column tiles per wave (a strip has up to 2 NJ).  ST: weight groups in the ring -- kSplitStages is the kernel as it was
// before the ring had a depth; a deeper ring (kSplitDeepStages, the thin variants) asks for weights ST - 1 groups ahead and for
// halo chunks split_halo_slots(ST) - 1 chunks ahead, waits for the bias in front of the K loop instead of inside it, and changes
// nothing else: not the K order, not the epilogue.  Any ST from 3 to 22 is a valid kernel (an entry in kSplitEntries builds it).
template <int NJ, int ST>
__global__ __launch_bounds__(256) void conv_split_kernel(const SplitParams sp) {
    static_assert(ST >= 3 && 3 * (ST - 2) < 64, "the counted wait is a 6-bit vmcnt");
    constexpr int HS = split_halo_slots(ST), HL = HS - 1;  // halo slots, and how many chunks ahead a halo chunk is asked for
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ConvParams& p = sp.c;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // channel tile fastest: neighbouring workgroup ids share a strip's halo, and a die that gets every eighth id meets
    // one or two of the layer's weight slabs, not all of them
    const int kt = blockIdx.x % sp.kts, item = blockIdx.x / sp.kts;
    const int strip = item % sp.smax, sample = sp.n0 + item / sp.smax;
    const int bs = p.g.bsz[sample];
    const int rp = split_rows(bs, sp.strips), row0 = strip * rp;
    if (row0 >= bs) return;  // this board has fewer strips than the grid: the whole workgroup leaves, in front of every barrier
    const int nrows = min(rp, bs - row0), npix = nrows * bs, ncols = (npix + 15) >> 4;
    const int w2 = bs + 2, npos = p.npos, b_bytes = npos * 64;
    const int wave_m = wave & 1, wave_n = wave >> 1;
    const int nj0 = (ncols + 1) >> 1, col0 = wave_n ? nj0 : 0, nj = wave_n ? ncols - nj0 : nj0;
    const int kg = lane >> 4, px = lane & 15;
    const uint32_t a_ring = (uint32_t)(uintptr_t)smem, b_ring = a_ring + ST * kSplitABytes;
    const int first_row = sample * p.g.slot_pix + row0 * bs;  // activation row of the strip's first pixel

    // x / n as (int)((x + 0.5) * rcp(n)): x < 1024, n >= 2 -- the quotient is never within 0.015 of an integer boundary
    const float r_w2 = __builtin_amdgcn_rcpf((float)w2), r_bs = __builtin_amdgcn_rcpf((float)bs);

    // ---- epilogue addresses and the residual rows: asked for first (plain loads, ahead of every DMA in the memory queue),
    // consumed last
    const int R = lane >> 4;
    const int cb = kt * kSplitKO + wave_m * 32 + (R & 1) * 16 + (R >> 1) * 8;  // after the lane exchange: 8 channels from here
    int orow[NJ], lp[NJ];
    f16x8 rr[NJ];
    const unsigned char* rbase = p.res ? (const unsigned char*)p.res : (const unsigned char*)p.in - kZeroPrefix;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = (col0 + j) * 16 + px;
        const int y = (int)(((float)q + 0.5f) * r_bs), x = q - y * bs;
        const bool in = j < nj && q < npix;
        orow[j] = in ? first_row + q : -1;
        lp[j] = in ? y * w2 + x : 0;  // halo position of the pixel's tap (0, 0); an unused slot reads position 0
        // every lane loads, without a branch: a lane with nothing to add (and a layer without residual) reads 16 bytes that
        // are always there -- the head of the residual, or of the input's zero prefix -- and board_store_pair ignores them
        const uint32_t roff = p.res && in && cb < p.cout_s ? ((uint32_t)orow[j] * (uint32_t)p.cout_s + (uint32_t)cb) * 2u : 0u;
        rr[j] = *(const f16x8*)(rbase + roff);
    }

    // ---- DMA.  Weights: piece q = wave + 4 i of a K group is (tap in the row q >> 2, k-group q & 3) = 64 rows x 16 bytes.
    // Halo: piece i of a wave is k-group plane `wave` of the position block i (64 positions); a position outside the board
    // reads the buffer's zero prefix.  Every wave issues the same number of pieces: the counted waits below rely on it.
    const unsigned char* gin0 = (const unsigned char*)p.in - kZeroPrefix;
    const unsigned char* gw = (const unsigned char*)p.w;
    const int nchunks = p.cin_s / kChunk, ngroups = nchunks * 3, npb = npos >> 6;
    const size_t tap_stride = (size_t)nchunks * 4 * p.ko_pad * 16, chunk_stride = (size_t)4 * p.ko_pad * 16;
    const uint32_t lane16 = lane * 16;
    auto issue_a = [&](int G, int stage) {
        const int chunk = G / 3, row = G - chunk * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int q = wave + 4 * i, dx = q >> 2, kgq = q & 3;
            const unsigned char* base = gw + (size_t)(row * 3 + dx) * tap_stride + (size_t)chunk * chunk_stride +
                                        (size_t)((kgq * p.ko_pad + kt * kSplitKO) * 16);
            glds16_s(lane16, base, a_ring + stage * kSplitABytes + q * 1024);
        }
    };
    uint32_t boff[kSplitMaxPos / 64];
#pragma unroll
    for (int i = 0; i < kSplitMaxPos / 64; ++i) {
        const int pos = i * 64 + lane;
        const int r = (int)(((float)pos + 0.5f) * r_w2), xc = pos - r * w2, y = row0 - 1 + r;
        const bool in = r < nrows + 2 && y >= 0 && y < bs && xc >= 1 && xc <= bs;
        boff[i] = (in ? (uint32_t)kZeroPrefix + (uint32_t)(sample * p.g.slot_pix + y * bs + xc - 1) * (uint32_t)(p.cin_s * 2) : 0u) + wave * 16;
    }
    auto issue_b = [&](int chunk, int slot) {  // slot = chunk mod HS: with two slots the chunk's parity, else the caller's count
#pragma unroll
        for (int i = 0; i < kSplitMaxPos / 64; ++i)
            if (i < npb)
                glds16_s(boff[i], gin0 + chunk * (kChunk * 2), b_ring + (HS == 2 ? chunk & 1 : slot) * b_bytes + (wave * npos + i * 64) * 16);
    };
    // The prologue: A(0), the halo chunks 0 .. HL - 1, A(1) .. A(ST - 2) -- never beyond the layer.  A layer has at least one
    // chunk and three groups, which is all the three-stage ring asks for here; a 32-channel layer has no more than that, and
    // the input convolution two chunks and six groups: fewer than the deep ring, which therefore asks before it issues.
    issue_a(0, 0);
    issue_b(0, 0);
    if constexpr (HL > 1) {
#pragma unroll
        for (int h = 1; h < HL; ++h)
            if (h < nchunks) issue_b(h, h);
    }
    issue_a(1, 1);
    if constexpr (ST > 3) {
#pragma unroll
        for (int g = 2; g <= ST - 2; ++g)
            if (g == 2 || g < ngroups) issue_a(g, g);  // (a layer has at least three groups)
    }

    // accumulators start at the bias: D rows 4 * (lane >> 4) + r of row tile i are 4 consecutive output channels
    f32x4 acc[2][NJ], b4[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) b4[i] = *(const f32x4*)(p.bias + kt * kSplitKO + wave_m * 32 + i * 16 + 4 * kg);
    // The bias is the one load of hipcc's own that the K loop consumes.  Left alone, hipcc waits for it where the loop first uses
    // an accumulator -- an s_waitcnt vmcnt(0) INSIDE the loop, in the first group of every chunk, which also waits for every
    // DMA piece in flight: the ring is drained once per chunk, whatever its depth (the three-stage kernel has that wait; it
    // stays as it is).  A deeper ring uses the values here, so that the wait is in front of the loop, where group 0 needs A(0)
    // and the first halo chunk anyway; the loop then holds no vmcnt but the counted ones.  That wait also covers the rest of
    // the prologue, A(1) ... A(ST - 2): the price of every further stage (DESIGN.md Kernel 1h).
    if constexpr (ST > kSplitStages) asm volatile("" : "+v"(b4[0]), "+v"(b4[1]));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = b4[i];
    }
    // per-lane fragment offsets: A = (k-group plane, this wave's rows), B = (k-group plane, the pixel's tap (0, 0))
    const uint32_t a_off = (uint32_t)((kg * kSplitKO + wave_m * 32 + px) * 16);
    uint32_t b_off[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) b_off[j] = (uint32_t)(ST * kSplitABytes) + (uint32_t)(kg * npos + lp[j]) * 16u;

    // ---- K loop.  Group G (of chunk c = G / 3) issues, behind its barrier, the halo of chunk c + HL (in a chunk's first group
    // only) and then A(G + ST - 1), so every wave's memory queue is, oldest first,
    //     ... A(G) | A(G + 1) ... A(G + ST - 2)        with halo chunks between some of them,
    // three pieces per wave and weight group, the same number of pieces from every wave.  The wait at the head of group G lets
    // the 3 (ST - 2) youngest pieces be outstanding -- and nothing at all in a layer's last ST - 2 groups, where fewer groups
    // are left than the count assumes: vmcnt is an immediate, and one two-way choice keeps the loop the shape it had (what
    // those groups wait for in excess was asked for at least three groups earlier):
    //   weights  A(G) is older than A(G + 1) ... A(G + ST - 2), and than any halo piece between them: it has landed.  A halo
    //            chunk among the youngest only makes the wait ask for more than it needs, by at most that chunk's pieces.
    //   halo     chunk c is first read in group 3c and was asked for in group 3 (c - HL), in front of that group's weights
    //            (chunks below HL: in the prologue, in front of A(1)).  Younger than it at the head of group 3c are the 3 HL
    //            weight groups issued since, A(3 (c - HL) + ST - 1) ... A(3c + ST - 2), less those beyond the layer's end.  The
    //            wait lets A(3c + 1) ... A(3c + ST - 2) be outstanding (or nothing): a subset of them as long as
    //            3 (c - HL) + ST - 1 <= 3c + 1, which is ST - 2 <= 3 HL.  Hence HL = ceil((ST - 2) / 3): one chunk ahead and two
    //            slots up to five stages (the rings in use), two ahead and three slots from six to eight.
    // The barrier then says the same for all four waves, and that all of them are done with group G - 1: its weight stage,
    // (G - 1) mod ST, is where A(G + ST - 1) goes, and the halo slot of chunk c - 1, (c - 1) mod HS, is where chunk c + HL goes.
    int G = 0, stage = 0, slot = 0;
    for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma unroll
        for (int row = 0; row < 3; ++row) {
            if (G + ST - 2 < ngroups) wait_vmcnt<3 * (ST - 2)>();
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");  // no fragment read of this group moves above the barrier
            if (row == 0 && chunk + HL < nchunks) issue_b(chunk + HL, slot >= 1 ? slot - 1 : HS - 1);
            const int refill = stage >= 1 ? stage - 1 : ST - 1;
            if constexpr (ST > kSplitStages) {
                // (the hint keeps hipcc from laying this group's head out behind the loop as a small loop of its own, which
                // tests/test_latency_cpu.py's reading of the code object would take for a wait on global memory)
                if (__builtin_expect(G + ST - 1 < ngroups, 1)) issue_a(G + ST - 1, refill);
            } else {
                if (G + ST - 1 < ngroups) issue_a(G + ST - 1, refill);
            }
            const unsigned char* as = smem + stage * kSplitABytes + a_off;
            const unsigned char* bsl = smem + (HS == 2 ? chunk & 1 : slot) * b_bytes + row * (w2 * 16);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const f16x8 a0 = *(const f16x8*)(as + dx * (4 * kSplitKO * 16));
                const f16x8 a1 = *(const f16x8*)(as + dx * (4 * kSplitKO * 16) + 256);
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    // (no test for j < nj: a group stays one straight run of reads and MFMAs that hipcc can overlap; a column
                    // tile the wave does not own multiplies halo position 0 and is never stored)
                    const f16x8 b = *(const f16x8*)(bsl + b_off[j] + dx * 16);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b, acc[1][j], 0, 0, 0);
                }
            }
            ++G;
            stage = stage + 1 == ST ? 0 : stage + 1;
        }
        slot = slot + 1 == HS ? 0 : slot + 1;
    }

    switch (p.act) {
    case kMish: split_epilogue<NJ, kMish>(p, acc, rr, orow, nj, cb); break;
    case kIdentity: split_epilogue<NJ, kIdentity>(p, acc, rr, orow, nj, cb); break;
    case kReLU: split_epilogue<NJ, kReLU>(p, acc, rr, orow, nj, cb); break;
    case kSwish: split_epilogue<NJ, kSwish>(p, acc, rr, orow, nj, cb); break;
    case kELU: split_epilogue<NJ, kELU>(p, acc, rr, orow, nj, cb); break;
    case kSELU: split_epilogue<NJ, kSELU>(p, acc, rr, orow, nj, cb); break;
    case kGELU: split_epilogue<NJ, kGELU>(p, acc, rr, orow, nj, cb); break;
    default: split_epilogue<NJ, kHardSwish>(p, acc, rr, orow, nj, cb); break;
    }
}

}  // namespace sayuri
