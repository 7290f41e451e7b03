// Implicit-GEMM convolution forward on the gfx950 fp32 matrix cores.
//
//   Y[m][n] = act( (sum_k A[m][k] * Wt[n][k]) * scale[n] + bias[n] (+ R[m][n]) )
//   m = (image b, out row oy, out col ox)   M = N*Ho*Wo      (GEMM rows = pixels)
//   n = output channel                                        (GEMM cols)
//   k = (r, s, c) filter tap x input channel, c fastest       K = R*S*Cin
//
// Activations are NHWC, so for a fixed tap (r,s) a 32-wide k-tile is 128
// contiguous bytes of one input pixel: the A operand is gathered on the fly
// (zero-filled outside the image), never materialised (no im2col buffer).
// Weights are pre-packed [CoutPad][K] (vatl_pack_conv_weight) so both operands
// are K-contiguous and staged with 16-byte loads.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate) —
// the reference path is fp32 and parity is 1e-4 relative through 50+ layers,
// which bf16 inputs do not hold (SURVEY.md §7 hard part 1).  Peak for this
// instruction is 157.3 TFLOP/s (MI355X_MICROARCH.md).
//
// Block = 256 threads = 4 waves, tile BM x BN x 32, wave tile WM x WN made of
// 32x32 MFMA tiles.  K-loop: LDS double buffer, one barrier per k-tile; the next
// tile's global loads are issued before the current tile's 16 k-steps of MFMAs
// and written to the other LDS buffer after them (register staging), so HBM/L2
// latency hides under >= 2048 cycles of matrix work per wave.
// LDS rows are exactly one k-tile (32 floats = 128 bytes), bank conflicts are avoided by an XOR swizzle of
// the 16-byte chunk position: chunk c of tile row r lives at position c ^ ((r >> 1) & 7).  A ds_read_b128
// fragment read (16 consecutive rows at one logical chunk per lane group) then touches all 16 chunk slots of
// the 256-byte bank row, and a ds_write_b128 staging pass (8 rows x 8 chunks per wave) still covers whole
// rows: both conflict-free.  Against the 36-float padded rows of the first version this saves 11 % of LDS:
// the 64x128 and 128x64 tiles drop from 55 KB to 48 KB per block = THREE resident blocks per CU instead of two
// (their 132-138 VGPRs allow three waves per SIMD), which is what small-batch launches (fine-tune steps: one to
// three rounds of resident blocks) need to fill the chip.
//
// One ds_read_b128 feeds four MFMA k-steps: lanes 0-31 hold k = 8g+t, lanes
// 32-63 hold k = 8g+4+t at step t (same permutation for A and B, so the sum
// over the 8 k's of group g is complete after t = 0..3).  The per-output
// reduction order is fixed and independent of the batch position (needed for
// the THC de-duplication, SURVEY.md §7 hard part 3).
//
// The same kernel runs ConvTranspose2d(4,2,1) as four 2x2 sub-pixel phases
// (blockIdx.y = py*2+px): pad = (1-py, 1-px), output scattered to (2y+py, 2x+px).
#include "conv_igemm.h"
#include "tile_order.h"
#include "tune.h"

#include <algorithm>
#include <atomic>
#include <cstdlib>

namespace vatl {

// VAR selects the k-loop schedule (tuning knob, see vatl_tune_set).  Measured on MI355X, 3x3 512->512
// @8x6, batch 1024 (tools/conv_bench.py, TFLOP/s): VAR0 126, VAR2 132, VAR3 131, VAR4 138; ablations of
// VAR2: no global loads / LDS writes 150, no barrier 130, no fragment reads 140 (profiles/r01_notes.md).
//   0  two-phase: [address math + global loads] [64 MFMA with fragment reads] [LDS writes] barrier
//   2  fine-grained: the next tile's loads/address math and the next group's fragment reads are
//      issued in the shadow of the MFMAs (one 32x32x2 MFMA occupies the matrix pipe for 64 cycles;
//      the wave is free to issue other instructions meanwhile), pinned with sched_group_barrier
//   4  2 + distance-2 prefetch through two staging register sets (DEFAULT)
//   5  LDS-DMA kernel below (buffer_load ... lds, source-side XOR swizzle): 134 — equal to VAR2, the saved
//      ds_write pass (+5 %, ablation VAR13) is offset by its distance-1 prefetch
// (a rotated loop that buries the tile hand-over in the last MFMA group measured equal to VAR2 and was dropped)
template <int BM, int BN, int WM, int WN, bool STEM, int VAR, bool DUAL = false, int NT = 256, bool BNB = false>
__global__ __launch_bounds__(NT, 2) void conv_igemm_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                          // [2][BM][LDK]
    float* Bs = smem + 2 * BM * LDK;           // [2][BN][LDK]

    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int RP = NT / 8;                 // tile rows staged per pass (8 threads x 16 bytes cover the 32-wide k-tile)
    constexpr int LA = BM / RP, LB = BN / RP;  // 16-byte loads per thread per k-tile
    static_assert((BM / WM) * (BN / WN) == NT / 64, "one wave per wave tile");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;

    // XCD-aware tile order (tile_order.h): each XCD a contiguous run of tiles with the n-tile fastest, so the
    // blocks sharing an A panel hit the same L2
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int t = xcd_contiguous_index(bid, nblk);
    int m_tile, n_tile;
    if (p.order == 0) { m_tile = t / p.n_tiles; n_tile = t - m_tile * p.n_tiles; }
    else              { n_tile = t / p.m_tiles; m_tile = t - n_tile * p.m_tiles; }
    const int m0 = m_tile * BM, n0 = n_tile * BN;

    // All resident blocks of a launch start together and take the same time, so chip-wide the matrix-bound
    // k-loops and the memory-bound epilogues would alternate instead of overlapping.  Delaying the second block
    // of every CU (blocks 256..511 under in-order dispatch; later blocks inherit the phase of the slot they
    // take over) by half a k-loop puts the two phases side by side.  Performance only.
    if (p.stagger && bid >= 256 && bid < 512 && nblk >= 1024) {
        for (int i = 0; i < p.stagger; ++i) __builtin_amdgcn_s_sleep(127);
    }
    int pad_y = p.pad_y, pad_x = p.pad_x, ooy = p.ooy, oox = p.oox;
    const float* wbase = p.w;
    if (p.deconv) {
        const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
        pad_y = 1 - py; pad_x = 1 - px; ooy = py; oox = px;
        wbase += (long long)blockIdx.y * p.CoutPad * p.K;
    }
    // All global traffic goes through buffer descriptors: 32-bit byte offsets, and an
    // out-of-range offset (OOB) reads zeros / drops the store, so image borders, M
    // tails and the optional residual need no branches (branches made hipcc drain
    // vmcnt before the MFMAs in the first version of this kernel).
    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t wr = buf_rsrc(wbase, p.w_bytes);
    const __amdgpu_buffer_rsrc_t xr2 = buf_rsrc(DUAL ? p.x2 : p.x, DUAL ? p.x2_bytes : p.x_bytes);

    // ---- per-thread gather state --------------------------------------------
    const int lrow = tid >> 3;        // 0..RP-1
    const int kq = tid & 7;           // which float4 of the 32-wide k-tile
    const int wpos = (kq ^ ((lrow >> 1) & 7)) * 4;   // its swizzled position in the LDS row (RP is a multiple of 16: same for every pass)
    int abase[LA], iy0[LA], ix0[LA];  // element offset of (b, iy0, ix0, kq*4); may be negative
    int abase2[DUAL ? LA : 1];        // DUAL: element offset of the row's pixel in the second source
    const int HoWo = p.Ho * p.Wo;
    // 1x1 / stride 1 / pad 0: the input pixel of GEMM row m is pixel m — no (image, row, column) split, i.e. none of the two integer
    // divisions per staged row (8 per thread and block for a 128-row tile)
    const bool flat = !STEM && !DUAL && p.R == 1 && p.S == 1 && p.stride == 1 && pad_y == 0 && pad_x == 0 && p.H == p.Ho && p.W == p.Wo;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int m = m0 + lrow + RP * i;
        if (flat && m < p.M) {
            iy0[i] = 0; ix0[i] = 0;
            abase[i] = m * p.Cin + kq * 4;
        } else if (m < p.M) {
            const int b = fdiv(m, p.d_HoWo);
            const int rem = m - b * HoWo;
            const int oy = fdiv(rem, p.d_Wo);
            const int ox = rem - oy * p.Wo;
            iy0[i] = oy * p.stride - pad_y;
            ix0[i] = ox * p.stride - pad_x;
            abase[i] = ((b * p.H + iy0[i]) * p.W + ix0[i]) * p.Cin + kq * 4;
            if (DUAL) abase2[i] = ((b * p.H2 + oy * p.stride2) * p.W2 + ox * p.stride2) * p.C2 + kq * 4;
        } else {
            iy0[i] = -(1 << 20); ix0[i] = -(1 << 20); abase[i] = 0;
            if (DUAL) abase2[i] = 0;
        }
    }
    unsigned boff[LB];
#pragma unroll
    for (int j = 0; j < LB; ++j) boff[j] = (unsigned)(((n0 + lrow + RP * j) * p.K + kq * 4) * 4);

    f32x4 ra[LA], rb[LB];
    int kbase = 0;                     // split-K: first k-tile of this block's share
    if (p.splits > 1) {
        kbase = blockIdx.z * p.kt_per_split;
        p.ktiles = min(p.kt_per_split, p.ktiles - kbase);
    }
    int g_r = 0, g_s = 0, g_off = 0;
    bool g_sel = false;                // DUAL: this k-tile reads the second source
    auto gtap = [&](int kt) {          // filter tap / channel offset of k-tile kt (wave-uniform)
        kt += kbase;
        if (STEM) {                    // k-tile = one filter row: 8 taps x 4 channels
            g_r = kt; g_s = kq; g_off = kt * p.W * p.Cin;
        } else if (DUAL) {             // 1x1 over [source 1 channels | source 2 channels]
            g_sel = kt >= p.k1;
            g_r = 0; g_s = 0; g_off = (g_sel ? kt - p.k1 : kt) * BK;
        } else {
            const int rs = kt / p.kpr;
            const int c0 = (kt - rs * p.kpr) * BK;
            g_r = rs / p.S; g_s = rs - g_r * p.S;
            g_off = (g_r * p.W + g_s) * p.Cin + c0;
        }
    };
    auto a_load = [&](int i, bool live) -> f32x4 {     // the A-operand float4 of tile row lrow + 32 i for the current tap
        const bool ok = live && (unsigned)(iy0[i] + g_r) < (unsigned)p.H && (unsigned)(ix0[i] + g_s) < (unsigned)p.W;
        if (DUAL) return buf_load4(g_sel ? xr2 : xr, ok ? (unsigned)((g_sel ? abase2[i] : abase[i]) + g_off) << 2 : OOB);
        return buf_load4(xr, ok ? (unsigned)(abase[i] + g_off) << 2 : OOB);
    };
    auto gloadA = [&](int i, bool live) { ra[i] = a_load(i, live); };
    auto gloadB = [&](int j, int kt, bool live) {
        rb[j] = buf_load4(wr, live ? boff[j] + (unsigned)(kt + kbase) * (BK * 4) : OOB);
    };
    auto gload = [&](int kt, bool live) {
        gtap(kt);
#pragma unroll
        for (int i = 0; i < LA; ++i) gloadA(i, live);
#pragma unroll
        for (int j = 0; j < LB; ++j) gloadB(j, kt, live);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < LA; ++i)
            *reinterpret_cast<f32x4*>(&As[(buf * BM + lrow + RP * i) * LDK + wpos]) = ra[i];
#pragma unroll
        for (int j = 0; j < LB; ++j)
            *reinterpret_cast<f32x4*>(&Bs[(buf * BN + lrow + RP * j) * LDK + wpos]) = rb[j];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // fragment addressing: row frow (+ 32 i), logical chunk 2g + (lane >> 5), stored at chunk ^ ((frow >> 1) & 7)
    const int frow = lane & 31;
    int koff[BK / 8];
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) koff[g] = ((2 * g + (lane >> 5)) ^ ((frow >> 1) & 7)) * 4;

    gload(0, true);
    lstore(0);
    __syncthreads();

    auto frag_read = [&](f32x4 (&af)[TM], f32x4 (&bf)[TN], int buf, int g) {
        const float* Ab = As + (buf * BM + wm * WM + frow) * LDK + koff[g];
        const float* Bb = Bs + (buf * BN + wn * WN + frow) * LDK + koff[g];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * LDK);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * LDK);
    };
    auto mfma_group = [&](const f32x4 (&af)[TM], const f32x4 (&bf)[TN]) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][tt], bf[j][tt], acc[i][j], 0, 0, 0);
    };

    if (VAR == 0) {
        for (int kt = 0; kt < p.ktiles; ++kt) {
            const int buf = kt & 1;
            const bool more = kt + 1 < p.ktiles;
            if (more) gload(kt + 1, true);
#pragma unroll
            for (int g = 0; g < BK / 8; ++g) {
                f32x4 af[TM], bf[TN];
                frag_read(af, bf, buf, g);
                mfma_group(af, bf);
            }
            if (more) lstore(buf ^ 1);
            __syncthreads();
        }
    } else if (VAR == 4) {
        // Distance-2 prefetch: tile kt+2 is requested while tile kt is multiplied and is written to
        // LDS a full k-tile later (two staging register sets, loop unrolled by two so that the sets
        // are statically indexed).  Covers L2-miss latency (MALL/HBM, ~2 us) with >= 4096 pipe cycles.
        constexpr int NG = BK / 8;
        constexpr int MPG = 4 * TM * TN;
        f32x4 sa[2][LA], sb[2][LB];
        auto issue = [&](f32x4 (&da)[LA], f32x4 (&db)[LB], int kt) {      // kt may be past the end: OOB loads
            const bool live = kt < p.ktiles;
            gtap(kt);
#pragma unroll
            for (int i = 0; i < LA; ++i) da[i] = a_load(i, live);
#pragma unroll
            for (int j = 0; j < LB; ++j) db[j] = buf_load4(wr, live ? boff[j] + (unsigned)(kt + kbase) * (BK * 4) : OOB);
        };
        auto stash = [&](const f32x4 (&da)[LA], const f32x4 (&db)[LB], int buf) {
#pragma unroll
            for (int i = 0; i < LA; ++i) *reinterpret_cast<f32x4*>(&As[(buf * BM + lrow + RP * i) * LDK + wpos]) = da[i];
#pragma unroll
            for (int j = 0; j < LB; ++j) *reinterpret_cast<f32x4*>(&Bs[(buf * BN + lrow + RP * j) * LDK + wpos]) = db[j];
        };
        issue(sa[0], sb[0], 1);
        for (int kt = 0; kt < p.ktiles; kt += 2) {
            // step kt   : stash set0 (tile kt+1), request tile kt+2 into set1
            // step kt+1 : stash set1 (tile kt+2), request tile kt+3 into set0
            {
                const int buf = kt & 1;
                f32x4 af[2][TM], bf[2][TN];
                frag_read(af[0], bf[0], buf, 0);
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (g + 1 < NG) frag_read(af[(g + 1) & 1], bf[(g + 1) & 1], buf, g + 1);
                    if (g == 0) issue(sa[1], sb[1], kt + 2);
                    if (g == NG - 1) stash(sa[0], sb[0], buf ^ 1);
                    mfma_group(af[g & 1], bf[g & 1]);
                    if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
#pragma unroll
                    for (int q = 0; q < MPG; ++q) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x216, 2, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                __syncthreads();
            }
            if (kt + 1 < p.ktiles) {
                const int buf = (kt + 1) & 1;
                f32x4 af[2][TM], bf[2][TN];
                frag_read(af[0], bf[0], buf, 0);
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (g + 1 < NG) frag_read(af[(g + 1) & 1], bf[(g + 1) & 1], buf, g + 1);
                    if (g == 0) issue(sa[0], sb[0], kt + 3);
                    if (g == NG - 1) stash(sa[1], sb[1], buf ^ 1);
                    mfma_group(af[g & 1], bf[g & 1]);
                    if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
#pragma unroll
                    for (int q = 0; q < MPG; ++q) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x216, 2, 0);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                __syncthreads();
            }
        }
    } else {
        // VAR 2 = fine-grained schedule with distance-1 prefetch.  VAR 10..13 are ABLATIONS for profiling only (wrong results):
        // 10 = no global loads / LDS writes, 11 = no barrier, 12 = no fragment reads in the loop.
#ifdef VATL_ABLATION
        constexpr bool NO_GL = VAR == 10, NO_BAR = VAR == 11, NO_FRAG = VAR == 12, NO_ST = VAR == 13;   // 13 = loads kept, no LDS writes
#else
        static_assert(VAR < 10, "schedule variants 10..13 are profiling ablations: build with -DVATL_ABLATION (build.py --ablation)");
        constexpr bool NO_GL = false, NO_BAR = false, NO_FRAG = false, NO_ST = false;
#endif
        constexpr int NG = BK / 8;                          // 4 fragment groups per k-tile
        constexpr int MPG = 4 * TM * TN;                    // MFMAs per group
        f32x4 af[2][TM], bf[2][TN];
        if (NO_FRAG) { frag_read(af[0], bf[0], 0, 0); frag_read(af[1], bf[1], 0, 1); }
        for (int kt = 0; kt < p.ktiles; ++kt) {
            const int buf = kt & 1;
            const bool live = kt + 1 < p.ktiles;
            if (!NO_FRAG) frag_read(af[0], bf[0], buf, 0);
            gtap(kt + 1);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (g + 1 < NG && !NO_FRAG) frag_read(af[(g + 1) & 1], bf[(g + 1) & 1], buf, g + 1);
                // the next tile's global loads ride in the first two groups (A then B) so that
                // two groups of MFMAs (>= 2048 pipe cycles) cover their latency before the LDS writes
                if (g == 0 && !NO_GL) {
#pragma unroll
                    for (int i = 0; i < LA; ++i) gloadA(i, live);
                }
                if (g == 1 && !NO_GL) {
#pragma unroll
                    for (int j = 0; j < LB; ++j) gloadB(j, kt + 1, live);
                }
                mfma_group(af[g & 1], bf[g & 1]);
                // pin the interleave: fragment reads first, then MFMAs with the VALU/VMEM work in their shadow
                if (g + 1 < NG && !NO_FRAG) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
#pragma unroll
                for (int q = 0; q < MPG; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x016, 2, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (!NO_GL && !NO_ST) lstore(buf ^ 1);
            if (NO_ST) {                                   // keep the loaded registers alive
#pragma unroll
                for (int i = 0; i < LA; ++i) asm volatile("" ::"v"(ra[i]));
#pragma unroll
                for (int j = 0; j < LB; ++j) asm volatile("" ::"v"(rb[j]));
            }
            if (!NO_BAR) __syncthreads();
        }
        if (NO_BAR) __syncthreads();
    }

    if (p.splits > 1) {                // raw partial sums into this split's slice; scale / bias / residual / ReLU happen in the reduction
        p.y = p.part + (long long)blockIdx.z * p.part_slice;
        p.scale = nullptr; p.bias = nullptr; p.res = nullptr; p.relu = 0; p.out_nchw = 0; p.stats = nullptr;
    }
#ifdef VATL_ABLATION
    if (p.ablate & 1) {                // profiling build only: keep the accumulators alive, skip the write-out
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) s += acc[i][j][e];
        if (s == 12345.678f) p.y[0] = s;
        return;
    }
#endif
    conv_epilogue<BM, BN, WM, WN, NT, BNB>(p, acc, smem, m0, n0, ooy, oox, wm, wn, tid, lane, HoWo);
}

}  // namespace vatl

#include "gemm1x1_persistent.h"   // the persistent 1x1 family; why it is compiled in this unit: see the file

namespace vatl {

// LDS-DMA variant (VAR 5): operand tiles go HBM/L2 -> LDS directly (buffer_load ... lds, 1 KiB per wave
// instruction, no staging VGPRs, no ds_write pass).  The DMA destination is lane-linear (base + lane*16 B), so
// the LDS rows are unpadded 32-float rows and bank conflicts are avoided by an XOR swizzle applied on the
// SOURCE side: LDS chunk position p of tile row r holds global chunk p ^ ((r>>1)&7); the fragment reader asks
// for chunk (2g+half) ^ ((r>>1)&7).  16 consecutive rows then cover all 16 16-byte slots of a 256-byte bank row
// (conflict-free ds_read_b128).  Out-of-image taps / tail tiles use out-of-range offsets: the DMA writes zeros
// (verified on MI355X).  Two stages of 32 KiB; the epilogue reuses the space.
// ---------------------------------------------------------------------------------------------------------
// (body in a __device__ function: with the DMA builtin called from a lambda directly inside the __global__
// template, hipcc 7.2 silently drops the HOST stub of the kernel and the library fails to load)
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void conv_igemm_dma_body(const ConvParams& p, float* smem) {
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int STAGE = (BM + BN) * BK;            // floats per stage: A rows, then B rows, 32 floats each
    constexpr int IA = BM / 32, IB = BN / 32;        // DMA instructions per wave per stage (8 rows x 128 B each)
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves per block");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;

    const int t = xcd_contiguous_index(blockIdx.x, gridDim.x);
    const int m_tile = t / p.n_tiles;
    const int n_tile = t - m_tile * p.n_tiles;
    const int m0 = m_tile * BM, n0 = n_tile * BN;

    int pad_y = p.pad_y, pad_x = p.pad_x, ooy = p.ooy, oox = p.oox;
    const float* wbase = p.w;
    if (p.deconv) {
        const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
        pad_y = 1 - py; pad_x = 1 - px; ooy = py; oox = px;
        wbase += (long long)blockIdx.y * p.CoutPad * p.K;
    }
    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t wr = buf_rsrc(wbase, p.w_bytes);

    // ---- loader state: instruction i of wave w fills tile rows (4i + w)*8 .. +7; lane -> (row, chunk position)
    const int lrow = lane >> 3;                       // row inside the 8-row group
    const int lpos = lane & 7;                        // 16-byte position inside the LDS row
    const int lswz = ((lane >> 4) + 4 * (wave & 1)) & 7;   // ((row >> 1) & 7) for every row this lane loads
    const int lchk = lpos ^ lswz;                     // global 16-byte chunk that belongs at this position
    int abase[IA], iy0[IA], ix0[IA];
    const int HoWo = p.Ho * p.Wo;
#pragma unroll
    for (int i = 0; i < IA; ++i) {
        const int m = m0 + (4 * i + wave) * 8 + lrow;
        if (m < p.M) {
            const int b = fdiv(m, p.d_HoWo);
            const int rem = m - b * HoWo;
            const int oy = fdiv(rem, p.d_Wo);
            const int ox = rem - oy * p.Wo;
            iy0[i] = oy * p.stride - pad_y;
            ix0[i] = ox * p.stride - pad_x;
            abase[i] = ((b * p.H + iy0[i]) * p.W + ix0[i]) * p.Cin + lchk * 4;
        } else {
            iy0[i] = -(1 << 20); ix0[i] = -(1 << 20); abase[i] = 0;
        }
    }
    unsigned boff[IB];
#pragma unroll
    for (int j = 0; j < IB; ++j) boff[j] = (unsigned)(((n0 + (4 * j + wave) * 8 + lrow) * p.K + lchk * 4) * 4);

    auto issue = [&](int buf, int kt) {               // DMA of k-tile kt into stage buf (zeros past the end)
        const bool live = kt < p.ktiles;
        const int rs = kt / p.kpr;
        const int c0 = (kt - rs * p.kpr) * BK;
        const int r = rs / p.S, sx = rs - r * p.S;
        const int off = (r * p.W + sx) * p.Cin + c0;
        float* stage = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < IA; ++i) {
            const bool ok = live && (unsigned)(iy0[i] + r) < (unsigned)p.H && (unsigned)(ix0[i] + sx) < (unsigned)p.W;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void*)(stage + (4 * i + wave) * 8 * BK), 16,
                                                     ok ? (unsigned)(abase[i] + off) << 2 : OOB, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < IB; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wr, (lds_void*)(stage + (BM + (4 * j + wave) * 8) * BK), 16,
                                                     live ? boff[j] + (unsigned)kt * (BK * 4) : OOB, 0, 0, 0);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // fragment addressing: row = frow (+32 i), logical chunk 2g + half, stored at position chunk ^ ((frow>>1)&7)
    const int frow = lane & 31;
    const int half = lane >> 5;
    const int fswz = (frow >> 1) & 7;
    int koff[BK / 8];
#pragma unroll
    for (int g = 0; g < BK / 8; ++g) koff[g] = ((2 * g + half) ^ fswz) * 4;
    auto frag_read = [&](f32x4 (&af)[TM], f32x4 (&bf)[TN], int buf, int g) {
        const float* Ab = smem + buf * STAGE + (wm * WM + frow) * BK + koff[g];
        const float* Bb = smem + buf * STAGE + (BM + wn * WN + frow) * BK + koff[g];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * BK);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bb + j * 32 * BK);
    };

    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    constexpr int NG = BK / 8;
    constexpr int MPG = 4 * TM * TN;
    for (int kt = 0; kt < p.ktiles; ++kt) {
        const int buf = kt & 1;
        f32x4 af[2][TM], bf[2][TN];
        frag_read(af[0], bf[0], buf, 0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) frag_read(af[(g + 1) & 1], bf[(g + 1) & 1], buf, g + 1);
            if (g == 0) issue(buf ^ 1, kt + 1);
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[g & 1][i][tt], bf[g & 1][j][tt], acc[i][j], 0, 0, 0);
            if (g + 1 < NG) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
#pragma unroll
            for (int q2 = 0; q2 < MPG; ++q2) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x016, 2, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next stage has landed in LDS
        __syncthreads();
    }
    conv_epilogue<BM, BN, WM, WN>(p, acc, smem, m0, n0, ooy, oox, wm, wn, tid, lane, HoWo);
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv_igemm_dma_kernel(ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    conv_igemm_dma_body<BM, BN, WM, WN>(p, smem);
}

static std::atomic<int> g_var{4};      // k-loop schedule (vatl_tune_set(0, v)); 4 = shipped default
static std::atomic<int> g_order{0};    // tile order (vatl_tune_set(1, v))
static std::atomic<int> g_ablate{0};   // vatl_tune_set(6, bits): 1 = no epilogue, 2 = one k-tile only (profiling ablations, wrong results)
static std::atomic<int> g_bm{0};       // tile rows (vatl_tune_set(5, v)): 0 = by grid size, 64 or 128 = forced
static std::atomic<int> g_stagger{0};  // block stagger in percent of the k-loop time (vatl_tune_set(2, v)); 0 = off
static std::atomic<int> g_splitk_policy{0};  // vatl_tune_set(9, v): 0 = cut by the launch's own block count, 1 = batch-invariant cut (per-image geometry)
int igemm_set_schedule(int v) { g_var.store(v, std::memory_order_relaxed); return 0; }
int igemm_set_order(int v) { g_order.store(v, std::memory_order_relaxed); return 0; }
int igemm_set_ablate(int bits) { g_ablate.store(bits, std::memory_order_relaxed); return 0; }
int igemm_set_tile_rows(int v) { g_bm.store(v, std::memory_order_relaxed); return 0; }
int igemm_set_stagger(int v) { g_stagger.store(v, std::memory_order_relaxed); return 0; }
int igemm_set_splitk_policy(int v) { g_splitk_policy.store(v, std::memory_order_relaxed); return 0; }
int igemm_ablate_bits() { return g_ablate.load(std::memory_order_relaxed); }

// Split-K (opt-in, vatl_set_splitk_workspace): y = act(sum_z part[z] * scale + bias (+ residual)), slices summed in order.
// One thread per four channels of one output pixel (Cout % 4 == 0) or per element.
__global__ void splitk_reduce_kernel(const float* __restrict__ part, long long slice, int splits, const float* __restrict__ scale,
                                     const float* __restrict__ bias, const float* __restrict__ res, float* __restrict__ y, long long total, int Cout,
                                     int OHW, int relu, int out_nchw) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cout);
        float v = 0.f;
        for (int z = 0; z < splits; ++z) v += part[(long long)z * slice + i];
        v = v * (scale ? scale[c] : 1.f) + (bias ? bias[c] : 0.f);
        long long o = i;
        if (out_nchw) {
            const long long pix = i / Cout;
            const long long b = pix / OHW;
            o = (b * Cout + c) * OHW + (pix - b * OHW);
        }
        if (res) v += res[o];
        y[o] = relu ? fmaxf(v, 0.f) : v;
    }
}

// caller-owned split-K workspaces (vatl_set_splitk_workspace), one slot per device: a launch only ever uses the workspace that
// was registered while its own device was current.  All NULL = split-K off (g_splitk_any skips the device query).
constexpr int kMaxDevices = 16;
static std::atomic<float*> g_splitk_ws[kMaxDevices];
static std::atomic<long long> g_splitk_floats[kMaxDevices];
static std::atomic<int> g_splitk_any{0};

// ... and the calling host thread's own workspace (vatl_set_splitk_workspace_thread): what the launches of THIS thread use while it
// is set, with the batch-invariant cut policy — several host threads (DataParallel replica threads, one stream each) can run
// small-batch calls side by side without sharing partial-sum buffers or any global switch.
static thread_local float* tl_splitk_ws = nullptr;
static thread_local long long tl_splitk_floats = 0;

float* splitk_workspace(long long* floats, int* policy) {
    if (tl_splitk_ws) { *floats = tl_splitk_floats; *policy = 1; return tl_splitk_ws; }
    *policy = g_splitk_policy.load(std::memory_order_relaxed);
    if (!g_splitk_any.load(std::memory_order_acquire)) return nullptr;
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) return nullptr;
    *floats = g_splitk_floats[d].load(std::memory_order_relaxed);
    return g_splitk_ws[d].load(std::memory_order_acquire);
}

template <int BM, int BN, int WM, int WN, bool STEM, int VAR, bool DUAL = false, int NT = 256, bool BNB = false>
static int launch(const ConvParams& p, int phases, hipStream_t st) {
    auto kern = conv_igemm_kernel<BM, BN, WM, WN, STEM, VAR, DUAL, NT, BNB>;
    constexpr int smem = conv_smem_floats(BM, BN) * (int)sizeof(float);
    static std::atomic<unsigned> configured{0};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, configured, "conv_igemm")) return rc;
    ConvParams q = p;
    q.n_tiles = p.CoutPad / BN;
    q.m_tiles = cdiv(p.M, BM);
    q.order = g_order.load(std::memory_order_relaxed);
#ifdef VATL_ABLATION
    q.ablate = g_ablate.load(std::memory_order_relaxed);
    if ((q.ablate & 2) && q.ktiles > 1) q.ktiles = 1;
#else
    q.ablate = 0;
#endif
    // one s_sleep(127) = 8128 cycles; a k-tile costs ~8192 cycles when two blocks share the SIMDs
    q.stagger = (int)((long long)g_stagger.load(std::memory_order_relaxed) * p.ktiles / 100);
    const int m_tiles = cdiv(p.M, BM);
    const long long blocks = (long long)m_tiles * q.n_tiles * phases;
    long long ws_floats = 0;
    int sk_policy = 0;
    float* ws = splitk_workspace(&ws_floats, &sk_policy);
    q.splits = 1;
    if (ws && !STEM && !DUAL && !q.stats && !q.ablate && q.ktiles >= 16) {
        const long long out_elems = (long long)q.y_bytes / 4;
        int splits = 0;
        if (sk_policy == 1) {
            // batch-invariant policy (module calls with <= 16 crops, vatl_tune_set(9, 1)): the cut depends on the layer's
            // per-image geometry only — block count of a nominal 4-crop batch in 64-row tiles, workspace need of a 16-crop
            // batch — so a crop's bits do not depend on how many crops share its call
            const long long per_img_rows = p.M / (p.N > 0 ? p.N : 1), per_img_out = out_elems / (p.N > 0 ? p.N : 1);
            const long long blocks4 = (long long)cdiv(4 * per_img_rows, 64) * q.n_tiles * phases;
            if (blocks4 < 512) {
                splits = (int)std::min<long long>(q.ktiles / 8, (1024 + blocks4 - 1) / blocks4);
                const long long fit16 = ws_floats / (per_img_out > 0 ? 16 * per_img_out : 1);
                if (splits > fit16) splits = (int)fit16;
                if ((long long)splits * out_elems > ws_floats) splits = 0;          // more than 16 crops under this policy: unsplit
            }
        } else if (blocks < 256) {
            // small launch with a long reduction (single-frame / small-batch inference): cut K so that ~512 blocks are in flight
            splits = (int)std::min<long long>(q.ktiles / 8, (512 + blocks - 1) / blocks);
            const long long fit = ws_floats / (out_elems > 0 ? out_elems : 1);
            if (splits > fit) splits = (int)fit;
        }
        if (splits >= 2) {
            q.kt_per_split = (q.ktiles + splits - 1) / splits;
            q.splits = (q.ktiles + q.kt_per_split - 1) / q.kt_per_split;
            q.part = ws;
            q.part_slice = out_elems;
        }
    }
    dim3 grid((unsigned)(m_tiles * q.n_tiles), (unsigned)phases, (unsigned)q.splits);
    hipLaunchKernelGGL(kern, grid, dim3(NT), smem, st, q);
    meter_add(0, 2.0 * ((double)m_tiles * BM) * ((double)q.n_tiles * BN) * ((double)q.ktiles * BK) * phases);
    meter_route(BNB ? kRouteIgemmBnBwd : kRouteIgemm);
    if (q.splits > 1) {
        const long long total = q.part_slice;
        long long gsz = (total + 255) / 256; if (gsz > 8192) gsz = 8192;
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)gsz), dim3(256), 0, st, q.part, q.part_slice, q.splits, p.scale, p.bias, p.res, p.y, total,
                           p.Cout, p.OH * p.OW, p.relu, p.out_nchw);
    }
    return check_launch("conv_igemm");
}

template <int BM, int BN, int WM, int WN>
static int launch_dma(const ConvParams& p, int phases, hipStream_t st) {
    auto kern = conv_igemm_dma_kernel<BM, BN, WM, WN>;
    constexpr int stage_bytes = 2 * (BM + BN) * BK * (int)sizeof(float);
    constexpr int epi_bytes = BM * (BN + 4) * (int)sizeof(float);
    constexpr int smem = stage_bytes > epi_bytes ? stage_bytes : epi_bytes;
    static std::atomic<unsigned> configured{0};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, configured, "conv_igemm_dma")) return rc;
    ConvParams q = p;
    q.n_tiles = p.CoutPad / BN;
    q.m_tiles = cdiv(p.M, BM);
    q.order = 0; q.stagger = 0;
    dim3 grid((unsigned)(q.m_tiles * q.n_tiles), (unsigned)phases, 1);
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, st, q);
    meter_add(0, 2.0 * ((double)q.m_tiles * BM) * ((double)q.n_tiles * BN) * ((double)q.ktiles * BK) * phases);
    meter_route(kRouteIgemmDma);
    return check_launch("conv_igemm_dma");
}

// CoutPad granularity the packer must honour for a given Cout.
static int tile_n_for(int Cout) { return Cout <= 32 ? 32 : (Cout <= 64 ? 64 : 128); }

// Rows per block tile (measured on MI355X, tools/conv_bench.py --bm 128,64 at batches 120..1024, profiles/r01_notes.md):
//  * 64-channel outputs: the 64x64 tile (36.8 KB of LDS, four blocks = 16 waves per CU) beats 128x64 (two blocks) at
//    every size (+10..20 %);
//  * 128-wide tiles: 128 rows unless the launch has fewer than ~1.5 rounds of the 512 resident blocks (small batches:
//    the B = 120 fine-tune step, single-frame inference), where 64-row tiles fill the chip better (+15..30 %).
static int tile_m_for(const ConvParams& p, int phases, int bn, bool stem) {
    if (stem || bn < 64) return 128;                      // (a 256x32 tile measured 8 % slower than 128x32 on the HRNet 32-channel branch)
    const int forced = g_bm.load(std::memory_order_relaxed);
    if (forced == 64 || forced == 128) return forced;
    const long long blocks128 = (long long)cdiv(p.M, 128) * (p.CoutPad / bn) * phases;
    // 64-channel outputs: with the swizzled LDS rows the 128x64 tile has three resident blocks per CU and beats the 64x64 tile
    // (four blocks) by 2.5-3 % once the launch has a few rounds of them (l1.c2 1873 -> 1827 us, hr.b64 487 -> 474 us at 1024 crops)
    if (bn == 64) return blocks128 >= 1536 ? 128 : 64;
    return blocks128 < 768 ? 64 : 128;
}

static int dispatch(const ConvParams& p_in, int phases, bool stem, hipStream_t st, int64_t* row_blocks = nullptr) {
    ConvParams p = p_in;
    p.d_HoWo = make_fastdiv((unsigned)(p.Ho * p.Wo)); p.d_Wo = make_fastdiv((unsigned)p.Wo);
    const int bn = tile_n_for(p.Cout);
    if (p.CoutPad % bn != 0) return fail(VATL_EINVAL, "CoutPad %d must be a multiple of %d for Cout %d", p.CoutPad, bn, p.Cout);
    const int var = g_var.load(std::memory_order_relaxed);
    const bool stem64 = stem && bn == 64 && var != 0;     // the 7x7 stem runs the 64x64 tile (see below)
    const int bm = stem64 ? 64 : tile_m_for(p, phases, bn, stem);
    if (row_blocks) *row_blocks = (int64_t)cdiv(p.M, bm) * phases;   // what the statistics epilogue of the chosen tile writes
    if (stem) {
        // 7x7 stem, 1024 crops (tools/conv_bench.py): 128x64 two-phase 3.65 ms, 128x64 prefetch 3.40 ms, 64x64 prefetch 3.06 ms
        if (stem64) return launch<64, 64, 32, 32, true, 4>(p, phases, st);
        if (bn == 64) return launch<128, 64, 64, 32, true, 0>(p, phases, st);
        if (bn == 128) return launch<128, 128, 64, 64, true, 0>(p, phases, st);
        return launch<128, 32, 32, 32, true, 0>(p, phases, st);
    }
    if (streamk_wanted(p, phases, bn, bm, stem)) {
        if (p.bz) {
            if (!p.stats || p.out_nchw) return fail(VATL_EINVAL, "conv bn-backward fusion: needs a statistics buffer and an NHWC output with Cout %% 4 == 0");
            return launch_streamk<true>(p, st);
        }
        return launch_streamk<false>(p, st);
    }
    if (p.bz) {
        // data-gradient launch that also runs the reduction pass of the consumer layer's BatchNorm backward (fine-tune step)
        if (!p.stats || (p.Cout & 3) || p.out_nchw) return fail(VATL_EINVAL, "conv bn-backward fusion: needs a statistics buffer and an NHWC output with Cout %% 4 == 0");
        if (bn == 32) return launch<128, 32, 32, 32, false, 4, false, 256, true>(p, phases, st);
        if (bn == 64 && bm == 64) return launch<64, 64, 32, 32, false, 4, false, 256, true>(p, phases, st);
        if (bn == 64) return launch<128, 64, 64, 32, false, 4, false, 256, true>(p, phases, st);
        if (bm == 64) return launch<64, 128, 32, 64, false, 4, false, 256, true>(p, phases, st);
        return launch<128, 128, 64, 64, false, 4, false, 256, true>(p, phases, st);
    }
    if (bm == 64) {
        if (bn == 128) return launch<64, 128, 32, 64, false, 4>(p, phases, st);
        return launch<64, 64, 32, 32, false, 4>(p, phases, st);
    }
    // short-K 1x1 / stride-1 layers on whole 128x128 tiles: the persistent GEMM kernel
    if (persistent_wanted(p, phases, bn, var)) return launch_persistent(p, st);
    // long-K 1x1 layers on whole 128x128 tiles: the LDS-DMA ring kernel
    if (ring_wanted(p, phases, bn, bm, var)) return launch_ring(p, st);
    if (bn == 128 && var == 5) return launch_dma<128, 128, 64, 64>(p, phases, st);
    if (bn == 64 && var == 5) return launch_dma<128, 64, 64, 32>(p, phases, st);
    if (bn == 128) {
        if (var == 2) return launch<128, 128, 64, 64, false, 2>(p, phases, st);
        if (var == 4) return launch<128, 128, 64, 64, false, 4>(p, phases, st);
#ifdef VATL_ABLATION
        if (var == 10) return launch<128, 128, 64, 64, false, 10>(p, phases, st);
        if (var == 11) return launch<128, 128, 64, 64, false, 11>(p, phases, st);
        if (var == 12) return launch<128, 128, 64, 64, false, 12>(p, phases, st);
        if (var == 13) return launch<128, 128, 64, 64, false, 13>(p, phases, st);
#endif
        if (var == 0) return launch<128, 128, 64, 64, false, 0>(p, phases, st);
        return launch<128, 128, 64, 64, false, 4>(p, phases, st);
    }
    if (bn == 64) {
        // (a 256x64 tile — two 128-row tiles on one filter tile, 64x64 wave tiles, 238 VGPRs, two blocks per CU — measured 4 % SLOWER than
        // 128x64 with three: hr.b64 480 -> 502 us, l1.c2 1838 -> 1904 us at 1024 crops; not kept)
        if (var == 2) return launch<128, 64, 64, 32, false, 2>(p, phases, st);
        if (var == 0) return launch<128, 64, 64, 32, false, 0>(p, phases, st);
        return launch<128, 64, 64, 32, false, 4>(p, phases, st);
    }
    if (var == 2) return launch<128, 32, 32, 32, false, 2>(p, phases, st);
    if (var == 0 || p.ktiles < 4) return launch<128, 32, 32, 32, false, 0>(p, phases, st);   // K <= 96: nothing to pipeline
    return launch<128, 32, 32, 32, false, 4>(p, phases, st);
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_set_splitk_workspace_thread(float* workspace, int64_t floats) {
    if (workspace && floats <= 0) return fail(VATL_EINVAL, "set_splitk_workspace_thread: empty workspace");
    tl_splitk_ws = workspace;
    tl_splitk_floats = workspace ? (long long)floats : 0;
    return 0;
}

extern "C" int vatl_set_splitk_workspace(float* workspace, int64_t floats) {
    if (workspace && floats <= 0) return fail(VATL_EINVAL, "set_splitk_workspace: empty workspace");
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) return fail(VATL_EINVAL, "set_splitk_workspace: no current device (or index >= %d)", kMaxDevices);
    g_splitk_floats[d].store(workspace ? (long long)floats : 0, std::memory_order_relaxed);
    g_splitk_ws[d].store(workspace, std::memory_order_release);
    int any = 0;
    for (int i = 0; i < kMaxDevices; ++i) any |= g_splitk_ws[i].load(std::memory_order_relaxed) != nullptr;
    g_splitk_any.store(any, std::memory_order_release);
    return 0;
}

extern "C" int vatl_conv_cout_pad(int Cout) {
    const int bn = tile_n_for(Cout);
    return (Cout + bn - 1) / bn * bn;
}

static int conv2d_fwd_impl(const float* x, const float* w, const float* scale, const float* bias, const float* residual,
                           float* y, int N, int H, int W, int Cin, int Cout, int CoutPad, int R, int S, int stride, int pad,
                           int relu, int out_nchw, double* stats, int64_t* row_blocks, void* stream) {
    if (!x || !w || !y || N <= 0) return fail(VATL_EINVAL, "conv2d_fwd: null pointer or empty batch");
    if (stats && ((Cout & 3) || out_nchw)) return fail(VATL_EINVAL, "conv2d_fwd_stats: Cout %d must be a multiple of 4 (NHWC output)", Cout);
    const bool stem = (Cin == 4);
    if (!stem && Cin % 32 != 0) return fail(VATL_EINVAL, "conv2d_fwd: Cin %d must be a multiple of 32 (or 4 for the stem)", Cin);
    if (!stats && !out_nchw) {                            // narrow 3x3 layers: the persistent halo-tile kernel (bit-identical results)
        const int rc = conv3x3_halo_try(x, w, scale, bias, residual, y, N, H, W, Cin, Cout, CoutPad, R, S, stride, pad, relu, (hipStream_t)stream);
        if (rc <= 0) return rc;                           // 1 = not one of its shapes: fall through to the implicit GEMM
    }
    if (stem && S > 8) return fail(VATL_EINVAL, "conv2d_fwd: stem filter width %d > 8", S);
    ConvParams p{};
    p.x = x; p.w = w; p.scale = scale; p.bias = bias; p.res = residual; p.y = y;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.CoutPad = CoutPad;
    p.R = R; p.S = S; p.stride = stride; p.pad_y = pad; p.pad_x = pad;
    p.Ho = (H + 2 * pad - R) / stride + 1;
    p.Wo = (W + 2 * pad - S) / stride + 1;
    p.M = N * p.Ho * p.Wo;
    p.OH = p.Ho; p.OW = p.Wo; p.osy = 1; p.osx = 1; p.ooy = 0; p.oox = 0;
    p.relu = relu; p.out_nchw = out_nchw; p.deconv = 0;
    if (stem) { p.kpr = 1; p.ktiles = R; p.K = R * 8 * 4; }
    else      { p.kpr = Cin / BK; p.ktiles = R * S * p.kpr; p.K = R * S * Cin; }
    const long long xe = (long long)N * H * W * Cin, ye = (long long)p.M * Cout, we = (long long)CoutPad * p.K;
    if (xe >= (1LL << 30) || ye >= (1LL << 30) || we >= (1LL << 30))
        return fail(VATL_EINVAL, "conv2d_fwd: a tensor exceeds 2^30 elements (32-bit buffer offsets); split the batch");
    p.x_bytes = (unsigned)(xe * 4); p.y_bytes = (unsigned)(ye * 4); p.w_bytes = (unsigned)(we * 4);
    p.stats = stats;
    return dispatch(p, 1, stem, (hipStream_t)stream, row_blocks);
}

extern "C" int vatl_conv2d_fwd(const float* x, const float* w, const float* scale, const float* bias, const float* residual,
                               float* y, int N, int H, int W, int Cin, int Cout, int CoutPad, int R, int S, int stride, int pad,
                               int relu, int out_nchw, void* stream) {
    return conv2d_fwd_impl(x, w, scale, bias, residual, y, N, H, W, Cin, Cout, CoutPad, R, S, stride, pad, relu, out_nchw, nullptr, nullptr, stream);
}

extern "C" int64_t vatl_conv_stats_row_blocks(int64_t gemm_rows, int phases) { return (gemm_rows + 63) / 64 * phases; }   // capacity

extern "C" int vatl_conv2d_fwd_stats(const float* x, const float* w, float* y, double* stats, int64_t* row_blocks_used, int N, int H, int W,
                                     int Cin, int Cout, int CoutPad, int R, int S, int stride, int pad, void* stream) {
    if (!stats || !row_blocks_used) return fail(VATL_EINVAL, "conv2d_fwd_stats: null statistics buffer");
    return conv2d_fwd_impl(x, w, nullptr, nullptr, nullptr, y, N, H, W, Cin, Cout, CoutPad, R, S, stride, pad, 0, 0, stats, row_blocks_used, stream);
}

static int deconv4x4s2_fwd_impl(const float* x, const float* w, const float* scale, const float* bias, float* y,
                                int N, int H, int W, int Cin, int Cout, int CoutPad, int relu, double* stats, int64_t* row_blocks, void* stream) {
    if (!x || !w || !y || N <= 0) return fail(VATL_EINVAL, "deconv4x4s2_fwd: null pointer or empty batch");
    if (stats && (Cout & 3)) return fail(VATL_EINVAL, "deconv4x4s2_fwd_stats: Cout %d must be a multiple of 4", Cout);
    if (Cin % 32 != 0) return fail(VATL_EINVAL, "deconv4x4s2_fwd: Cin %d must be a multiple of 32", Cin);
    ConvParams p{};
    p.x = x; p.w = w; p.scale = scale; p.bias = bias; p.res = nullptr; p.y = y;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.CoutPad = CoutPad;
    p.R = 2; p.S = 2; p.stride = 1; p.pad_y = 0; p.pad_x = 0;
    p.Ho = H; p.Wo = W; p.M = N * H * W;
    p.OH = 2 * H; p.OW = 2 * W; p.osy = 2; p.osx = 2; p.ooy = 0; p.oox = 0;
    p.relu = relu; p.out_nchw = 0; p.deconv = 1;
    p.kpr = Cin / BK; p.ktiles = 4 * p.kpr; p.K = 4 * Cin;
    const long long xe = (long long)N * H * W * Cin, ye = 4LL * p.M * Cout, we = (long long)CoutPad * p.K;
    if (xe >= (1LL << 30) || ye >= (1LL << 30) || 4 * we >= (1LL << 30))
        return fail(VATL_EINVAL, "deconv4x4s2_fwd: a tensor exceeds 2^30 elements (32-bit buffer offsets); split the batch");
    p.x_bytes = (unsigned)(xe * 4); p.y_bytes = (unsigned)(ye * 4); p.w_bytes = (unsigned)(we * 4);   // w: one phase
    p.stats = stats;
    return dispatch(p, 4, false, (hipStream_t)stream, row_blocks);
}

extern "C" int vatl_deconv4x4s2_fwd(const float* x, const float* w, const float* scale, const float* bias, float* y,
                                    int N, int H, int W, int Cin, int Cout, int CoutPad, int relu, void* stream) {
    return deconv4x4s2_fwd_impl(x, w, scale, bias, y, N, H, W, Cin, Cout, CoutPad, relu, nullptr, nullptr, stream);
}

extern "C" int vatl_deconv4x4s2_fwd_stats(const float* x, const float* w, float* y, double* stats, int64_t* row_blocks_used, int N, int H, int W,
                                          int Cin, int Cout, int CoutPad, void* stream) {
    if (!stats || !row_blocks_used) return fail(VATL_EINVAL, "deconv4x4s2_fwd_stats: null statistics buffer");
    return deconv4x4s2_fwd_impl(x, w, nullptr, nullptr, y, N, H, W, Cin, Cout, CoutPad, 0, stats, row_blocks_used, stream);
}

// Last 1x1 conv of a bottleneck fused with the block's projection shortcut (Resnet.py:104-128 with a `downsample`):
//   y = act( W1' a  +  W2' x[strided]  +  bias ),   a (N,Ho,Wo,C1) = output of the 3x3, x (N,H2,W2,C2) = block input,
// one implicit GEMM over K = C1 + C2 whose A operand comes from two tensors.  w: [CoutPad][C1 + C2] with the two folded
// BatchNorm scales already multiplied into the rows (vatl_pack_conv1x1_dual_weight); bias = bias1 + bias2.  The
// projection's output never exists in HBM (for layer 1 of a ResNet-50 that is 3.2 GB written + read per 1024 crops).
extern "C" int vatl_conv1x1_dual_fwd(const float* a, const float* x, const float* w, const float* bias, float* y, int N, int Ho, int Wo,
                                     int C1, int H2, int W2, int C2, int stride2, int Cout, int CoutPad, int relu, void* stream) {
    if (!a || !x || !w || !y || N <= 0) return fail(VATL_EINVAL, "conv1x1_dual_fwd: null pointer or empty batch");
    if ((C1 % 32) || (C2 % 32)) return fail(VATL_EINVAL, "conv1x1_dual_fwd: channel counts %d / %d must be multiples of 32", C1, C2);
    if (Cout < 128 || (Cout & 3)) return fail(VATL_EINVAL, "conv1x1_dual_fwd: Cout %d must be >= 128 and a multiple of 4", Cout);
    if (stride2 < 1 || (Ho - 1) * stride2 >= H2 || (Wo - 1) * stride2 >= W2) return fail(VATL_EINVAL, "conv1x1_dual_fwd: stride %d does not map %dx%d onto %dx%d", stride2, Ho, Wo, H2, W2);
    ConvParams p{};
    p.x = a; p.x2 = x; p.w = w; p.scale = nullptr; p.bias = bias; p.res = nullptr; p.y = y;
    p.N = N; p.H = Ho; p.W = Wo; p.Cin = C1; p.Cout = Cout; p.CoutPad = CoutPad;
    p.R = 1; p.S = 1; p.stride = 1; p.pad_y = 0; p.pad_x = 0;
    p.Ho = Ho; p.Wo = Wo; p.M = N * Ho * Wo;
    p.OH = Ho; p.OW = Wo; p.osy = 1; p.osx = 1; p.ooy = 0; p.oox = 0;
    p.relu = relu; p.out_nchw = 0; p.deconv = 0;
    p.k1 = C1 / BK; p.C2 = C2; p.H2 = H2; p.W2 = W2; p.stride2 = stride2;
    p.kpr = (C1 + C2) / BK; p.ktiles = p.kpr; p.K = C1 + C2;
    const long long xe = (long long)p.M * C1, x2e = (long long)N * H2 * W2 * C2, ye = (long long)p.M * Cout, we = (long long)CoutPad * p.K;
    if (xe >= (1LL << 30) || x2e >= (1LL << 30) || ye >= (1LL << 30) || we >= (1LL << 30))
        return fail(VATL_EINVAL, "conv1x1_dual_fwd: a tensor exceeds 2^30 elements (32-bit buffer offsets); split the batch");
    p.x_bytes = (unsigned)(xe * 4); p.x2_bytes = (unsigned)(x2e * 4); p.y_bytes = (unsigned)(ye * 4); p.w_bytes = (unsigned)(we * 4);
    if (CoutPad % 128) return fail(VATL_EINVAL, "conv1x1_dual_fwd: CoutPad %d must be a multiple of 128", CoutPad);
    const int bm = tile_m_for(p, 1, 128, false);
    p.d_HoWo = make_fastdiv((unsigned)(p.Ho * p.Wo)); p.d_Wo = make_fastdiv((unsigned)p.Wo);
    if (bm == 64) return launch<64, 128, 32, 64, false, 4, true>(p, 1, (hipStream_t)stream);
    if (ring_wanted(p, 1, 128, bm, g_var.load(std::memory_order_relaxed))) return launch_ring(p, (hipStream_t)stream);
    return launch<128, 128, 64, 64, false, 4, true>(p, 1, (hipStream_t)stream);
}

// General form behind the data-gradient paths: explicit GEMM pixel grid (Ho x Wo), separate paddings and an
// output scatter (oy*osy+ooy, ox*osx+oox) into an OH x OW image.  Transposed-conv style gradients are
// phase-decomposed by the caller (alphapose/models/hip_train.py): e.g. the data gradient of a 3x3/2 conv is
// four launches with 1x1 / 1x2 / 2x1 / 2x2 taps over the output-gradient grid, scattered with osy = osx = 2.
static int conv2d_fwd_ex_impl(const float* x, const float* w, const float* scale, const float* bias, const float* residual, float* y,
                              int N, int H, int W, int Cin, int Cout, int CoutPad, int R, int S, int stride, int pad_y, int pad_x,
                              int Ho, int Wo, int OH, int OW, int osy, int osx, int ooy, int oox, int relu, const float* bn_z, const float* bn_mask_y,
                              const float* bn_scale, const float* bn_bias, const float* bn_mean, const float* bn_invstd, double* stats,
                              int64_t* row_blocks_used, void* stream) {
    if (!x || !w || !y || N <= 0) return fail(VATL_EINVAL, "conv2d_fwd_ex: null pointer or empty batch");
    if (Cin % 32 != 0) return fail(VATL_EINVAL, "conv2d_fwd_ex: Cin %d must be a multiple of 32", Cin);
    ConvParams p{};
    p.x = x; p.w = w; p.scale = scale; p.bias = bias; p.res = residual; p.y = y;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.CoutPad = CoutPad;
    p.R = R; p.S = S; p.stride = stride; p.pad_y = pad_y; p.pad_x = pad_x;
    p.Ho = Ho; p.Wo = Wo; p.M = N * Ho * Wo;
    p.OH = OH; p.OW = OW; p.osy = osy; p.osx = osx; p.ooy = ooy; p.oox = oox;
    p.relu = relu; p.out_nchw = 0; p.deconv = 0;
    p.kpr = Cin / BK; p.ktiles = R * S * p.kpr; p.K = R * S * Cin;
    const long long xe = (long long)N * H * W * Cin, ye = (long long)N * OH * OW * Cout, we = (long long)CoutPad * p.K;
    if (xe >= (1LL << 30) || ye >= (1LL << 30) || we >= (1LL << 30))
        return fail(VATL_EINVAL, "conv2d_fwd_ex: a tensor exceeds 2^30 elements (32-bit buffer offsets); split the batch");
    p.x_bytes = (unsigned)(xe * 4); p.y_bytes = (unsigned)(ye * 4); p.w_bytes = (unsigned)(we * 4);
    if (bn_z) {                                           // (vatl_conv2d_fwd_ex_bnbwd, which checked the fusion arguments and passes no scale / bias / ReLU)
        p.bz = bn_z; p.bmy = bn_mask_y; p.bsc = bn_scale; p.bbi = bn_bias; p.bmu = bn_mean; p.bis = bn_invstd; p.stats = stats;
    }
    return dispatch(p, 1, false, (hipStream_t)stream, row_blocks_used);
}

extern "C" int vatl_conv2d_fwd_ex(const float* x, const float* w, const float* scale, const float* bias, const float* residual, float* y,
                                  int N, int H, int W, int Cin, int Cout, int CoutPad, int R, int S, int stride, int pad_y, int pad_x,
                                  int Ho, int Wo, int OH, int OW, int osy, int osx, int ooy, int oox, int relu, void* stream) {
    return conv2d_fwd_ex_impl(x, w, scale, bias, residual, y, N, H, W, Cin, Cout, CoutPad, R, S, stride, pad_y, pad_x, Ho, Wo, OH, OW, osy, osx, ooy, oox,
                              relu, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

// Data-gradient launch fused with the reduction pass of a BatchNorm backward (ActiveLearning.py:672, loss.backward()): y receives
// g = (W^T dz + residual) * [consumer layer's ReLU mask] and `stats` the per-(row block, channel) double partials of
// (sum g, sum g * xhat) in the layout vatl_bn_bwd_from_stats reduces.  bn_z = that layer's conv output (layout of y);
// mask = bn_mask_y > 0 when given (layers whose ReLU follows a residual sum), else bn_z*bn_scale+bn_bias > 0 when bn_scale is
// given, else none.  row_blocks_used returns how many row blocks were written (<= vatl_conv_stats_row_blocks(N*Ho*Wo, 1)).
extern "C" int vatl_conv2d_fwd_ex_bnbwd(const float* x, const float* w, const float* residual, float* y, int N, int H, int W, int Cin, int Cout,
                                        int CoutPad, int R, int S, int stride, int pad_y, int pad_x, int Ho, int Wo, int OH, int OW, int osy, int osx,
                                        int ooy, int oox, const float* bn_z, const float* bn_mask_y, const float* bn_scale, const float* bn_bias,
                                        const float* bn_mean, const float* bn_invstd, double* stats, int64_t* row_blocks_used, void* stream) {
    if (int rc = bnbwd_args_check("conv2d_fwd_ex_bnbwd", bn_z, bn_scale, bn_bias, bn_mean, bn_invstd, stats, row_blocks_used)) return rc;
    return conv2d_fwd_ex_impl(x, w, nullptr, nullptr, residual, y, N, H, W, Cin, Cout, CoutPad, R, S, stride, pad_y, pad_x, Ho, Wo, OH, OW, osy, osx, ooy,
                              oox, 0, bn_z, bn_mask_y, bn_scale, bn_bias, bn_mean, bn_invstd, stats, row_blocks_used, stream);
}
