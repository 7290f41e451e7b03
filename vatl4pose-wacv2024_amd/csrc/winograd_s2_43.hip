// 3x3 / stride 2 / pad 1 convolution forward as Winograd F(4x3, 2x2) summed over the four input phases (inference; Bottleneck.conv2 of the first
// block of ResNet stages 2 - 4).
//
// Pad the filter to 4x4 with a zero last row and column and write its tap r = 2a + b: y[o] = sum_b sum_a g_b[a] P_b[o + a] with the input phase
// P_b[i] = x[2i + b - 1] (zero outside the image) and g_b[a] = w[2a + b].  In 2-D that is four 2x2-tap stride-1 correlations — phase (by, bx):
// P[i][j] = x[2i + by - 1][2j + bx - 1], g[a][b] = w[2a + by][2b + bx] — each one exactly the F(4x3, 2x2) problem of winograd_deconv43.hip (a 4-row x
// 3-column output tile from a 5x4 tile of the phase image, the same B4^T, B3^T, G4, G3, A4^T, A3^T).  All four produce the SAME output tile through the
// same output transform, so their transform-domain products add into one accumulator set: the reduction runs over (phase, input channel), one
// launch, no partial sums in memory, one output transform per tile.
//
// The single-tap phases have g[1] = 0 and G4's last row is [0 1]: for the two by = 1 phases the transformed filter is identically zero at row position
// xi = 4.  That half of the reduction runs with four row positions (16 MFMAs per group instead of 20, four fragment loads, the fifth input row neither
// staged nor read): 20 + 20 + 16 + 16 = 72 multiplies per 12 outputs against the direct sum's 108 (1.5x fewer MFMAs), and the 32x24 / 16x12 / 8x6 output
// grids of the 256x192 networks are whole tiles.  (For the bx = 1 phases column position nu = 3 is zero as well; that would only idle one wave of a block
// that runs in lock-step and is not exploited.)
//
// The block is winograd_deconv43_body's: 32 tiles x 64 output channels, four waves, wave nu = column position nu x all row positions, two filter-fragment
// sets alternating between the 32-channel halves, LDS-DMA staging into column arrays with a zero entry, chunk swizzle on the source side, XCD-contiguous
// tile order, xi sum in registers and nu sum through the two stage buffers, two blocks per CU.  What differs:
//   * no phase in the tile unit: a block is (m-tile, 64-channel filter tile) and walks 4 * Cin / 16 stages — phase (0,0), (0,1) with five row positions,
//     then (1,0), (1,1) with four (the position count is a compile-time parameter of the stage body).
//   * the phase image is a stride-2 view: its pixel (yy, xx) = 4 ty + i - pad_y, 3 tx + r - pad_x (pad = 1 - b, inside for 0 <= yy < H / 2,
//     0 <= xx < W / 2) is image pixel (2 yy + pad_y, 2 xx + pad_x).  Which pieces are outside the image — and which of two tiles a shared column-array
//     entry serves at a row end — depends on the phase, and the descriptor's range check does not catch them (they land in a neighbouring row or image).
//     The eight staging offsets and the two fragment-read column indices of a lane are therefore recomputed at the three phase changes of a block
//     (the offsets one stage ahead, with the DMA that uses them) instead of kept four-fold in registers.
//   * the filter stream of a block is contiguous: [n / 64][by = 0: bx, step = c / 8, 20 positions | by = 1: bx, step, 16 positions][n / 32 % 2][lane][c % 4]
//     (winograd_pack.h: wino_s2_43_pack_block), U = G4 g G3^T in float64 rounded once.
//   * epilogue: dense NHWC output, scale / bias / ReLU, no residual.
// The executed FLOPs, 2 * (tiles rounded up to 32) * 72 * Cin * Cout, are booked in the meter's DIRECT class: the launch is reached through conv2d_fwd, whose
// time the benchmark books under its implicit-GEMM group; in the Winograd class they would add FLOPs without time to the other group's fraction.
// The per-output arithmetic depends only on the tile's own pixels: results do not depend on the batch position.
#include "common.h"
#include "buffer.h"

#include <algorithm>
#include <atomic>
#include <type_traits>

namespace vatl {

struct S2W43Params {
    const float* x;
    const float* u;
    const float* scale;
    const float* bias;
    float* y;
    int N, H, W, Cin, Cout;
    int OH, OW;                       // output grid = grid of every phase image's valid pixels (H / 2, W / 2)
    int TH, TW, tpi, Mtiles;          // tiles per image column / row / image (OH / 4, OW / 3), tiles in the launch
    int m_tiles, n_tiles;             // 32-tile groups, 64-channel filter tiles
    int relu;
    int sp;                           // stages per phase: Cin / 16
    int rn;                           // filter tiles per group of the tile order
    unsigned x_bytes, u_bytes, y_bytes;
    FastDivU d_TH, d_TW, d_tpi, d_grp, d_rn, d_rn_last;
};

constexpr unsigned S2W_OOB = 0xFFFF0000u;      // staging offset of a zero piece: out of range for every tensor the host accepts, still so with stage * 64 bytes added
constexpr int S2W_TB = 32;                     // tiles per block
constexpr int S2W_CK = 16;                     // channels per LDS stage
constexpr int S2W_NQ = S2W_TB + 1;             // entries of a column array: one per tile + the halo of the last tile
constexpr int S2W_ROWE = 3 * S2W_NQ + 1;       // entries per input row: three column arrays + the zero entry
constexpr int S2W_ROWF = S2W_ROWE * S2W_CK;    // floats per input row
constexpr int S2W_ITEMS = 5 * S2W_ROWE * 4;    // 16-byte pieces of a stage
constexpr int S2W_NDMA = (S2W_ITEMS + 63) / 64;
constexpr int S2W_ROW4_DMA = 4 * S2W_ROWE * 4 / 64;      // first DMA instruction of the fifth input row
constexpr int S2W_STAGE = S2W_NDMA * 256;      // floats per stage
constexpr int S2W_NLD = S2W_NDMA / 4;          // DMA instructions per wave and stage
constexpr int S2W_LDS_BYTES = 2 * S2W_STAGE * 4;
static_assert(S2W_NDMA % 4 == 0 && 16 * S2W_TB * 32 * 4 == S2W_LDS_BYTES, "stage buffers = output-transform tiles");
static_assert(4 * S2W_ROWE * 4 % 64 == 0, "the fifth input row starts a DMA instruction");

// (body in a __device__ function, as winograd_body: with the DMA builtin inside the __global__ function hipcc drops the kernel's host stub)
__device__ __forceinline__ void winograd_s2_43_body(const S2W43Params& p, float* smem) {
    constexpr int NW = 4;
    float* Rs = smem;                                      // [2][5 rows][3 arrays x 33 entries + zero entry][16 channels], chunk-swizzled
    const int tid = threadIdx.x, lane = tid & 63, nu = __builtin_amdgcn_readfirstlane(tid >> 6);

    // XCD-aware tile order of winograd_body: block b runs on XCD b % 8; each XCD gets a contiguous run of
    //     for (group of rn filter tiles) for (m-tile) for (filter tile in the group)
    const int bid = blockIdx.x, nblk = gridDim.x;
    const int xcd = bid & 7, loc = bid >> 3, q8 = nblk >> 3, r8 = nblk & 7;
    const int t = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
    const int grp = fdiv(t, p.d_grp), rem = t - grp * (p.m_tiles * p.rn);
    const bool last_grp = p.n_tiles - grp * p.rn < p.rn;
    const int rn_g = last_grp ? p.n_tiles - grp * p.rn : p.rn;
    const int m_tile = fdiv(rem, last_grp ? p.d_rn_last : p.d_rn), n_tile = grp * p.rn + (rem - m_tile * rn_g);
    const int m0 = m_tile * S2W_TB, n0 = n_tile * 64;

    const __amdgpu_buffer_rsrc_t xr = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t ur = buf_rsrc(p.u, p.u_bytes);

    // ---- U fragments: [n_tile][by = 0: 2 * steps x 20 positions | by = 1: 2 * steps x 16 positions][half][lane][4], position = xi * 4 + nu ----------
    const int steps = p.sp * 2;                            // 8-channel steps per phase
    const int gsteps = 4 * steps, gsteps5 = 2 * steps;     // steps of the block; of them with five row positions
    const unsigned ubase = (unsigned)n_tile * (unsigned)steps * 147456u + ((unsigned)((nu * 2) * 64 + lane) << 4);     // bytes; + xi * 8 KB + half * 1 KB
    auto u_load = [&](auto np, f32x4 (&dst)[5], int gstep_, int half) {
        constexpr int NP = decltype(np)::value;
        const int g = min(gstep_, gsteps - 1);             // past the last step: the last step's fragments again, no per-lane select
        const unsigned soff = g < gsteps5 ? (unsigned)g * 40960u : (unsigned)gsteps5 * 40960u + (unsigned)(g - gsteps5) * 32768u;
        const unsigned off = ubase + (unsigned)half * 1024u + soff;
#pragma unroll
        for (int xi = 0; xi < NP; ++xi) dst[xi] = buf_load4(ur, off + xi * 8192u);
    };
    f32x4 ua[5], ub[5];
    u_load(std::integral_constant<int, 5>{}, ua, 0, 0);

    // ---- staging by LDS-DMA: winograd_deconv43_body's loader on the phase image (pad_y, pad_x) = (1 - by, 1 - bx) ----------------------------------
    unsigned goff[S2W_NLD];
    // (m0 and the lane go through an empty asm: without it the compiler hoists the phase-independent part of every call out of the stage loops
    // and keeps it in registers the loop does not have)
    auto set_goff = [&](int pad_y, int pad_x) {
        int m0 = m_tile * S2W_TB, ln = lane;
        asm volatile("" : "+s"(m0), "+v"(ln));
#pragma unroll
        for (int u = 0; u < S2W_NLD; ++u) {
            __builtin_amdgcn_sched_barrier(0);             // one offset at a time: the accumulators and a fragment set are live around the later calls
            const int pz = (nu + NW * u) * 64 + ln;
            goff[u] = S2W_OOB;
            if (pz >= S2W_ITEMS) continue;
            const int cpos = pz & 3, e = pz >> 2;
            const int i = e / S2W_ROWE, re = e - i * S2W_ROWE;
            const int r = re / S2W_NQ, q = re - r * S2W_NQ;
            if (r >= 3) continue;                          // the row's zero entry
            const int chunk = cpos ^ ((q >> 2) & 3);
            int m = m0 + q;                                // column r of tile m ...
            int gr = fdiv(m, p.d_TW), tx = m - gr * p.TW;
            int xx = 3 * tx + r - pad_x;
            if (m >= p.Mtiles || (tx == 0 && xx < 0)) {    // ... or, when that is outside, column 3 + r of the tile before (a row end / the halo)
                m -= 1;
                if (m < 0) continue;
                gr = fdiv(m, p.d_TW); tx = m - gr * p.TW;
                xx = 3 * tx + 3 + r - pad_x;
            }
            const int b = fdiv(gr, p.d_TH), ty = gr - b * p.TH;
            const int yy = 4 * ty - pad_y + i;
            if (m < p.Mtiles && (unsigned)yy < (unsigned)p.OH && (unsigned)xx < (unsigned)p.OW)
                goff[u] = (unsigned)(((b * p.H + 2 * yy + pad_y) * p.W + 2 * xx + pad_x) * p.Cin + chunk * 4) << 2;
        }
    };
    // st: stage inside the phase the offsets were made for; rows5: that phase has five row positions (else the fifth input row is not staged)
    auto stage_dma = [&](int buf, int st, bool rows5) {
        unsigned so = (unsigned)st * (S2W_CK * 4);
        asm volatile("" : "+s"(so));                       // (opaque: otherwise the loop keeps a second, advancing copy of the eight offsets)
#pragma unroll
        for (int u = 0; u < S2W_NLD; ++u) {
            if (!rows5 && nu + NW * u >= S2W_ROW4_DMA) continue;           // (wave-uniform)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (lds_void*)(Rs + buf * S2W_STAGE + (nu + NW * u) * 256), 16,
                                                     goff[u] + so, 0, 0, 0);
        }
    };
    set_goff(1, 1);
    stage_dma(0, 0, true);

    // ---- fragment addressing: lane = (tile l & 31, channel quad l >> 5); this wave's column combination is d[ja] + sgn * d[jb]
    // (B3^T rows: d0 - d2, d1 + d2, d2 - d1, d1 - d3).  ca / cb: float index (relative to a stage's input row, first 8-channel step) of the
    // two columns of the lane's tile; the second step is the same index ^ 8; a column outside the phase image = the row's zero entry.
    const int ja = nu == 0 ? 0 : (nu == 2 ? 2 : 1);
    const int jb = nu == 0 ? 2 : (nu == 1 ? 2 : (nu == 2 ? 1 : 3));
    const float sgn = nu == 1 ? 1.f : -1.f;
    int ca, cb;
    auto set_cols = [&](int pad_x) {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int tl = ln & 31, h = ln >> 5;
        const int m = min(m0 + tl, p.Mtiles - 1);
        const int gr = fdiv(m, p.d_TW), tx = m - gr * p.TW;
        auto col = [&](int j) {
            const int xx = 3 * tx + j - pad_x;
            const int q = tl + j / 3;
            return (unsigned)xx < (unsigned)p.OW ? ((j % 3) * S2W_NQ + q) * S2W_CK + ((h ^ ((q >> 2) & 3)) << 2) : 3 * S2W_NQ * S2W_CK + (h << 2);
        };
        ca = col(ja); cb = col(jb);
    };

    f32x16 accs[2][5];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int xi = 0; xi < 5; ++xi)
#pragma unroll
            for (int e = 0; e < 16; ++e) accs[hh][xi][e] = 0.f;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's DMA pieces have landed
    __syncthreads();

    // V = B4^T d B3 of the lane's tile: this wave's NP row positions, four channels (NP = 4: rows 0 .. 3 of B4^T read input rows 0 .. 3 only)
    auto make_v = [&](auto np, f32x4 (&v)[5], const float* Rb, int x8) {
        constexpr int NP = decltype(np)::value;
        f32x4 tc[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const f32x4 da = *reinterpret_cast<const f32x4*>(Rb + i * S2W_ROWF + (ca ^ x8));
            const f32x4 db = *reinterpret_cast<const f32x4*>(Rb + i * S2W_ROWF + (cb ^ x8));
            tc[i] = da + sgn * db;
        }
        const f32x4 s = tc[3] - tc[1];
        v[0] = 2.f * (tc[0] - tc[2]) + s;                  // 2 t0 -   t1 - 2 t2 +   t3
        v[1] = s - (tc[1] + tc[2]);                        //      - 2 t1 -   t2 +   t3
        v[2] = 2.f * tc[1] + (tc[3] - 3.f * tc[2]);        //        2 t1 - 3 t2 +   t3
        v[3] = s;                                          //      -   t1        +   t3
        if constexpr (NP == 5) v[4] = (tc[4] - tc[2]) - 2.f * s;      //        2 t1 -   t2 - 2 t3 + t4
    };
    auto mfma_group = [&](auto np, f32x16 (&ac)[5], const f32x4 (&v)[5], const f32x4 (&uu)[5]) {
        constexpr int NP = decltype(np)::value;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int xi = 0; xi < NP; ++xi)
                ac[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[xi][tt], uu[xi][tt], ac[xi], 0, 0, 0);
    };

    // One phase: its Cin / 16 stages.  The two fragment sets alternate between the halves with a look-ahead of one group of MFMAs, as in winograd_deconv43_body;
    // the scheduler barriers keep the requests where they are written.  gs0: the phase's first stage in the block's count (fragment steps and the stage buffer
    // follow it).  The DMA issued in a stage fills the other buffer for the next stage; in a phase's last stage that is the next phase's first one, so the
    // offsets change before it.  (A fragment request that crosses into the four-position half with NP = 5 reads one fragment it does not use.)
    auto run_phase = [&](auto np, int ph, int gs0) {
        constexpr int NP = decltype(np)::value;
        set_cols(1 - (ph & 1));
        for (int st = 0; st < p.sp; ++st) {
            const int gs = gs0 + st, buf = gs & 1;
            const float* Rb = Rs + buf * S2W_STAGE;
            const bool wrap = st + 1 == p.sp;
            if (wrap && ph < 3) set_goff(1 - ((ph + 1) >> 1), 1 - ((ph + 1) & 1));
            f32x4 v[5];
            u_load(np, ub, 2 * gs, 1);
            __builtin_amdgcn_sched_barrier(0);
            make_v(np, v, Rb, 0);
            mfma_group(np, accs[0], v, ua);
            __builtin_amdgcn_sched_barrier(0);
            u_load(np, ua, 2 * gs + 1, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(np, accs[1], v, ub);
            __builtin_amdgcn_sched_barrier(0);
            u_load(np, ub, 2 * gs + 1, 1);
            if (!(wrap && ph == 3)) stage_dma(buf ^ 1, wrap ? 0 : st + 1, wrap ? ph + 1 < 2 : ph < 2);      // (behind the fragments of this stage's second step: loads retire in order)
            __builtin_amdgcn_sched_barrier(0);
            make_v(np, v, Rb, 8);
            mfma_group(np, accs[0], v, ua);
            __builtin_amdgcn_sched_barrier(0);
            u_load(np, ua, 2 * gs + 2, 0);
            __builtin_amdgcn_sched_barrier(0);
            mfma_group(np, accs[1], v, ub);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces of the next stage have landed
            __syncthreads();
        }
    };
    run_phase(std::integral_constant<int, 5>{}, 0, 0);
    run_phase(std::integral_constant<int, 5>{}, 1, p.sp);
    run_phase(std::integral_constant<int, 4>{}, 2, 2 * p.sp);
    run_phase(std::integral_constant<int, 4>{}, 3, 3 * p.sp);

    // ---- output transform (winograd_deconv43_body's, dense output) ------------------------------------------------------------------------
    // thread = (tile tid >> 3, channel quad tid & 7); its 4 x 3 output pixels are base + a * row stride + b * column stride
    const __amdgpu_buffer_rsrc_t yr = buf_rsrc(p.y, p.y_bytes);
    const int c4 = tid & 7, tl = tid >> 3;
    const unsigned cstep = (unsigned)p.Cout << 2, rstep = (unsigned)(p.OW * p.Cout) << 2;      // bytes between neighbouring columns / rows
    const bool valid = m0 + tl < p.Mtiles;
    unsigned obase;
    {
        const int m = min(m0 + tl, p.Mtiles - 1);
        const int b = fdiv(m, p.d_tpi), r = m - b * p.tpi;
        const int ty = fdiv(r, p.d_TW), tx = r - ty * p.TW;
        obase = (unsigned)(((b * p.OH + 4 * ty) * p.OW + 3 * tx) * p.Cout + n0 + c4 * 4) << 2;
    }
    const float lo = p.relu ? 0.f : -INFINITY;
    float* Ps = smem;                                      // [nu][row a][tile][32 channels]
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {                       // one filter half at a time through the same LDS tiles
        const int n = n0 + 32 * hh + c4 * 4;
        f32x4 sc = {1.f, 1.f, 1.f, 1.f}, bi = {0.f, 0.f, 0.f, 0.f};
        if (p.scale) sc = *reinterpret_cast<const f32x4*>(p.scale + n);       // requested before the accumulators go through LDS
        if (p.bias) bi = *reinterpret_cast<const f32x4*>(p.bias + n);
        // xi sum in registers (rows of A4^T): P0 = M0 + M1 + M2 + M3, P1 = M1 - M2 + 2 M3, P2 = M1 + M2 + 4 M3, P3 = M1 - M2 + 8 M3 + M4
        {
            const int cl = lane & 31;
            f32x16 (&ac)[5] = accs[hh];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const float sum = ac[1][e] + ac[2][e], dif = ac[1][e] - ac[2][e], m3 = ac[3][e];
                Ps[((nu * 4 + 0) * S2W_TB + row) * 32 + cl] = ac[0][e] + sum + m3;
                Ps[((nu * 4 + 1) * S2W_TB + row) * 32 + cl] = dif + 2.f * m3;
                Ps[((nu * 4 + 2) * S2W_TB + row) * 32 + cl] = sum + 4.f * m3;
                Ps[((nu * 4 + 3) * S2W_TB + row) * 32 + cl] = dif + 8.f * m3 + ac[4][e];
            }
        }
        lds_barrier();
        // nu sum (rows of A3^T) per (tile, output row a, channel quad); 16-byte stores of NHWC channel runs
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            f32x4 pq[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) pq[k] = *reinterpret_cast<const f32x4*>(&Ps[((k * 4 + a) * S2W_TB + tl) * 32 + c4 * 4]);
            f32x4 yv[3];
            yv[0] = pq[0] + pq[1] + pq[2];
            yv[1] = pq[1] - pq[2];
            yv[2] = pq[1] + pq[2] + pq[3];
            if (valid) {
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    f32x4 o;
#pragma unroll
                    for (int c = 0; c < 4; ++c) o[c] = fmaxf(yv[b][c] * sc[c] + bi[c], lo);
                    buf_store4(yr, obase + (unsigned)hh * 128u + (unsigned)a * rstep + (unsigned)b * cstep, o);
                }
            }
        }
        if (hh == 0) lds_barrier();                        // the second half's tiles go where this one's were read (the stores stay in flight)
    }
}

__global__ __launch_bounds__(256, 2) void winograd_s2_43_kernel(S2W43Params p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    winograd_s2_43_body(p, smem);
}

static std::atomic<unsigned> g_s2w43_lds_done;

// tensors within the 32-bit byte offsets of the buffer descriptors (the bounds of winograd_deconv43.hip's host check)
static bool s2w43_in_range(long long N, int H, int W, int Cin, int Cout) {
    const long long mt = N * (H / 8) * (W / 6), xe = N * H * W * Cin, ye = N * (H / 2) * (W / 2) * Cout, ue = 72LL * Cout * Cin;
    return xe <= (long long)(S2W_OOB / 4) && ye < (1LL << 30) && ue < (1LL << 28) && mt < (1LL << 30) && Cin / S2W_CK < 1024 &&
           (mt + S2W_TB - 1) / S2W_TB * (Cout / 64) < (1LL << 31);
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_conv3x3s2_winograd43_supported(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
    if (H % 8 != 0 || W % 6 != 0 || Cin % 16 != 0 || Cout % 64 != 0) return 0;         // H, W even, (H / 2) % 4 == 0, (W / 2) % 3 == 0
    return s2w43_in_range(N, H, W, Cin, Cout) ? 1 : 0;
}

extern "C" int vatl_conv3x3s2_winograd43_fwd(const float* x, const float* u, const float* scale, const float* bias, float* y, int N, int H, int W,
                                             int Cin, int Cout, int relu, void* stream) {
    if (!x || !u || !y) return fail(VATL_EINVAL, "conv3x3s2_winograd43_fwd: null pointer");
    if (!vatl_conv3x3s2_winograd43_supported(N, H, W, Cin, Cout))
        return fail(VATL_EINVAL, "conv3x3s2_winograd43_fwd: %d x %dx%d x %d -> %d is outside H %% 8 == 0, W %% 6 == 0, Cin %% 16 == 0, Cout %% 64 == 0 and 32-bit offsets",
                    N, H, W, Cin, Cout);
    S2W43Params p{};
    p.x = x; p.u = u; p.scale = scale; p.bias = bias; p.y = y;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.relu = relu;
    p.OH = H / 2; p.OW = W / 2;
    p.TH = p.OH / 4; p.TW = p.OW / 3; p.tpi = p.TH * p.TW;
    p.Mtiles = N * p.tpi;
    p.m_tiles = cdiv(p.Mtiles, S2W_TB);
    p.n_tiles = Cout / 64;
    p.sp = Cin / S2W_CK;
    p.x_bytes = (unsigned)((long long)N * H * W * Cin * 4);
    p.y_bytes = (unsigned)((long long)N * p.OH * p.OW * Cout * 4);
    p.u_bytes = (unsigned)(72LL * Cout * Cin * 4);
    // a filter tile (64 channels, all four phases) is Cin * 18 KB; the tiles of a group (<= 2 MB, at least two) stay in an XCD's L2 over the sweep of the m-tiles
    p.rn = std::max(1, std::min(p.n_tiles, std::max(2, 2048 / (18 * Cin))));
    p.d_TH = make_fastdiv(p.TH); p.d_TW = make_fastdiv(p.TW); p.d_tpi = make_fastdiv(p.tpi);
    p.d_grp = make_fastdiv((unsigned)(p.m_tiles * p.rn)); p.d_rn = make_fastdiv(p.rn);
    p.d_rn_last = make_fastdiv(p.n_tiles % p.rn ? p.n_tiles % p.rn : p.rn);
    if (int rc = ensure_dynamic_lds((const void*)winograd_s2_43_kernel, S2W_LDS_BYTES, g_s2w43_lds_done, "winograd_s2_43")) return rc;
    hipLaunchKernelGGL(winograd_s2_43_kernel, dim3((unsigned)(p.m_tiles * p.n_tiles)), dim3(256), S2W_LDS_BYTES, (hipStream_t)stream, p);
    meter_add(0, 2.0 * ((double)p.m_tiles * S2W_TB) * 72.0 * (double)Cin * (double)Cout);
    meter_route(kRouteWinoS2_43);
    return check_launch("winograd_s2_43");
}
