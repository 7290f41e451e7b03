// The ResNet stem of csrc/stem_pool.hip (NCHW crops -> conv 7x7 / stride 2 / pad 3 (3 -> 64) -> folded BatchNorm -> ReLU -> max-pool 3x3 / stride 2 / pad 1 -> NHWC)
// with a 1-D Winograd transform along the image rows: 99 (executed: 108) multiplies per output and output channel instead of 168.  Inference only, same contract
// as vatl_stem7x7s2_pool_fwd, same precision class, not the same bits.
//
// The algebra.  A row splits into its even and odd pixels, E[q] = x[2q], O[q] = x[2q + 1].  For a fixed (channel c, filter row ky) a stem output is
//     y[ox] = sum_{i<4} w[2i] O[ox + i - 2]  +  sum_{i<3} w[2i + 1] E[ox + i - 1]:
// a 4-tap correlation on O plus a 3-tap correlation on E, both stride 1.  A TILE is two neighbouring outputs ox = 2t, 2t + 1: F(2,4) on O[2t - 2 .. 2t + 2] takes
// 5 products for 8, F(2,3) on E[2t - 1 .. 2t + 2] takes 4 for 6, both land on the same two outputs.  With the 9 input pixels p[j] = x[4t - 3 + j] of a tile
// (O = p0 p2 p4 p6 p8, E = p1 p3 p5 p7; out-of-image pixels are zero BEFORE the transform), the nine POSITIONS are
//     V0 = 2 p0 - p2 - 2 p4 + p6    V1 = 2 p2 + p4 - p6    V2 = -2 p2 + 3 p4 - p6    V3 = p6 - p2    V4 = 2 p2 - p4 - 2 p6 + p8         (F(2,4), points 0 1 -1 2 inf,
//     V5 = p1 - p5                  V6 = p3 + p5           V7 = p5 - p3              V8 = p7 - p3                                         rows scaled to integers)
// the filter side, with g = w[c][ky][0::2], f = w[c][ky][1::2], formed in float64 and rounded once by the packer below, is
//     U0 = g0 / 2   U1 = (g0 + g1 + g2 + g3) / 2   U2 = (g0 - g1 + g2 - g3) / 6   U3 = (g0 + 2 g1 + 4 g2 + 8 g3) / 6   U4 = g3
//     U5 = f0       U6 = (f0 + f1 + f2) / 2        U7 = (f0 - f1 + f2) / 2        U8 = f2
// M_p = sum over (ky, c) of V_p U_p is a GEMM per position with K = 21, and y[2t] = M0 + M1 + M2 + M3 + M5 + M6 + M7,  y[2t + 1] = M1 - M2 + 2 M3 + M4 + M6 - M7 + M8.
// The transforms run along the row only, so a transformed input row is formed ONCE, when the row arrives, and is read by the 3 - 4 stem rows and 64 channels using it.
//
// The kernel.  As in stem_pool.hip a block of four waves owns an image (or a band of its pooled rows) and slides down it one pooled row = two stem rows = four
// input rows per step; the next step's input rows travel through registers while the MFMAs run.  What differs:
//   * LDS holds TRANSFORMED rows: a ring of 10 slots, [channel][position][tile] per slot (TILES = W / 4).  A step reads the 9 rows 4i - 3 .. 4i + 5; the four new
//     rows overwrite rows of this step and are therefore stored after the step's barrier.
//   * MFMA = v_mfma_f32_16x16x4_f32: rows = 16 tiles, columns = 16 output channels, k = 4 entries of the (ky, c) list kk = 3 ky + c, padded from 21 to 24 (the
//     filter of entries 21 - 23 is zero and their lanes read a zero region).  Wave w computes channels [16 w, 16 w + 16) of ALL tiles of both stem rows: 2 x MB
//     units of 16 tiles, 9 x 6 MFMAs each, the same work for every wave.  One LDS dword per MFMA and lane: lanes 0 - 15 read consecutive tiles, and the slot and
//     channel strides are = 16 (mod 32) with a ring of even length, so the two 16-lane groups of a 32-lane half always sit on opposite halves of the 32 banks.
//     The reads of a k-step are issued one k-step ahead of its MFMAs.
//   * The whole filter of a wave is 54 registers.  Positions that enter the two outputs with the same coefficients share an accumulator (M0 + M5, M1 + M6,
//     M2 + M7, M3, M4 + M8: the MFMA does the addition), so a unit needs 5 x 4 accumulator registers and six vector operations per output pair.  A lane ends up
//     with both pixels of four neighbouring tiles of one channel, so pooled column q = max(y[2q - 1], y[2q], y[2q + 1]) takes
//     its left neighbour from the same lane three times out of four and from lane - 16 (the unit before for lanes 0 - 15) otherwise, and both stem rows of the step
//     and the carried odd row of the step before are in the same lane too: the pooling never leaves the registers.  The pooled row is transposed through LDS so
//     that the write-out is whole 256-byte pixels.
// Post-ReLU values are >= 0, so 0 is the neutral element of every maximum (image borders).  The arithmetic of a pixel depends on its own image and x position only:
// results are independent of the batch position and of the band cut.
#include "common.h"

namespace vatl {

template <int MB> struct StemW1dLds {
    static constexpr int TILES = 16 * MB;                                   // tiles of an input row = pooled columns (W / 4)
    static constexpr int CH = 9 * TILES + ((9 * TILES) % 32 == 16 ? 0 : 16);   // floats of one channel of a slot: [9 positions][TILES], = 16 (mod 32)
    static constexpr int SLOT = 3 * CH;                                     // = 16 (mod 32) as well
    static constexpr int RING = 10;                                         // 9 rows in use; even, so that consecutive rows are an odd number of slots apart
    static constexpr int ZREG = (9 * TILES + 32 + 31) / 32 * 32;            // zeros: the reads of the padded k entries land here whatever their position and unit
    static constexpr int OSTR = 68;                                         // floats of a pooled pixel in the output tile (= 4 mod 8: the four tile groups of a wave on distinct banks)
    static constexpr int FLOATS = ZREG + RING * SLOT + TILES * OSTR;
    static_assert(CH % 32 == 16 && SLOT % 32 == 16 && RING % 2 == 0, "bank layout of the MFMA operand reads");
};

struct StemW1dParams {
    const float* x;          // (N, 3, H, W) fp32
    const float* w;          // packed: [4 channel blocks][9 positions][6 k-steps][64 lanes]
    const float* scale;      // folded BatchNorm (64)
    const float* bias;
    float* y;                // (N, H / 4, W / 4, 64)
    int N, H, W;
    int bands, steps_per_band;   // a block = (image, band of pooled rows)
};

typedef float f32x2_w1d __attribute__((ext_vector_type(2)));
struct StemW1dPiece { f32x4 a, b; f32x2_w1d c; };    // pixels 4t - 4 .. 4t + 5 of one (row, channel, tile)

template <int MB>
__global__ __launch_bounds__(256, 2) void stem_pool_w1d_kernel(StemW1dParams p) {
    using L = StemW1dLds<MB>;
    constexpr int TILES = L::TILES, CH = L::CH, SLOT = L::SLOT, RING = L::RING, ZREG = L::ZREG, OSTR = L::OSTR;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* In = smem + ZREG;
    float* Out = In + RING * SLOT;

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;      // MFMA: operand row (tile) / column (channel) n, k entry g; results: channel n, tiles 4 g .. 4 g + 3 of the unit
    const int b = blockIdx.x / p.bands, band = blockIdx.x - b * p.bands;
    const int PH = p.H >> 2;                     // pooled rows
    const int i_first = band * p.steps_per_band, i_end = min(i_first + p.steps_per_band, PH);
    if (i_first >= i_end) return;
    const int i_begin = i_first > 0 ? i_first - 1 : i_first;   // a band that does not start at the top first recomputes the odd stem row above it (results not stored)

    // ---- filter fragments of this wave's 16 channels: [position][k-step], lane (n, g) holds U[position][channel 16 wave + n][kk = 4 ks + g]
    float wr[54];
    {
        const float* wp = p.w + (long long)wave * 54 * 64 + lane;
#pragma unroll
        for (int k = 0; k < 54; ++k) wr[k] = wp[k * 64];
    }
    const int ch = 16 * wave + n;
    const float sc = p.scale[ch], bi = p.bias[ch];

    for (int k = tid; k < ZREG; k += 256) smem[k] = 0.f;

    // ---- input rows: global (planar, W floats per row) -> registers -> transform -> LDS.  Item id = (r * 3 + c) * TILES + t of the four rows of a step; what
    // stays the same from step to step is computed once
    constexpr int ITEMS = 4 * 3 * TILES;
    constexpr int NIT = (ITEMS + 255) / 256;
    const float* xb = p.x + (long long)b * 3 * p.H * p.W;
    int it_r[NIT], it_src[NIT], it_dst[NIT];     // row of the item inside the step (4: no item); float offset of its pixel 4 t in row 0; float index of its position 0 in slot 0
    bool it_lf[NIT], it_rt[NIT];                 // the tile has pixels to its left / right inside the image
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int id = tid + 256 * u;
        const int r = id / (3 * TILES), rem = id - r * (3 * TILES);
        const int c = rem / TILES, t = rem - c * TILES;
        it_r[u] = id < ITEMS ? r : 4;
        it_src[u] = c * p.H * p.W + 4 * t;
        it_dst[u] = ZREG + c * CH + t;
        it_lf[u] = t > 0;
        it_rt[u] = t < TILES - 1;
    }
    auto load_rows = [&](StemW1dPiece (&regs)[NIT], int row0, int nrows) {      // rows row0 .. row0 + nrows - 1 (nrows <= 4); rows outside the image are zeros
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            const int row = row0 + it_r[u];
            StemW1dPiece v;
            v.a = f32x4{0.f, 0.f, 0.f, 0.f}; v.b = v.a; v.c = f32x2_w1d{0.f, 0.f};
            if (it_r[u] < nrows && (unsigned)row < (unsigned)p.H) {
                const float* src = xb + (it_src[u] + row * p.W);
                if (it_lf[u]) v.a = *reinterpret_cast<const f32x4*>(src - 4);
                v.b = *reinterpret_cast<const f32x4*>(src);
                if (it_rt[u]) v.c = *reinterpret_cast<const f32x2_w1d*>(src + 4);
            }
            regs[u] = v;
        }
    };
    auto store_rows = [&](const StemW1dPiece (&regs)[NIT], int row0, int nrows) {
        int s0 = row0 % RING; if (s0 < 0) s0 += RING;                            // (the same for the whole block)
#pragma unroll
        for (int u = 0; u < NIT; ++u) {
            if (it_r[u] < nrows) {
                int slot = s0 + it_r[u]; if (slot >= RING) slot -= RING;
                float* dst = smem + it_dst[u] + slot * SLOT;
                const float p0 = regs[u].a[1], p1 = regs[u].a[2], p2 = regs[u].a[3], p3 = regs[u].b[0], p4 = regs[u].b[1], p5 = regs[u].b[2], p6 = regs[u].b[3],
                            p7 = regs[u].c[0], p8 = regs[u].c[1];
                const float d62 = p6 - p2;
                dst[0 * TILES] = 2.f * (p0 - p4) + d62;
                dst[1 * TILES] = 2.f * p2 + (p4 - p6);
                dst[2 * TILES] = 3.f * p4 - (2.f * p2 + p6);
                dst[3 * TILES] = d62;
                dst[4 * TILES] = (p8 - p4) - 2.f * d62;
                dst[5 * TILES] = p1 - p5;
                dst[6 * TILES] = p3 + p5;
                dst[7 * TILES] = p5 - p3;
                dst[8 * TILES] = p7 - p3;
            }
        }
    };
    StemW1dPiece rg[NIT];
    // prologue: the 9 rows 4 i_begin - 3 .. 4 i_begin + 5
    for (int r0 = 4 * i_begin - 3; r0 < 4 * i_begin + 6; r0 += 4) {
        const int nr = min(4, 4 * i_begin + 6 - r0);
        load_rows(rg, r0, nr);
        store_rows(rg, r0, nr);
    }
    __syncthreads();

    // ---- this lane's k entries: k-step ks multiplies kk = 4 ks + g = 3 ky + c; entries 21 .. 23 (lanes 16 .. 63 of k-step 5) are padding and read zeros.  Entry 20's
    // row 4 i + 2 rs + 3 is odd and so is its slot: its lanes sit on banks 16 .. 31, the zeros of entry 21 go to banks 0 .. 15, those of 22 / 23 to 0 .. 15 / 16 .. 31
    int kof[6], sl[6];                           // float index of (channel c, position 0, tile n) in slot 0; float offset of the slot of row 4 i + ky - 3, kept from step to step
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
        const int kk = 4 * ks + g, ky = kk / 3;
        kof[ks] = ZREG + (kk - 3 * ky) * CH + n;
        int slot = (4 * i_begin + ky - 3) % RING; if (slot < 0) slot += RING;
        sl[ks] = slot * SLOT;
    }
    const bool padded = g > 0;
    const int zoff = (g == 3 ? 16 : 0) + n;
    f32x4 carry[MB];                             // horizontally pooled odd stem row of the step before: this lane's (4 pooled columns of unit mb, channel)
#pragma unroll
    for (int k = 0; k < MB; ++k) carry[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int left_lane = ((lane + 48) & 63) * 4;   // lane - 16 (mod 64): holds the four tiles to the left

    for (int i = i_begin; i < i_end; ++i) {
        const bool more = i + 1 < i_end;
        if (more) load_rows(rg, 4 * i + 6, 4);   // rows of the next step, in flight while this one is multiplied
        int rb[2][6];                            // float index of (stem row 2 i + rs, k-step, position 0, unit 0) for this lane
#pragma unroll
        for (int ks = 0; ks < 6; ++ks) {
            int s1 = sl[ks] + 2 * SLOT, s4 = sl[ks] + 4 * SLOT;
            if (s1 >= RING * SLOT) s1 -= RING * SLOT;
            if (s4 >= RING * SLOT) s4 -= RING * SLOT;
            rb[0][ks] = sl[ks] + kof[ks];
            rb[1][ks] = s1 + kof[ks];
            sl[ks] = s4;
        }
        if (padded) rb[0][5] = rb[1][5] = zoff;

        // 2 MB units (16 tiles of stem row 2 i + rs) x 6 k-steps; a stage = 9 operand reads + 9 MFMAs, the reads of the next stage are issued before this stage's MFMAs.
        // Positions that enter the outputs with the same coefficients share an accumulator: A = M0 + M5, B = M1 + M6, C = M2 + M7, D = M3, E = M4 + M8, so that
        // y[2t] = A + B + C + D and y[2t + 1] = B - C + 2 D + E
        float av[2][9];
        f32x4 acc[5], hp0;
        float prev[2] = {0.f, 0.f};              // y[2t + 1] of the tile left of the unit (left of the image: neutral)
#pragma unroll
        for (int q = 0; q < 9; ++q) av[0][q] = smem[rb[0][0] + q * TILES];
#pragma unroll
        for (int st = 0; st < 12 * MB; ++st) {
            const int ks = st % 6, rs = (st / 6) & 1, mb = st / 12;
            if (st + 1 < 12 * MB) {
                const int ks2 = (st + 1) % 6, rs2 = ((st + 1) / 6) & 1, mb2 = (st + 1) / 12;
#pragma unroll
                for (int q = 0; q < 9; ++q) av[(st + 1) & 1][q] = smem[rb[rs2][ks2] + q * TILES + 16 * mb2];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (ks == 0) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            const float* a = av[st & 1];
#pragma unroll
            for (int q = 0; q < 5; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], wr[q * 6 + ks], acc[q], 0, 0, 0);
#pragma unroll
            for (int q = 5; q < 9; ++q) acc[q == 8 ? 4 : q - 5] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q], wr[q * 6 + ks], acc[q == 8 ? 4 : q - 5], 0, 0, 0);
            if (ks < 5) continue;
            f32x4 y0 = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            f32x4 y1 = (acc[1] - acc[2]) + (2.f * acc[3] + acc[4]);
            // folded BatchNorm + ReLU, then the horizontal 3-window maximum of pooled column q = tile q: y[2q - 1], y[2q], y[2q + 1]
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y0[e] = fmaxf(fmaf(y0[e], sc, bi), 0.f);
                y1[e] = fmaxf(fmaf(y1[e], sc, bi), 0.f);
            }
            const float lft = __int_as_float(__builtin_amdgcn_ds_bpermute(left_lane, __float_as_int(y1[3])));
            const float l0 = g == 0 ? prev[rs] : lft;
            prev[rs] = lft;                      // (read by lanes 0 - 15 only: lane 48 + n's last tile of this unit)
            f32x4 hp;
            hp[0] = fmaxf(fmaxf(l0, y0[0]), y1[0]);
#pragma unroll
            for (int e = 1; e < 4; ++e) hp[e] = fmaxf(fmaxf(y1[e - 1], y0[e]), y1[e]);
            if (rs == 0) { hp0 = hp; continue; }
            // vertical maximum: odd stem row of the step before, even row, odd row
#pragma unroll
            for (int e = 0; e < 4; ++e) Out[(16 * mb + 4 * g + e) * OSTR + ch] = fmaxf(fmaxf(carry[mb][e], hp0[e]), hp[e]);
            carry[mb] = hp;
        }
        lds_barrier();                           // the pooled row is in Out; every wave is done reading this step's input rows (LDS hand-offs only: no wait for the stores below)

        if (more) store_rows(rg, 4 * i + 6, 4);
        if (i >= i_first) {
#pragma unroll
            for (int k = 0; k < MB; ++k) {       // TILES * 16 float4 pieces of the pooled row
                const int id = tid + 256 * k;
                *reinterpret_cast<f32x4*>(p.y + (((long long)b * PH + i) * TILES) * 64 + id * 4) = *reinterpret_cast<const f32x4*>(Out + (id >> 4) * OSTR + (id & 15) * 4);
            }
        }
        lds_barrier();                           // Out is free again, the new input rows are visible
    }
}

// w (64, 3, 7, 7) OIHW -> [channel block n / 16][position][k-step = kk / 4][lane = 16 (kk % 4) + n % 16], kk = 3 ky + c (21 .. 23: zeros); positions 0 - 4 = G4 w[n][c][ky][0::2],
// 5 - 8 = G3 w[n][c][ky][1::2] with the G4, G3 of the header.  Float64 arithmetic, rounded once.
__global__ void stem_pool_w1d_pack_kernel(const float* __restrict__ w, float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 4 * 54 * 64) return;
    const int lane = idx & 63, ks = (idx >> 6) % 6, pos = (idx / 384) % 9, nb = idx / (54 * 64);
    const int n = 16 * nb + (lane & 15), kk = 4 * ks + (lane >> 4);
    double v = 0.0;
    if (kk < 21) {
        const int ky = kk / 3, c = kk - 3 * ky;
        const float* r = w + ((n * 3 + c) * 7 + ky) * 7;
        const double g0 = r[0], g1 = r[2], g2 = r[4], g3 = r[6], f0 = r[1], f1 = r[3], f2 = r[5];
        switch (pos) {
            case 0: v = g0 / 2.0; break;
            case 1: v = (g0 + g1 + g2 + g3) / 2.0; break;
            case 2: v = (g0 - g1 + g2 - g3) / 6.0; break;
            case 3: v = (g0 + 2.0 * g1 + 4.0 * g2 + 8.0 * g3) / 6.0; break;
            case 4: v = g3; break;
            case 5: v = f0; break;
            case 6: v = (f0 + f1 + f2) / 2.0; break;
            case 7: v = (f0 - f1 + f2) / 2.0; break;
            default: v = f2; break;
        }
    }
    out[idx] = (float)v;
}

}  // namespace vatl

using namespace vatl;

extern "C" int64_t vatl_stem_pool_w1d_weight_floats(void) { return 4 * 54 * 64; }

extern "C" int vatl_pack_stem_pool_w1d_weight(const float* w_oihw, float* packed, void* stream) {
    if (!w_oihw || !packed) return fail(VATL_EINVAL, "pack_stem_pool_w1d_weight: null pointer");
    hipLaunchKernelGGL(stem_pool_w1d_pack_kernel, dim3(4 * 54 * 64 / 256), dim3(256), 0, (hipStream_t)stream, w_oihw, packed);
    return check_launch("stem_pool_w1d_pack");
}

// 1 when the 1-D Winograd stem serves this input size: rows of 16, 32 or 48 tiles of four pixels (W = 64, 128, 192), H a multiple of 4; else 0
extern "C" int vatl_stem_pool_w1d_supported(int H, int W) {
    return (H > 0 && (H & 3) == 0 && (W == 64 || W == 128 || W == 192)) ? 1 : 0;
}

template <int MB>
static int launch_stem_pool_w1d(const StemW1dParams& p, hipStream_t st) {
    auto kern = stem_pool_w1d_kernel<MB>;
    static std::atomic<unsigned> configured{0};
    constexpr int smem = StemW1dLds<MB>::FLOATS * (int)sizeof(float);
    static_assert(smem <= 80 * 1024, "two blocks per CU");
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, configured, "stem_pool_w1d")) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)(p.N * p.bands)), dim3(256), smem, st, p);
    // executed MFMA FLOPs: every step multiplies 2 stem rows x (W / 4) tiles x 9 positions x 64 channels x K = 24 (21 + 3 of padding), + one recomputed step per band below the first
    // (a band that starts past the last pooled row — PH = 33 in 8 bands of 5 — leaves at once and recomputes nothing)
    const int PH = p.H >> 2, nonempty = (PH + p.steps_per_band - 1) / p.steps_per_band;
    const double steps = (double)p.N * (PH + nonempty - 1);
    meter_add(0, 2.0 * steps * 2.0 * (p.W / 4) * 9.0 * 24.0 * 64.0);
    meter_route(kRouteStemPoolW1d);
    return check_launch("stem_pool_w1d");
}

extern "C" int vatl_stem7x7s2_pool_w1d_fwd(const float* x_nchw, const float* w_packed, const float* scale, const float* bias, float* y_nhwc, int N, int H, int W,
                                           void* stream) {
    if (N <= 0) return 0;
    if (!x_nchw || !w_packed || !scale || !bias || !y_nhwc) return fail(VATL_EINVAL, "stem7x7s2_pool_w1d_fwd: null pointer");
    if (!vatl_stem_pool_w1d_supported(H, W)) return fail(VATL_EINVAL, "stem7x7s2_pool_w1d_fwd: %dx%d input not served (W must be 64, 128 or 192, H %% 4 == 0)", H, W);
    if ((((uintptr_t)x_nchw) & 15) != 0 || (((uintptr_t)y_nhwc) & 15) != 0) return fail(VATL_EINVAL, "stem7x7s2_pool_w1d_fwd: input and output must be 16-byte aligned");
    StemW1dParams p{};
    p.x = x_nchw; p.w = w_packed; p.scale = scale; p.bias = bias; p.y = y_nhwc; p.N = N; p.H = H; p.W = W;
    // bands as in stem_pool.hip: one block per image once the images alone fill the 512 block slots; fewer images are cut into bands of pooled rows
    const int PH = H >> 2;
    int bands = 1;
    while ((long long)N * bands < 512 && bands * 2 <= PH / 4) bands *= 2;
    p.bands = bands; p.steps_per_band = (PH + bands - 1) / bands;
    hipStream_t st = (hipStream_t)stream;
    if (W == 64) return launch_stem_pool_w1d<1>(p, st);
    if (W == 128) return launch_stem_pool_w1d<2>(p, st);
    return launch_stem_pool_w1d<3>(p, st);
}
