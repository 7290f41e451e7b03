// What the two F(4x3, 2x2) kernels share (winograd_deconv43.hip: the transposed conv, one phase per block; winograd_s2_43.hip: the stride-2 conv,
// four phases summed in a block): a 4-row x 3-column output tile from a 5x4 input tile — F(4,2) vertically on the points (0, 1, -1, 2, inf),
// F(3,2) horizontally — on the stage of winograd_stage.h with five input rows.
//
//     B4^T = [2 -1 -2 1 0; 0 -2 -1 1 0; 0 2 -3 1 0; 0 -1 0 1 0; 0 2 -1 -2 1]      A4^T = [1 1 1 1 0; 0 1 -1 2 0; 0 1 1 4 0; 0 1 -1 8 1]
//     B3^T, A3^T: those of conv_winograd.hip (rows d0 - d2, d1 + d2, d2 - d1, d1 - d3;  [1 1 1 0; 0 1 -1 0; 0 1 1 1])
//
// Block: 32 tiles x 64 output channels, four waves, two blocks per CU.  Wave nu owns COLUMN position nu and all five row positions: 5 positions
// x 2 halves x 16 = 160 accumulator registers.
#pragma once
#include "common.h"
#include "winograd_stage.h"

namespace vatl {

using W43Stage = WinoStage<3, 5>;              // [5 rows][3 column arrays of 33 entries + one zero entry][16 channels] = 2000 sixteen-byte pieces, 32 LDS-DMA instructions, 32 KB
constexpr int W43_NLD = W43Stage::NLD;         // DMA instructions per wave and stage
constexpr int W43_LDS_BYTES = 2 * W43Stage::FLOATS * 4;
static_assert(W43Stage::NDMA % 4 == 0 && 16 * W_TB * 32 * 4 == W43_LDS_BYTES, "stage buffers = output-transform tiles");

// This wave's column combination is d[ja] + sgn * d[jb] (B3^T rows: d0 - d2, d1 + d2, d2 - d1, d1 - d3)
__device__ __forceinline__ int w43_col_a(int nu) { return nu == 0 ? 0 : (nu == 2 ? 2 : 1); }
__device__ __forceinline__ int w43_col_b(int nu) { return nu == 0 ? 2 : (nu == 1 ? 2 : (nu == 2 ? 1 : 3)); }

// V = B4^T d B3 of the lane's tile: this wave's NP row positions, four channels (NP = 4: rows 0 .. 3 of B4^T read input rows 0 .. 3 only).
// Rb: the stage; ca / cb: wino_frag_col of the wave's two columns; x8: 0 / 8, the 8-channel step.
template <int NP>
__device__ __forceinline__ void w43_make_v(f32x4 (&v)[5], const float* Rb, int ca, int cb, float sgn, int x8) {
    f32x4 tc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const f32x4 da = *reinterpret_cast<const f32x4*>(Rb + i * W43Stage::ROWF + (ca ^ x8));
        const f32x4 db = *reinterpret_cast<const f32x4*>(Rb + i * W43Stage::ROWF + (cb ^ x8));
        tc[i] = da + sgn * db;
    }
    const f32x4 s = tc[3] - tc[1];
    v[0] = 2.f * (tc[0] - tc[2]) + s;                  // 2 t0 -   t1 - 2 t2 +   t3
    v[1] = s - (tc[1] + tc[2]);                        //      - 2 t1 -   t2 +   t3
    v[2] = 2.f * tc[1] + (tc[3] - 3.f * tc[2]);        //        2 t1 - 3 t2 +   t3
    v[3] = s;                                          //      -   t1        +   t3
    if constexpr (NP == 5) v[4] = (tc[4] - tc[2]) - 2.f * s;      //        2 t1 -   t2 - 2 t3 + t4
}

// One group of 4 NP MFMAs 32x32x2: the four channels of v against one 32-channel half of the filter fragments
template <int NP>
__device__ __forceinline__ void w43_mfma_group(f32x16 (&ac)[5], const f32x4 (&v)[5], const f32x4 (&uu)[5]) {
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int xi = 0; xi < NP; ++xi)
            ac[xi] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[xi][tt], uu[xi][tt], ac[xi], 0, 0, 0);
}

// Host: tensors within the 32-bit byte offsets of the buffer descriptors (the bounds of conv_winograd.hip's host check).  mt: tiles, xe / ye / ue:
// elements of input, output and packed filter, units: blocks per 32-tile group.  The counts are products of up to five ints, formed by the callers
// in 128 bits: in 64 they overflow for shapes far outside the range (found by the sanitizer run of tools/probes/wino43_range_check.hip).
typedef __int128 w43_count;
static inline bool w43_in_range(w43_count mt, w43_count xe, w43_count ye, w43_count ue, int Cin, int units) {
    return xe <= (w43_count)(WOOB_G / 4) && ye < ((w43_count)1 << 30) && ue < ((w43_count)1 << 28) && mt < ((w43_count)1 << 30) && Cin / W_CK < 1024 &&
           (mt + W_TB - 1) / W_TB * units < ((w43_count)1 << 31);
}

}  // namespace vatl
