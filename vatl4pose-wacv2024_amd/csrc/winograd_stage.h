// The column-array LDS stage of the 32-tile Winograd inference kernels (conv_winograd.hip, winograd_deconv43.hip, winograd_s2_43.hip): its
// layout, which pixel each 16-byte piece of it holds, and where a lane reads a column of its tile.
//
// Staging is by LDS-DMA (buffer_load ... lds: no staging registers, no ds_write pass).  The destination of a wave instruction is
// lane-linear (base + lane * 16 bytes), so the chunk swizzle is applied on the SOURCE side: LDS position p = (entry p >> 2, chunk
// position p & 3) receives the entry's global chunk (p & 3) ^ ((q >> 2) & 3).
// Column arrays: pixel column j of tile t (x = MO tx + j - pad) lives in array r = j % MO at entry q = t + j / MO — the tile index
// is FLAT, so consecutive tiles are consecutive 64-byte entries even across tile-row ends and the 16 lanes of a ds_read_b128 group
// ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}) hit 16 different 16-byte bank slots (with one slot per distinct pixel column —
// stride MO between tiles and a gap at row ends — every fragment read was a 3-way bank conflict: SQ_LDS_BANK_CONFLICT 65 % of the
// LDS cycles).  At a row end entry (r, q) is asked for by two tiles: column r of tile q (first of its row: x = r - pad) and
// column MO + r of tile q - 1 (last of its row: x = MO TW + r - pad) — never both inside the image; the entry holds whichever is,
// and a tile whose column is outside the image reads the row's zero entry instead.  A piece outside the image must be REQUESTED out of
// range (WOOB_G: the DMA writes zeros): its in-range neighbour address would be a pixel of the next row or image, which the
// descriptor's range check does not catch.
#pragma once
#include "common.h"

namespace vatl {

constexpr unsigned WOOB_G = 0xFFFF0000u;        // staging offset of a zero piece: still out of range with stage * 64 bytes added (stages < 1024, tensors <= 0xFFFF0000 bytes: checked on the host), so the per-stage offset needs no select
constexpr int W_TB = 32;                        // tiles per block
constexpr int W_CK = 16;                        // channels per LDS stage
constexpr int W_NQ = W_TB + 1;                  // entries of a column array: one per tile + the halo of the last tile

// LDS stage: [ROWS input rows i][MO column arrays r][33 entries q][16 channels]; entry (r, q) = column r of tile q (= column MO + r of tile q - 1).
// MO is the tile's column step; ROWS the rows of its input tile.
template <int MO, int ROWS = 4> struct WinoStage {
    static constexpr int ROWE = MO * W_NQ + 1;             // entries per input row: MO column arrays of W_NQ + ONE ZERO ENTRY (its four pieces are requested out of range by
                                                           // every stage): the column of a tile that lies outside the image reads it — at the same index in every row, so the
                                                           // fragment reads need no per-lane select (2 per column and step before; vector instructions are not hidden behind the MFMAs)
    static constexpr int ROWF = ROWE * W_CK;               // floats per input row
    static constexpr int ITEMS = ROWS * ROWE * 4;          // 16-byte pieces
    static constexpr int NDMA = (ITEMS + 63) / 64;         // wave-wide LDS-DMA instructions (1 KB each; the last one is partly used)
    static constexpr int FLOATS = NDMA * 256;
    static constexpr int NLD = (NDMA + 3) / 4;             // per wave
};

// Staging offset (bytes into the NHWC input, first stage) of piece pz (0 .. NLD * 256 - 1) of the stage of the block whose first tile is m0, or
// WOOB_G where the piece has no pixel behind it.
//   RSTEP          tile step along the rows: tile (ty, tx) covers grid rows RSTEP ty - pad_y + i, columns MO tx - pad_x + j
//   VIEW2          the GH x GW grid the tiles cover is the image itself (false), or the stride-2 phase view of a 2 GH x 2 GW image whose
//                  pixel (yy, xx) is image pixel (2 yy + pad_y, 2 xx + pad_x) (true)
//   mlim           tiles in the launch (of the period, for the persistent walk); tiles are numbered flat over (image, tile row, tile column)
//   p              a parameter struct with Cin, TH, TW and the divisors d_TH, d_TW
template <class ST, int MO, int RSTEP, bool VIEW2, class P>
__device__ __forceinline__ unsigned wino_piece_offset(const P& p, int pz, int m0, int mlim, int pad_y, int pad_x, int GH, int GW) {
    if (pz >= ST::ITEMS) return WOOB_G;
    const int cpos = pz & 3, e = pz >> 2;
    const int i = e / ST::ROWE, re = e - i * ST::ROWE;
    const int r = re / W_NQ, q = re - r * W_NQ;
    if (r >= MO) return WOOB_G;                            // the row's zero entry
    const int chunk = cpos ^ ((q >> 2) & 3);
    int m = m0 + q;                                        // column r of tile m ...
    int gr = fdiv(m, p.d_TW), tx = m - gr * p.TW;
    int xx = MO * tx + r - pad_x;
    if (m >= mlim || (tx == 0 && xx < 0)) {                // ... or, when that is outside, column MO + r of the tile before (a row end / the halo)
        m -= 1;
        if (m < 0) return WOOB_G;
        gr = fdiv(m, p.d_TW); tx = m - gr * p.TW;
        xx = MO * tx + MO + r - pad_x;
    }
    const int b = fdiv(gr, p.d_TH), ty = gr - b * p.TH;
    const int yy = RSTEP * ty - pad_y + i;
    if (m < mlim && (unsigned)yy < (unsigned)GH && (unsigned)xx < (unsigned)GW) {
        if (VIEW2) return (unsigned)(((b * 2 * GH + 2 * yy + pad_y) * 2 * GW + 2 * xx + pad_x) * p.Cin + chunk * 4) << 2;
        return (unsigned)(((b * GH + yy) * GW + xx) * p.Cin + chunk * 4) << 2;
    }
    return WOOB_G;
}

// Fragment column index, which must agree with wino_piece_offset: float index (relative to a stage's input row, first 8-channel step) of column j
// of the lane's tile — lane = (tile tl, channel quad h), tx = the tile's column in its tile row; the second step of a stage is the same
// index ^ 8; a column outside the grid = the row's zero entry.
template <int MO>
__device__ __forceinline__ int wino_frag_col(int j, int tl, int h, int tx, int pad_x, int GW) {
    const int xx = MO * tx + j - pad_x;
    const int q = tl + j / MO;
    return (unsigned)xx < (unsigned)GW ? ((j % MO) * W_NQ + q) * W_CK + ((h ^ ((q >> 2) & 3)) << 2) : MO * W_NQ * W_CK + (h << 2);
}

}  // namespace vatl
