// Float64 REFERENCE weight gradient (alphapose/models/hip_train_f64.py) on v_mfma_f64_16x16x4_f64:
//     dW[co][r][s][ci] = sum over output pixels p = (n, oy, ox) of dz[p][co] * x[n][oy*stride - pad + r][ox*stride - pad + s][ci]
// as ONE GEMM per layer with rows = Cout, columns = (r, s, ci) over R*S*Cin and the reduction over the M = N*Ho*Wo pixels.  It stands
// beside conv_f64.hip and is a yardstick, not a timed route: it feeds no FLOP meter, has no tuning knob and reads no environment variable.
//   * x and dz are float64 NHWC with ANY channel count (3, 17, 64 .. 2048): nothing is padded in memory;
//   * pixels outside the image (padding taps), pixels past the end of a chunk and rows / columns past the end of a tile are exact
//     zeros in the staged tiles.  Tiles are padded, never masked: every MFMA runs with all lanes active;
//   * the reduction has ONE fixed order and no atomics: M is cut into chunks of VATL_WGRAD_F64_CHUNK pixels (a header constant: the
//     number of splits is a function of M only), a block walks its chunk sixteen pixels at a time in ascending order and writes one
//     float64 partial slab per split into the caller's workspace [split][row][R][S][col]; vatl_wgrad_f64_reduce adds the slabs in
//     ascending split order and writes the parameter's own layout (OIHW).  Bits do not depend on grid size, occupancy or stream;
//   * a transposed conv (ConvTranspose2d(4,2,1), weight (Cin,Cout,4,4)) is the same sum with the operands' roles exchanged, as in
//     wgrad_h16.hip: its forward input is the "dz side" (rows = its Cin) and its output gradient the "x side" of a 4x4 / stride 2 /
//     pad 1 conv; the row-major [row][col][ky][kx] result is then the IOHW layout of the ConvTranspose2d parameter.
// Block = 256 threads = 2 x 2 waves on a 64-row x 64-column tile, a wave owns 32 x 32 (2 x 2 MFMA tiles).  Both operands are
// pixel-major in memory and are staged pixel-major: a wave moves 64 consecutive channels of one pixel into one row of a
// [16 pixels][64 channels] LDS image, the next sixteen pixels' loads in flight while the current image is multiplied.  MFMA operands
// (one f64 per lane, as conv_f64.hip): A[row lane&15][k lane>>4], B[k lane>>4][col lane&15]; result col lane&15, row (lane>>4) + 4*reg.
// A lane group of sixteen therefore reads sixteen consecutive channels of one staged pixel: no transposing read.
// LDS banks: a row of the image is kWg64Ld = 80 doubles = 160 dwords.  ds_read_b64 is served per 32-lane half over 64 banks: a half
// reads pixel rows k and k + 1, sixteen consecutive doubles (32 banks) of each, and 160 = 32 (mod 64) puts the second row on the other
// 32 banks — conflict-free.  ds_write_b64 is served per sixteen lanes over 32 banks: sixteen consecutive doubles, conflict-free.
#include "wgrad_generic.h"

namespace vatl {

typedef double wg64_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kWg64Tile = 64;                    // rows and columns of a block's tile
constexpr int kWg64K = 16;                       // pixels per staged image
constexpr int kWg64Ld = kWg64Tile + 16;          // LDS row pitch in doubles (see the bank argument above)

__global__ __launch_bounds__(256) void wgrad_f64_kernel(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ ws, WgradGeom g) {
    __shared__ double As[kWg64K][kWg64Ld];
    __shared__ double Bs[kWg64K][kWg64Ld];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int col0 = blockIdx.x * kWg64Tile, row0 = blockIdx.y * kWg64Tile;
    const long long m_begin = (long long)blockIdx.z * g.chunk;
    const long long m_end = m_begin + g.chunk < g.M ? m_begin + g.chunk : g.M;

    // staging: thread -> row / column `lane` of the tile, pixels wave + 4 i of the image
    const int arow = row0 + lane;
    const bool a_in = arow < g.Ca;
    const int n = col0 + lane;                                // this thread's column: one tap, one channel
    const bool b_in = n < g.ncol;
    const int tap = b_in ? n / g.Cb : 0, bc = b_in ? n - tap * g.Cb : 0;
    const int tr = tap / g.S, ts = tap - tr * g.S;
    const int hw = g.Ho * g.Wo;

    double ra[4], rb[4];
    auto fetch = [&](long long m0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long m = m0 + wave + 4 * i;
            ra[i] = 0.0;
            rb[i] = 0.0;
            if (m < m_end) {
                if (a_in) ra[i] = a[m * g.Ca + arow];
                if (b_in) {
                    const long long img = m / hw;
                    const int rem = (int)(m - img * hw);
                    const int oy = rem / g.Wo, ox = rem - oy * g.Wo;
                    const int iy = oy * g.stride - g.pad + tr, ix = ox * g.stride - g.pad + ts;
                    if ((unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W) rb[i] = b[((img * g.H + iy) * g.W + ix) * g.Cb + bc];
                }
            }
        }
    };

    wg64_f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (wg64_f64x4){0.0, 0.0, 0.0, 0.0};

    const int l16 = lane & 15, lg = lane >> 4;
    fetch(m_begin);
    for (long long m0 = m_begin; m0 < m_end; m0 += kWg64K) {          // uniform over the block
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            As[wave + 4 * i][lane] = ra[i];
            Bs[wave + 4 * i][lane] = rb[i];
        }
        __syncthreads();
        if (m0 + kWg64K < m_end) fetch(m0 + kWg64K);
#pragma unroll
        for (int kk = 0; kk < kWg64K; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = As[kk + lg][wr * 32 + i * 16 + l16];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = Bs[kk + lg][wc * 32 + j * 16 + l16];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // partial slab of this split: ws[split][row][col], sixteen lanes on sixteen consecutive columns
    double* out = ws + (long long)blockIdx.z * g.Ca * g.ncol;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = col0 + 32 * wc + 16 * j + l16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = row0 + 32 * wr + 16 * i + lg + 4 * e;
                if (row < g.Ca && col < g.ncol) out[(long long)row * g.ncol + col] = acc[i][j][e];
            }
        }
}

}  // namespace vatl

using namespace vatl;

extern "C" int64_t vatl_wgrad_f64_splits(int64_t M) { return wgrad_splits(M, VATL_WGRAD_F64_CHUNK); }

extern "C" int64_t vatl_conv2d_wgrad_f64_workspace_doubles(int Cout, int Cin, int R, int S, int64_t M) {
    return wgrad_splits(M, VATL_WGRAD_F64_CHUNK) * (int64_t)Cout * R * S * Cin;
}

extern "C" int vatl_conv2d_wgrad_f64(const double* x, const double* dz, double* workspace, int64_t workspace_doubles, int N, int H, int W, int Cin, int Cout,
                                     int R, int S, int stride, int pad, int transposed, void* stream) {
    const char* what = "conv2d_wgrad_f64";
    if (!x || !dz) return fail(VATL_EINVAL, "%s: null pointer", what);
    if (!workspace) return fail(VATL_EINVAL, "%s: null workspace", what);
    if (Cin < 1 || Cout < 1) return fail(VATL_EINVAL, "%s: %d -> %d channels", what, Cin, Cout);
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dz) | reinterpret_cast<uintptr_t>(workspace)) & 7u)
        return fail(VATL_EINVAL, "%s: float64 tensors must be 8-byte aligned", what);
    WgradGeom g;
    if (const int rc = wgrad_geom(what, VATL_WGRAD_F64_CHUNK, N, H, W, Cin, Cout, R, S, stride, pad, transposed, &g)) return rc;
    if (cdiv(g.Ca, kWg64Tile) > 65535) return fail(VATL_EINVAL, "%s: tensor too large", what);
    if (const int rc = wgrad_workspace_contract(what, "doubles", workspace_doubles, g)) return rc;
    hipLaunchKernelGGL(wgrad_f64_kernel, wgrad_grid(g, kWg64Tile), dim3(256), 0, (hipStream_t)stream, transposed ? x : dz, transposed ? dz : x, workspace, g);
    return check_launch(what);
}

extern "C" int vatl_wgrad_f64_reduce(const double* workspace, double* dw, int64_t M, int Cout, int Cin, int R, int S, int transposed, void* stream) {
    return wgrad_reduce("wgrad_f64_reduce", workspace, dw, M, VATL_WGRAD_F64_CHUNK, Cout, Cin, R, S, transposed, 1, stream);
}
