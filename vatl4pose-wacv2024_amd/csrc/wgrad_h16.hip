// Weight gradient of the opt-in bf16 fine-tune step (alphapose/models/hip_train_h16.py) on v_mfma_f32_16x16x32_{f16,bf16}:
//     dW[co][r][s][ci] = sum over output pixels p = (n, oy, ox) of dz[p][co] * x[n][oy*stride - pad + r][ox*stride - pad + s][ci]
// as ONE GEMM per layer with rows = Cout8 (the channels dz is stored with), columns = (r, s, ci) over R*S*Cin8 and the reduction over
// the M = N*Ho*Wo pixels — the STRIDED dimension of both NHWC operands.  It stands beside conv_h16.hip: it feeds no FLOP meter, has no
// tuning knob and reads no environment variable.
// Arithmetic contract:
//   * x and dz are a 16-bit storage type T in {float16, bfloat16}, NHWC, channels in multiples of 8; a product of two T values is exact
//     in fp32 and every product is accumulated in fp32 by the MFMA;
//   * pixels outside the image (padding taps), pixels past the end of a chunk and the channels past the end of a tile are exact zeros;
//   * the reduction has ONE fixed order and no atomics: M is cut into chunks of VATL_WGRAD_H16_CHUNK pixels (a header constant: the
//     boundaries depend on the layer's geometry only), a block walks its chunk 64 pixels at a time in ascending order and writes one fp32
//     partial per split into the caller's workspace [split][Cout8][R][S][Cin8]; vatl_wgrad_h16_reduce adds the partials in ascending split
//     order in fp32 and writes the parameter's own layout (OIHW), dropping the padded channels.  A gradient is bit-reproducible run to run.
//   * A transposed conv (ConvTranspose2d(4,2,1), weight (Cin,Cout,4,4)) is the same sum with the operands' roles exchanged: its forward
//     input is the "dz side" (rows = its Cin) and its output gradient the "x side" of a 4x4 / stride 2 / pad 1 conv; the row-major
//     [row][col][ky][kx] result is then the IOHW layout of the ConvTranspose2d parameter.
// Block = 256 threads = 2 x 2 waves on a 64-row x 64-column tile, a wave owns 32 x 32 (2 x 2 MFMA tiles).  Both operands are staged
// PIXEL-major, as they lie in memory: a thread moves 16 bytes = eight channels of one pixel (coalesced NHWC loads) into a
// [64 pixels][64 channels] LDS image, the next 64 pixels' loads in flight while the current image is multiplied.  The MFMA wants eight
// consecutive k (pixels) of one channel per lane: two ds_read_b64_tr_b16 per fragment deliver them (lane 4q+p of a 16-lane group gives the
// address of pixel row q, channels 4p..4p+3, and receives channel `lane & 15` of the four rows).  The instruction needs EXEC all ones and
// 8-byte aligned addresses: the images are always full (zeros where there is no data) and no lane leaves before the last read.
// LDS banks (64 banks of 4 bytes for this read, conflicts counted per 32-lane half): an image row is 128 bytes = 32 banks; a half reads
// the eight pixel rows {0..3, 8..11} + 4h of one 16-channel column tile, 32 bytes of each.  Unswizzled, rows of equal parity would fall
// on the same 8 banks (4-way conflict).  The 16-byte chunk `ch` of pixel row `r` is therefore stored at chunk ch ^ 2*f(r),
// f(r) = ((r >> 1) & 1) | (((r >> 3) & 1) << 1): the four rows of equal parity in a half take four different 32-byte column slots, the two
// parities the two halves of the 64 banks — conflict-free by construction.
// Operand lane maps (as conv_h16.hip): A[row lane&15][k 8(lane>>4)+j], B[k 8(lane>>4)+j][col lane&15]; result col lane&15, row 4(lane>>4)+reg.
#include "h16.h"
#include "wgrad_generic.h"

namespace vatl {

constexpr int kWgTile = 64;                      // rows and columns of a block's tile, and pixels per staged image
typedef short wg_s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int wg_swz(int row, int ch) { return ch ^ ((((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1); }

// eight consecutive k (pixel rows k0 + 8*lg .. +7 of the image) of channel 16*t + (lane & 15): the MFMA operand of column tile t
__device__ __forceinline__ h16_u32x4 wg_frag(const unsigned short* img, int k0, int t, int lane) {
    const int lg = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    unsigned w[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int row = k0 + 8 * lg + 4 * h + q;
        const unsigned short* a = img + row * kWgTile + wg_swz(row, 2 * t + (p >> 1)) * 8 + 4 * (p & 1);
        const wg_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) wg_s16x4*)a);
        w[2 * h] = (unsigned)(unsigned short)v[0] | ((unsigned)(unsigned short)v[1] << 16);
        w[2 * h + 1] = (unsigned)(unsigned short)v[2] | ((unsigned)(unsigned short)v[3] << 16);
    }
    return (h16_u32x4){w[0], w[1], w[2], w[3]};
}

template <typename T>
__global__ __launch_bounds__(256) void wgrad_h16_kernel(const unsigned short* __restrict__ a, const unsigned short* __restrict__ b, float* __restrict__ ws,
                                                        WgradGeom g) {
    __shared__ __attribute__((aligned(16))) unsigned short As[kWgTile * kWgTile];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[kWgTile * kWgTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int col0 = blockIdx.x * kWgTile, row0 = blockIdx.y * kWgTile;
    const long long m_begin = (long long)blockIdx.z * g.chunk;
    const long long m_end = m_begin + g.chunk < g.M ? m_begin + g.chunk : g.M;

    // staging: thread -> 16-byte chunk tid & 7 (eight channels) of pixel rows (tid >> 3) and (tid >> 3) + 32 of both images
    const int ch = tid & 7, pr = tid >> 3;
    const int arow = row0 + 8 * ch;                           // first of this thread's eight dz channels
    const bool a_in = arow < g.Ca;
    const int n = col0 + 8 * ch;                              // first of this thread's eight columns: one tap, eight channels
    const bool b_in = n < g.ncol;
    const int tap = b_in ? n / g.Cb : 0, bc = b_in ? n - tap * g.Cb : 0;
    const int tr = tap / g.S, ts = tap - tr * g.S;
    const int hw = g.Ho * g.Wo;

    const h16_u32x4 zero = {0u, 0u, 0u, 0u};
    h16_u32x4 ra[2], rb[2];
    auto fetch = [&](long long m0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const long long m = m0 + pr + 32 * i;
            ra[i] = zero;
            rb[i] = zero;
            if (m < m_end) {
                if (a_in) ra[i] = *reinterpret_cast<const h16_u32x4*>(a + m * g.Ca + arow);
                if (b_in) {
                    const long long img = m / hw;
                    const int rem = (int)(m - img * hw);
                    const int oy = rem / g.Wo, ox = rem - oy * g.Wo;
                    const int iy = oy * g.stride - g.pad + tr, ix = ox * g.stride - g.pad + ts;
                    if ((unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W)
                        rb[i] = *reinterpret_cast<const h16_u32x4*>(b + ((img * g.H + iy) * g.W + ix) * g.Cb + bc);
                }
            }
        }
    };

    h16_f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (h16_f32x4){0.f, 0.f, 0.f, 0.f};

    fetch(m_begin);
    for (long long m0 = m_begin; m0 < m_end; m0 += kWgTile) {         // uniform over the block: no lane leaves before the transposed reads
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = pr + 32 * i;
            *reinterpret_cast<h16_u32x4*>(&As[row * kWgTile + wg_swz(row, ch) * 8]) = ra[i];
            *reinterpret_cast<h16_u32x4*>(&Bs[row * kWgTile + wg_swz(row, ch) * 8]) = rb[i];
        }
        __syncthreads();
        if (m0 + kWgTile < m_end) fetch(m0 + kWgTile);
#pragma unroll
        for (int ks = 0; ks < kWgTile / 32; ++ks) {
            h16_u32x4 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = wg_frag(As, 32 * ks, 2 * wr + i, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = wg_frag(Bs, 32 * ks, 2 * wc + j, lane);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = T::mfma(af[i], bf[j], acc[i][j]);
        }
        __syncthreads();
    }

    // partial of this split: ws[split][row][col], sixteen lanes on sixteen consecutive columns
    float* out = ws + (long long)blockIdx.z * g.Ca * g.ncol;
    const int l16 = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = col0 + 32 * wc + 16 * j + l16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = row0 + 32 * wr + 16 * i + 4 * lg + e;
                if (row < g.Ca && col < g.ncol) out[(long long)row * g.ncol + col] = acc[i][j][e];
            }
        }
}

}  // namespace vatl

using namespace vatl;

extern "C" int64_t vatl_wgrad_h16_splits(int64_t M) { return wgrad_splits(M, VATL_WGRAD_H16_CHUNK); }

extern "C" int64_t vatl_conv2d_wgrad_h16_workspace_floats(int Cout8, int Cin8, int R, int S, int64_t M) {
    return wgrad_splits(M, VATL_WGRAD_H16_CHUNK) * (int64_t)Cout8 * R * S * Cin8;
}

extern "C" int vatl_conv2d_wgrad_h16(const void* x, const void* dz, float* workspace, int64_t workspace_floats, int N, int H, int W, int Cin8, int Cout8, int R,
                                     int S, int stride, int pad, int transposed, int dtype, void* stream) {
    const char* what = "conv2d_wgrad_h16";
    if (!x || !dz) return fail(VATL_EINVAL, "%s: null pointer", what);
    if (!workspace) return fail(VATL_EINVAL, "%s: null workspace", what);
    if (!h16_dtype_ok(dtype)) return fail(VATL_EINVAL, "%s: dtype %d is neither float16 (0) nor bfloat16 (1)", what, dtype);
    if (Cin8 < 8 || (Cin8 & 7)) return fail(VATL_EINVAL, "%s: Cin %d is not a multiple of 8 (pad the input with zero channels)", what, Cin8);
    if (Cout8 < 8 || (Cout8 & 7)) return fail(VATL_EINVAL, "%s: Cout %d is not a multiple of 8 (pad the output gradient with zero channels)", what, Cout8);
    if (!h16_aligned16(x) || !h16_aligned16(dz) || (reinterpret_cast<uintptr_t>(workspace) & 3u)) return fail(VATL_EINVAL, "%s: 16-bit tensors must be 16-byte aligned", what);
    WgradGeom g;
    if (const int rc = wgrad_geom(what, VATL_WGRAD_H16_CHUNK, N, H, W, Cin8, Cout8, R, S, stride, pad, transposed, &g)) return rc;
    if (const int rc = wgrad_workspace_contract(what, "floats", workspace_floats, g)) return rc;
    const dim3 grid = wgrad_grid(g, kWgTile);
    const unsigned short *as = (const unsigned short*)(transposed ? x : dz), *bs = (const unsigned short*)(transposed ? dz : x);
    if (dtype == kH16F16) hipLaunchKernelGGL(wgrad_h16_kernel<F16>, grid, dim3(256), 0, (hipStream_t)stream, as, bs, workspace, g);
    else hipLaunchKernelGGL(wgrad_h16_kernel<BF16>, grid, dim3(256), 0, (hipStream_t)stream, as, bs, workspace, g);
    return check_launch(what);
}

extern "C" int vatl_wgrad_h16_reduce(const float* workspace, float* dw, int64_t M, int Cout, int Cin, int R, int S, int transposed, void* stream) {
    return wgrad_reduce("wgrad_h16_reduce", workspace, dw, M, VATL_WGRAD_H16_CHUNK, Cout, Cin, R, S, transposed, 8, stream);
}
