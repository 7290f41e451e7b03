// What the two generic weight-gradient GEMMs (wgrad_f64.hip: the float64 reference, wgrad_h16.hip: the bf16 step) share around their
// MFMA kernels, ONE copy of each: the launch geometry both kernels take by value, its builder with the `transposed` role exchange and
// the shape contract, the split count, the workspace contract and the kernel that adds the per-split slabs in ascending split order.
#pragma once
#include "common.h"

namespace vatl {

struct WgradGeom {
    long long M;                                 // pixels of the dz side
    int chunk;                                   // pixels per split
    int Ho, Wo, Ca;                              // dz side: plane and stored channels (rows of the GEMM)
    int H, W, Cb;                                // x side: plane and stored channels
    int R, S, stride, pad, ncol;                 // ncol = R*S*Cb
};

// the number of splits is a function of M and the kernel's chunk (a header constant) only
static inline long long wgrad_splits(long long M, int chunk) { return M <= 0 ? 0 : (M + chunk - 1) / chunk; }

// Geometry of vatl_conv2d_wgrad_{f64,h16} from the entry point's arguments (Cin, Cout: the channels as stored).  A transposed conv
// (ConvTranspose2d(4,2,1)) exchanges the roles: its forward input x is the dz side of a 4x4 / 2 / pad 1 conv of its output gradient, so
// the caller passes (a, b) = (x, dz) there and (dz, x) otherwise.
inline int wgrad_geom(const char* what, int chunk, int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int transposed, WgradGeom* out) {
    if (N < 1 || H < 1 || W < 1 || R < 1 || S < 1 || R > 7 || S > 7 || (stride != 1 && stride != 2) || pad < 0)
        return fail(VATL_EINVAL, "%s: N %d, %dx%d, %dx%d / %d, pad %d is not served (R, S <= 7, stride 1 or 2)", what, N, H, W, R, S, stride, pad);
    WgradGeom g{};
    if (transposed) {
        if (R != 4 || S != 4 || stride != 2 || pad != 1) return fail(VATL_EINVAL, "%s: the transposed form serves ConvTranspose2d(4, 2, 1) only", what);
        g.Ho = H; g.Wo = W; g.Ca = Cin; g.H = 2 * H; g.W = 2 * W; g.Cb = Cout;
    } else {
        if (H + 2 * pad < R || W + 2 * pad < S) return fail(VATL_EINVAL, "%s: a %dx%d filter does not fit a %dx%d plane with pad %d", what, R, S, H, W, pad);
        g.Ho = (H + 2 * pad - R) / stride + 1; g.Wo = (W + 2 * pad - S) / stride + 1; g.Ca = Cout; g.H = H; g.W = W; g.Cb = Cin;
    }
    g.M = (long long)N * g.Ho * g.Wo;
    g.chunk = chunk;
    g.R = R; g.S = S; g.stride = stride; g.pad = pad; g.ncol = R * S * g.Cb;
    if (g.M >= (1LL << 31) || (long long)N * g.H * g.W * g.Cb >= (1LL << 40) || g.M * g.Ca >= (1LL << 40) || wgrad_splits(g.M, chunk) > 65535)
        return fail(VATL_EINVAL, "%s: tensor too large", what);
    *out = g;
    return 0;
}

// the workspace [split][Ca][R][S][Cb] the caller brought, `unit` its element's word ("doubles", "floats")
inline int wgrad_workspace_contract(const char* what, const char* unit, long long have, const WgradGeom& g) {
    const long long need = wgrad_splits(g.M, g.chunk) * g.Ca * g.ncol;
    if (have < need) return fail(VATL_EINVAL, "%s: the workspace holds %lld %s, %lld are needed", what, have, unit, need);
    return 0;
}

// blocks of tile x tile outputs, one grid plane per split
inline dim3 wgrad_grid(const WgradGeom& g, int tile) { return dim3((unsigned)cdiv(g.ncol, tile), (unsigned)cdiv(g.Ca, tile), (unsigned)wgrad_splits(g.M, g.chunk)); }

// dw[row][c][r][s] = sum over splits, ascending, of ws[split][row][r][s][c] for row < rows, c < cols of slabs stored with rows_stored x
// cols_stored channels (the 16-bit route pads both to 8; float64 stores them as they are): thread per output element, in the workspace's
// order (c fastest): the reads — `splits` times the bytes of the writes — are the coalesced side
template <typename T>
__global__ void wgrad_reduce_kernel(const T* __restrict__ ws, T* __restrict__ dw, int splits, int rows, int cols, int rows_stored, int cols_stored, int RS) {
    const long long total = (long long)rows * cols * RS, slab = (long long)rows_stored * RS * cols_stored;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cols);
        const long long t = i / cols;
        const int tap = (int)(t % RS);
        const long long row = t / RS;
        const T* src = ws + (row * RS + tap) * cols_stored + c;
        T s = 0;
        for (int k = 0; k < splits; ++k) s += src[k * slab];
        dw[(row * cols + c) * RS + tap] = s;
    }
}

// vatl_wgrad_{f64,h16}_reduce: the slabs of `chunk`-pixel splits -> the parameter's own layout; `align`: what the stored channels are padded to
template <typename T>
inline int wgrad_reduce(const char* what, const T* workspace, T* dw, long long M, int chunk, int Cout, int Cin, int R, int S, int transposed, int align, void* stream) {
    if (!workspace || !dw || M < 1 || Cout < 1 || Cin < 1 || R < 1 || S < 1) return fail(VATL_EINVAL, "%s: bad arguments", what);
    const int rows = transposed ? Cin : Cout, cols = transposed ? Cout : Cin;
    const long long total = (long long)rows * cols * R * S;
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(wgrad_reduce_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, workspace, dw, (int)wgrad_splits(M, chunk), rows, cols,
                       (rows + align - 1) / align * align, (cols + align - 1) / align * align, R * S);
    return check_launch(what);
}

}  // namespace vatl
