// Every 16-bit filter re-pack of one bf16 training step in ONE launch (vatl_pack_weights_h16_multi): what the per-tensor packers of
// conv_h16.hip (vatl_pack_conv_weight_h16, vatl_pack_deconv4x4s2_weight_h16, vatl_pack_conv_weight_dgrad_h16) write one launch each,
// from a device table of jobs.  The source-index functions are theirs (conv_generic.h, dgrad_phase.h), so the bytes cannot differ.
// A block of 256 threads owns 1024 consecutive elements of one job's destination; it finds its job by a binary search of first_block.
// The kernel is bound by the integer divisions of the index functions: they run in 32 bits wherever the job has fewer than 2^31
// elements (every filter of the pose networks), and what does not depend on the element — the job, and for a data-gradient job the
// taps and the start of each phase filter — is worked out once per block.
#include "dgrad_phase.h"
#include "h16.h"

namespace vatl {

constexpr int kPackH16Conv = 0, kPackH16Deconv = 1, kPackH16Dgrad = 2;      // VatlPackJobH16.kind
constexpr int kPackH16Slice = 1024;                                         // destination elements per block

struct PackH16Block {               // what a block knows about its job
    int job;
    int phases;                     // data-gradient jobs: stride*stride phase filters, one after the other ...
    long long start[5];             // ... filter q holds the elements start[q] .. start[q+1]-1 (empty where no tap reaches the phase)
    DgradAxis ay[4], ax[4];
};

// The 1024 elements from `base` on of a job of `total` elements; I: the type the element index is divided in.
template <typename T, typename I>
__device__ __forceinline__ void pack_h16_slice(const VatlPackJobH16& J, const PackH16Block& B, long long base, long long total) {
    const float* __restrict__ src = J.src;
    unsigned short* __restrict__ dst = static_cast<unsigned short*>(J.dst);
    const int kind = J.kind, Cout = J.Cout, Cin = J.Cin, R = J.R, S = J.S;
    const int Cin8 = (Cin + 7) & ~7, Cout8 = (Cout + 7) & ~7;
#pragma unroll
    for (int e = 0; e < kPackH16Slice / 256; ++e) {
        const long long i = base + e * 256 + threadIdx.x;
        if (i >= total) continue;               // the part of the slice past the job's end
        long long j;
        if (kind == kPackH16Conv) {
            j = conv_weight_src<true>((I)i, Cin, Cin8, R, S);
        } else if (kind == kPackH16Deconv) {
            j = deconv_weight_src<true>((I)i, Cin, Cin8, Cout);
        } else {
            int q = 0;
            while (q + 1 < B.phases && i >= B.start[q + 1]) ++q;
            j = dgrad_weight_src<true>((I)(i - B.start[q]), B.ay[q], B.ax[q], Cout, Cin, Cout8, R, S, J.stride);
        }
        dst[i] = j >= 0 ? T::from_f32(src[j]) : (unsigned short)0;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pack_h16_multi_kernel(const VatlPackJobH16* __restrict__ jobs, int njobs, long long total_blocks) {
    if ((long long)blockIdx.x >= total_blocks) return;
    __shared__ PackH16Block B;
    if (threadIdx.x == 0) {
        int lo = 0, hi = njobs - 1;
        const long long b = blockIdx.x;
        while (lo < hi) {                       // the last job with first_block <= b: at most log2(njobs) + 1 rounds
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].first_block <= b) lo = mid; else hi = mid - 1;
        }
        B.job = lo;
        B.phases = 0;
        const VatlPackJobH16& J = jobs[lo];
        if (J.kind == kPackH16Dgrad && (J.stride == 1 || J.stride == 2)) {
            const long long cc = (long long)((J.Cin + 7) & ~7) * ((J.Cout + 7) & ~7);
            B.phases = J.stride * J.stride;
            for (int q = 0; q < B.phases; ++q) {
                B.ay[q] = dgrad_axis(J.R, J.stride, J.pad, q / J.stride);
                B.ax[q] = dgrad_axis(J.S, J.stride, J.pad, q % J.stride);
                B.start[q] = dgrad_phase_offset(J.R, J.S, J.stride, J.pad, q, cc);
            }
            B.start[B.phases] = dgrad_phase_offset(J.R, J.S, J.stride, J.pad, B.phases, cc);      // the end of the last one
        }
    }
    __syncthreads();
    const VatlPackJobH16& J = jobs[B.job];
    const long long bl = (long long)blockIdx.x - J.first_block;
    if (bl < 0) return;                         // a table that does not start at block 0
    const int Cin8 = (J.Cin + 7) & ~7, Cout8 = (J.Cout + 7) & ~7;
    const long long total = J.kind == kPackH16Conv ? (long long)J.Cout * J.R * J.S * Cin8
                          : J.kind == kPackH16Deconv ? 16LL * J.Cout * Cin8
                          : B.phases ? B.start[B.phases] : 0;          // an unknown kind or stride writes nothing
    if (total < (1LL << 31)) pack_h16_slice<T, unsigned>(J, B, bl * kPackH16Slice, total);
    else pack_h16_slice<T, long long>(J, B, bl * kPackH16Slice, total);
}

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_pack_weights_h16_multi(const VatlPackJobH16* jobs_device, int njobs, int64_t total_blocks, int dtype, void* stream) {
    if (njobs == 0) return 0;
    if (!jobs_device || njobs < 0 || total_blocks <= 0 || total_blocks > 0x7FFFFFFF || !h16_dtype_ok(dtype))
        return fail(VATL_EINVAL, "pack_weights_h16_multi: bad arguments");
    const auto kernel = dtype == kH16F16 ? pack_h16_multi_kernel<F16> : pack_h16_multi_kernel<BF16>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, jobs_device, njobs, (long long)total_blocks);
    return check_launch("pack_weights_h16_multi");
}
