// K-Means / weighted query filters on the device (ActiveLearning.py:553-582, 593-611): the clustering the reference asks
// scikit-learn for — KMeans(n_clusters=k, random_state=318): k-means++ seeding, one Lloyd run, max_iter 300, tol 1e-4,
// float64 throughout — restated so that it selects the same items (sklearn/cluster/_kmeans.py, _k_means_lloyd.pyx).
//   prepare   column means, centred float64 copy, tol = mean(var(X, axis=0)) * 1e-4              (_tolerance, KMeans.fit)
//   seed      k-means++ with the host's random draws: scan -> searchsorted -> candidate distances -> potentials -> adopt,
//             2k launches chained on the stream, no host round trip                                (_kmeans_plusplus)
//   assign    nearest centre by |c|^2 - 2 x.c on v_mfma_f64_16x16x4_f64, arg-min in the write-out  (_update_chunk_dense)
//   update    weighted mean per cluster and the squared centre shift                               (lloyd_iter_chunked_dense)
//   finish    per cluster the member nearest its centre in the uncentred space, and the inertia
// Every sum has a fixed order (no floating-point atomics): two runs give the same bits.  Flags are raised with plain stores
// of the same value from every writer.
#include "common.h"

namespace vatl {

constexpr int kMaxTrials = 16;            // 2 + int(log(k)) candidates per seeding step: k < e^14
constexpr double kTieRel = 1e-9;          // relative gap below which two float64 sums over D ~ 2048 count as tied

typedef double double4_t __attribute__((ext_vector_type(4)));

// Sum over the block in a fixed order (butterfly inside a wave, then the waves in order); every thread gets the result.
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += sh[w];
    __syncthreads();
    return t;
}

// ---------------------------------------------------------------------------------------------------------------- prepare
// One thread per column, rows in order (numpy's order for X.mean(axis=0)): mean, centred copy, variance.
__global__ __launch_bounds__(64) void km_center_kernel(const float* __restrict__ x, double* __restrict__ xc, double* __restrict__ mean,
                                                       double* __restrict__ colvar, long long n, int D) {
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (long long i = 0; i < n; ++i) s += (double)x[i * D + d];
    const double m = s / (double)n;
    double v = 0.0;
    for (long long i = 0; i < n; ++i) {
        const double c = (double)x[i * D + d] - m;
        xc[i * D + d] = c;
        v += c * c;
    }
    mean[d] = m;
    colvar[d] = v / (double)n;
}

__global__ __launch_bounds__(256) void km_tol_kernel(const double* __restrict__ colvar, double* __restrict__ tol, int D) {
    __shared__ double sh[4];
    double s = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) s += colvar[d];
    s = block_sum<4>(s, sh);
    if (threadIdx.x == 0) tol[0] = s / (double)D * 1e-4;
}

// ------------------------------------------------------------------------------------------------------------------- seed
// dc[t][i] = min(closest[i], |x_i - x_cand[t]|^2) by direct differences, one wave per point.  first_index >= 0: the first
// centre (one candidate, no previous distances); it also seeds cand[0] for the adoption that follows.
__global__ __launch_bounds__(256) void km_seed_dist_kernel(const double* __restrict__ xc, int32_t* __restrict__ cand, int T, int first_index,
                                                           const double* __restrict__ closest, double* __restrict__ dc, long long n, int D) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (first_index >= 0 && blockIdx.x == 0 && threadIdx.x == 0) cand[0] = first_index;
    if (row >= n) return;
    const double* cr[kMaxTrials];
#pragma unroll
    for (int t = 0; t < kMaxTrials; ++t) cr[t] = xc + (long long)(first_index >= 0 ? first_index : (t < T ? cand[t] : 0)) * D;
    const double* xr = xc + row * D;
    double s[kMaxTrials];
#pragma unroll
    for (int t = 0; t < kMaxTrials; ++t) s[t] = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double xv = xr[d];
#pragma unroll
        for (int t = 0; t < kMaxTrials; ++t)
            if (t < T) { const double v = xv - cr[t][d]; s[t] += v * v; }
    }
#pragma unroll
    for (int t = 0; t < kMaxTrials; ++t)
        if (t < T) {
            const double v = wave_sum(s[t]);
            if (lane == 0) dc[t * n + row] = first_index >= 0 ? v : fmin(closest[row], v);
        }
}

// One block: adopt the best of the Tprev candidates of centre `c` (weighted potentials, first arg-min, tie flag), then, when
// `draws` is given, draw the T candidates of the next centre: prefix sum of w * closest, searchsorted(left) of rand * pot.
__global__ __launch_bounds__(1024) void km_seed_select_kernel(const double* __restrict__ w, double* __restrict__ closest, double* __restrict__ cum,
                                                              const double* __restrict__ dc, int32_t* __restrict__ cand, int Tprev,
                                                              const double* __restrict__ draws, int T, int32_t* __restrict__ indices, int c,
                                                              int32_t* __restrict__ tie_flag, long long n) {
    __shared__ double sh[16];
    __shared__ double pots[kMaxTrials];
    __shared__ int best_s;
    const int tid = threadIdx.x;
    for (int t = 0; t < Tprev; ++t) {
        double p = 0.0;
        for (long long i = tid; i < n; i += 1024) p += dc[t * n + i] * w[i];
        p = block_sum<16>(p, sh);
        if (tid == 0) pots[t] = p;
    }
    if (tid == 0) {
        int b = 0;
        for (int t = 1; t < Tprev; ++t)
            if (pots[t] < pots[b]) b = t;
        for (int t = 0; t < Tprev; ++t)
            if (cand[t] != cand[b] && (pots[b] == 0.0 || pots[t] - pots[b] <= kTieRel * pots[b])) tie_flag[0] = 1;
        indices[c] = cand[b];
        best_s = b;
    }
    __syncthreads();
    const int b = best_s;
    const double pot = pots[b];
    if (!draws) {
        for (long long i = tid; i < n; i += 1024) closest[i] = dc[b * n + i];
        return;
    }
    // each thread owns a contiguous chunk; exclusive scan of the chunk totals over the block.  Another association than np.cumsum's
    // running sum: entries differ from it by rounding, and where w * closest is 0 (points already chosen) two neighbours at a chunk
    // boundary can come out one ulp out of order; the search below stays well defined.  A draw that lands within that rounding
    // (~1e-13 relative) of an entry could pick the neighbouring candidate: the tie flag does not see that case (about 1e-13 per draw).
    const long long chunk = (n + 1023) / 1024;
    const long long lo = (long long)tid * chunk < n ? (long long)tid * chunk : n;
    const long long hi = lo + chunk < n ? lo + chunk : n;
    double tot = 0.0;
    for (long long i = lo; i < hi; ++i) { const double v = dc[b * n + i]; closest[i] = v; tot += w[i] * v; }
    double inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const double u = __shfl_up(inc, o, 64); if ((tid & 63) >= o) inc += u; }
    double run = __shfl_up(inc, 1, 64);                        // exclusive prefix inside the wave
    if ((tid & 63) == 0) run = 0.0;
    if ((tid & 63) == 63) sh[tid >> 6] = inc;
    __syncthreads();
    for (int v = 0; v < (tid >> 6); ++v) run += sh[v];
    for (long long i = lo; i < hi; ++i) { run += w[i] * closest[i]; cum[i] = run; }
    __syncthreads();
    if (tid < T) {
        const double rv = draws[tid] * pot;
        long long a = 0, e = n;
        while (a < e) { const long long m = (a + e) >> 1; if (cum[m] < rv) a = m + 1; else e = m; }
        cand[tid] = (int32_t)(a < n - 1 ? a : n - 1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ Lloyd
__global__ __launch_bounds__(256) void km_cnorm_kernel(const double* __restrict__ centers, double* __restrict__ cnorm, double* __restrict__ status, int k, int D) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { status[0] = 0.0; status[2] = 0.0; }
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= k) return;
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) { const double v = centers[(long long)j * D + d]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) cnorm[j] = s;
}

// labels[i] = first arg-min_j |c_j|^2 - 2 x_i . c_j.  One block per 16 points, 64 centres per pass; the four waves take the
// 16-column steps of D in turn and their partial products are added in wave order.  MFMA operands (one f64 per lane):
// A[row lane&15][k lane>>4], B[k lane>>4][col lane&15]; a lane loads four consecutive columns and feeds them to four MFMAs,
// which only permutes the order of the sum over D, the same way for A and B.  Result: col lane&15, row (lane>>4) + 4*reg.
__global__ __launch_bounds__(256) void km_assign_kernel(const double* __restrict__ xc, const double* __restrict__ centers, const double* __restrict__ cnorm,
                                                        const int32_t* __restrict__ labels_prev, int32_t* __restrict__ labels,
                                                        double* __restrict__ status, long long n, int D, int k) {
    __shared__ double part[4][4][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, r16 = lane & 15;
    long long row = (long long)blockIdx.x * 16 + r16;
    if (row > n - 1) row = n - 1;
    const double* xa = xc + row * D + 4 * g;
    double best = INFINITY;
    int bestj = 0x7FFFFFFF;
    for (int j0 = 0; j0 < k; j0 += 64) {
        double4_t acc[4];
        const double* cb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
            const int cj = j0 + t * 16 + r16;
            cb[t] = centers + (long long)(cj < k ? cj : k - 1) * D + 4 * g;
        }
        for (int d0 = wave * 16; d0 < D; d0 += 64) {
            const double4_t a = *(const double4_t*)(xa + d0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (j0 + t * 16 < k) {
                    const double4_t bv = *(const double4_t*)(cb[t] + d0);
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], bv[m], acc[t], 0, 0, 0);
                }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[wave][t][r][lane] = acc[t][r];
        __syncthreads();
        // this wave finishes result register `wave`: points (lane>>4) + 4*wave, centre column lane&15
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = j0 + t * 16 + r16;
            const double dot = ((part[0][t][wave][lane] + part[1][t][wave][lane]) + part[2][t][wave][lane]) + part[3][t][wave][lane];
            const double score = j < k ? cnorm[j] - 2.0 * dot : INFINITY;
            if (score < best) { best = score; bestj = j; }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const double ov = __shfl_xor(best, o, 64);
        const int oj = __shfl_xor(bestj, o, 64);
        if (ov < best || (ov == best && oj < bestj)) { best = ov; bestj = oj; }
    }
    const long long prow = (long long)blockIdx.x * 16 + g + 4 * wave;
    if (r16 == 0 && prow < n) {
        if (bestj >= k) bestj = 0;                         // every score nan: np.argmin returns 0
        labels[prow] = bestj;
        if (!labels_prev || labels_prev[prow] != bestj) status[0] = 1.0;
    }
}

// centers_new[j] = sum_i w_i x_i / sum_i w_i over the members in index order; shift_part[j][chunk] = this block's share of
// |centers_new[j] - centers[j]|^2.  A cluster without weight keeps its centre and raises status[2].
__global__ __launch_bounds__(256) void km_update_kernel(const double* __restrict__ xc, const double* __restrict__ w, const int32_t* __restrict__ labels,
                                                        const double* __restrict__ centers, double* __restrict__ centers_new,
                                                        double* __restrict__ shift_part, double* __restrict__ status, long long n, int D) {
    __shared__ double sh[4];
    const int j = blockIdx.x;
    const int d = blockIdx.y * 256 + threadIdx.x;
    const bool in = d < D;
    double acc = 0.0, wsum = 0.0;
    for (long long i = 0; i < n; ++i)
        if (labels[i] == j) {
            const double wi = w[i];
            wsum += wi;
            if (in) acc += wi * xc[i * D + d];
        }
    double sq = 0.0;
    if (in) {
        const double old = centers[(long long)j * D + d];
        const double nw = wsum > 0.0 ? acc * (1.0 / wsum) : old;
        centers_new[(long long)j * D + d] = nw;
        sq = (nw - old) * (nw - old);
    }
    sq = block_sum<4>(sq, sh);
    if (threadIdx.x == 0) {
        shift_part[j * gridDim.y + blockIdx.y] = sq;
        if (!(wsum > 0.0)) status[2] = 1.0;
    }
}

__global__ __launch_bounds__(256) void km_sum_kernel(const double* __restrict__ v, double* __restrict__ out, long long m) {
    __shared__ double sh[4];
    double s = 0.0;
    for (long long i = threadIdx.x; i < m; i += 256) s += v[i];
    s = block_sum<4>(s, sh);
    if (threadIdx.x == 0) out[0] = s;
}

// ----------------------------------------------------------------------------------------------------------------- finish
// One block per cluster.  Its waves take the points in turn; for a member: w * |xc - c|^2 (inertia term) and
// dis = |emb - (c + mean)|^2 (the reference's distance in the uncentred space).  reps[j] = lowest member index whose dis is
// within kTieRel of the cluster's smallest, -1 for a cluster without members.
__global__ __launch_bounds__(256) void km_rep_kernel(const float* __restrict__ emb, const double* __restrict__ xc, const double* __restrict__ mean,
                                                     const double* __restrict__ w, const double* __restrict__ centers, const int32_t* __restrict__ labels,
                                                     int32_t* __restrict__ reps, double* __restrict__ inertia_row, double* __restrict__ dis,
                                                     long long n, int D) {
    __shared__ double smin[4];
    __shared__ long long sidx[4];
    const int j = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* c = centers + (long long)j * D;
    double mn = INFINITY;
    for (long long i = wave; i < n; i += 4) {
        if (labels[i] != j) continue;
        double si = 0.0, sd = 0.0;
        for (int d = lane; d < D; d += 64) {
            const double cv = c[d];
            const double a = xc[i * D + d] - cv;
            const double u = (double)emb[i * D + d] - (cv + mean[d]);
            si += a * a;
            sd += u * u;
        }
        si = wave_sum(si);
        sd = wave_sum(sd);
        if (lane == 0) { inertia_row[i] = w[i] * si; dis[i] = sd; }
        mn = fmin(mn, sd);
    }
    if (lane == 0) smin[wave] = mn;
    __syncthreads();                                           // also orders the dis[] stores before the reads below
    mn = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
    const double thr = mn + kTieRel * mn;
    long long bi = 0x7FFFFFFFFFFFFFFFLL;
    for (long long i = threadIdx.x; i < n; i += 256)
        if (labels[i] == j && dis[i] <= thr && i < bi) bi = i;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const long long oi = __shfl_xor(bi, o, 64); if (oi < bi) bi = oi; }
    if (lane == 0) sidx[wave] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < 4; ++v) if (sidx[v] < bi) bi = sidx[v];
        reps[j] = bi == 0x7FFFFFFFFFFFFFFFLL ? -1 : (int32_t)bi;
    }
}

static bool km_shape_ok(int64_t n, int D, int k) { return n > 0 && n <= 0x7FFFFFFF && D > 0 && k >= 1 && (int64_t)k <= n; }

}  // namespace vatl

using namespace vatl;

extern "C" int vatl_kmeans_prepare(const float* emb, int64_t n, int D, double* xc, double* mean, double* tol, double* workspace, void* stream) {
    if (!emb || !xc || !mean || !tol || !workspace || n <= 0 || n > 0x7FFFFFFF || D <= 0) return fail(VATL_EINVAL, "kmeans_prepare: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(km_center_kernel, dim3((unsigned)((D + 63) / 64)), dim3(64), 0, st, emb, xc, mean, workspace, (long long)n, D);
    hipLaunchKernelGGL(km_tol_kernel, dim3(1), dim3(256), 0, st, workspace, tol, D);
    return check_launch("kmeans_prepare");
}

extern "C" int64_t vatl_kmeans_seed_workspace_doubles(int64_t n, int trials) {
    if (n <= 0 || trials < 1 || trials > kMaxTrials) return 0;
    return (2 + (int64_t)trials) * n + kMaxTrials / 2;
}

extern "C" int vatl_kmeans_seed(const double* xc, const double* weight, int64_t n, int D, int k, int first_index, const double* rand_dev, int trials,
                                int32_t* indices_dev, int32_t* tie_flag_dev, double* workspace, void* stream) {
    if (!xc || !weight || !indices_dev || !tie_flag_dev || !workspace || !km_shape_ok(n, D, k) || first_index < 0 || first_index >= n ||
        trials < 1 || trials > kMaxTrials || (k > 1 && !rand_dev))
        return fail(VATL_EINVAL, "kmeans_seed: bad arguments (need 1 <= k <= n, 0 <= first_index < n, 1 <= trials <= %d)", kMaxTrials);
    hipStream_t st = (hipStream_t)stream;
    double* closest = workspace;
    double* cum = workspace + n;
    double* dc = workspace + 2 * n;
    int32_t* cand = (int32_t*)(workspace + (2 + (int64_t)trials) * n);
    const dim3 rows((unsigned)((n + 3) / 4));
    hipLaunchKernelGGL(km_seed_dist_kernel, rows, dim3(256), 0, st, xc, cand, 1, first_index, closest, dc, (long long)n, D);
    for (int c = 1; c < k; ++c) {
        hipLaunchKernelGGL(km_seed_select_kernel, dim3(1), dim3(1024), 0, st, weight, closest, cum, dc, cand, c == 1 ? 1 : trials,
                           rand_dev + (int64_t)(c - 1) * trials, trials, indices_dev, c - 1, tie_flag_dev, (long long)n);
        hipLaunchKernelGGL(km_seed_dist_kernel, rows, dim3(256), 0, st, xc, cand, trials, -1, closest, dc, (long long)n, D);
    }
    hipLaunchKernelGGL(km_seed_select_kernel, dim3(1), dim3(1024), 0, st, weight, closest, cum, dc, cand, k == 1 ? 1 : trials, (const double*)nullptr, trials,
                       indices_dev, k - 1, tie_flag_dev, (long long)n);
    return check_launch("kmeans_seed");
}

extern "C" int vatl_kmeans_assign(const double* xc, const double* centers, int64_t n, int D, int k, const int32_t* labels_prev_or_null, int32_t* labels,
                                  double* status, double* workspace, void* stream) {
    if (!xc || !centers || !labels || !status || !workspace || !km_shape_ok(n, D, k) || D % 16 != 0)
        return fail(VATL_EINVAL, "kmeans_assign: bad arguments (need 1 <= k <= n, D a positive multiple of 16)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(km_cnorm_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, st, centers, workspace, status, k, D);
    hipLaunchKernelGGL(km_assign_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, xc, centers, workspace, labels_prev_or_null, labels, status,
                       (long long)n, D, k);
    return check_launch("kmeans_assign");
}

extern "C" int64_t vatl_kmeans_update_workspace_doubles(int D, int k) {
    if (D <= 0 || k <= 0) return 0;
    return (int64_t)k * ((D + 255) / 256);
}

extern "C" int vatl_kmeans_update(const double* xc, const double* weight, const int32_t* labels, const double* centers, int64_t n, int D, int k,
                                  double* centers_new, double* status, double* workspace, void* stream) {
    if (!xc || !weight || !labels || !centers || !centers_new || !status || !workspace || !km_shape_ok(n, D, k))
        return fail(VATL_EINVAL, "kmeans_update: bad arguments (need 1 <= k <= n, D > 0)");
    hipStream_t st = (hipStream_t)stream;
    const int ny = (D + 255) / 256;
    hipLaunchKernelGGL(km_update_kernel, dim3((unsigned)k, (unsigned)ny), dim3(256), 0, st, xc, weight, labels, centers, centers_new, workspace, status,
                       (long long)n, D);
    hipLaunchKernelGGL(km_sum_kernel, dim3(1), dim3(256), 0, st, workspace, status + 1, (long long)k * ny);
    return check_launch("kmeans_update");
}

extern "C" int vatl_kmeans_finish(const float* emb, const double* xc, const double* mean, const double* weight, const double* centers,
                                  const int32_t* labels, int64_t n, int D, int k, int32_t* representatives, double* inertia, double* workspace,
                                  void* stream) {
    if (!emb || !xc || !mean || !weight || !centers || !labels || !representatives || !inertia || !workspace || !km_shape_ok(n, D, k))
        return fail(VATL_EINVAL, "kmeans_finish: bad arguments (need 1 <= k <= n, D > 0)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(km_rep_kernel, dim3((unsigned)k), dim3(256), 0, st, emb, xc, mean, weight, centers, labels, representatives, workspace, workspace + n,
                       (long long)n, D);
    hipLaunchKernelGGL(km_sum_kernel, dim3(1), dim3(256), 0, st, workspace, inertia, (long long)n);
    return check_launch("kmeans_finish");
}
