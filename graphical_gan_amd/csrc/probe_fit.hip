// Least-squares linear probe (include/ggan.h): a ridge-regularised least-squares classifier on standardised rows, in closed form.
//   ggan_probe_moments  mean, 1 / std (0 for a constant column) and the class counts of labelled rows Z [n, d];
//   ggan_probe_normal   G = Zs^T Zs / n and R[:, c] = (1/n) sum_{y_i = c} zs_i, zs_i = (z_i - mean) * inv_std formed on the fly;
//   ggan_probe_solve    W = (G + ridge I)^-1 R by an fp64 Cholesky factorisation in one workgroup's LDS, bias = counts / n;
//   ggan_probe_predict  argmax_c of bias + zs W per row (the lowest class on a tie), the number of rows that hit their label.
// The reduction of the normal equations runs over the ROW index -- tens of thousands of rows into at most 128 x (128 + 32) outputs --, the
// transpose of the set-level Gram sweeps of set_rows.h, so it has a skeleton of its own (row_blocks.h, shared with frechet.hip): the rows
// are cut into blocks of kRB = 256, a workgroup sums ONE block in fp32 in row order (v_mfma_f32_32x32x2_f32: the standardised rows are both
// operands of the G tiles, and a one-hot of the label made in registers is the B operand of the R tiles), and a second launch adds the
// block partials in fp64 in block order.  The moments are two such passes with fp64 partials (the second centred by the fp64 mean: no E[z^2] - mean^2).  Nothing here
// depends on the launch shape and there is no floating-point atomic: two calls give the same bits.
#include <math.h>
#include "row_blocks.h"
using namespace ggan;

namespace {

constexpr int kMaxD = GGAN_PROBE_MAX_DIM, kMaxC = GGAN_PROBE_MAX_CLASSES;
constexpr int kMaxRows = 131072;
constexpr int kPR = 64;            // rows per workgroup of probe_predict_k
constexpr int kCnt = kMaxC + 1;    // label histogram of a block: the classes and, last, the labels out of range
static_assert(kMaxC == 32 && kMaxD % 32 == 0, "the kernels below assume these");

inline bool shape_ok(int rows, int d, int C) { return rows >= 1 && rows <= kMaxRows && d >= 1 && d <= kMaxD && C >= 1 && C <= kMaxC; }

// ---- moments ----------------------------------------------------------------------------------------------------------------------
// one block of kRB rows: part[blk][c] = sum over its rows of z (PASS 0) or of (z - mu_c)^2 (PASS 1), in fp64 (block_colsum_*).
// PASS 0 also counts the block's labels: cnt[blk][0 .. 32) per class, cnt[blk][32] those outside [0, C) (no label is an index).
template <int PASS>
__global__ __launch_bounds__(256) void probe_colsum_k(const float* __restrict__ Z, const int* __restrict__ y, int n, int d, int C, int lg,
                                                      const double* __restrict__ mu, double* __restrict__ part, int* __restrict__ cnt) {
    __shared__ double sm[256];
    __shared__ int hist[kCnt];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * kRB, r1 = min(r0 + kRB, n);
    sm[tid] = block_colsum_thread<PASS>(Z, n, d, lg, mu);
    if (PASS == 0 && tid < kCnt) hist[tid] = 0;
    __syncthreads();
    if (PASS == 0 && r0 + tid < r1) {
        const int l = y[r0 + tid];
        atomicAdd(&hist[(l >= 0 && l < C) ? l : kMaxC], 1);
    }
    block_colsum_store(sm, d, lg, part);
    if (PASS == 0) {
        __syncthreads();
        if (tid < kCnt) cnt[(size_t)blockIdx.x * kCnt + tid] = hist[tid];
    }
}

// mu[c] = (the block sums in block order) / n, kept in fp64 for the second pass
__global__ __launch_bounds__(kMaxD) void probe_mean_k(const double* __restrict__ part, int nblk, int n, int d, double* __restrict__ mu) {
    const int c = threadIdx.x;
    if (c >= d) return;
    mu[c] = blocks_sum(part, nblk, d, c) / (double)n;
}

__global__ __launch_bounds__(kMaxD) void probe_moments_final_k(const double* __restrict__ part, const int* __restrict__ cnt,
                                                               const double* __restrict__ mu, int nblk, int n, int d, int C,
                                                               float* __restrict__ mean, float* __restrict__ inv_std,
                                                               int* __restrict__ counts, int* __restrict__ status) {
    __shared__ int flag;
    const int c = threadIdx.x;
    if (c == 0) flag = 0;
    __syncthreads();
    int bits = 0;
    if (c < d) {
        const double v = blocks_sum(part, nblk, d, c) / (double)n, m = mu[c];
        const float s = v > 0.0 ? (float)(1.0 / sqrt(v)) : 0.f;
        if (!isfinite(m) || !isfinite(v) || !isfinite(s)) bits |= GGAN_PROBE_NONFINITE;
        mean[c] = (float)m;
        inv_std[c] = s;
    }
    if (c < kCnt) {
        int t = 0;
        for (int b = 0; b < nblk; ++b) t += cnt[(size_t)b * kCnt + c];
        if (c < C) counts[c] = t;
        if (c == kMaxC && t) bits |= GGAN_PROBE_BAD_LABEL;
    }
    if (bits) atomicOr(&flag, bits);
    __syncthreads();
    if (c == 0) *status = flag;
}

// ---- normal equations ---------------------------------------------------------------------------------------------------------------
struct NormalParams {
    const float *Z, *mean, *inv_std;
    const int* y;
    float* part;       // [blocks][d * d + d * C]
    int n, d, C;
};

// one block of kRB rows through block_gram (row_blocks.h): the T * T tiles of G and T tiles of R, the rows standardised as they are staged,
// the B operand of an R tile a one-hot of the staged label made in a register
template <int T>
__global__ __launch_bounds__(256) void probe_normal_k(const NormalParams P) {
    using S = GramBlock<T, T>;
    __shared__ float zs[kKC * S::LD];
    __shared__ float mu_s[S::DP], is_s[S::DP];
    __shared__ int lab[kKC];
    const int tid = threadIdx.x;
    for (int c = tid; c < S::DP; c += 256) {
        mu_s[c] = c < P.d ? P.mean[c] : 0.f;
        is_s[c] = c < P.d ? P.inv_std[c] : 0.f;
    }
    float* out = P.part + (size_t)blockIdx.x * ((size_t)P.d * P.d + (size_t)P.d * P.C);
    block_gram<T, T>(
        P.n, P.d, zs, [&](int r, int c) { return (P.Z[(size_t)r * P.d + c] - mu_s[c]) * is_s[c]; },
        [&](int rs) {
            if (tid < kKC) lab[tid] = rs + tid < P.n ? P.y[rs + tid] : -1;      // (a row past the end matches no class)
        },
        [&](int k, int j) { return lab[k] == j ? 1.f : 0.f; },
        [&](bool is_g, int i, int j, float v) {
            if (is_g) {
                if (j < P.d) out[(size_t)i * P.d + j] = v;
            } else if (j < P.C) {
                out[(size_t)P.d * P.d + (size_t)i * P.C + j] = v;
            }
        });
}

// element e of [G; R]: the block partials in fp64 in block order, over n, rounded once
__global__ __launch_bounds__(256) void probe_normal_combine_k(const float* __restrict__ part, int nblk, int per, int dd, int n,
                                                              float* __restrict__ G, float* __restrict__ R) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    double t = 0.0;
    for (int b = 0; b < nblk; ++b) t += (double)part[(size_t)b * per + e];
    const float v = (float)(t / (double)n);
    if (e < dd) G[e] = v;
    else R[e - dd] = v;
}

// ---- solve --------------------------------------------------------------------------------------------------------------------------
// one workgroup: L L^T = G + ridge I column by column in the packed lower triangle (row i at i (i + 1) / 2), thread i owning row i; then
// thread c < C takes right-hand side c through the forward and the back substitution.  All fp64; W is rounded once at the end.
__global__ __launch_bounds__(256) void probe_solve_k(const float* __restrict__ G, const float* __restrict__ R, const int* __restrict__ counts,
                                                     int n, int d, int C, float ridge, float* __restrict__ W, float* __restrict__ bias,
                                                     int* __restrict__ status) {
    extern __shared__ double probe_sh[];
    double* L = probe_sh;
    double* X = probe_sh + d * (d + 1) / 2;      // [d][C]
    __shared__ double piv;
    __shared__ int flag;
    const int tid = threadIdx.x;
    if (tid == 0) flag = 0;
    __syncthreads();
    int bits = 0;
    for (int e = tid; e < d * d; e += 256) {
        const int i = e / d, j = e % d;
        const float g = G[e];
        if (!isfinite(g)) bits |= GGAN_PROBE_NONFINITE;
        if (j <= i) L[i * (i + 1) / 2 + j] = (double)g + (i == j ? (double)ridge : 0.0);
    }
    for (int e = tid; e < d * C; e += 256) {
        const float r = R[e];
        if (!isfinite(r)) bits |= GGAN_PROBE_NONFINITE;
        X[e] = (double)r;
    }
    if (bits) atomicOr(&flag, bits);
    __syncthreads();
    const int i = tid;
    double* Li = L + i * (i + 1) / 2;            // (only dereferenced for i < d)
    for (int j = 0; j < d; ++j) {
        double s = 0.0;
        if (i >= j && i < d) {
            const double* Lj = L + j * (j + 1) / 2;
            s = Li[j];
            for (int k = 0; k < j; ++k) s -= Li[k] * Lj[k];
            if (i == j) {
                if (!(s > 0.0) || !isfinite(s)) {      // not positive definite in fp64, or poisoned: say so and keep going on a harmless pivot
                    atomicOr(&flag, GGAN_PROBE_BAD_PIVOT);
                    s = 1.0;
                }
                piv = sqrt(s);
            }
        }
        __syncthreads();
        if (i >= j && i < d) Li[j] = (i == j) ? piv : s / piv;
        __syncthreads();
    }
    if (tid < C) {
        const int c = tid;
        for (int r = 0; r < d; ++r) {
            const double* Lr = L + r * (r + 1) / 2;
            double s = X[r * C + c];
            for (int k = 0; k < r; ++k) s -= Lr[k] * X[k * C + c];
            X[r * C + c] = s / Lr[r];
        }
        for (int r = d - 1; r >= 0; --r) {
            double s = X[r * C + c];
            for (int k = r + 1; k < d; ++k) s -= L[k * (k + 1) / 2 + r] * X[k * C + c];
            X[r * C + c] = s / L[r * (r + 1) / 2 + r];
        }
        bias[c] = (float)((double)counts[c] / (double)n);
    }
    __syncthreads();
    const int bad = flag;
    for (int e = tid; e < d * C; e += 256) W[e] = bad ? __builtin_nanf("") : (float)X[e];
    if (tid == 0 && bad) atomicOr(status, bad);
}

// ---- predict ------------------------------------------------------------------------------------------------------------------------
// kPR rows per workgroup, staged standardised; thread (row, cg) = (tid / 4, tid % 4) carries the scores of classes 8 cg .. 8 cg + 7 -- one
// fmaf chain per class, from the bias, over the columns in order -- and the four threads of a row agree on the maximum, the lowest class
// on equal scores
__global__ __launch_bounds__(256) void probe_predict_k(const float* __restrict__ Z, const int* __restrict__ y, int m, int d, int C,
                                                       const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                       const float* __restrict__ W, const float* __restrict__ bias, int* __restrict__ pred,
                                                       int* __restrict__ correct) {
    __shared__ float zs[kPR * (kMaxD + 1)];
    __shared__ float Ws[kMaxD * kMaxC];
    __shared__ float bs[kMaxC];
    const int tid = threadIdx.x, LD = d | 1, r0 = blockIdx.x * kPR;
    for (int e = tid; e < kPR * d; e += 256) {
        const int k = e / d, c = e % d, r = r0 + k;
        zs[k * LD + c] = r < m ? (Z[(size_t)r * d + c] - mean[c]) * inv_std[c] : 0.f;
    }
    for (int e = tid; e < d * kMaxC; e += 256) {
        const int j = e / kMaxC, c = e % kMaxC;
        Ws[e] = c < C ? W[j * C + c] : 0.f;
    }
    if (tid < kMaxC) bs[tid] = tid < C ? bias[tid] : 0.f;
    __syncthreads();
    const int row = tid >> 2, cg = tid & 3;
    float acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = bs[cg * 8 + q];
    for (int j = 0; j < d; ++j) {
        const float zt = zs[row * LD + j];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = fmaf(zt, Ws[j * kMaxC + cg * 8 + q], acc[q]);
    }
    constexpr int kNone = 0x7fffffff;
    float best = -INFINITY;
    int bi = kNone;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int c = cg * 8 + q;
        if (c < C && (acc[q] > best || (acc[q] == best && c < bi))) { best = acc[q]; bi = c; }
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (bi == kNone) bi = 0;                       // (every score NaN)
    const int r = r0 + row;
    bool hit = false;
    if (cg == 0 && r < m) {
        if (pred) pred[r] = bi;
        if (correct) hit = bi == y[r];
    }
    if (correct) {
        const int hits = __popcll(__ballot(hit));
        if ((tid & 63) == 0 && hits) atomicAdd(correct, hits);
    }
}

}  // namespace

extern "C" {

size_t ggan_probe_moments_workspace(int n, int d, int classes) {
    if (!shape_ok(n, d, classes) || n < 2) return 0;
    const size_t nb = row_blocks(n);
    return align16(nb * d * sizeof(double)) + align16((size_t)d * sizeof(double)) + align16(nb * kCnt * sizeof(int));
}

int ggan_probe_moments(const float* Z, const int32_t* y, int n, int d, int classes, float* mean, float* inv_std, int32_t* counts,
                       int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Z && y && mean && inv_std && counts && status && ws, "null pointer");
    GGAN_CHECK_ARG(shape_ok(n, d, classes), "1 <= n <= 131072, 1 <= d <= 128, 1 <= classes <= 32");
    GGAN_CHECK_ARG(n >= 2, "n < 2: a fit needs two rows");
    GGAN_CHECK_ARG(ws_bytes >= ggan_probe_moments_workspace(n, d, classes), "workspace too small (ggan_probe_moments_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    const int nb = row_blocks(n), lg = log2_ceil(d);
    double* part = (double*)ws;
    double* mu = (double*)((char*)ws + align16((size_t)nb * d * sizeof(double)));
    int* cnt = (int*)((char*)mu + align16((size_t)d * sizeof(double)));
    hipStream_t st = (hipStream_t)stream;
    const double bytes = 4.0 * n * d;
    GGAN_LAUNCH("probe_colsum", 1.0 * n * d, bytes, probe_colsum_k<0>, dim3(nb), dim3(256), 0, st, Z, y, n, d, classes, lg,
                (const double*)nullptr, part, cnt);
    GGAN_LAUNCH("probe_mean", 0, 8.0 * nb * d, probe_mean_k, dim3(1), dim3(kMaxD), 0, st, (const double*)part, nb, n, d, mu);
    GGAN_LAUNCH("probe_colsum_sq", 2.0 * n * d, bytes, probe_colsum_k<1>, dim3(nb), dim3(256), 0, st, Z, y, n, d, classes, lg,
                (const double*)mu, part, cnt);
    GGAN_LAUNCH("probe_moments_final", 0, 8.0 * nb * d, probe_moments_final_k, dim3(1), dim3(kMaxD), 0, st, (const double*)part,
                (const int*)cnt, (const double*)mu, nb, n, d, classes, mean, inv_std, counts, status);
    return 0;
}

size_t ggan_probe_normal_workspace(int n, int d, int classes) {
    if (!shape_ok(n, d, classes) || n < 2) return 0;
    return align16((size_t)row_blocks(n) * ((size_t)d * d + (size_t)d * classes) * sizeof(float));
}

int ggan_probe_normal(const float* Z, const int32_t* y, int n, int d, int classes, const float* mean, const float* inv_std, float* G,
                      float* R, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Z && y && mean && inv_std && G && R && ws, "null pointer");
    GGAN_CHECK_ARG(shape_ok(n, d, classes), "1 <= n <= 131072, 1 <= d <= 128, 1 <= classes <= 32");
    GGAN_CHECK_ARG(n >= 2, "n < 2: a fit needs two rows");
    GGAN_CHECK_ARG(ws_bytes >= ggan_probe_normal_workspace(n, d, classes), "workspace too small (ggan_probe_normal_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    NormalParams P;
    P.Z = Z; P.mean = mean; P.inv_std = inv_std; P.y = y; P.part = (float*)ws;
    P.n = n; P.d = d; P.C = classes;
    const int nb = row_blocks(n), T = cdiv(d, 32), per = d * d + d * classes;
    hipStream_t st = (hipStream_t)stream;
    const double flops = 2.0 * nb * kRB * (32.0 * T) * (32.0 * T + 32.0), bytes = 4.0 * n * d + 4.0 * nb * per;
    switch (T) {
        case 1: { GGAN_LAUNCH("probe_normal_t1", flops, bytes, probe_normal_k<1>, dim3(nb), dim3(256), 0, st, P); } break;
        case 2: { GGAN_LAUNCH("probe_normal_t2", flops, bytes, probe_normal_k<2>, dim3(nb), dim3(256), 0, st, P); } break;
        case 3: { GGAN_LAUNCH("probe_normal_t3", flops, bytes, probe_normal_k<3>, dim3(nb), dim3(256), 0, st, P); } break;
        default: { GGAN_LAUNCH("probe_normal_t4", flops, bytes, probe_normal_k<4>, dim3(nb), dim3(256), 0, st, P); } break;
    }
    GGAN_LAUNCH("probe_normal_combine", 1.0 * nb * per, 4.0 * nb * per, probe_normal_combine_k, dim3(cdiv(per, 256)), dim3(256), 0, st,
                (const float*)P.part, nb, per, d * d, n, G, R);
    return 0;
}

int ggan_probe_solve(const float* G, const float* R, const int32_t* counts, int n, int d, int classes, float ridge, float* W, float* bias,
                     int32_t* status, ggan_stream_t stream) {
    GGAN_CHECK_ARG(G && R && counts && W && bias && status, "null pointer");
    GGAN_CHECK_ARG(shape_ok(n, d, classes), "1 <= n <= 131072, 1 <= d <= 128, 1 <= classes <= 32");
    GGAN_CHECK_ARG(n >= 2, "n < 2: a fit needs two rows");
    GGAN_CHECK_ARG(ridge > 0.f && isfinite(ridge), "ridge must be finite and positive");
    const size_t shmem = ((size_t)d * (d + 1) / 2 + (size_t)d * classes) * sizeof(double);
    // the packed triangle at d = 128 and 32 right-hand sides take 97 KB, above the 64 KiB default; the kernel's two static words come on top,
    // so the request is the largest this entry can make, not the whole 160 KiB of a CU
    constexpr int kMaxShmem = (kMaxD * (kMaxD + 1) / 2 + kMaxD * kMaxC) * (int)sizeof(double);
    static std::atomic<unsigned long long> once{0};
    if (first_on_device(once) &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(probe_solve_k), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShmem) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: the device refuses %d bytes of dynamic LDS", __func__, kMaxShmem);
        return -3;
    }
    GGAN_LAUNCH("probe_solve", 1.0 * d * d * d / 3.0 + 2.0 * d * d * classes, 4.0 * (d * d + 2.0 * d * classes), probe_solve_k, dim3(1),
                dim3(256), shmem, (hipStream_t)stream, G, R, (const int*)counts, n, d, classes, ridge, W, bias, status);
    return 0;
}

int ggan_probe_predict(const float* Z, const int32_t* y, int m, int d, int classes, const float* mean, const float* inv_std,
                       const float* W, const float* bias, int32_t* pred, int32_t* correct, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Z && mean && inv_std && W && bias, "null pointer");
    GGAN_CHECK_ARG(pred || correct, "nothing to write: pred and correct are both null");
    GGAN_CHECK_ARG(!correct || y, "correct needs the labels y");
    GGAN_CHECK_ARG(shape_ok(m, d, classes), "1 <= m <= 131072, 1 <= d <= 128, 1 <= classes <= 32");
    hipStream_t st = (hipStream_t)stream;
    if (correct && hipMemsetAsync(correct, 0, sizeof(int), st) != hipSuccess) {
        set_error("%s: memset failed", __func__);
        return -2;
    }
    GGAN_LAUNCH("probe_predict", 2.0 * m * d * classes, 4.0 * m * (d + 2.0), probe_predict_k, dim3(cdiv(m, kPR)), dim3(256), 0, st, Z,
                (const int*)y, m, d, classes, mean, inv_std, W, bias, pred, correct);
    return 0;
}

}  // extern "C"
