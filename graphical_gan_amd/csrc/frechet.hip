// Frechet distance between Gaussians fitted to two row sets (include/ggan.h): |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2).
//   ggan_frechet_moments   the fp64 mean and the fp64 covariance (over n - 1) of fp32 rows X [n, d]: the skeleton of the probe's moments and
//                          normal equations (row_blocks.h) with inv_std = 1 and no R tiles -- column sums in fp64 per block of 256 rows, the
//                          blocks added in block order; the rows centred by that fp64 mean as they are staged, a block's products summed in
//                          fp32 by v_mfma_f32_32x32x2_f32, the block partials added in fp64 in block order and KEPT in fp64 (the next stage
//                          subtracts traces).  No E[x^2] - mean^2.
//   ggan_frechet_distance  one workgroup, all fp64: P^T S1 P = L L^T by a diagonally pivoted Cholesky factorisation that tolerates a
//                          semi-definite S1, M = L^T S2 L (its non-zero spectrum is that of S1 S2), the eigenvalues of M by two-sided Jacobi
//                          rotations in round-robin ordering, tr (S1 S2)^(1/2) = sum sqrt(max(lambda, 0)).
// No floating-point atomic and no sum whose order depends on the launch: two calls give the same bits.
#include <math.h>
#include "row_blocks.h"
using namespace ggan;

namespace {

constexpr int kMaxD = GGAN_FRECHET_MAX_DIM;
constexpr int kMaxRows = 131072;
constexpr int kSweepCap = 20;          // twice the most sweeps the float64 model of this ordering takes over the tests' grid (docs/KERNELS.md)
constexpr double kTol = 1e-14;         // off(M)_F <= kTol ||M at the start||_F
constexpr double kEps = 2.220446049250313e-16;
static_assert(kMaxD == 128 && kMaxD % 32 == 0, "the kernels below assume these");

inline bool shape_ok(int n, int d) { return n >= 2 && n <= kMaxRows && d >= 1 && d <= kMaxD; }

// ---- moments ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void frechet_colsum_k(const float* __restrict__ X, int n, int d, int lg, double* __restrict__ part) {
    __shared__ double sm[256];
    sm[threadIdx.x] = block_colsum_thread<0>(X, n, d, lg, nullptr);
    __syncthreads();
    block_colsum_store(sm, d, lg, part);
}

// mean[c] = (the block sums in block order) / n
__global__ __launch_bounds__(kMaxD) void frechet_mean_k(const double* __restrict__ part, int nblk, int n, int d, double* __restrict__ mean) {
    const int c = threadIdx.x;
    if (c < d) mean[c] = blocks_sum(part, nblk, d, c) / (double)n;
}

// one block of rows through block_gram: the T * T tiles of C^T C, C the rows centred by the fp64 mean and rounded once as they are staged
template <int T>
__global__ __launch_bounds__(256) void frechet_cov_k(const float* __restrict__ X, const double* __restrict__ mean, int n, int d,
                                                      float* __restrict__ part) {
    using S = GramBlock<T, 0>;
    __shared__ float vs[kKC * S::LD];
    __shared__ double mu_s[S::DP];
    for (int c = threadIdx.x; c < S::DP; c += 256) mu_s[c] = c < d ? mean[c] : 0.0;
    float* out = part + (size_t)blockIdx.x * d * d;
    block_gram<T, 0>(
        n, d, vs, [&](int r, int c) { return (float)((double)X[(size_t)r * d + c] - mu_s[c]); }, [](int) {}, [](int, int) { return 0.f; },
        [&](bool, int i, int j, float v) {
            if (j < d) out[(size_t)i * d + j] = v;
        });
}

// element e of the covariance: the block partials in fp64 in block order, over n - 1, kept in fp64; a non-finite mean or entry raises the
// status bit (the word is zeroed by the entry point in front of this launch)
__global__ __launch_bounds__(256) void frechet_cov_combine_k(const float* __restrict__ part, const double* __restrict__ mean, int nblk, int d,
                                                              int n, double* __restrict__ cov, int* __restrict__ status) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (e < d * d) {
        double t = 0.0;
        for (int b = 0; b < nblk; ++b) t += (double)part[(size_t)b * d * d + e];
        const double v = t / (double)(n - 1);
        cov[e] = v;
        bad = !isfinite(v) || (e < d && !isfinite(mean[e]));
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, GGAN_FRECHET_NONFINITE);
}

// ---- distance -----------------------------------------------------------------------------------------------------------------------------
// pair k of step `step` of a sweep over m columns (m even): column m - 1 stays, the others walk a circle -- m / 2 disjoint pairs a step,
// every pair once in the m - 1 steps of a sweep
__device__ __forceinline__ void rr_pair(int m, int step, int k, int& p, int& q) {
    const int a = k ? (step + k) % (m - 1) : m - 1, b = k ? (step - k + m - 1) % (m - 1) : step;
    p = min(a, b);
    q = max(a, b);
}

// dynamic LDS: A [m * m] (first L^T, then M), cs [3][m / 2] (c, s, t of a step's rotations), red [256], dg [m] (during the iteration: the
// step's pairs, p | q << 16, as ints)
__host__ __device__ inline size_t distance_lds(int d) {
    const int m = d + (d & 1);
    return ((size_t)m * m + 3 * (m / 2) + 256 + m) * sizeof(double);
}

// One workgroup of 256 threads.  Every decision a barrier depends on -- the pivot of a column, non-finite input, convergence -- is made
// once, written to LDS and read by every thread, so that all barriers sit in uniform control flow; the sweep loop has a fixed trip count.
__global__ __launch_bounds__(256) void frechet_distance_k(const double* __restrict__ mean1, const double* __restrict__ S1,
                                                           const double* __restrict__ mean2, const double* __restrict__ S2, int d,
                                                           double* Lg, double* Tt, double* __restrict__ out,
                                                           int* __restrict__ status) {
    extern __shared__ double frechet_sh[];
    const int tid = threadIdx.x, m = d + (d & 1), h = m / 2;
    double* A = frechet_sh;                    // [m][m]
    double* cs = A + (size_t)m * m;            // c [h], s [h], t [h]
    double* red = cs + 3 * h;                  // [256]
    double* dg = red + 256;                    // [m]
    int* pq = reinterpret_cast<int*>(dg);      // [h], once the factorisation is done with dg
    __shared__ double sh_val[4];               // tr S1, the pivot, ||M||_F^2 at the start, the last off-diagonal norm squared
    __shared__ int sh_int[3];                  // the non-finite flag, the pivot's index, go on / stop

    // ---- the inputs: finite?  tr S1 for the pivot threshold
    if (tid == 0) sh_int[0] = 0;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < d * d; e += 256) bad |= !isfinite(S1[e]) || !isfinite(S2[e]);
    for (int e = tid; e < d; e += 256) bad |= !isfinite(mean1[e]) || !isfinite(mean2[e]);
    if (bad) atomicOr(&sh_int[0], 1);
    for (int e = tid; e < m * m; e += 256) A[e] = 0.0;
    if (tid < m) dg[tid] = tid < d ? S1[(size_t)tid * d + tid] : -INFINITY;
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < d; ++i) t += S1[(size_t)i * d + i];
        sh_val[0] = t;
    }
    __syncthreads();
    if (sh_int[0]) {                           // (the same for every thread)
        if (tid < 4) out[tid] = __builtin_nan("");
        if (tid == 0) *status = GGAN_FRECHET_NONFINITE;
        return;
    }
    const double thr = fmax((double)d * kEps * sh_val[0], 0.0);

    // ---- P^T S1 P = L L^T, L^T kept as A[column j][row i].  Column j: the largest remaining diagonal entry is the pivot (the lowest index on
    // a tie); at or below thr every remaining column is zero -- a semi-definite S1 is no failure.  Row i of the column is S1[p][i] minus the
    // row's dot product with row p over the columns before; rows that were pivots before are zero.
    for (int j = 0; j < d; ++j) {
        if (tid < 64) {
            double v = tid < m ? dg[tid] : -INFINITY;
            int at = tid < m ? tid : m;
            if (tid + 64 < m && dg[tid + 64] > v) { v = dg[tid + 64]; at = tid + 64; }
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const double ov = __shfl_xor(v, o, 64);
                const int oa = __shfl_xor(at, o, 64);
                if (ov > v || (ov == v && oa < at)) { v = ov; at = oa; }
            }
            if (tid == 0) { sh_val[1] = v; sh_int[1] = at; }
        }
        __syncthreads();
        const double piv = sh_val[1];
        const int p = sh_int[1];
        if (!(piv > thr)) break;               // (the same for every thread)
        if (tid < d) {
            double v = 0.0;
            if (dg[tid] != -INFINITY) {
                v = S1[(size_t)p * d + tid];
                for (int k = 0; k < j; ++k) v -= A[k * m + tid] * A[k * m + p];
                v /= sqrt(piv);
            }
            A[j * m + tid] = v;
            if (dg[tid] != -INFINITY) dg[tid] = tid == p ? -INFINITY : dg[tid] - v * v;
        }
        __syncthreads();
    }
    __syncthreads();

    // ---- L to global memory as Lg[i][a], then Tt[b][i] = (S2 L)[i][b]: S2[k][i] is read along i (S2 is symmetric), L[k][b] is a broadcast
    for (int e = tid; e < d * d; e += 256) {
        const int i = e / d, a = e % d;
        Lg[e] = A[a * m + i];
    }
    for (int e = tid; e < d * d; e += 256) {
        const int b = e / d, i = e % d;
        double t = 0.0;
        for (int k = 0; k < d; ++k) t += S2[(size_t)k * d + i] * A[b * m + k];
        Tt[e] = t;
    }
    __threadfence_block();
    __syncthreads();
    // ---- M[a][b] = sum_i L[i][a] (S2 L)[i][b] into LDS in the place of L^T (no longer read): the lower triangle is computed and mirrored,
    // so M is symmetric bit for bit
    for (int e = tid; e < m * m; e += 256) A[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < d * d; e += 256) {
        const int b = e / d, a = e % d;
        if (a >= b) {
            double t = 0.0;
            for (int i = 0; i < d; ++i) t += Lg[(size_t)i * d + a] * Tt[(size_t)b * d + i];
            A[a * m + b] = t;
            A[b * m + a] = t;
        }
    }
    __syncthreads();

    // ---- the eigenvalues of M: two-sided Jacobi, round-robin.  In front of every sweep the off-diagonal norm is summed in a fixed order and
    // thread 0 decides; at most kSweepCap sweeps
    for (int sweep = 0;; ++sweep) {
        double off2 = 0.0, dia2 = 0.0;
        for (int e = tid; e < m * m; e += 256) {
            const double v = A[e];
            if (e / m == e % m) dia2 += v * v;
            else off2 += v * v;
        }
        red[tid] = off2;
        if (sweep == 0) {
            __syncthreads();
            if (tid == 0) {
                double t = 0.0;
                for (int i = 0; i < 256; ++i) t += red[i];
                sh_val[3] = t;
            }
            __syncthreads();
            red[tid] = dia2;
        }
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int i = 0; i < 256; ++i) t += red[i];
            if (sweep == 0) {
                sh_val[2] = t + sh_val[3];     // ||M||_F^2 at the start: the yardstick stays, it does not shrink with the iteration
                t = sh_val[3];
            }
            sh_val[3] = t;
            const bool conv = t <= kTol * kTol * sh_val[2];
            sh_int[2] = conv ? 0 : (sweep < kSweepCap ? 1 : 2);      // 0: converged, 1: one more sweep, 2: the cap is spent
        }
        __syncthreads();
        if (sh_int[2] != 1) break;             // (the same for every thread)
        for (int step = 0; step < m - 1; ++step) {
            if (tid < h) {
                int p, q;
                rr_pair(m, step, tid, p, q);
                const double app = A[p * m + p], aqq = A[q * m + q], apq = A[p * m + q];
                double t = 0.0;
                if (apq != 0.0) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                }
                const double c = 1.0 / sqrt(1.0 + t * t);
                cs[tid] = c;
                cs[h + tid] = t * c;
                cs[2 * h + tid] = t;
                pq[tid] = p | (q << 16);
            }
            __syncthreads();
            // block (k, l) = rows (p_k, q_k) x columns (p_l, q_l) <- J_k^T B J_l.  Every new entry is (the terms on b00 and b11) + (the
            // terms on b01 and b10), each product rounded on its own: block (l, k) adds the same numbers, so M stays symmetric bit for bit
            for (int e = tid; e < h * h; e += 256) {
                const int k = e / h, l = e % h;
                const int pk = pq[k] & 0xffff, qk = pq[k] >> 16, pl = pq[l] & 0xffff, ql = pq[l] >> 16;
                double* r0 = A + pk * m;
                double* r1 = A + qk * m;
                const double b00 = r0[pl], b01 = r0[ql], b10 = r1[pl], b11 = r1[ql];
                if (k == l) {
                    const double t = cs[2 * h + k];
                    r0[pl] = b00 - t * b01;
                    r1[ql] = b11 + t * b01;
                    r0[ql] = 0.0;
                    r1[pl] = 0.0;
                } else {
                    const double ck = cs[k], sk = cs[h + k], cl = cs[l], sl = cs[h + l];
                    const double cc = __dmul_rn(ck, cl), sS = __dmul_rn(sk, sl), csw = __dmul_rn(ck, sl), scw = __dmul_rn(sk, cl);
                    r0[pl] = __dadd_rn(__dadd_rn(__dmul_rn(cc, b00), __dmul_rn(sS, b11)), -__dadd_rn(__dmul_rn(csw, b01), __dmul_rn(scw, b10)));
                    r0[ql] = __dadd_rn(__dadd_rn(__dmul_rn(csw, b00), -__dmul_rn(scw, b11)), __dadd_rn(__dmul_rn(cc, b01), -__dmul_rn(sS, b10)));
                    r1[pl] = __dadd_rn(__dadd_rn(__dmul_rn(scw, b00), -__dmul_rn(csw, b11)), __dadd_rn(-__dmul_rn(sS, b01), __dmul_rn(cc, b10)));
                    r1[ql] = __dadd_rn(__dadd_rn(__dmul_rn(sS, b00), __dmul_rn(cc, b11)), __dadd_rn(__dmul_rn(scw, b01), __dmul_rn(csw, b10)));
                }
            }
            __syncthreads();
        }
    }

    if (tid == 0) {
        double trs = 0.0, tr = 0.0, dmu2 = 0.0;
        for (int i = 0; i < d; ++i) {
            trs += sqrt(fmax(A[i * m + i], 0.0));
            tr += S1[(size_t)i * d + i] + S2[(size_t)i * d + i];
            const double dm = mean1[i] - mean2[i];
            dmu2 += dm * dm;
        }
        out[0] = dmu2 + tr - 2.0 * trs;        // not clipped at 0: two samples of one distribution may land a hair below
        out[1] = dmu2;
        out[2] = tr;
        out[3] = 2.0 * trs;
        *status = sh_int[2] == 2 ? GGAN_FRECHET_NOT_CONVERGED : 0;
    }
}

}  // namespace

extern "C" {

size_t ggan_frechet_moments_workspace(int n, int d) {
    if (!shape_ok(n, d)) return 0;
    const size_t nb = row_blocks(n);
    return align16(nb * d * sizeof(double)) + align16(nb * d * d * sizeof(float));
}

int ggan_frechet_moments(const float* X, int n, int d, double* mean, double* cov, int32_t* status, void* ws, size_t ws_bytes,
                         ggan_stream_t stream) {
    GGAN_CHECK_ARG(X && mean && cov && status && ws, "null pointer");
    GGAN_CHECK_ARG(n >= 2, "n < 2: a covariance needs two rows");
    GGAN_CHECK_ARG(shape_ok(n, d), "2 <= n <= 131072, 1 <= d <= 128");
    GGAN_CHECK_ARG(ws_bytes >= ggan_frechet_moments_workspace(n, d), "workspace too small (ggan_frechet_moments_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    GGAN_CHECK_ARG(((uintptr_t)mean & 7) == 0 && ((uintptr_t)cov & 7) == 0, "mean and cov must be 8-byte aligned");
    const int nb = row_blocks(n), lg = log2_ceil(d), T = cdiv(d, 32), dd = d * d;
    double* cpart = (double*)ws;
    float* gpart = (float*)((char*)ws + align16((size_t)nb * d * sizeof(double)));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
        set_error("%s: memset failed", __func__);
        return -2;
    }
    GGAN_LAUNCH("frechet_colsum", 1.0 * n * d, 4.0 * n * d, frechet_colsum_k, dim3(nb), dim3(256), 0, st, X, n, d, lg, cpart);
    GGAN_LAUNCH("frechet_mean", 0, 8.0 * nb * d, frechet_mean_k, dim3(1), dim3(kMaxD), 0, st, (const double*)cpart, nb, n, d, mean);
    const double flops = 2.0 * nb * kRB * (32.0 * T) * (32.0 * T), bytes = 4.0 * n * d + 4.0 * nb * dd;
    switch (T) {
        case 1: { GGAN_LAUNCH("frechet_cov_t1", flops, bytes, frechet_cov_k<1>, dim3(nb), dim3(256), 0, st, X, (const double*)mean, n, d, gpart); } break;
        case 2: { GGAN_LAUNCH("frechet_cov_t2", flops, bytes, frechet_cov_k<2>, dim3(nb), dim3(256), 0, st, X, (const double*)mean, n, d, gpart); } break;
        case 3: { GGAN_LAUNCH("frechet_cov_t3", flops, bytes, frechet_cov_k<3>, dim3(nb), dim3(256), 0, st, X, (const double*)mean, n, d, gpart); } break;
        default: { GGAN_LAUNCH("frechet_cov_t4", flops, bytes, frechet_cov_k<4>, dim3(nb), dim3(256), 0, st, X, (const double*)mean, n, d, gpart); } break;
    }
    GGAN_LAUNCH("frechet_cov_combine", 1.0 * nb * dd, 4.0 * nb * dd, frechet_cov_combine_k, dim3(cdiv(dd, 256)), dim3(256), 0, st,
                (const float*)gpart, (const double*)mean, nb, d, n, cov, status);
    return 0;
}

size_t ggan_frechet_distance_workspace(int d) {
    if (d < 1 || d > kMaxD) return 0;
    return 2 * align16((size_t)d * d * sizeof(double));
}

int ggan_frechet_distance(const double* mean1, const double* cov1, const double* mean2, const double* cov2, int d, double* out,
                          int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(mean1 && cov1 && mean2 && cov2 && out && status && ws, "null pointer");
    GGAN_CHECK_ARG(d >= 1 && d <= kMaxD, "1 <= d <= 128");
    GGAN_CHECK_ARG(ws_bytes >= ggan_frechet_distance_workspace(d), "workspace too small (ggan_frechet_distance_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    GGAN_CHECK_ARG((((uintptr_t)mean1 | (uintptr_t)cov1 | (uintptr_t)mean2 | (uintptr_t)cov2 | (uintptr_t)out) & 7) == 0,
                   "the fp64 arrays must be 8-byte aligned");
    // M at d = 128 takes 128 KiB of the CU's 160 KiB, above the 64 KiB default; the request is the largest this entry can make
    const int kMaxShmem = (int)distance_lds(kMaxD);
    static std::atomic<unsigned long long> once{0};
    if (first_on_device(once) &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(frechet_distance_k), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShmem) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: the device refuses %d bytes of dynamic LDS", __func__, kMaxShmem);
        return -3;
    }
    double* Lg = (double*)ws;
    double* Tt = (double*)((char*)ws + align16((size_t)d * d * sizeof(double)));
    GGAN_LAUNCH("frechet_distance", 1.0 * d * d * d / 3.0 + 4.0 * d * d * d + 1.0 * kSweepCap * 12.0 * d * d * d, 8.0 * 6.0 * d * d,
                frechet_distance_k, dim3(1), dim3(256), distance_lds(d), (hipStream_t)stream, mean1, cov1, mean2, cov2, d, Lg, Tt, out, status);
    return 0;
}

}  // extern "C"
