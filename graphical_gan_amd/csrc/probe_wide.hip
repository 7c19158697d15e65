// The wide least-squares probe (include/ggan.h: ggan_wprobe_*): the chain of probe_fit.hip for 1 <= d <= GGAN_WPROBE_MAX_DIM = 4096 columns,
// where neither the normal equations nor their factor fit one workgroup.  The definition is probe_fit.hip's; what changes is who sums what:
//   ggan_wprobe_moments  a thread owns ONE column of a block of kRB = 256 rows and adds it in fp64 in row order; the blocks in block order;
//   ggan_wprobe_normal   a workgroup owns one pair (ti >= tj) of 64-column tiles of G (or one tile of R) and walks ALL row blocks: a block is
//                        summed in fp32 in row order by v_mfma_f32_32x32x2_f32 (the rows standardised as they are staged, a one-hot of the
//                        label made in registers for R), then added to fp64 accumulators in block order -- the order of probe_fit.hip with
//                        no partials in memory; G and R are written in fp64, the upper triangle as the mirrored store of the lower;
//   ggan_wprobe_factor   L L^T = G + ridge I in place on the lower triangle, fp64, blocked and right-looking: per panel of kNB = 64 columns
//                        the diagonal block in one workgroup's LDS (column by column, as probe_solve_k), the panel below solved against it
//                        a row per thread, the trailing lower-triangle tiles updated by v_mfma_f64_16x16x4_f64.  The host loop never waits;
//   ggan_wprobe_solve    one workgroup per right-hand side, a blocked sweep down and up L in steps of 64 rows, fp64, W rounded once;
//   ggan_wprobe_predict  a row's score of a class is one fmaf chain per chunk of 128 columns, the chunks added in fp64 in chunk order.
// No floating-point atomic anywhere, and no sum whose order depends on the launch shape: two calls give the same bits.
#include <math.h>
#include "row_blocks.h"
using namespace ggan;

namespace {

constexpr int kMaxD = GGAN_WPROBE_MAX_DIM, kMaxC = GGAN_PROBE_MAX_CLASSES;
constexpr int kMaxRows = 131072;
constexpr int kT = GGAN_WPROBE_TILE;       // columns of a tile of the normal equations
constexpr int kNB = GGAN_WPROBE_PANEL;     // columns of a panel of the factorisation, rows of a step of the solve
constexpr int kCH = GGAN_WPROBE_CHUNK;     // columns of one fp32 chain of the prediction
constexpr int kPR = 64;                    // rows per workgroup of wprobe_predict_k
constexpr int kCnt = kMaxC + 1;            // label histogram of a block: the classes and, last, the labels out of range
constexpr int kBad = GGAN_PROBE_NONFINITE | GGAN_PROBE_BAD_PIVOT;      // the bits that void a fit
static_assert(kMaxC == 32 && (kT == 64 || kT == 128) && kNB == 64 && kCH == 128 && kMaxD % kT == 0, "the kernels below assume these");

typedef double f64x4 __attribute__((ext_vector_type(4)));

inline bool shape_ok(int rows, int d, int C) { return rows >= 1 && rows <= kMaxRows && d >= 1 && d <= kMaxD && C >= 1 && C <= kMaxC; }
inline int tri(int t) { return t * (t + 1) / 2; }

// workgroup idx of a lower triangle of tiles dealt row by row -> (ti >= tj)
__device__ __forceinline__ void tri_decode(int idx, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= idx) ++ti;
    tj = idx - ti * (ti + 1) / 2;
}

// ---- moments ----------------------------------------------------------------------------------------------------------------------
// block blockIdx.x of kRB rows, columns 256 blockIdx.y ..: thread = column, the rows in row order in fp64 -- part[blk][c] = the sum of z
// (PASS 0) or of (z - mu_c)^2 (PASS 1).  PASS 0, blockIdx.y == 0 also counts the block's labels, as probe_colsum_k does.
template <int PASS>
__global__ __launch_bounds__(256) void wprobe_colsum_k(const float* __restrict__ Z, const int* __restrict__ y, int n, int d, int C,
                                                       const double* __restrict__ mu, double* __restrict__ part, int* __restrict__ cnt) {
    __shared__ int hist[kCnt];
    const int tid = threadIdx.x, c = blockIdx.y * 256 + tid;
    const int r0 = blockIdx.x * kRB, r1 = min(r0 + kRB, n);
    if (c < d) {
        const double m = PASS ? mu[c] : 0.0;
        double acc = 0.0;
        for (int r = r0; r < r1; ++r) {
            const double v = (double)Z[(size_t)r * d + c] - m;
            acc += PASS ? v * v : v;
        }
        part[(size_t)blockIdx.x * d + c] = acc;
    }
    if (PASS == 0 && blockIdx.y == 0) {        // (the same for the whole workgroup)
        if (tid < kCnt) hist[tid] = 0;
        __syncthreads();
        if (r0 + tid < r1) {
            const int l = y[r0 + tid];
            atomicAdd(&hist[(l >= 0 && l < C) ? l : kMaxC], 1);
        }
        __syncthreads();
        if (tid < kCnt) cnt[(size_t)blockIdx.x * kCnt + tid] = hist[tid];
    }
}

__global__ __launch_bounds__(256) void wprobe_mean_k(const double* __restrict__ part, int nblk, int n, int d, double* __restrict__ mu) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    mu[c] = blocks_sum(part, nblk, d, c) / (double)n;
}

// status was zeroed on the stream before this launch; a workgroup ORs its bits in (an integer OR: no order to depend on)
__global__ __launch_bounds__(256) void wprobe_moments_final_k(const double* __restrict__ part, const int* __restrict__ cnt,
                                                              const double* __restrict__ mu, int nblk, int n, int d, int C,
                                                              float* __restrict__ mean, float* __restrict__ inv_std,
                                                              int* __restrict__ counts, int* __restrict__ status) {
    __shared__ int flag;
    const int tid = threadIdx.x, c = blockIdx.x * 256 + tid;
    if (tid == 0) flag = 0;
    __syncthreads();
    int bits = 0;
    if (c < d) {
        const double v = blocks_sum(part, nblk, d, c) / (double)n, m = mu[c];
        const float s = v > 0.0 ? (float)(1.0 / sqrt(v)) : 0.f;
        if (!isfinite(m) || !isfinite(v) || !isfinite(s)) bits |= GGAN_PROBE_NONFINITE;
        mean[c] = (float)m;
        inv_std[c] = s;
    }
    if (blockIdx.x == 0 && tid < kCnt) {
        int t = 0;
        for (int b = 0; b < nblk; ++b) t += cnt[(size_t)b * kCnt + tid];
        if (tid < C) counts[tid] = t;
        if (tid == kMaxC && t) bits |= GGAN_PROBE_BAD_LABEL;
    }
    if (bits) atomicOr(&flag, bits);
    __syncthreads();
    if (tid == 0 && flag) atomicOr(status, flag);
}

// ---- normal equations ---------------------------------------------------------------------------------------------------------------
struct WNormalParams {
    const float *Z, *mean, *inv_std;
    const int* y;
    double *G, *R;
    int n, d, C, npairs;
};

// Workgroup idx < npairs: the T x T tile (ti >= tj) of G, T = kT; idx >= npairs: the T x 32 tile ti = idx - npairs of R.  Wave (wi, wj) =
// (wave / 2, wave % 2) owns the quarter (wi, wj) of the tile, S x S accumulators of 32 x 32, S = T / 64 -- lane l holds
// A[i = l & 31][k = l >> 5] = V[row k][column i] and B[k][j = l & 31] = V[row k][column j] of tile tj, or the one-hot of row k's label (R:
// the waves wj = 1 only help staging).  The rows are staged KC = 4096 / T at a time as vs[row][the tile ti's columns | the tile tj's
// columns], stride LD = 32 mod 64.  Registers per lane: 16 S^2 fp32 + 16 S^2 fp64 values.
template <int T>
__global__ __launch_bounds__(256) void wprobe_normal_k(const WNormalParams P) {
    static_assert(T == 64 || T == 128, "a tile is 2 x 2 waves of S x S MFMA tiles");
    constexpr int S = T / 64, KC = 4096 / T, LD = 2 * T + 32;
    __shared__ float vs[KC * LD];
    __shared__ float mu_s[2 * T], is_s[2 * T];
    __shared__ int lab[KC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int wi = wave >> 1, wj = wave & 1;
    const bool is_r = (int)blockIdx.x >= P.npairs;
    int ti, tj;
    if (is_r) { ti = tj = blockIdx.x - P.npairs; } else { tri_decode(blockIdx.x, ti, tj); }
    const bool one = ti == tj;                            // (R tiles too) only the tile ti's columns are staged, and are both operands
    const int ncols = one ? T : 2 * T, boff = one ? 0 : T;
    const int n = P.n, d = P.d;
    auto column = [&](int c) { return c < T ? ti * T + c : tj * T + c - T; };
    if (tid < ncols) {
        const int col = column(tid);
        mu_s[tid] = col < d ? P.mean[col] : 0.f;
        is_s[tid] = col < d ? P.inv_std[col] : 0.f;
    }
    const bool active = !is_r || wj == 0;                 // (wave-uniform)
    constexpr int SB = S;                                 // (R: only b = 0 is used)
    f32x16 acc[S * S];
    double acc64[S * S][16];
#pragma unroll
    for (int q = 0; q < S * S; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[q][r] = 0.f; acc64[q][r] = 0.0; }
    const int nblk = (n + kRB - 1) / kRB;
    for (int blk = 0; blk < nblk; ++blk) {
        for (int s = 0; s < kRB / KC; ++s) {
            const int rs = blk * kRB + s * KC;
            if (rs >= n) break;                            // (the same for the whole workgroup)
            __syncthreads();                               // the reads of the step before; mu_s, is_s the first time
            for (int e = tid; e < KC * ncols; e += 256) {
                const int k = e / ncols, c = e % ncols, r = rs + k, col = column(c);      // (ncols is a power of two)
                float v = 0.f;
                if (r < n && col < d) v = (P.Z[(size_t)r * d + col] - mu_s[c]) * is_s[c];
                vs[k * LD + c] = v;
            }
            if (is_r && tid < KC) lab[tid] = rs + tid < n ? P.y[rs + tid] : -1;      // (a row past the end matches no class)
            __syncthreads();
            if (active) {
                for (int kk = 0; kk < KC; kk += 2) {
                    const int k = kk + half;
                    float a[S], b[SB];
#pragma unroll
                    for (int u = 0; u < S; ++u) a[u] = vs[k * LD + (wi * S + u) * 32 + l31];
                    if (is_r) {
                        const float hot = lab[k] == l31 ? 1.f : 0.f;
#pragma unroll
                        for (int u = 0; u < S; ++u) acc[u * S] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], hot, acc[u * S], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int v = 0; v < SB; ++v) b[v] = vs[k * LD + boff + (wj * S + v) * 32 + l31];
#pragma unroll
                        for (int u = 0; u < S; ++u)
#pragma unroll
                            for (int v = 0; v < SB; ++v)
                                acc[u * S + v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[v], acc[u * S + v], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < S * S; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc64[q][r] += (double)acc[q][r]; acc[q][r] = 0.f; }      // the block's fp32 sum joins in block order
    }
    if (!active) return;
    const double dn = (double)n;
#pragma unroll
    for (int u = 0; u < S; ++u)
#pragma unroll
        for (int v = 0; v < SB; ++v) {
            if (is_r && v) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = ti * T + (wi * S + u) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;      // the 32x32 accumulator map: column = lane & 31
                if (i >= d) continue;
                const double val = acc64[u * S + v][r] / dn;
                if (is_r) {
                    if (l31 < P.C) P.R[(size_t)i * P.C + l31] = val;
                } else {
                    const int j = tj * T + (wj * S + v) * 32 + l31;
                    if (j <= i) {                          // (so j < d) the lower triangle, and its mirror
                        P.G[(size_t)i * d + j] = val;
                        if (j != i) P.G[(size_t)j * d + i] = val;
                    }
                }
            }
        }
}

// ---- factorisation ------------------------------------------------------------------------------------------------------------------
// the w x w diagonal block at (p, p), w <= kNB: + ridge on its diagonal, then L L^T column by column in LDS, thread i owning row i
__global__ __launch_bounds__(kNB) void wprobe_chol_diag_k(double* __restrict__ G, int d, int p, int w, double ridge, int* __restrict__ status) {
    constexpr int LD = kNB + 1;
    __shared__ double Ls[kNB * LD];
    __shared__ double piv;
    __shared__ int flag;
    const int tid = threadIdx.x;
    if (tid == 0) flag = 0;
    __syncthreads();
    int bits = 0;
    for (int e = tid; e < w * w; e += kNB) {
        const int i = e / w, j = e % w;
        if (j > i) continue;
        const double g = G[(size_t)(p + i) * d + p + j];
        if (!isfinite(g)) bits |= GGAN_PROBE_NONFINITE;
        Ls[i * LD + j] = g + (i == j ? ridge : 0.0);
    }
    if (bits) atomicOr(&flag, bits);
    __syncthreads();
    const int i = tid;
    double* Li = Ls + i * LD;
    for (int j = 0; j < w; ++j) {
        double s = 0.0;
        if (i >= j && i < w) {
            const double* Lj = Ls + j * LD;
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
        if (i >= j && i < w) Li[j] = (i == j) ? piv : s / piv;
        __syncthreads();
    }
    for (int e = tid; e < w * w; e += kNB) {
        const int r = e / w, c = e % w;
        if (c <= r) G[(size_t)(p + r) * d + p + c] = Ls[r * LD + c];
    }
    if (tid == 0 && flag) atomicOr(status, flag);
}

// the panel below a full diagonal block: row i of A21 becomes row i of L21 = A21 L11^-T, a row per thread in registers, L11 in LDS (every
// thread reads the same word of it at the same time)
__global__ __launch_bounds__(kNB) void wprobe_chol_panel_k(double* __restrict__ G, int d, int p, int* __restrict__ status) {
    constexpr int LD = kNB + 1;
    __shared__ double Ls[kNB * LD];
    const int tid = threadIdx.x;
    for (int e = tid; e < kNB * kNB; e += kNB) {
        const int r = e / kNB, c = e % kNB;
        if (c <= r) Ls[r * LD + c] = G[(size_t)(p + r) * d + p + c];
    }
    __syncthreads();
    const int i = p + kNB + blockIdx.x * kNB + tid;
    if (i >= d) return;
    double* row = G + (size_t)i * d + p;
    double x[kNB];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < kNB; ++j) {
        x[j] = row[j];
        bad |= !isfinite(x[j]);
    }
#pragma unroll
    for (int j = 0; j < kNB; ++j) {
        double s = x[j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= x[k] * Ls[j * LD + k];
        x[j] = s / Ls[j * LD + j];
    }
#pragma unroll
    for (int j = 0; j < kNB; ++j) row[j] = x[j];
    if (bad) atomicOr(status, GGAN_PROBE_NONFINITE);
}

// the 64 x 64 tile (ti >= tj) of the trailing lower triangle, origin t0 = p + kNB: A22 -= L21 L21^T over the panel's kNB columns.  Wave w
// owns the tile's rows 16 w .. 16 w + 15 and four 16-column accumulators; lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]
// = L21[row j][k]; the fp64 C/D map is column = l & 15, row = (l >> 4) + 4 * register (NOT the fp32 map).
__global__ __launch_bounds__(256) void wprobe_chol_trail_k(double* __restrict__ G, int d, int p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    int ti, tj;
    tri_decode(blockIdx.x, ti, tj);
    const int t0 = p + kNB, I = t0 + ti * kNB + wave * 16, J = t0 + tj * kNB;
    const int ra = I + li;
    double a[kNB / 4];
#pragma unroll
    for (int s = 0; s < kNB / 4; ++s) a[s] = ra < d ? G[(size_t)ra * d + p + 4 * s + lk] : 0.0;
    f64x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int rb = J + c * 16 + li;
        acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
        double b[kNB / 4];
#pragma unroll
        for (int s = 0; s < kNB / 4; ++s) b[s] = rb < d ? G[(size_t)rb * d + p + 4 * s + lk] : 0.0;
#pragma unroll
        for (int s = 0; s < kNB / 4; ++s) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s], acc[c], 0, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = I + lk + 4 * r, col = J + c * 16 + li;
            if (row < d && col <= row) G[(size_t)row * d + col] -= acc[c][r];      // (col <= row < d; columns >= t0: no operand is among them)
        }
}

// ---- solve --------------------------------------------------------------------------------------------------------------------------
// Workgroup c takes right-hand side c down L (L y = r) and up L^T (L^T x = y) in steps of kNB rows, x[d] in LDS.  Down, step b: wave w
// takes rows 16 w .. 16 w + 15 of the step, lane l the columns l, l + 64, ... before the step, the 64 lanes' sums joined by a butterfly;
// up: thread (g, col) = (tid / 64, tid % 64) takes rows g, g + 4, ... after the step, the four groups joined in group order.  Then wave 0
// solves the step's diagonal block from LDS, lane i owning unknown i.  All fp64, a fixed order; W is rounded once at the end.
__global__ __launch_bounds__(256) void wprobe_solve_k(const double* __restrict__ L, const double* __restrict__ R, const int* __restrict__ counts,
                                                      int n, int d, int C, float* __restrict__ W, float* __restrict__ bias,
                                                      int* __restrict__ status) {
    extern __shared__ double wprobe_sh[];
    const int dp = (d + kNB - 1) / kNB * kNB;
    double* xs = wprobe_sh;                  // [dp]
    double* Ld = xs + dp;                    // [kNB][kNB]: the diagonal block, transposed on the way down
    double* ps = Ld + kNB * kNB;             // [256]
    __shared__ int flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.x;
    if (tid == 0) flag = 0;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < d * C; e += 256) bad |= !isfinite(R[e]);      // (every workgroup looks at all of R: W is all NaN or not at all)
    if (bad) atomicOr(&flag, GGAN_PROBE_NONFINITE);
    for (int r = tid; r < dp; r += 256) xs[r] = r < d ? R[(size_t)r * C + c] : 0.0;
    __syncthreads();
    const int nstep = dp / kNB;
    for (int b = 0; b < nstep; ++b) {
        const int r0 = b * kNB, w = min(kNB, d - r0);
        double acc[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0;
        for (int kc = 0; kc < r0; kc += 64) {
            const double xk = xs[kc + lane];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = r0 + wave * 16 + q;
                if (row < d) acc[q] += L[(size_t)row * d + kc + lane] * xk;
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            double t = acc[q];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
            if (lane == 0) ps[wave * 16 + q] = t;
        }
        for (int e = tid; e < w * kNB; e += 256) {
            const int i = e / kNB, j = e % kNB;
            if (j <= i) Ld[j * kNB + i] = L[(size_t)(r0 + i) * d + r0 + j];
        }
        __syncthreads();
        if (wave == 0) {
            double s = lane < w ? xs[r0 + lane] - ps[lane] : 0.0;
            for (int j = 0; j < w; ++j) {
                const double xj = __shfl(s, j, 64) / Ld[j * kNB + j];
                if (lane == j) s = xj;
                else if (lane > j && lane < w) s -= Ld[j * kNB + lane] * xj;
            }
            if (lane < w) xs[r0 + lane] = s;
        }
        __syncthreads();
    }
    for (int b = nstep - 1; b >= 0; --b) {
        const int r0 = b * kNB, w = min(kNB, d - r0), col = r0 + lane;
        double acc = 0.0;
        if (col < d) {
#pragma unroll 4
            for (int j = r0 + kNB + wave; j < d; j += 4) acc += L[(size_t)j * d + col] * xs[j];
        }
        ps[wave * 64 + lane] = acc;
        for (int e = tid; e < w * kNB; e += 256) {
            const int j = e / kNB, i = e % kNB;
            if (i <= j) Ld[j * kNB + i] = L[(size_t)(r0 + j) * d + r0 + i];
        }
        __syncthreads();
        if (wave == 0) {
            double s = 0.0;
            if (lane < w) s = xs[r0 + lane] - (((ps[lane] + ps[64 + lane]) + ps[128 + lane]) + ps[192 + lane]);
            for (int j = w - 1; j >= 0; --j) {
                const double xj = __shfl(s, j, 64) / Ld[j * kNB + j];
                if (lane == j) s = xj;
                else if (lane < j) s -= Ld[j * kNB + lane] * xj;
            }
            if (lane < w) xs[r0 + lane] = s;
        }
        __syncthreads();
    }
    const bool nan = ((*status | flag) & kBad) != 0;      // (status: what the launches before this one raised; nobody ORs a kBad bit into it now
                                                          //  that this workgroup's own flag would not carry)
    for (int r = tid; r < d; r += 256) W[(size_t)r * C + c] = nan ? __builtin_nanf("") : (float)xs[r];
    if (tid == 0) bias[c] = (float)((double)counts[c] / (double)n);
    __syncthreads();
    if (tid == 0 && c == 0 && flag) atomicOr(status, flag);
}

// ---- predict ------------------------------------------------------------------------------------------------------------------------
// probe_predict_k a chunk of kCH columns at a time: thread (row, cg) = (tid / 4, tid % 4) carries classes 8 cg .. 8 cg + 7 -- per chunk one
// fmaf chain per class in fp32 (from the bias in the first chunk, from 0 after it), the chunks added in fp64 in chunk order
__global__ __launch_bounds__(256) void wprobe_predict_k(const float* __restrict__ Z, const int* __restrict__ y, int m, int d, int C,
                                                        const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                        const float* __restrict__ W, const float* __restrict__ bias, int* __restrict__ pred,
                                                        int* __restrict__ correct) {
    constexpr int LD = kCH + 1;
    __shared__ float zs[kPR * LD];
    __shared__ float Ws[kCH * kMaxC];
    __shared__ float bs[kMaxC];
    const int tid = threadIdx.x, r0 = blockIdx.x * kPR;
    const int row = tid >> 2, cg = tid & 3;
    if (tid < kMaxC) bs[tid] = tid < C ? bias[tid] : 0.f;
    double tot[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) tot[q] = 0.0;
    for (int c0 = 0; c0 < d; c0 += kCH) {
        const int cw = min(kCH, d - c0);
        __syncthreads();                                   // the reads of the chunk before; bs the first time
        for (int e = tid; e < kPR * kCH; e += 256) {
            const int k = e / kCH, c = e % kCH, r = r0 + k, col = c0 + c;
            zs[k * LD + c] = (r < m && c < cw) ? (Z[(size_t)r * d + col] - mean[col]) * inv_std[col] : 0.f;
        }
        for (int e = tid; e < kCH * kMaxC; e += 256) {
            const int j = e / kMaxC, cl = e % kMaxC;
            Ws[e] = (j < cw && cl < C) ? W[(size_t)(c0 + j) * C + cl] : 0.f;
        }
        __syncthreads();
        float acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = c0 == 0 ? bs[cg * 8 + q] : 0.f;
        for (int j = 0; j < cw; ++j) {
            const float zt = zs[row * LD + j];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] = fmaf(zt, Ws[j * kMaxC + cg * 8 + q], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) tot[q] += (double)acc[q];
    }
    constexpr int kNone = 0x7fffffff;
    double best = -INFINITY;
    int bi = kNone;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int cl = cg * 8 + q;
        if (cl < C && (tot[q] > best || (tot[q] == best && cl < bi))) { best = tot[q]; bi = cl; }
    }
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {
        const double ov = __shfl_xor(best, o, 64);
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

constexpr const char* kShape = "1 <= n <= 131072, 1 <= d <= 4096, 1 <= classes <= 32";

}  // namespace

extern "C" {

size_t ggan_wprobe_moments_workspace(int n, int d, int classes) {
    if (!shape_ok(n, d, classes) || n < 2) return 0;
    const size_t nb = row_blocks(n);
    return align16(nb * d * sizeof(double)) + align16((size_t)d * sizeof(double)) + align16(nb * kCnt * sizeof(int));
}

int ggan_wprobe_moments(const float* Z, const int32_t* y, int n, int d, int classes, float* mean, float* inv_std, int32_t* counts,
                        int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Z && y && mean && inv_std && counts && status && ws, "null pointer");
    GGAN_CHECK_ARG(shape_ok(n, d, classes), kShape);
    GGAN_CHECK_ARG(n >= 2, "n < 2: a fit needs two rows");
    GGAN_CHECK_ARG(ws_bytes >= ggan_wprobe_moments_workspace(n, d, classes), "workspace too small (ggan_wprobe_moments_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    const int nb = row_blocks(n), cb = cdiv(d, 256);
    double* part = (double*)ws;
    double* mu = (double*)((char*)ws + align16((size_t)nb * d * sizeof(double)));
    int* cnt = (int*)((char*)mu + align16((size_t)d * sizeof(double)));
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
        set_error("%s: memset failed", __func__);
        return -2;
    }
    const double bytes = 4.0 * n * d;
    GGAN_LAUNCH("wprobe_colsum", 1.0 * n * d, bytes, wprobe_colsum_k<0>, dim3(nb, cb), dim3(256), 0, st, Z, y, n, d, classes,
                (const double*)nullptr, part, cnt);
    GGAN_LAUNCH("wprobe_mean", 0, 8.0 * nb * d, wprobe_mean_k, dim3(cb), dim3(256), 0, st, (const double*)part, nb, n, d, mu);
    GGAN_LAUNCH("wprobe_colsum_sq", 2.0 * n * d, bytes, wprobe_colsum_k<1>, dim3(nb, cb), dim3(256), 0, st, Z, y, n, d, classes,
                (const double*)mu, part, cnt);
    GGAN_LAUNCH("wprobe_moments_final", 0, 8.0 * nb * d, wprobe_moments_final_k, dim3(cb), dim3(256), 0, st, (const double*)part,
                (const int*)cnt, (const double*)mu, nb, n, d, classes, mean, inv_std, counts, status);
    return 0;
}

int ggan_wprobe_normal(const float* Z, const int32_t* y, int n, int d, int classes, const float* mean, const float* inv_std, double* G,
                       double* R, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Z && y && mean && inv_std && G && R, "null pointer");
    GGAN_CHECK_ARG(shape_ok(n, d, classes), kShape);
    GGAN_CHECK_ARG(n >= 2, "n < 2: a fit needs two rows");
    GGAN_CHECK_ARG((((uintptr_t)G | (uintptr_t)R) & 7) == 0, "G and R must be 8-byte aligned");
    WNormalParams P;
    P.Z = Z; P.mean = mean; P.inv_std = inv_std; P.y = y; P.G = G; P.R = R;
    P.n = n; P.d = d; P.C = classes;
    const int nt = cdiv(d, kT);
    P.npairs = tri(nt);
    const double rows = 1.0 * row_blocks(n) * kRB;
    const double flops = 2.0 * rows * kT * (kT * P.npairs + 32.0 * nt), bytes = 4.0 * n * kT * (2.0 * P.npairs + nt) + 8.0 * d * (d + classes);
    GGAN_LAUNCH(kT == 64 ? "wprobe_normal_t64" : "wprobe_normal_t128", flops, bytes, wprobe_normal_k<kT>, dim3(P.npairs + nt), dim3(256), 0,
                (hipStream_t)stream, P);
    return 0;
}

int ggan_wprobe_factor(double* G, int d, float ridge, int32_t* status, ggan_stream_t stream) {
    GGAN_CHECK_ARG(G && status, "null pointer");
    GGAN_CHECK_ARG(d >= 1 && d <= kMaxD, "1 <= d <= 4096");
    GGAN_CHECK_ARG(ridge > 0.f && isfinite(ridge), "ridge must be finite and positive");
    GGAN_CHECK_ARG(((uintptr_t)G & 7) == 0, "G must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (int p = 0; p < d; p += kNB) {
        const int w = min(kNB, d - p), below = d - p - kNB;      // (below > 0 only under a full block)
        GGAN_LAUNCH("wprobe_chol_diag_nb64", 1.0 * w * w * w / 3.0, 16.0 * w * w, wprobe_chol_diag_k, dim3(1), dim3(kNB), 0, st, G, d, p, w,
                    (double)ridge, status);
        if (below <= 0) break;
        GGAN_LAUNCH("wprobe_chol_panel_nb64", 1.0 * below * kNB * kNB, 16.0 * below * kNB, wprobe_chol_panel_k, dim3(cdiv(below, kNB)),
                    dim3(kNB), 0, st, G, d, p, status);
        const int nt = cdiv(below, kNB);
        GGAN_LAUNCH("wprobe_chol_trail_nb64", 2.0 * kNB * kNB * kNB * tri(nt), 32.0 * kNB * kNB * tri(nt), wprobe_chol_trail_k,
                    dim3(tri(nt)), dim3(256), 0, st, G, d, p);
    }
    return 0;
}

int ggan_wprobe_solve(const double* L, const double* R, const int32_t* counts, int n, int d, int classes, float* W, float* bias,
                      int32_t* status, ggan_stream_t stream) {
    GGAN_CHECK_ARG(L && R && counts && W && bias && status, "null pointer");
    GGAN_CHECK_ARG(shape_ok(n, d, classes), kShape);
    GGAN_CHECK_ARG(n >= 2, "n < 2: a fit needs two rows");
    GGAN_CHECK_ARG((((uintptr_t)L | (uintptr_t)R) & 7) == 0, "L and R must be 8-byte aligned");
    const size_t shmem = ((size_t)cdiv(d, kNB) * kNB + kNB * kNB + 256) * sizeof(double);
    // x at d = 4096, the diagonal block and the partial sums take 66 KB, above the 64 KiB default; the kernel's static word comes on top
    constexpr int kMaxShmem = (kMaxD + kNB * kNB + 256) * (int)sizeof(double);
    static std::atomic<unsigned long long> once{0};
    if (first_on_device(once) &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(wprobe_solve_k), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShmem) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: the device refuses %d bytes of dynamic LDS", __func__, kMaxShmem);
        return -3;
    }
    GGAN_LAUNCH("wprobe_solve_nb64", 2.0 * d * d * classes, 8.0 * d * d * classes, wprobe_solve_k, dim3(classes), dim3(256), shmem,
                (hipStream_t)stream, L, R, (const int*)counts, n, d, classes, W, bias, status);
    return 0;
}

int ggan_wprobe_predict(const float* Z, const int32_t* y, int m, int d, int classes, const float* mean, const float* inv_std,
                        const float* W, const float* bias, int32_t* pred, int32_t* correct, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Z && mean && inv_std && W && bias, "null pointer");
    GGAN_CHECK_ARG(pred || correct, "nothing to write: pred and correct are both null");
    GGAN_CHECK_ARG(!correct || y, "correct needs the labels y");
    GGAN_CHECK_ARG(shape_ok(m, d, classes), "1 <= m <= 131072, 1 <= d <= 4096, 1 <= classes <= 32");
    hipStream_t st = (hipStream_t)stream;
    if (correct && hipMemsetAsync(correct, 0, sizeof(int), st) != hipSuccess) {
        set_error("%s: memset failed", __func__);
        return -2;
    }
    GGAN_LAUNCH("wprobe_predict_c128", 2.0 * m * d * classes, 4.0 * m * (d + 2.0), wprobe_predict_k, dim3(cdiv(m, kPR)), dim3(256), 0, st, Z,
                (const int*)y, m, d, classes, mean, inv_std, W, bias, pred, correct);
    return 0;
}

}  // extern "C"
