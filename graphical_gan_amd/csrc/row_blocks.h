// What the kernels that reduce over the ROW index share (probe_fit.hip, frechet.hip): tens of thousands of rows into at most 128 x 128 (+ 32)
// outputs, the transpose of the set-level Gram sweeps of set_rows.h.  The rows are cut into blocks of kRB = 256; a workgroup sums ONE
// block -- column sums in fp64, products in fp32 in row order by v_mfma_f32_32x32x2_f32 -- and a second launch adds the block partials
// in fp64 in block order.  Nothing here depends on the launch shape and there is no floating-point atomic: two calls give the same bits.
#pragma once
#include "common.h"

namespace ggan {
namespace {

constexpr int kRB = GGAN_PROBE_ROW_BLOCK;      // rows of a block
constexpr int kKC = 64;                        // rows of a block staged per step of block_gram
static_assert(kRB == 256 && kRB % kKC == 0, "the kernels below assume these");

inline int row_blocks(int n) { return cdiv(n, kRB); }
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
inline int log2_ceil(int d) {
    int lg = 0;
    while ((1 << lg) < d) ++lg;
    return lg;
}

// ---- column sums -----------------------------------------------------------------------------------------------------------------------
// block blockIdx.x of kRB rows: the sum over its rows of z (PASS 0) or of (z - mu_c)^2 (PASS 1), in fp64.  cw = 1 << lg = the power of
// two >= d: thread (g, col) = (tid / cw, tid % cw) walks the rows g, g + 256 / cw, ... of its column (block_colsum_thread); behind a
// barrier over sm[256] the groups are added in group order (block_colsum_store).
template <int PASS>
__device__ __forceinline__ double block_colsum_thread(const float* __restrict__ Z, int n, int d, int lg, const double* __restrict__ mu) {
    const int tid = threadIdx.x, cw = 1 << lg, col = tid & (cw - 1), g = tid >> lg, ng = 256 >> lg;
    const int r0 = blockIdx.x * kRB, r1 = min(r0 + kRB, n);
    double acc = 0.0;
    if (col < d) {
        const double m = PASS ? mu[col] : 0.0;
        for (int r = r0 + g; r < r1; r += ng) {
            const double v = (double)Z[(size_t)r * d + col] - m;
            acc += PASS ? v * v : v;
        }
    }
    return acc;
}
__device__ __forceinline__ void block_colsum_store(const double* sm, int d, int lg, double* __restrict__ part) {
    const int tid = threadIdx.x, cw = 1 << lg, ng = 256 >> lg;
    if (tid < cw && tid < d) {
        double t = 0.0;
        for (int q = 0; q < ng; ++q) t += sm[q * cw + tid];
        part[(size_t)blockIdx.x * d + tid] = t;
    }
}
// column c of the block partials part[nblk][d], added in block order
__device__ __forceinline__ double blocks_sum(const double* __restrict__ part, int nblk, int d, int c) {
    double t = 0.0;
    for (int b = 0; b < nblk; ++b) t += part[(size_t)b * d + c];
    return t;
}

// ---- products --------------------------------------------------------------------------------------------------------------------------
// One block of kRB rows of n, d padded to DP = 32 T columns (a padded column is all zeros).  The outputs are T * T tiles G = V^T V of the
// staged values V and NR further tiles V^T B, 32 x 32 each, dealt to the four waves round-robin; the reduction index of every MFMA is the
// row: lane l holds A[i = l & 31][k = l >> 5] = V[row k][column i] and B[k][j = l & 31] = V[row k][column j] (G) or bop(k, j) (the
// further tiles), so a tile is the fp32 sum over the block's rows in row order.  The rows are staged kKC at a time as vs[row][column]: a
// fragment read is 32 consecutive floats per half-wave, and the row stride LD = 32 mod 64 puts the two halves of a wave on different banks.
//   value(r, c)      the staged value of row r < n, column c < d
//   side(rs)         called by every thread while a step is staged: what bop needs of the rows rs .. rs + kKC
//   bop(k, j)        B[k][j] of the further tiles, k the row within the step
//   out(is_g, i, j, v)  element (i, j) of G, or (i, j) of the further tiles, i < d
template <int T, int NR>
struct GramBlock {
    static constexpr int DP = 32 * T, LD = (DP % 64 == 0) ? DP + 32 : DP, NT = T * T + NR, NQ = (NT + 3) / 4;
};
template <int T, int NR, class Value, class Side, class BOp, class Out>
__device__ __forceinline__ void block_gram(int n, int d, float* vs /*[kKC * LD]*/, Value&& value, Side&& side, BOp&& bop, Out&& out) {
    using S = GramBlock<T, NR>;
    constexpr int DP = S::DP, LD = S::LD, NT = S::NT, NQ = S::NQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    f32x16 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    const int r0 = blockIdx.x * kRB;
    for (int s = 0; s < kRB / kKC; ++s) {
        const int rs = r0 + s * kKC;
        if (rs >= n) break;                        // (the same for the whole workgroup)
        __syncthreads();                           // the reads of the step before; the caller's staged constants the first time
        for (int e = tid; e < kKC * DP; e += 256) {
            const int k = e / DP, c = e % DP, r = rs + k;
            float v = 0.f;
            if (r < n && c < d) v = value(r, c);
            vs[k * LD + c] = v;
        }
        side(rs);
        __syncthreads();
        for (int kk = 0; kk < kKC; kk += 2) {
            const int k = kk + half;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int t = wave + 4 * q;
                if (t < NT) {                      // (wave-uniform)
                    const bool is_g = t < T * T;
                    const int ti = is_g ? t / T : t - T * T;
                    const float a = vs[k * LD + ti * 32 + l31];
                    const float b = is_g ? vs[k * LD + (t % T) * 32 + l31] : bop(k, l31);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[q], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int t = wave + 4 * q;
        if (t >= NT) continue;
        const bool is_g = t < T * T;
        const int ti = is_g ? t / T : t - T * T, j = is_g ? (t % T) * 32 + l31 : l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;       // the 32x32 accumulator map: column = lane & 31
            if (i >= d) continue;
            out(is_g, i, j, acc[q][r]);
        }
    }
}

}  // namespace
}  // namespace ggan
