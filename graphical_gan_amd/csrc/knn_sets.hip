// k-NN balls of row sets: the two primitives behind improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage
// (Naeem et al. 2020), include/ggan.h.  With squared Euclidean distances D(a, b) = ||a - b||^2:
//   ggan_knn_radii    r2[i] = the k-th smallest of { D(z_i, z_l) : l != i }          (a multiset order statistic, self left out by INDEX)
//   ggan_ball_counts  cnt[a] = #{ j : D(a, b_j) <= rB2[j] },  min2[a] = min_j D(a, b_j)
// Both sweep 128 x 128 Gram tiles of mmd_sets.hip's shape (16 k per step, 2 x 2 waves of 64 x 64, four 32x32x2 fp32 accumulators per
// wave, branch-free clamped loads, norms from a pre-pass), distances as max(n_i + n_j - 2 g_ij, 0); nothing of size rows^2 reaches memory.
//
// Orientation: the QUERY rows (the rows a result is written for) are the MFMA's N side, the CANDIDATE rows its M side.  Accumulator
// register r of lane l is g[candidate (r & 3) + 8 (r >> 2) + 4 (l >> 5)][query l & 31] of a 32x32 block, so a lane owns ONE query per
// block column -- two per 64 x 64 wave tile -- and sees 32 candidates of each per tile.  What it keeps per owned query lives in
// registers across the whole sweep: the K smallest distances so far (a sorted list, K a template argument, every index a compile-time
// constant), or a count and a minimum.  Every query block sweeps all candidate blocks (no symmetric half: every row needs its own
// list); grid (query blocks, S): workgroup (b, s) takes the candidate blocks s, s + S, ...  After the sweep -- once per workgroup, not
// per tile -- the two lane halves that share a query are merged by a lane exchange, the two waves that share it through LDS, and the
// workgroup leaves one partial per query and split; a last small kernel merges the S partials of each row.
//
// Candidates are left out by index, never by value: l == i (radii), and rows beyond the set (the tile's ghost rows).  Lists are merged
// as multisets (a duplicate row counts), counts are integers, minima are order-free: no floating-point atomics anywhere, and two calls
// give the same bits.
#include "common.h"
#include "set_rows.h"
using namespace ggan;

namespace {

constexpr int kMaxK = 8;
constexpr int kTargetWgs = 2048;

struct SweepParams : RowSets {     // queries: rows [0, nq) of Z; candidates: rows [c0, c0 + nc) of Z
    const float* rad;              // ball_counts: [nc] squared radii of the candidates
    float* pf;                     // partials: radii [S][K][nq] lists, ball_counts [S][nq] minima
    int* pi;                       // ball_counts: [S][nq] counts
    int nq, nc, c0;
    int nbc, S;                    // candidate blocks, splits of them
};

// v into the ascending list L of the K smallest values seen so far: tested against the K-th first; then every slot takes the median of
// its lower neighbour, itself and v (the lower neighbour is never the larger of the two).  Equal values are kept: a multiset.
template <int K>
__device__ __forceinline__ void list_insert(float (&L)[K], float v) {
    if (v < L[K - 1]) {
#pragma unroll
        for (int q = K - 1; q > 0; --q) L[q] = fmaxf(L[q - 1], fminf(L[q], v));
        L[0] = fminf(L[0], v);
    }
}

template <int K, bool VEC>
__global__ __launch_bounds__(256, 2) void knn_radii_k(const SweepParams P) {
    warm_kernarg(P);
    __shared__ __attribute__((aligned(16))) float As[2][KS * LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][KS * LD];
    __shared__ float nC[BT], nQ[BT];
    __shared__ float mg[4][64][K];                       // the waves' lists, one per owned query
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, half = lane >> 5, l31 = lane & 31;
    const int r0q = blockIdx.x * BT, s = blockIdx.y;
    float L[2][K];
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int q = 0; q < K; ++q) L[bj][q] = INFINITY;

    float4 ra[2], rb[2];
    if (s < P.nbc) load_step<VEC>(P, P.c0 + s * BT, r0q, 0, ra, rb);
    for (int c = s; c < P.nbc; c += P.S) {
        const int r0c = c * BT, cn = c + P.S;
        if (tid < BT) nC[tid] = r0c + tid < P.nc ? P.norms[P.c0 + r0c + tid] : 0.f;
        else nQ[tid - BT] = r0q + tid - BT < P.nq ? P.norms[r0q + tid - BT] : 0.f;
        f32x16 acc[2][2];
        gram_tile<VEC>(P, P.c0 + r0c, r0q, cn < P.nbc, P.c0 + cn * BT, r0q, As, Bs, ra, rb, acc);
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const int jl = wn * 64 + bj * 32 + l31, j = r0q + jl;
            const float nj = nQ[jl];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int il = wm * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, i = r0c + il;
                    const float dist = fmaxf(nC[il] + nj - 2.f * acc[bi][bj][r], 0.f);
                    list_insert<K>(L[bj], (i < P.nc && P.c0 + i != j) ? dist : INFINITY);
                }
            }
        }
        __syncthreads();                                   // nC / nQ are rewritten by the next tile
    }

    // lanes l and l ^ 32 own the same queries (other candidates): each takes the other's list
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        float o[K];
#pragma unroll
        for (int q = 0; q < K; ++q) o[q] = __shfl_xor(L[bj][q], 32, 64);
#pragma unroll
        for (int q = 0; q < K; ++q) list_insert<K>(L[bj], o[q]);
        if (half == 0) {
#pragma unroll
            for (int q = 0; q < K; ++q) mg[wave][bj * 32 + l31][q] = L[bj][q];
        }
    }
    __syncthreads();
    // waves (0, wn) and (1, wn) own the same 64 queries: thread ql < 128 merges the pair of query ql and writes the workgroup's list
    if (tid < BT) {
        const int w0 = 2 * (tid >> 6), ql = tid & 63, j = r0q + tid;
        float a[K];
#pragma unroll
        for (int q = 0; q < K; ++q) a[q] = mg[w0][ql][q];
#pragma unroll
        for (int q = 0; q < K; ++q) list_insert<K>(a, mg[w0 + 1][ql][q]);
        if (j < P.nq) {
#pragma unroll
            for (int q = 0; q < K; ++q) P.pf[((size_t)s * K + q) * P.nq + j] = a[q];
        }
    }
}

// row j: the S partial lists merged, the K-th value out
template <int K>
__global__ __launch_bounds__(256) void knn_final_k(const float* __restrict__ part, int n, int S, float* __restrict__ r2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float L[K];
#pragma unroll
    for (int q = 0; q < K; ++q) L[q] = INFINITY;
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int q = 0; q < K; ++q) list_insert<K>(L, part[((size_t)s * K + q) * n + j]);
    }
    r2[j] = L[K - 1];
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void ball_counts_k(const SweepParams P) {
    warm_kernarg(P);
    __shared__ __attribute__((aligned(16))) float As[2][KS * LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][KS * LD];
    __shared__ float nC[BT], rC[BT], nQ[BT];
    __shared__ int mc[4][64];
    __shared__ float mm[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, half = lane >> 5, l31 = lane & 31;
    const int r0q = blockIdx.x * BT, s = blockIdx.y;
    int cnt[2] = {0, 0};
    float mn[2] = {INFINITY, INFINITY};

    float4 ra[2], rb[2];
    if (s < P.nbc) load_step<VEC>(P, P.c0 + s * BT, r0q, 0, ra, rb);
    for (int c = s; c < P.nbc; c += P.S) {
        const int r0c = c * BT, cn = c + P.S;
        if (tid < BT) {
            const bool ok = r0c + tid < P.nc;
            nC[tid] = ok ? P.norms[P.c0 + r0c + tid] : 0.f;
            rC[tid] = ok ? P.rad[r0c + tid] : 0.f;
        } else {
            nQ[tid - BT] = r0q + tid - BT < P.nq ? P.norms[r0q + tid - BT] : 0.f;
        }
        f32x16 acc[2][2];
        gram_tile<VEC>(P, P.c0 + r0c, r0q, cn < P.nbc, P.c0 + cn * BT, r0q, As, Bs, ra, rb, acc);
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const float nj = nQ[wn * 64 + bj * 32 + l31];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int il = wm * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const bool ok = r0c + il < P.nc;
                    const float dist = fmaxf(nC[il] + nj - 2.f * acc[bi][bj][r], 0.f);
                    cnt[bj] += (ok && dist <= rC[il]) ? 1 : 0;
                    mn[bj] = fminf(mn[bj], ok ? dist : INFINITY);
                }
            }
        }
        __syncthreads();                                   // nC / rC / nQ are rewritten by the next tile
    }

    // lane halves, then the two waves of a query through LDS (as knn_radii_k)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        cnt[bj] += __shfl_xor(cnt[bj], 32, 64);
        mn[bj] = fminf(mn[bj], __shfl_xor(mn[bj], 32, 64));
        if (half == 0) { mc[wave][bj * 32 + l31] = cnt[bj]; mm[wave][bj * 32 + l31] = mn[bj]; }
    }
    __syncthreads();
    if (tid < BT) {
        const int w0 = 2 * (tid >> 6), ql = tid & 63, j = r0q + tid;
        if (j < P.nq) {
            P.pi[(size_t)s * P.nq + j] = mc[w0][ql] + mc[w0 + 1][ql];
            P.pf[(size_t)s * P.nq + j] = fminf(mm[w0][ql], mm[w0 + 1][ql]);
        }
    }
}

__global__ __launch_bounds__(256) void ball_final_k(const int* __restrict__ pi, const float* __restrict__ pf, int m, int S,
                                                    int* __restrict__ cnt, float* __restrict__ min2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    int c = 0;
    float v = INFINITY;
    for (int s = 0; s < S; ++s) {
        c += pi[(size_t)s * m + j];
        v = fminf(v, pf[(size_t)s * m + j]);
    }
    cnt[j] = c;
    min2[j] = v;
}

inline int blocks_of(int rows) { return (rows + BT - 1) / BT; }
// splits of the candidate blocks: about kTargetWgs workgroups, so that a small query set still fills the chip
inline int splits_of(int nbq, int nbc) {
    int S = (kTargetWgs + nbq - 1) / nbq;
    if (S > nbc) S = nbc;
    return S < 1 ? 1 : S;
}
inline bool rows_ok(int n) { return n >= 1 && n <= kMaxRows; }

}  // namespace

extern "C" {

size_t ggan_knn_radii_workspace(int n, int k) {
    if (!rows_ok(n) || k < 1 || k > kMaxK || k > n - 1) return 0;
    const int nb = blocks_of(n);
    return norms_bytes(n) + (size_t)splits_of(nb, nb) * k * n * sizeof(float);
}

int ggan_knn_radii(const float* Z, int n, int d, int k, float* r2, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Z && r2 && ws, "null pointer");
    GGAN_CHECK_ARG(rows_ok(n), "1 <= n <= 131072");
    GGAN_CHECK_ARG(d >= 1, "d < 1");
    GGAN_CHECK_ARG(k >= 1 && k <= kMaxK, "1 <= k <= 8");
    GGAN_CHECK_ARG(k <= n - 1, "k > n - 1: a row has only n - 1 neighbours");
    GGAN_CHECK_ARG(ws_bytes >= ggan_knn_radii_workspace(n, k), "workspace too small (ggan_knn_radii_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    SweepParams P;
    P.X = Z; P.Y = Z; P.m = n; P.T = n; P.d = d;
    P.vec = (d % 4 == 0) && ((uintptr_t)Z & 15) == 0;
    float* norms = (float*)ws;
    P.norms = norms;
    P.rad = nullptr; P.pi = nullptr;
    P.pf = (float*)((char*)ws + norms_bytes(n));
    P.nq = n; P.nc = n; P.c0 = 0;
    P.nbc = blocks_of(n);
    P.S = splits_of(P.nbc, P.nbc);
    hipStream_t st = (hipStream_t)stream;
    GGAN_LAUNCH("knn_norms", 2.0 * n * d, 4.0 * n * d, set_norms_k, dim3(cdiv(n, 4)), dim3(256), 0, st, P, norms);
    const double tiles = (double)P.nbc * P.nbc;
    const double flops = tiles * 2.0 * BT * BT * d, bytes = tiles * 2.0 * BT * d * 4.0;
    const dim3 grid(P.nbc, P.S);
#define RADII_CASE(K)                                                                                                                  \
    case K:                                                                                                                            \
        if (P.vec) { GGAN_LAUNCH("knn_radii", flops, bytes, (knn_radii_k<K, true>), grid, dim3(256), 0, st, P); }                      \
        else { GGAN_LAUNCH("knn_radii", flops, bytes, (knn_radii_k<K, false>), grid, dim3(256), 0, st, P); }                           \
        GGAN_LAUNCH("knn_final", 0, 4.0 * P.S * K * n, knn_final_k<K>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float*)P.pf, n,    \
                    P.S, r2);                                                                                                          \
        break;
    switch (k) {
        RADII_CASE(1) RADII_CASE(2) RADII_CASE(3) RADII_CASE(4) RADII_CASE(5) RADII_CASE(6) RADII_CASE(7) RADII_CASE(8)
    }
#undef RADII_CASE
    return 0;
}

size_t ggan_ball_counts_workspace(int m, int n) {
    if (!rows_ok(m) || !rows_ok(n)) return 0;
    const int S = splits_of(blocks_of(m), blocks_of(n));
    return norms_bytes((long)m + n) + 2 * (((size_t)S * m * 4 + 15) & ~(size_t)15);
}

int ggan_ball_counts(const float* A, const float* B, int m, int n, int d, const float* rB2, int* cnt, float* min2, void* ws,
                     size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(A && B && rB2 && cnt && min2 && ws, "null pointer");
    GGAN_CHECK_ARG(rows_ok(m) && rows_ok(n), "1 <= m, n <= 131072");
    GGAN_CHECK_ARG(d >= 1, "d < 1");
    GGAN_CHECK_ARG(ws_bytes >= ggan_ball_counts_workspace(m, n), "workspace too small (ggan_ball_counts_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    SweepParams P;
    P.X = A; P.Y = B; P.m = m; P.T = m + n; P.d = d;              // Z = [A; B]: the queries first, the candidates behind them
    P.vec = (d % 4 == 0) && ((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0;
    float* norms = (float*)ws;
    P.norms = norms;
    P.rad = rB2;
    P.nq = m; P.nc = n; P.c0 = m;
    P.nbc = blocks_of(n);
    const int nbq = blocks_of(m);
    P.S = splits_of(nbq, P.nbc);
    const size_t part = ((size_t)P.S * m * 4 + 15) & ~(size_t)15;
    P.pf = (float*)((char*)ws + norms_bytes((long)m + n));
    P.pi = (int*)((char*)P.pf + part);
    hipStream_t st = (hipStream_t)stream;
    GGAN_LAUNCH("ball_norms", 2.0 * P.T * d, 4.0 * P.T * d, set_norms_k, dim3(cdiv(P.T, 4)), dim3(256), 0, st, P, norms);
    const double tiles = (double)nbq * P.nbc;
    const double flops = tiles * 2.0 * BT * BT * d, bytes = tiles * 2.0 * BT * d * 4.0;
    if (P.vec) { GGAN_LAUNCH("ball_counts", flops, bytes, ball_counts_k<true>, dim3(nbq, P.S), dim3(256), 0, st, P); }
    else { GGAN_LAUNCH("ball_counts", flops, bytes, ball_counts_k<false>, dim3(nbq, P.S), dim3(256), 0, st, P); }
    GGAN_LAUNCH("ball_final", 0, 8.0 * P.S * m, ball_final_k, dim3(cdiv(m, 256)), dim3(256), 0, st, (const int*)P.pi, (const float*)P.pf,
                m, P.S, cnt, min2);
    return 0;
}

}  // extern "C"
