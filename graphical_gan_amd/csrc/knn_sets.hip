// k-NN balls of row sets: the two primitives behind improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage
// (Naeem et al. 2020), include/ggan.h.  With squared Euclidean distances D(a, b) = ||a - b||^2:
//   ggan_knn_radii    r2[i] = the k-th smallest of { D(z_i, z_l) : l != i }          (a multiset order statistic, self left out by INDEX)
//   ggan_ball_counts  cnt[a] = #{ j : D(a, b_j) <= rB2[j] },  min2[a] = min_j D(a, b_j)
// Both sweep the 128 x 128 Gram tiles of set_rows.h (gram_tile: 16 k per step, 2 x 2 waves of 64 x 64, four 32x32x2 fp32 accumulators per
// wave, branch-free clamped loads, norms from a pre-pass), distances as max(n_i + n_j - 2 g_ij, 0); nothing of size rows^2 reaches memory.
//
// Orientation (sweep_tiles): the QUERY rows (the rows a result is written for) are the MFMA's N side, the CANDIDATE rows its M side, so
// by the accumulator layout (for_each_acc) a lane owns ONE query per block column -- two per 64 x 64 wave tile -- and sees 32 candidates
// of each per tile.  What it keeps per owned query lives in registers across the whole sweep: the K smallest distances so far (a sorted
// list, K a template argument, every index a compile-time constant), or a count and a minimum.  Every query block sweeps all candidate
// blocks (no symmetric half: every row needs its own list); grid (query blocks, S): workgroup (b, s) takes the candidate blocks s,
// s + S, ...  After the sweep -- once per workgroup, not per tile -- the two lane halves that share a query are merged by a lane
// exchange, the two waves that share it through LDS (lists_store), and the workgroup leaves one partial per query and split; a last
// small kernel merges the S partials of each row.
//
// Candidates are left out by index, never by value: l == i (radii), and rows beyond the set (the tile's ghost rows).  Lists are merged
// as multisets (a duplicate row counts), counts are integers, minima are order-free: no floating-point atomics anywhere, and two calls
// give the same bits.
#include "common.h"
#include "set_rows.h"
using namespace ggan;

namespace {

constexpr int kMaxK = 8;

struct BallParams : SweepParams {  // (set_rows.h: the row list, queries and candidates, the splits)
    const float* rad;              // ball_counts: [nc] squared radii of the candidates
    float* pf;                     // partials: radii [S][K][nq] lists, ball_counts [S][nq] minima
    int* pi;                       // ball_counts: [S][nq] counts
};

template <int K, bool VEC>
__global__ __launch_bounds__(256, 2) void knn_radii_k(const BallParams P) {
    warm_kernarg(P);
    const int r0q = blockIdx.x * BT;
    float L[2][K];
    list_clear(L[0]);
    list_clear(L[1]);
    sweep_tiles<VEC, 0>(P, nullptr, [&](int r0c, f32x16 (&acc)[2][2], const float (&ni)[2][16], const float (&nj)[2], const float (&)[1][BT]) {
        for_each_acc([&](int il, int jl, int bi, int bj, int r) {
            const int i = r0c + il, j = r0q + jl;
            const float dist = gram_dist(ni[bi][r], nj[bj], acc[bi][bj][r]);
            const bool real = (i < P.nc) & (P.c0 + i != j);     // (`&`: one select, where `&&` compiled to a branch around the distance)
            list_insert<K>(L[bj], real ? dist : INFINITY);
        });
    });
    lists_store<K>(L, P.pf, P.nq);
}

// row j: the S partial lists merged, the K-th value out
template <int K>
__global__ __launch_bounds__(256) void knn_final_k(const float* __restrict__ part, int n, int S, float* __restrict__ r2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float L[K];
    lists_merge_splits<K>(part, n, S, j, L);
    r2[j] = L[K - 1];
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void ball_counts_k(const BallParams P) {
    warm_kernarg(P);
    __shared__ int mc[4][64];
    __shared__ float mm[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int r0q = blockIdx.x * BT, s = blockIdx.y;
    int cnt[2] = {0, 0};
    float mn[2] = {INFINITY, INFINITY};
    // the candidates' radii are staged with their norms: cand[1]
    sweep_tiles<VEC, 1>(P, P.rad, [&](int r0c, f32x16 (&acc)[2][2], const float (&ni)[2][16], const float (&nj)[2], const float (&cand)[2][BT]) {
        for_each_acc([&](int il, int jl, int bi, int bj, int r) {
            const bool ok = r0c + il < P.nc;
            const float dist = gram_dist(ni[bi][r], nj[bj], acc[bi][bj][r]);
            cnt[bj] += (ok && dist <= cand[1][il]) ? 1 : 0;
            mn[bj] = fminf(mn[bj], ok ? dist : INFINITY);
        });
    });

    // lane halves, then the two waves of a query through LDS (as lists_store)
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
    BallParams P;
    SweepLaunch L;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = sweep_setup(P, L, "knn_norms", Z, nullptr, n, n, d, ws, st)) return rc;
    P.rad = nullptr; P.pi = nullptr;
    P.pf = (float*)L.part;
    return dispatch_k_vec(k, P.vec, [&](auto K, auto VEC) {
        constexpr int kk = decltype(K)::value;
        if (trace_sets_on()) trace_sweep("knn_radii", kk, decltype(VEC)::value, P, L.grid);
        GGAN_LAUNCH("knn_radii", L.flops, L.bytes, (knn_radii_k<kk, decltype(VEC)::value>), L.grid, dim3(256), 0, st, P);
        GGAN_LAUNCH("knn_final", 0, 4.0 * P.S * kk * n, knn_final_k<kk>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float*)P.pf, n, P.S, r2);
        return 0;
    });
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
    BallParams P;
    SweepLaunch L;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = sweep_setup(P, L, "ball_norms", A, B, m, n, d, ws, st)) return rc;
    P.rad = rB2;
    P.pf = (float*)L.part;
    P.pi = (int*)((char*)L.part + (((size_t)P.S * m * 4 + 15) & ~(size_t)15));
    if (const int rc = dispatch_vec(P.vec, [&](auto VEC) {
            if (trace_sets_on()) trace_sweep("ball_counts", 0, decltype(VEC)::value, P, L.grid);
            GGAN_LAUNCH("ball_counts", L.flops, L.bytes, ball_counts_k<decltype(VEC)::value>, L.grid, dim3(256), 0, st, P);
            return 0;
        }))
        return rc;
    GGAN_LAUNCH("ball_final", 0, 8.0 * P.S * m, ball_final_k, dim3(cdiv(m, 256)), dim3(256), 0, st, (const int*)P.pi, (const float*)P.pf,
                m, P.S, cnt, min2);
    return 0;
}

}  // extern "C"
