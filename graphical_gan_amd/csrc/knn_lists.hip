// Labelled neighbour lists across two row sets (include/ggan.h):
//   ggan_knn_lists  idx[i, 0..k) = the k candidates c_j nearest to query q_i, ascending in the TOTAL order (D(i, j), j) -- a tie in distance
//                   goes to the lower candidate index --, d2[i, 0..k) their squared distances; skip_diag leaves out j == i by index;
//   ggan_knn_vote   pred[i] = the label most frequent among labels_c[idx[i, :]] (a tied vote to the smallest label), the correct count
//                   and the confusion matrix against labels_q.
// The sweep is knn_sets.hip's: 128 x 128 Gram tiles (set_rows.h), the QUERY rows on the MFMA's N side, so that a lane owns one query per
// 32-wide block column -- two per 64 x 64 wave tile -- for the whole sweep, grid (query blocks, S splits of the candidate blocks).  What a
// lane keeps per owned query is a sorted list of K 64-bit KEYS
//   key = (bit pattern of D) << 32 | candidate index
// D = max(n_i + n_j - 2 g_ij, 0) is a non-negative float (never -0: n_i + n_j >= +0 and an exact zero of a round-to-nearest sum is +0),
// whose bit pattern orders like its value, so one unsigned 64-bit compare IS the pair order, and the insert / merge networks of
// knn_sets.hip carry over with min / max on keys.  Keys of distinct candidates are distinct, so the K smallest of a set of keys do not
// depend on the order they are met in: lane halves, wave pairs and split partials are merged by the same insert, and the result is the
// same for every launch shape.  A candidate left out -- a ghost row of a ragged tile, j == i under skip_diag -- gets the key ~0, above
// every real one (a real key's upper word is at most the bit pattern of +inf); with k <= the number of real candidates it never reaches
// an output.  No floating-point atomics: two calls give the same bits.
#include "common.h"
#include "set_rows.h"
using namespace ggan;

namespace {

typedef unsigned long long nkey;
constexpr int kMaxK = 8;
constexpr int kTargetWgs = 2048;
constexpr int kMaxClasses = 1024;
constexpr nkey kNoKey = ~(nkey)0;

struct ListParams : RowSets {      // Z = [Q; C]: queries rows [0, nq), candidates rows [c0, c0 + nc)
    nkey* pk;                     // partials [S][K][nq]
    int nq, nc, c0;
    int nbc, S;                    // candidate blocks, splits of them
    int skip;                      // leave out candidate j == query i (nq == nc)
};

__device__ __forceinline__ nkey kmin(nkey a, nkey b) { return a < b ? a : b; }
__device__ __forceinline__ nkey kmax(nkey a, nkey b) { return a < b ? b : a; }

// v into the ascending list L of the K smallest keys seen so far (knn_sets.hip's list_insert on keys)
template <int K>
__device__ __forceinline__ void key_insert(nkey (&L)[K], nkey v) {
    if (v < L[K - 1]) {
#pragma unroll
        for (int q = K - 1; q > 0; --q) L[q] = kmax(L[q - 1], kmin(L[q], v));
        L[0] = kmin(L[0], v);
    }
}

__device__ __forceinline__ nkey key_shfl_xor(nkey v, int mask) {
    const unsigned lo = __shfl_xor((unsigned)v, mask, 64), hi = __shfl_xor((unsigned)(v >> 32), mask, 64);
    return ((nkey)hi << 32) | lo;
}

template <int K, bool VEC>
__global__ __launch_bounds__(256, 2) void knn_lists_k(const ListParams P) {
    warm_kernarg(P);
    __shared__ __attribute__((aligned(16))) float As[2][KS * LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][KS * LD];
    __shared__ float nC[BT], nQ[BT];
    __shared__ nkey mg[4][64][K];                       // the waves' lists, one per owned query
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1, half = lane >> 5, l31 = lane & 31;
    const int r0q = blockIdx.x * BT, s = blockIdx.y;
    nkey L[2][K];
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int q = 0; q < K; ++q) L[bj][q] = kNoKey;

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
            const int jl = wn * 64 + bj * 32 + l31;
            const int jskip = P.skip ? r0q + jl : -1;    // the candidate index this query leaves out
            const float nj = nQ[jl];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int il = wm * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * half, i = r0c + il;
                    const float dist = fmaxf(nC[il] + nj - 2.f * acc[bi][bj][r], 0.f);
                    const nkey key = ((nkey)__float_as_uint(dist) << 32) | (unsigned)i;
                    key_insert<K>(L[bj], (i < P.nc && i != jskip) ? key : kNoKey);
                }
            }
        }
        __syncthreads();                                   // nC / nQ are rewritten by the next tile
    }

    // lanes l and l ^ 32 own the same queries (other candidates): each takes the other's list
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        nkey o[K];
#pragma unroll
        for (int q = 0; q < K; ++q) o[q] = key_shfl_xor(L[bj][q], 32);
#pragma unroll
        for (int q = 0; q < K; ++q) key_insert<K>(L[bj], o[q]);
        if (half == 0) {
#pragma unroll
            for (int q = 0; q < K; ++q) mg[wave][bj * 32 + l31][q] = L[bj][q];
        }
    }
    __syncthreads();
    // waves (0, wn) and (1, wn) own the same 64 queries: thread ql < 128 merges the pair of query ql and writes the workgroup's list
    if (tid < BT) {
        const int w0 = 2 * (tid >> 6), ql = tid & 63, j = r0q + tid;
        nkey a[K];
#pragma unroll
        for (int q = 0; q < K; ++q) a[q] = mg[w0][ql][q];
#pragma unroll
        for (int q = 0; q < K; ++q) key_insert<K>(a, mg[w0 + 1][ql][q]);
        if (j < P.nq) {
#pragma unroll
            for (int q = 0; q < K; ++q) P.pk[((size_t)s * K + q) * P.nq + j] = a[q];
        }
    }
}

// row j: the S partial lists merged, indices (and distances) out
template <int K>
__global__ __launch_bounds__(256) void knn_lists_final_k(const nkey* __restrict__ part, int m, int S, int* __restrict__ idx,
                                                         float* __restrict__ d2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    nkey L[K];
#pragma unroll
    for (int q = 0; q < K; ++q) L[q] = kNoKey;
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int q = 0; q < K; ++q) key_insert<K>(L, part[((size_t)s * K + q) * m + j]);
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {
        idx[(size_t)j * K + q] = (int)(unsigned)L[q];
        if (d2) d2[(size_t)j * K + q] = __uint_as_float((unsigned)(L[q] >> 32));
    }
}

// one thread per list: equal labels counted pairwise (k <= 8), the largest count wins, the smaller label on equal counts
__global__ __launch_bounds__(256) void knn_vote_k(const int* __restrict__ idx, const int* __restrict__ labels_c,
                                                  const int* __restrict__ labels_q, int m, int k, int classes, int* __restrict__ pred,
                                                  int* __restrict__ correct, int* __restrict__ confusion) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    if (i < m) {
        int l[kMaxK];
#pragma unroll
        for (int q = 0; q < kMaxK; ++q) l[q] = q < k ? labels_c[idx[(size_t)i * k + q]] : 0;
        int best = l[0], votes = 0;
#pragma unroll
        for (int q = 0; q < kMaxK; ++q) {
            int c = 0;
#pragma unroll
            for (int p = 0; p < kMaxK; ++p) c += (p < k && l[p] == l[q]) ? 1 : 0;
            if (q < k && (c > votes || (c == votes && l[q] < best))) { votes = c; best = l[q]; }
        }
        pred[i] = best;
        if (labels_q) {
            const int lq = labels_q[i];
            hit = best == lq;
            if (confusion && lq >= 0 && lq < classes && best >= 0 && best < classes) atomicAdd(&confusion[lq * classes + best], 1);
        }
    }
    if (correct) {
        const int hits = __popcll(__ballot(hit));
        if ((threadIdx.x & 63) == 0 && hits) atomicAdd(correct, hits);
    }
}

inline int blocks_of(int rows) { return (rows + BT - 1) / BT; }
// splits of the candidate blocks: about kTargetWgs workgroups, so that a small query set still fills the chip (as knn_sets.hip)
inline int splits_of(int nbq, int nbc) {
    int S = (kTargetWgs + nbq - 1) / nbq;
    if (S > nbc) S = nbc;
    return S < 1 ? 1 : S;
}
inline bool rows_ok(int n) { return n >= 1 && n <= kMaxRows; }

}  // namespace

extern "C" {

size_t ggan_knn_lists_workspace(int m, int n, int k) {
    if (!rows_ok(m) || !rows_ok(n) || k < 1 || k > kMaxK || k > n) return 0;
    return norms_bytes((long)m + n) + (size_t)splits_of(blocks_of(m), blocks_of(n)) * k * m * sizeof(nkey);
}

int ggan_knn_lists(const float* Q, const float* C, int m, int n, int d, int k, int skip_diag, int* idx, float* d2, void* ws,
                   size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Q && C && idx && ws, "null pointer");
    GGAN_CHECK_ARG(rows_ok(m) && rows_ok(n), "1 <= m, n <= 131072");
    GGAN_CHECK_ARG(d >= 1, "d < 1");
    GGAN_CHECK_ARG(k >= 1 && k <= kMaxK, "1 <= k <= 8");
    GGAN_CHECK_ARG(!skip_diag || m == n, "skip_diag needs m == n");
    GGAN_CHECK_ARG(k <= n - (skip_diag ? 1 : 0), "k > n - skip_diag: a query has fewer candidates than that");
    GGAN_CHECK_ARG(ws_bytes >= ggan_knn_lists_workspace(m, n, k), "workspace too small (ggan_knn_lists_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    ListParams P;
    P.X = Q; P.Y = C; P.m = m; P.T = m + n; P.d = d;              // Z = [Q; C]: the queries first, the candidates behind them
    P.vec = (d % 4 == 0) && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)C & 15) == 0;
    float* norms = (float*)ws;
    P.norms = norms;
    P.pk = (nkey*)((char*)ws + norms_bytes((long)m + n));
    P.nq = m; P.nc = n; P.c0 = m;
    P.nbc = blocks_of(n);
    const int nbq = blocks_of(m);
    P.S = splits_of(nbq, P.nbc);
    P.skip = skip_diag ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    GGAN_LAUNCH("knn_lists_norms", 2.0 * P.T * d, 4.0 * P.T * d, set_norms_k, dim3(cdiv(P.T, 4)), dim3(256), 0, st, P, norms);
    const double tiles = (double)nbq * P.nbc;
    const double flops = tiles * 2.0 * BT * BT * d, bytes = tiles * 2.0 * BT * d * 4.0;
    const dim3 grid(nbq, P.S);
#define LISTS_CASE(K)                                                                                                                  \
    case K:                                                                                                                            \
        if (P.vec) { GGAN_LAUNCH("knn_lists", flops, bytes, (knn_lists_k<K, true>), grid, dim3(256), 0, st, P); }                      \
        else { GGAN_LAUNCH("knn_lists", flops, bytes, (knn_lists_k<K, false>), grid, dim3(256), 0, st, P); }                           \
        GGAN_LAUNCH("knn_lists_final", 0, 8.0 * P.S * K * m, knn_lists_final_k<K>, dim3(cdiv(m, 256)), dim3(256), 0, st,               \
                    (const nkey*)P.pk, m, P.S, idx, d2);                                                                              \
        break;
    switch (k) {
        LISTS_CASE(1) LISTS_CASE(2) LISTS_CASE(3) LISTS_CASE(4) LISTS_CASE(5) LISTS_CASE(6) LISTS_CASE(7) LISTS_CASE(8)
    }
#undef LISTS_CASE
    return 0;
}

int ggan_knn_vote(const int* idx, const int* labels_c, const int* labels_q, int m, int k, int classes, int* pred, int* correct,
                  int* confusion, ggan_stream_t stream) {
    GGAN_CHECK_ARG(idx && labels_c && pred, "null pointer");
    GGAN_CHECK_ARG(rows_ok(m), "1 <= m <= 131072");
    GGAN_CHECK_ARG(k >= 1 && k <= kMaxK, "1 <= k <= 8");
    GGAN_CHECK_ARG(labels_q || (!correct && !confusion), "correct / confusion need labels_q");
    GGAN_CHECK_ARG(!confusion || (classes >= 1 && classes <= kMaxClasses), "1 <= classes <= 1024 with a confusion matrix");
    GGAN_LAUNCH("knn_vote", 0, 4.0 * m * (2.0 * k + 2), knn_vote_k, dim3(cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, idx, labels_c,
                labels_q, m, k, classes, pred, correct, confusion);
    return 0;
}

}  // extern "C"
