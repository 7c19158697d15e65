// Labelled neighbour lists across two row sets (include/ggan.h):
//   ggan_knn_lists  idx[i, 0..k) = the k candidates c_j nearest to query q_i, ascending in the TOTAL order (D(i, j), j) -- a tie in distance
//                   goes to the lower candidate index --, d2[i, 0..k) their squared distances; skip_diag leaves out j == i by index;
//   ggan_knn_vote   pred[i] = the label most frequent among labels_c[idx[i, :]] (a tied vote to the smallest label), the correct count
//                   and the confusion matrix against labels_q.
// The sweep is knn_sets.hip's (sweep_tiles of set_rows.h: 128 x 128 Gram tiles), the QUERY rows on the MFMA's N side, so that a lane owns
// one query per 32-wide block column -- two per 64 x 64 wave tile -- for the whole sweep, grid (query blocks, S splits of the candidate
// blocks).  What a lane keeps per owned query is a sorted list of K 64-bit KEYS
//   key = (bit pattern of D) << 32 | candidate index
// D = max(n_i + n_j - 2 g_ij, 0) is a non-negative float (never -0: n_i + n_j >= +0 and an exact zero of a round-to-nearest sum is +0),
// whose bit pattern orders like its value, so one unsigned 64-bit compare IS the pair order, and the insert / merge networks of
// set_rows.h (list_insert, lists_store) carry over with min / max on keys.  Keys of distinct candidates are distinct, so the K smallest
// of a set of keys do not depend on the order they are met in: lane halves, wave pairs and split partials are merged by the same
// insert, and the result is the same for every launch shape.  A candidate left out -- a ghost row of a ragged tile, j == i under skip_diag -- gets the key ~0, above
// every real one (a real key's upper word is at most the bit pattern of +inf); with k <= the number of real candidates it never reaches
// an output.  No floating-point atomics: two calls give the same bits.
#include "common.h"
#include "set_rows.h"
using namespace ggan;

namespace {

constexpr int kMaxK = 8;
constexpr int kMaxClasses = 1024;

struct ListParams : SweepParams {  // (set_rows.h: Z = [Q; C], queries and candidates, the splits)
    nkey* pk;                      // partials [S][K][nq]
    int skip;                      // leave out candidate j == query i (nq == nc)
};

template <int K, bool VEC>
__global__ __launch_bounds__(256, 2) void knn_lists_k(const ListParams P) {
    warm_kernarg(P);
    const int r0q = blockIdx.x * BT;
    nkey L[2][K];
    list_clear(L[0]);
    list_clear(L[1]);
    sweep_tiles<VEC, 0>(P, nullptr, [&](int r0c, f32x16 (&acc)[2][2], const float (&ni)[2][16], const float (&nj)[2], const float (&)[1][BT]) {
        for_each_acc([&](int il, int jl, int bi, int bj, int r) {
            const int i = r0c + il;
            const int jskip = P.skip ? r0q + jl : -1;    // the candidate index this query leaves out
            const float dist = gram_dist(ni[bi][r], nj[bj], acc[bi][bj][r]);
            const nkey key = ((nkey)__float_as_uint(dist) << 32) | (unsigned)i;
            list_insert<K>(L[bj], (i < P.nc && i != jskip) ? key : list_top<nkey>());
        });
    });
    lists_store<K>(L, P.pk, P.nq);
}

// row j: the S partial lists merged, indices (and distances) out
template <int K>
__global__ __launch_bounds__(256) void knn_lists_final_k(const nkey* __restrict__ part, int m, int S, int* __restrict__ idx,
                                                         float* __restrict__ d2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    nkey L[K];
    lists_merge_splits<K>(part, m, S, j, L);
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
    SweepLaunch L;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = sweep_setup(P, L, "knn_lists_norms", Q, C, m, n, d, ws, st)) return rc;
    P.pk = (nkey*)L.part;
    P.skip = skip_diag ? 1 : 0;
    return dispatch_k_vec(k, P.vec, [&](auto K, auto VEC) {
        constexpr int kk = decltype(K)::value;
        if (trace_sets_on()) trace_sweep("knn_lists", kk, decltype(VEC)::value, P, L.grid);
        GGAN_LAUNCH("knn_lists", L.flops, L.bytes, (knn_lists_k<kk, decltype(VEC)::value>), L.grid, dim3(256), 0, st, P);
        GGAN_LAUNCH("knn_lists_final", 0, 8.0 * P.S * kk * m, knn_lists_final_k<kk>, dim3(cdiv(m, 256)), dim3(256), 0, st, (const nkey*)P.pk, m,
                    P.S, idx, d2);
        return 0;
    });
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
