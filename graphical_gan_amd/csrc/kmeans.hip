// k-means fitted on the device, and the two scores read off a fitted partition (include/ggan.h):
//   ggan_kmeans_seed     k-means++ seeding from k host-drawn uniforms: per step one wave-per-row distance-to-one-centre launch that lowers
//                        mind[r], the smallest squared distance of row r to the centres chosen so far, and one one-workgroup pick launch;
//   ggan_kmeans_pick     the pick alone: the first row whose running fp64 sum of mind exceeds u * total;
//   ggan_kmeans_assign   nearest centre per row, a tie in distance to the LOWER centre index, the squared distance, the inertia, the rows that
//                        moved, the bin counts;
//   ggan_kmeans_update   centre c = the mean of its members, an empty cluster keeps the centre it had;
//   ggan_kmeans_fit      seed, `iters` times (assign, update), a final assign: a fixed number of launches and no host synchronisation;
//   ggan_bin_test        NDB: the bins whose two-proportion z statistic exceeds a threshold, their share, the Jensen-Shannon divergence;
//   ggan_cluster_scores  purity and normalised mutual information of an assignment against labels.
// The assignment is the query / candidate sweep of set_rows.h with the rows as queries and the centres as the ONE candidate block
// (k <= 128 = BT), the epilogue a K = 1 list of knn_lists.hip's keys (distance bits << 32 | centre index): one unsigned compare is the
// order (distance, index), so a tie goes to the lower centre whatever order the candidates are met in.  A ghost candidate row beyond k
// gets the key ~0 and never wins.  fmaxf drops a NaN, so a non-finite row would show as the distance 0: what is tested instead is the
// squared NORM of every row and every centre, which is non-finite exactly where a distance can be.
// The centre update is the transpose, a reduction over the row index at any width: the rows are cut into blocks of GGAN_KMEANS_ROW_BLOCK,
// a workgroup sums one (row block, 128 columns) as onehot(assign)^T X by v_mfma_f32_32x32x2_f32 -- every product is x * 1 or x * 0, so a
// block partial is the fp32 sum of the block's members in row order --, and a second launch adds the block partials in fp64 in block
// order and divides.  0 * inf is NaN: a non-finite row spoils every centre of its block.  That is acceptable only because the assign step
// that produced the assignment has already raised GGAN_KMEANS_NONFINITE for it.
// Determinism: no floating-point atomic (integer atomics on counters and status words only), every floating-point sum in an order fixed
// by constants of this file, one launch is one phase: two calls give the same bits.
#include <math.h>
#include "common.h"
#include "set_rows.h"
using namespace ggan;

namespace {

constexpr int kMaxK = GGAN_KMEANS_MAX_K;
constexpr int kMaxClasses = GGAN_KMEANS_MAX_CLASSES;
constexpr int kURB = GGAN_KMEANS_ROW_BLOCK;   // rows of a block of the update
constexpr int kUC = 128;                      // columns of a workgroup of the update: one 32-wide strip per wave
constexpr int kUK = 32;                       // rows staged per step
constexpr int kULD = kUC + 32;                // staged row (floats): = 32 (mod 64), the two k of a fragment read sit on different banks
constexpr int kUNL = kUK * kUC / 256;         // staged values per thread and step
constexpr int kPickChunk = 1024;              // rows per chunk of the pick
constexpr int kPickChunks = kMaxRows / kPickChunk;
static_assert(kMaxK == BT, "the centres are ONE candidate block of the sweep");
static_assert(kMaxK == 128 && kMaxClasses <= 64, "the finishing workgroups keep one slot per centre / class");
static_assert(kURB % kUK == 0 && kUK % 2 == 0 && kUNL * 256 == kUK * kUC, "the update's staging");

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
inline int update_blocks(int n) { return cdiv(n, kURB); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- norms ---------------------------------------------------------------------------------------------------------------------------------
// set_norms_k of set_rows.h from row r0 on: the rows X keep their norms over a whole fit, only the centres' are formed again
__global__ __launch_bounds__(256) void kmeans_norms_k(const RowSets P, float* __restrict__ norms, int r0) {
    const int r = r0 + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= P.T) return;
    const float* z = z_row(P, r);
    float s = 0.f;
    for (int k = lane; k < P.d; k += 64) s = fmaf(z[k], z[k], s);
    s = wave_sum(s);
    if (lane == 0) norms[r] = s;
}

// ---- seeding -------------------------------------------------------------------------------------------------------------------------------
// one wave per row: mind[r] = min(mind[r], D(r, centre idx[t])) in float32 Gram form clamped at 0 (t == 0: = D).  The dot product is summed
// as kmeans_norms_k sums a norm, so the chosen row itself gets n + n - 2 n = 0 exactly.
__global__ __launch_bounds__(256) void kmeans_mind_k(const float* __restrict__ X, const float* __restrict__ norms, const int* __restrict__ idx,
                                                     int t, int n, int d, float* __restrict__ mind) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n) return;
    const int c = min(max(idx[t], 0), n - 1);
    const float* x = X + (size_t)r * d;
    const float* y = X + (size_t)c * d;
    float s = 0.f;
    for (int k = lane; k < d; k += 64) s = fmaf(x[k], y[k], s);
    s = wave_sum(s);
    if (lane == 0) {
        const float dist = gram_dist(norms[r], norms[c], s);
        mind[r] = t == 0 ? dist : fminf(mind[r], dist);
    }
}

// one workgroup: the pick of step t.  first: row floor(u n).  Else chunk sums of mind in fp64 (chunk c by wave c % 4, lane-strided, the
// wave's butterfly), a serial scan of the chunk sums, and a walk of the ONE chunk that holds the boundary, 64 rows at a time: the first
// row whose running sum exceeds u * total.  total == 0 (every row coincides with a centre), or a total that is not a positive finite
// number: row floor(u n).  Where rounding leaves no row above the target, the last row with a positive mind.  The index never leaves
// [0, n).  X != nullptr: the row is copied to centres[t].
__global__ __launch_bounds__(256) void kmeans_pick_k(const float* __restrict__ mind, int n, const double* __restrict__ u, int t, int first,
                                                     const float* __restrict__ X, int d, float* __restrict__ centres, int* __restrict__ idx) {
    __shared__ double cs[kPickChunks];
    __shared__ int pick_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = (n + kPickChunk - 1) / kPickChunk;
    if (!first) {
        for (int c = wave; c < nch; c += 4) {
            const int e = min(n, (c + 1) * kPickChunk);
            double s = 0.0;
            for (int r = c * kPickChunk + lane; r < e; r += 64) s += (double)mind[r];
            s = wave_sum_f64(s);
            if (lane == 0) cs[c] = s;
        }
    }
    __syncthreads();
    if (wave == 0) {
        const double ut = u[t];
        int pick = (int)floor(ut * (double)n);
        pick = min(max(pick, 0), n - 1);
        if (!first) {
            double total = 0.0;
            for (int c = 0; c < nch; ++c) total += cs[c];
            if (total > 0.0) {                                  // (false for NaN)
                double target = ut * total, run = 0.0, base = 0.0;
                int cf = -1, lastpos = -1;
                for (int c = 0; c < nch; ++c) {
                    if (cf < 0 && run + cs[c] > target) { cf = c; base = run; }
                    if (cs[c] > 0.0) lastpos = c;
                    run += cs[c];
                }
                if (cf < 0) { cf = lastpos; target = INFINITY; base = 0.0; }     // nothing above the target: the last positive row
                if (cf >= 0) {
                    const int e = min(n, (cf + 1) * kPickChunk);
                    int found = -1, last = -1;
                    for (int r0 = cf * kPickChunk; r0 < e && found < 0; r0 += 64) {
                        const int r = r0 + lane;
                        const double v = r < e ? (double)mind[r] : 0.0;
                        double inc = v;
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const double up = __shfl_up(inc, o, 64);
                            if (lane >= o) inc += up;
                        }
                        const unsigned long long hit = __ballot(base + inc > target), pos = __ballot(v > 0.0);
                        if (pos) last = r0 + 63 - __clzll((long long)pos);
                        if (hit) found = r0 + __ffsll((long long)hit) - 1;
                        base += __shfl(inc, 63, 64);
                    }
                    if (found >= 0) pick = found;
                    else if (last >= 0) pick = last;
                }
            }
        }
        if (lane == 0) pick_s = min(max(pick, 0), n - 1);
    }
    __syncthreads();
    const int p = pick_s;
    if (tid == 0) idx[t] = p;
    if (X) {
        for (int c = tid; c < d; c += 256) centres[(size_t)t * d + c] = X[(size_t)p * d + c];
    }
}

// ---- assignment ----------------------------------------------------------------------------------------------------------------------------
struct AssignParams : SweepParams {
    nkey* pk;                      // the one list per row [1][1][nq]
};

template <bool VEC>
__global__ __launch_bounds__(256, 2) void kmeans_assign_k(const AssignParams P) {
    warm_kernarg(P);
    nkey L[2][1];
    list_clear(L[0]);
    list_clear(L[1]);
    sweep_tiles<VEC, 0>(P, nullptr, [&](int r0c, f32x16 (&acc)[2][2], const float (&ni)[2][16], const float (&nj)[2], const float (&)[1][BT]) {
        for_each_acc([&](int il, int jl, int bi, int bj, int r) {
            const int i = r0c + il;
            const float dist = gram_dist(ni[bi][r], nj[bj], acc[bi][bj][r]);
            const nkey key = ((nkey)__float_as_uint(dist) << 32) | (unsigned)i;
            list_insert<1>(L[bj], i < P.nc ? key : list_top<nkey>());
        });
    });
    lists_store<1>(L, P.pk, P.nq);
}

// row j: its key taken apart; the rows that moved, the bin counts (an LDS histogram first) and the status word by integer atomics
__global__ __launch_bounds__(256) void kmeans_assign_final_k(const nkey* __restrict__ pk, const float* __restrict__ norms, int n, int k,
                                                             const int* prev, int* assign, float* __restrict__ dist, int* __restrict__ moved,
                                                             int* __restrict__ counts, int* __restrict__ status) {
    __shared__ int hist[kMaxK];
    const int tid = threadIdx.x, j = blockIdx.x * 256 + tid;
    if (counts) {
        if (tid < kMaxK) hist[tid] = 0;
        __syncthreads();
    }
    bool bad = false, mv = false;
    if (j < n) {
        const nkey key = pk[j];
        const int a = (int)min((unsigned)key, (unsigned)(k - 1));      // (a real key's index is < k already)
        const float dv = __uint_as_float((unsigned)(key >> 32));
        bad = !isfinite(dv) || !isfinite(norms[j]);
        mv = prev ? prev[j] != a : true;
        assign[j] = a;
        dist[j] = dv;
        if (counts) atomicAdd(&hist[a], 1);
    }
    if (j < k) bad = bad || !isfinite(norms[n + j]);
    const unsigned long long anybad = __ballot(bad), anymv = __ballot(mv);
    if ((tid & 63) == 0) {
        if (anybad) atomicOr(status, GGAN_KMEANS_NONFINITE);
        if (moved && anymv) atomicAdd(moved, __popcll(anymv));
    }
    if (counts) {
        __syncthreads();
        if (tid < k && hist[tid]) atomicAdd(&counts[tid], hist[tid]);
    }
}

// one workgroup: thread t adds dist[t], dist[t + 256], ... in fp64 in that order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void kmeans_inertia_k(const float* __restrict__ dist, int n, double* __restrict__ inertia) {
    __shared__ double ls[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int r = tid; r < n; r += 256) s += (double)dist[r];
    ls[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) ls[tid] += ls[tid + o];
        __syncthreads();
    }
    if (tid == 0) inertia[0] = ls[0];
}

// ---- update --------------------------------------------------------------------------------------------------------------------------------
// workgroup (b, j): rows [b kURB, min((b + 1) kURB, n)), columns [j kUC, (j + 1) kUC), wave w the strip of 32 columns w.  The reduction index
// of every MFMA is the row: lane l holds A[i = l & 31][k = l >> 5] = (assign[row k] == 32 ti + i) and B[k][j = l & 31] = X[row k][column j];
// accumulator ti is the 32 centres 32 ti .. (only those below k are formed).  A ghost row beyond the block is the assignment -1 and zeros.
// part[(b k + c) d + column]; blkcnt[b k + c] = the block's members of centre c (column chunk 0 counts them).
__global__ __launch_bounds__(256) void kmeans_update_part_k(const float* __restrict__ X, const int* __restrict__ assign, int n, int d, int k,
                                                            float* __restrict__ part, int* __restrict__ blkcnt) {
    __shared__ float xs[kUK * kULD];
    __shared__ int as[kUK];
    __shared__ int hist[kMaxK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int b = blockIdx.x, c0 = blockIdx.y * kUC, r0 = b * kURB, r1 = min(r0 + kURB, n);
    const int nti = (k + 31) >> 5;
    if (blockIdx.y == 0) {
        if (tid < kMaxK) hist[tid] = 0;
        __syncthreads();
        for (int r = r0 + tid; r < r1; r += 256) {
            const int a = assign[r];
            if (a >= 0 && a < k) atomicAdd(&hist[a], 1);
        }
        __syncthreads();
        if (tid < k) blkcnt[(size_t)b * k + tid] = hist[tid];
    }
    f32x16 acc[4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ti][r] = 0.f;
    float v[kUNL];
    int av = -1;
    // a step into registers, every address clamped into the matrix and the value dropped afterwards: all loads of the step are in flight at once
    auto load = [&](int rs) {
        const int col = c0 + (tid & (kUC - 1)), cc = min(col, d - 1);
#pragma unroll
        for (int q = 0; q < kUNL; ++q) {
            const int r = rs + (tid >> 7) + 2 * q;
            v[q] = X[(size_t)min(r, n - 1) * d + cc];
        }
        if (tid < kUK) av = assign[min(rs + tid, n - 1)];
#pragma unroll
        for (int q = 0; q < kUNL; ++q) {
            const int r = rs + (tid >> 7) + 2 * q;
            v[q] = (r < r1 && col < d) ? v[q] : 0.f;
        }
        if (tid < kUK) av = rs + tid < r1 ? av : -1;
    };
    load(r0);
    for (int rs = r0; rs < r1; rs += kUK) {                 // (the same trips for the whole workgroup)
        __syncthreads();                                    // the reads of the step before
#pragma unroll
        for (int q = 0; q < kUNL; ++q) xs[((tid >> 7) + 2 * q) * kULD + (tid & (kUC - 1))] = v[q];
        if (tid < kUK) as[tid] = av;
        __syncthreads();
        if (rs + kUK < r1) load(rs + kUK);                  // in flight while the MFMA block runs
#pragma unroll
        for (int kk = 0; kk < kUK; kk += 2) {
            const int kx = kk + half;
            const float bv = xs[kx * kULD + wave * 32 + l31];
            const int a = as[kx];
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) {
                if (ti < nti)                               // (workgroup-uniform)
                    acc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(a == ti * 32 + l31 ? 1.f : 0.f, bv, acc[ti], 0, 0, 0);
            }
        }
    }
    const int col = c0 + wave * 32 + l31;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        if (ti >= nti) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;          // the 32x32 accumulator map: column = lane & 31
            if (i < k && col < d) part[((size_t)b * k + i) * d + col] = acc[ti][r];
        }
    }
}

// workgroup (c, j): centre c, columns [256 j, 256 (j + 1)): the block partials added in fp64 in block order, over the members' number; an
// empty cluster is left as it is
__global__ __launch_bounds__(256) void kmeans_update_final_k(const float* __restrict__ part, const int* __restrict__ blkcnt, int nblk, int d,
                                                             int k, float* __restrict__ centres, int* __restrict__ counts) {
    const int c = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    int cnt = 0;
    for (int b = 0; b < nblk; ++b) cnt += blkcnt[(size_t)b * k + c];
    if (blockIdx.y == 0 && threadIdx.x == 0) counts[c] = cnt;
    if (col < d && cnt > 0) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += (double)part[((size_t)b * k + c) * d + col];
        centres[(size_t)c * d + col] = (float)(s / (double)cnt);
    }
}

// ---- the two scores ------------------------------------------------------------------------------------------------------------------------
// one workgroup, one thread per bin, all fp64; the three sums by thread 0 in bin order
__global__ __launch_bounds__(kMaxK) void bin_test_k(const int* __restrict__ ca, const int* __restrict__ cb, int k, double zthr,
                                                    double* __restrict__ out) {
    __shared__ double jt[kMaxK];
    __shared__ int df[kMaxK];
    const int tid = threadIdx.x;
    long long s1 = 0, s2 = 0;
    for (int c = 0; c < k; ++c) { s1 += ca[c]; s2 += cb[c]; }
    const double N1 = (double)s1, N2 = (double)s2;
    if (tid < k) {
        const double a = (double)ca[tid], b = (double)cb[tid];
        const double p1 = a / N1, p2 = b / N2, P = (a + b) / (N1 + N2);
        const double se = sqrt(P * (1.0 - P) * (1.0 / N1 + 1.0 / N2));
        df[tid] = (se > 0.0 && fabs(p1 - p2) / se > zthr) ? 1 : 0;
        const double m = 0.5 * (p1 + p2);
        const double t1 = p1 > 0.0 ? p1 * log(p1 / m) : 0.0, t2 = p2 > 0.0 ? p2 * log(p2 / m) : 0.0;
        jt[tid] = 0.5 * t1 + 0.5 * t2;
    }
    __syncthreads();
    if (tid == 0) {
        int nd = 0;
        double js = 0.0;
        for (int c = 0; c < k; ++c) { nd += df[c]; js += jt[c]; }
        const bool empty = s1 <= 0 || s2 <= 0;
        const double nan = __builtin_nan("");
        out[0] = empty ? nan : (double)nd;
        out[1] = empty ? nan : (double)nd / (double)k;
        out[2] = empty ? nan : js;
    }
}

__global__ __launch_bounds__(256) void cluster_table_k(const int* __restrict__ assign, const int* __restrict__ labels, int n, int k, int classes,
                                                       int* __restrict__ table, int* __restrict__ status) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (r < n) {
        const int a = assign[r], y = labels[r];
        bad = a < 0 || a >= k || y < 0 || y >= classes;
        if (!bad) atomicAdd(&table[a * classes + y], 1);
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(status, GGAN_KMEANS_BAD_INDEX);
}

// one workgroup: thread c the cluster c (its size, its largest cell, its share of the mutual information, cells in class order), thread y
// the class sizes; thread 0 adds the clusters in cluster order
__global__ __launch_bounds__(256) void cluster_scores_final_k(const int* __restrict__ table, const int* __restrict__ status, int n, int k,
                                                              int classes, double* __restrict__ out) {
    __shared__ double rowmi[kMaxK];
    __shared__ int rowsum[kMaxK], rowmax[kMaxK], colsum[kMaxClasses];
    const int tid = threadIdx.x;
    const double nn = (double)n;
    if (tid < classes) {
        int s = 0;
        for (int c = 0; c < k; ++c) s += table[c * classes + tid];
        colsum[tid] = s;
    }
    if (tid < k) {
        int s = 0, m = 0;
        for (int y = 0; y < classes; ++y) {
            const int v = table[tid * classes + y];
            s += v;
            m = max(m, v);
        }
        rowsum[tid] = s;
        rowmax[tid] = m;
    }
    __syncthreads();
    if (tid < k) {
        double s = 0.0;
        for (int y = 0; y < classes; ++y) {
            const int v = table[tid * classes + y];
            if (v > 0) s += ((double)v / nn) * log(((double)v * nn) / ((double)rowsum[tid] * (double)colsum[y]));
        }
        rowmi[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double mi = 0.0, hu = 0.0, hv = 0.0;
        long long best = 0;
        for (int c = 0; c < k; ++c) {
            mi += rowmi[c];
            best += rowmax[c];
            if (rowsum[c] > 0) { const double p = (double)rowsum[c] / nn; hu -= p * log(p); }
        }
        for (int y = 0; y < classes; ++y) {
            if (colsum[y] > 0) { const double p = (double)colsum[y] / nn; hv -= p * log(p); }
        }
        const bool bad = status[0] != 0;
        const double nan = __builtin_nan("");
        out[0] = bad ? nan : (double)best / nn;
        out[1] = bad ? nan : ((hu == 0.0 && hv == 0.0) ? 1.0 : mi / (0.5 * (hu + hv)));
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------
inline bool shape_ok(int n, int d, int k) { return rows_ok(n) && d >= 1 && k >= 1 && k <= kMaxK; }

// The workspace, in this order, every piece rounded up to 16 bytes:
//   norms  float [n + k]      the squared norms of the rows and of the centres (the sweep's row list Z = [X; C])
//   keys   nkey [n]           the sweep's one list per row
//   mind   float [n]          the seeding's smallest distances
//   dist   float [n]          the fit's distances
//   part   float [nb k d]     the update's block partials, nb = ceil(n / GGAN_KMEANS_ROW_BLOCK)
//   blkcnt int [nb k]         the blocks' member counts
// GGAN_KMEANS_ROW_BLOCK = 512 is what bounds `part`: 20000 rows of 12288 columns and 128 centres are 40 blocks of 128 * 12288 floats,
// 240 MiB (a block of 256 rows would need 79 blocks, 474 MiB).
struct Workspace {
    float* norms;
    nkey* keys;
    float* mind;
    float* dist;
    float* part;
    int* blkcnt;
    size_t bytes;
};
inline Workspace carve(void* ws, int n, int d, int k) {
    Workspace W;
    const size_t nb = update_blocks(n);
    size_t off = 0;
    auto take = [&](size_t bytes) {                        // (ws == nullptr: the sizes alone)
        void* p = ws ? (char*)ws + off : nullptr;
        off += bytes;
        return p;
    };
    W.norms = (float*)take(norms_bytes((long)n + k));
    W.keys = (nkey*)take(align16((size_t)n * sizeof(nkey)));
    W.mind = (float*)take(align16((size_t)n * sizeof(float)));
    W.dist = (float*)take(align16((size_t)n * sizeof(float)));
    W.part = (float*)take(align16(nb * k * (size_t)d * sizeof(float)));
    W.blkcnt = (int*)take(align16(nb * k * sizeof(int)));
    W.bytes = off;
    return W;
}

inline int zero_async(const char* what, void* p, size_t bytes, hipStream_t st) {
    if (hipMemsetAsync(p, 0, bytes, st) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", what);
        return -2;
    }
    return 0;
}

inline RowSets row_sets(const float* X, const float* C, int n, int k, int d, const float* norms) {
    RowSets R;
    R.X = X; R.Y = C ? C : X; R.m = n; R.T = C ? n + k : n; R.d = d;
    R.vec = (d % 4 == 0) && ((uintptr_t)R.X & 15) == 0 && ((uintptr_t)R.Y & 15) == 0;
    R.norms = norms;
    return R;
}

int seed_launch(const float* X, int n, int d, int k, const double* u, float* centres, int* idx, const Workspace& W, hipStream_t st) {
    const RowSets R = row_sets(X, nullptr, n, 0, d, W.norms);
    GGAN_LAUNCH("kmeans_norms", 2.0 * n * d, 4.0 * n * d, kmeans_norms_k, dim3(cdiv(n, 4)), dim3(256), 0, st, R, W.norms, 0);
    for (int t = 0; t < k; ++t) {
        GGAN_LAUNCH("kmeans_pick", 1.0 * n, 4.0 * n + 8.0 * d, kmeans_pick_k, dim3(1), dim3(256), 0, st, (const float*)W.mind, n, u, t,
                    t == 0 ? 1 : 0, X, d, centres, idx);
        if (t + 1 < k) {
            GGAN_LAUNCH("kmeans_mind", 2.0 * n * d, 4.0 * n * d, kmeans_mind_k, dim3(cdiv(n, 4)), dim3(256), 0, st, X, (const float*)W.norms,
                        (const int*)idx, t, n, d, W.mind);
        }
    }
    return 0;
}

// x_norms: the norms of the rows X are in the workspace already (the seeding, or an earlier assignment of the same fit, left them there)
int assign_launch(const float* X, const float* C, int n, int d, int k, const int* prev, int* assign, float* dist, double* inertia, int* moved,
                  int* counts, int* status, const Workspace& W, bool x_norms, hipStream_t st) {
    AssignParams P;
    static_cast<RowSets&>(P) = row_sets(X, C, n, k, d, W.norms);
    P.nq = n; P.nc = k; P.c0 = n; P.nbc = 1; P.S = 1;
    P.pk = W.keys;
    const int r0 = x_norms ? n : 0, nbq = blocks_of(n);
    GGAN_LAUNCH("kmeans_norms", 2.0 * (P.T - r0) * d, 4.0 * (P.T - r0) * d, kmeans_norms_k, dim3(cdiv(P.T - r0, 4)), dim3(256), 0, st,
                static_cast<const RowSets&>(P), W.norms, r0);
    const int rc = dispatch_vec(P.vec, [&](auto VEC) {
        if (trace_sets_on()) trace_sweep("kmeans_assign", 0, decltype(VEC)::value, P, dim3(nbq, 1));
        GGAN_LAUNCH("kmeans_assign", tile_flops(nbq, d), tile_bytes(nbq, d), (kmeans_assign_k<decltype(VEC)::value>), dim3(nbq, 1), dim3(256), 0,
                    st, P);
        return 0;
    });
    if (rc) return rc;
    GGAN_LAUNCH("kmeans_assign_final", 0, 20.0 * n, kmeans_assign_final_k, dim3(cdiv(n, 256)), dim3(256), 0, st, (const nkey*)W.keys,
                (const float*)W.norms, n, k, prev, assign, dist, moved, counts, status);
    if (inertia) {
        GGAN_LAUNCH("kmeans_inertia", 1.0 * n, 4.0 * n, kmeans_inertia_k, dim3(1), dim3(256), 0, st, (const float*)dist, n, inertia);
    }
    return 0;
}

int update_launch(const float* X, const int* assign, int n, int d, int k, float* centres, int* counts, const Workspace& W, hipStream_t st) {
    const int nb = update_blocks(n);
    GGAN_LAUNCH("kmeans_update_part", 2.0 * n * d * 32.0 * ((k + 31) / 32), 4.0 * n * d + 4.0 * nb * k * d, kmeans_update_part_k,
                dim3(nb, cdiv(d, kUC)), dim3(256), 0, st, X, assign, n, d, k, W.part, W.blkcnt);
    GGAN_LAUNCH("kmeans_update_final", 1.0 * nb * k * d, 4.0 * nb * k * d, kmeans_update_final_k, dim3(k, cdiv(d, 256)), dim3(256), 0, st,
                (const float*)W.part, (const int*)W.blkcnt, nb, d, k, centres, counts);
    return 0;
}

}  // namespace

extern "C" {

size_t ggan_kmeans_workspace(int n, int d, int k) {
    if (!shape_ok(n, d, k)) return 0;
    return carve(nullptr, n, d, k).bytes;
}

#define KMEANS_CHECK_WS(n, d, k)                                                                                                  \
    GGAN_CHECK_ARG(shape_ok(n, d, k), "1 <= n <= 131072, d >= 1, 1 <= k <= 128");                                                \
    GGAN_CHECK_ARG(ws && ws_bytes >= ggan_kmeans_workspace(n, d, k), "workspace too small (ggan_kmeans_workspace)");              \
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned")

int ggan_kmeans_seed(const float* X, int n, int d, int k, const double* u, float* centres, int32_t* idx, void* ws, size_t ws_bytes,
                     ggan_stream_t stream) {
    KMEANS_CHECK_WS(n, d, k);
    GGAN_CHECK_ARG(X && u && centres && idx, "null pointer");
    return seed_launch(X, n, d, k, u, centres, (int*)idx, carve(ws, n, d, k), (hipStream_t)stream);
}

int ggan_kmeans_pick(const float* mind, int n, const double* u, int32_t* idx, ggan_stream_t stream) {
    GGAN_CHECK_ARG(rows_ok(n), "1 <= n <= 131072");
    GGAN_CHECK_ARG(mind && u && idx, "null pointer");
    GGAN_LAUNCH("kmeans_pick", 1.0 * n, 4.0 * n, kmeans_pick_k, dim3(1), dim3(256), 0, (hipStream_t)stream, mind, n, u, 0, 0,
                (const float*)nullptr, 0, (float*)nullptr, (int*)idx);
    return 0;
}

int ggan_kmeans_assign(const float* X, const float* C, int n, int d, int k, const int32_t* prev, int32_t* assign, float* dist, double* inertia,
                       int32_t* moved, int32_t* counts, int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    KMEANS_CHECK_WS(n, d, k);
    GGAN_CHECK_ARG(X && C && assign && dist && status, "null pointer");
    GGAN_CHECK_ARG(!prev || moved, "a previous assignment needs somewhere to count the rows that moved");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = zero_async(__func__, status, sizeof(int), st)) return rc;
    if (moved) {
        if (const int rc = zero_async(__func__, moved, sizeof(int), st)) return rc;
    }
    return assign_launch(X, C, n, d, k, (const int*)prev, (int*)assign, dist, inertia, (int*)moved, (int*)counts, (int*)status,
                         carve(ws, n, d, k), false, st);
}

int ggan_kmeans_update(const float* X, const int32_t* assign, int n, int d, int k, float* centres, int32_t* counts, void* ws, size_t ws_bytes,
                       ggan_stream_t stream) {
    KMEANS_CHECK_WS(n, d, k);
    GGAN_CHECK_ARG(X && assign && centres && counts, "null pointer");
    return update_launch(X, (const int*)assign, n, d, k, centres, (int*)counts, carve(ws, n, d, k), (hipStream_t)stream);
}

int ggan_kmeans_fit(const float* X, int n, int d, int k, int iters, const double* u, float* centres, int32_t* idx, int32_t* assign,
                    int32_t* counts, double* inertia, int32_t* moved, int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    KMEANS_CHECK_WS(n, d, k);
    GGAN_CHECK_ARG(iters >= 0 && iters <= GGAN_KMEANS_MAX_ITERS, "0 <= iters <= 1000");
    GGAN_CHECK_ARG(X && u && centres && idx && assign && counts && inertia && moved && status, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const Workspace W = carve(ws, n, d, k);
    if (const int rc = zero_async(__func__, status, sizeof(int), st)) return rc;
    if (const int rc = zero_async(__func__, moved, (size_t)(iters + 1) * sizeof(int), st)) return rc;
    if (const int rc = seed_launch(X, n, d, k, u, centres, (int*)idx, W, st)) return rc;
    for (int t = 0; t <= iters; ++t) {
        const bool last = t == iters;
        if (last) {
            if (const int rc = zero_async(__func__, counts, (size_t)k * sizeof(int), st)) return rc;
        }
        if (const int rc = assign_launch(X, centres, n, d, k, t ? (const int*)assign : nullptr, (int*)assign, W.dist, inertia + t,
                                         (int*)moved + t, last ? (int*)counts : nullptr, (int*)status, W, true, st))
            return rc;
        if (!last) {
            if (const int rc = update_launch(X, (const int*)assign, n, d, k, centres, (int*)counts, W, st)) return rc;
        }
    }
    return 0;
}

int ggan_bin_test(const int32_t* counts_ref, const int32_t* counts_test, int k, double z_threshold, double* out, ggan_stream_t stream) {
    GGAN_CHECK_ARG(k >= 1 && k <= kMaxK, "1 <= k <= 128");
    GGAN_CHECK_ARG(counts_ref && counts_test && out, "null pointer");
    GGAN_LAUNCH("bin_test", 40.0 * k, 8.0 * k, bin_test_k, dim3(1), dim3(kMaxK), 0, (hipStream_t)stream, (const int*)counts_ref,
                (const int*)counts_test, k, z_threshold, out);
    return 0;
}

int ggan_cluster_scores(const int32_t* assign, const int32_t* labels, int n, int k, int classes, int32_t* table, double* out, int32_t* status,
                        ggan_stream_t stream) {
    GGAN_CHECK_ARG(rows_ok(n), "1 <= n <= 131072");
    GGAN_CHECK_ARG(k >= 1 && k <= kMaxK, "1 <= k <= 128");
    GGAN_CHECK_ARG(classes >= 1 && classes <= kMaxClasses, "1 <= classes <= 32");
    GGAN_CHECK_ARG(assign && labels && table && out && status, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = zero_async(__func__, status, sizeof(int), st)) return rc;
    if (const int rc = zero_async(__func__, table, (size_t)k * classes * sizeof(int), st)) return rc;
    GGAN_LAUNCH("cluster_table", 0, 8.0 * n, cluster_table_k, dim3(cdiv(n, 256)), dim3(256), 0, st, (const int*)assign, (const int*)labels, n, k,
                classes, (int*)table, (int*)status);
    GGAN_LAUNCH("cluster_scores_final", 30.0 * k * classes, 8.0 * k * classes, cluster_scores_final_k, dim3(1), dim3(256), 0, st,
                (const int*)table, (const int*)status, n, k, classes, out);
    return 0;
}

}  // extern "C"
