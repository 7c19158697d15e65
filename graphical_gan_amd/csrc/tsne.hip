// t-SNE on the device: the latent-space pictures of the MNIST scripts (gan_inference_mnist.py:472-480, gmgan_inference_mnist.py:533-551
// call sklearn's TSNE().fit_transform on the host).  van der Maaten's algorithm with the schedule of that TSNE(); the repulsive term is
// summed exactly over all pairs instead of through a Barnes-Hut tree.
//
//   sqnorms      |x_i|^2, one wavefront per row
//   neighbours   G = X_blk X^T through ggan_gemm, then per row: d_ij = |x_i|^2 + |x_j|^2 - 2 G_ij in place and the K smallest
//                (key = distance bits << 32 | index, so a tie goes to the lower index): a bitwise search for the K-th smallest key
//                (45 counting passes over the row, which stays in cache), then a rank sort of the K survivors
//   affinities   one wavefront per row, two neighbours per lane: the bisection on beta in registers and cross-lane sums
//   symmetrise   P = (P + P^T) / 2N as a CSR: row i holds its K neighbours and then every j that lists i, ascending.  A j that is in
//                both relations appears twice, the second time with the value 0, so the layout is that of the reverse relation and
//                needs no second count.  The reverse lists are filled through an integer cursor and then rank-sorted: the layout is a
//                function of the input only
//   repulse      sum_j q_ij^2 (y_i - y_j) and sum_j q_ij over ONE split of the j range per workgroup: y_j tiles in LDS read as
//                broadcasts, y_i and the accumulators in registers; partial force sums [splits][2][N] and one z sum per workgroup
//   step         one wavefront per point: the partials and the workgroup z sums added in a fixed order, the attractive sum over the
//                point's CSR row, then gains / velocity / position (into the OTHER position buffer: every y_j read is the old one)
//
// No atomics on floats anywhere: the same input gives the same bits on every run.
#include <math.h>
#include "common.h"
using namespace ggan;

namespace {

constexpr int TS_THR = 256;
constexpr int TS_WAVES = TS_THR / 64;
constexpr int TS_KMAX = GGAN_TSNE_MAX_K;
constexpr int TS_SPLITS_MAX = GGAN_TSNE_MAX_SPLITS;
constexpr int TS_TILE = 1024;           // y_j per LDS tile (8 KB)

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(TS_THR) void tsne_sqnorm_k(const float* __restrict__ x, int N, int D, float* __restrict__ out) {
    const int row = blockIdx.x * TS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* p = x + (size_t)row * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) s = fmaf(p[k], p[k], s);
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

__device__ __forceinline__ unsigned long long knn_key(float d, int j) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
}

// one workgroup per row r of the block (point row0 + r); dots[r][:] = x_i . x_j on entry, the squared distances on exit
__global__ __launch_bounds__(TS_THR) void tsne_select_k(float* __restrict__ dots, const float* __restrict__ norms, int N, int row0, int K,
                                                        int idx_bits, int32_t* __restrict__ idx, float* __restrict__ dist) {
    __shared__ unsigned long long sel[TS_KMAX];
    __shared__ int cnt_w[TS_WAVES];
    __shared__ int nsel;
    const int r = blockIdx.x, i = row0 + r, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float* row = dots + (size_t)r * N;
    const float ni = norms[i];
    for (int j = tid; j < N; j += TS_THR) {
        const float d = fmaxf(ni + norms[j] - 2.f * row[j], 0.f);
        row[j] = (j == i) ? INFINITY : d;               // (self excluded: K < N, so an infinite key is never among the K smallest)
    }
    if (tid == 0) nsel = 0;
    __syncthreads();
    // the K-th smallest key, bit by bit from the top (bit 63 is the sign of a non-negative float; index bits above idx_bits are zero)
    unsigned long long prefix = 0;
    for (int bit = 62; bit >= 0; --bit) {
        if (bit < 32 && bit >= idx_bits) continue;
        const unsigned long long cand = prefix | (1ull << bit);
        int c = 0;
        for (int j = tid; j < N; j += TS_THR) c += knn_key(row[j], j) < cand ? 1 : 0;
        c = wave_sum_i(c);
        if (lane == 0) cnt_w[wid] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int w = 0; w < TS_WAVES; ++w) tot += cnt_w[w];
        __syncthreads();
        if (tot <= K - 1) prefix = cand;                // fewer than K keys below cand: the K-th smallest has this bit set
    }
    // keys are distinct, so exactly K of them are <= prefix; their order comes from the rank sort below, not from the cursor
    for (int j = tid; j < N; j += TS_THR) {
        const unsigned long long key = knn_key(row[j], j);
        if (key <= prefix) {
            const int s = atomicAdd(&nsel, 1);
            if (s < TS_KMAX) sel[s] = key;
        }
    }
    __syncthreads();
    if (tid < K) {
        const unsigned long long key = sel[tid];
        int rank = 0;
        for (int t = 0; t < K; ++t) rank += sel[t] < key ? 1 : 0;
        idx[(size_t)i * K + rank] = (int32_t)(key & 0xFFFFFFFFull);
        dist[(size_t)i * K + rank] = __uint_as_float((unsigned)(key >> 32));
    }
}

// sklearn's _binary_search_perplexity on the K neighbour distances of one row.  The distances are taken relative to the smallest one:
// p and the entropy log(s) + beta * sum(d p) / s do not change, and exp() cannot underflow for every neighbour at once.
__global__ __launch_bounds__(TS_THR) void tsne_affinity_k(const float* __restrict__ dist, int N, int K, float log_perp, int steps, float tol,
                                                          float* __restrict__ p, float* __restrict__ beta_out) {
    const int row = blockIdx.x * TS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float* d = dist + (size_t)row * K;
    const bool h0 = lane < K, h1 = lane + 64 < K;
    const float dmin = d[0];                             // (the neighbour lists are sorted by distance)
    const float d0 = h0 ? d[lane] - dmin : 0.f, d1 = h1 ? d[lane + 64] - dmin : 0.f;
    float beta = 1.f, used = 1.f, lo = -INFINITY, hi = INFINITY, p0 = 0.f, p1 = 0.f, s = 1.f;
    for (int it = 0; it < steps; ++it) {
        used = beta;
        p0 = h0 ? expf(-d0 * beta) : 0.f;
        p1 = h1 ? expf(-d1 * beta) : 0.f;
        s = wave_sum(p0 + p1);
        const float e = wave_sum(fmaf(d0, p0, d1 * p1));
        const float diff = logf(s) + beta * e / s - log_perp;       // the same bits in every lane: the branch below is uniform
        if (fabsf(diff) <= tol) break;
        if (diff > 0.f) {
            lo = beta;
            beta = (hi == INFINITY) ? beta * 2.f : (beta + hi) * 0.5f;
        } else {
            hi = beta;
            beta = (lo == -INFINITY) ? beta * 0.5f : (beta + lo) * 0.5f;
        }
    }
    if (h0) p[(size_t)row * K + lane] = p0 / s;
    if (h1) p[(size_t)row * K + lane + 64] = p1 / s;
    if (lane == 0) beta_out[row] = used;
}

__global__ __launch_bounds__(TS_THR) void tsne_rev_count_k(const int32_t* __restrict__ idx, int NK, int* __restrict__ cnt) {
    const int e = blockIdx.x * TS_THR + threadIdx.x;
    if (e < NK) atomicAdd(&cnt[idx[e]], 1);
}

// ptr[i] = i K + (number of reverse entries of the rows before i), one workgroup
__global__ __launch_bounds__(1024) void tsne_scan_k(const int* __restrict__ cnt, int N, int K, int* __restrict__ ptr) {
    __shared__ int sums[1024];
    const int tid = threadIdx.x, chunk = (N + 1023) / 1024;
    const int b = min(N, tid * chunk), e = min(N, b + chunk);
    int s = 0;
    for (int k = b; k < e; ++k) s += cnt[k];
    sums[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? sums[tid - o] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    int off = sums[tid] - s;
    for (int k = b; k < e; ++k) {
        ptr[k] = k * K + off;
        off += cnt[k];
    }
    if (tid == 1023) ptr[N] = N * K + sums[1023];
}

__global__ __launch_bounds__(TS_THR) void tsne_rev_fill_k(const int32_t* __restrict__ idx, int NK, int K, const int* __restrict__ ptr,
                                                          int* __restrict__ cursor, int* __restrict__ edges) {
    const int e = blockIdx.x * TS_THR + threadIdx.x;
    if (e >= NK) return;
    const int i = idx[e];
    edges[ptr[i] - i * K + atomicAdd(&cursor[i], 1)] = e;          // (any order: tsne_sym_k sorts each list)
}

// one wavefront per row i: the forward entries, then the reverse ones in ascending j (edge number e = j K + slot)
__global__ __launch_bounds__(TS_THR) void tsne_sym_k(const int32_t* __restrict__ idx, const float* __restrict__ pc, const int* __restrict__ ptr,
                                                     const int* __restrict__ edges, int N, int K, float inv2n, int32_t* __restrict__ col,
                                                     float* __restrict__ val) {
    const int i = blockIdx.x * TS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= N) return;
    const int base = ptr[i], L = ptr[i + 1] - base - K;
    const int32_t* mine = idx + (size_t)i * K;
    for (int s = lane; s < K; s += 64) {
        const int j = mine[s];
        const int32_t* theirs = idx + (size_t)j * K;
        float back = 0.f;
        for (int t = 0; t < K; ++t)
            if (theirs[t] == i) back = pc[(size_t)j * K + t];
        col[base + s] = j;
        val[base + s] = (pc[(size_t)i * K + s] + back) * inv2n;
    }
    const int* list = edges + (base - i * K);
    for (int m = lane; m < L; m += 64) {
        const int e = list[m], j = e / K;
        int rank = 0;
        for (int t = 0; t < L; ++t) rank += list[t] < e ? 1 : 0;
        bool mutual = false;
        for (int t = 0; t < K; ++t) mutual |= mine[t] == j;
        col[base + K + rank] = j;
        val[base + K + rank] = mutual ? 0.f : (pc[e] + 0.f) * inv2n;      // (a mutual pair is counted in the forward entry)
    }
}

// ---- the gradient ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void repulse_pair(const float2 yi, const float2 yj, bool self, float& ax, float& ay, float& az) {
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    float q = 1.f / (1.f + fmaf(dx, dx, dy * dy));
    q = self ? 0.f : q;
    const float qq = q * q;
    az += q;
    ax = fmaf(qq, dx, ax);
    ay = fmaf(qq, dy, ay);
}

// grid (ceil(N / 256), splits): a thread owns point i and walks the j range [split * chunk, (split + 1) * chunk)
__global__ __launch_bounds__(TS_THR) void tsne_repulse_k(const float2* __restrict__ Y, int N, int chunk, float* __restrict__ part,
                                                         float* __restrict__ zblk) {
    __shared__ float2 tile[TS_TILE];
    __shared__ float red[32];
    const int tid = threadIdx.x, i = blockIdx.x * TS_THR + tid, s = blockIdx.y;
    const int j0 = min(N, s * chunk), j1 = min(N, j0 + chunk);
    const float2 yi = Y[min(i, N - 1)];
    float ax[4] = {0.f, 0.f, 0.f, 0.f}, ay[4] = {0.f, 0.f, 0.f, 0.f}, az[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t0 = j0; t0 < j1; t0 += TS_TILE) {
        const int n = min(TS_TILE, j1 - t0);
        __syncthreads();
        for (int k = tid; k < n; k += TS_THR) tile[k] = Y[t0 + k];
        __syncthreads();
        int k = 0;
        for (; k + 4 <= n; k += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) repulse_pair(yi, tile[k + u], t0 + k + u == i, ax[u], ay[u], az[u]);
        }
        for (; k < n; ++k) repulse_pair(yi, tile[k], t0 + k == i, ax[0], ay[0], az[0]);
    }
    const float sx = (ax[0] + ax[1]) + (ax[2] + ax[3]), sy = (ay[0] + ay[1]) + (ay[2] + ay[3]);
    const float sz = i < N ? (az[0] + az[1]) + (az[2] + az[3]) : 0.f;
    if (i < N) {
        part[((size_t)s * 2 + 0) * N + i] = sx;
        part[((size_t)s * 2 + 1) * N + i] = sy;
    }
    const float zsum = block_sum(sz, red);
    if (tid == 0) zblk[s * gridDim.x + blockIdx.x] = zsum;
}

struct StepParams {
    const int* ptr;
    const int32_t* col;
    const float* val;
    const float2* yin;
    float2* yout;
    float* vel;
    float* gains;
    const float* part;
    const float* zblk;
    float *attr, *rep, *z, *klrow;          // MODE 1: the three terms; MODE 2: the rows of the KL sum
    int N, splits, nz;
    float exag, mom, lr, min_gain;
};

// MODE 0: one update.  1: attr [N,2] (not exaggerated), rep [N,2] (not divided by Z), z[0] = Z.  2: klrow[i] = sum_j P_ij log(P_ij / Q_ij)
template <int MODE>
__global__ __launch_bounds__(TS_THR) void tsne_step_k(StepParams p) {
    const int i = blockIdx.x * TS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= p.N) return;
    float z = 0.f;
    for (int k = lane; k < p.nz; k += 64) z += p.zblk[k];
    z = wave_sum(z);                                   // every wavefront adds the same values in the same order: one Z for all
    float rx = 0.f, ry = 0.f;
    if (lane < p.splits) {
        rx = p.part[((size_t)lane * 2 + 0) * p.N + i];
        ry = p.part[((size_t)lane * 2 + 1) * p.N + i];
    }
    rx = wave_sum(rx);
    ry = wave_sum(ry);
    const float2 yi = p.yin[i];
    const float logz = MODE == 2 ? logf(z) : 0.f;
    float ax = 0.f, ay = 0.f, kl = 0.f;
    const int e1 = p.ptr[i + 1];
    for (int e = p.ptr[i] + lane; e < e1; e += 64) {
        const float pv = p.val[e];
        const float2 yj = p.yin[p.col[e]];
        const float dx = yi.x - yj.x, dy = yi.y - yj.y;
        const float d1 = 1.f + fmaf(dx, dx, dy * dy);
        const float w = pv / d1;
        ax = fmaf(w, dx, ax);
        ay = fmaf(w, dy, ay);
        if (MODE == 2 && pv > 0.f) kl = fmaf(pv, logf(pv) + logz + logf(d1), kl);
    }
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (MODE == 1) {
        if (lane == 0) {
            p.attr[2 * i] = ax; p.attr[2 * i + 1] = ay;
            p.rep[2 * i] = rx; p.rep[2 * i + 1] = ry;
            if (i == 0) p.z[0] = z;
        }
        return;
    }
    if (MODE == 2) {
        kl = wave_sum(kl);
        if (lane == 0) p.klrow[i] = kl;
        return;
    }
    if (lane < 2) {
        const float a = lane ? ay : ax, r = lane ? ry : rx, y = lane ? yi.y : yi.x;
        const float g = 4.f * (p.exag * a - r / z);
        float v = p.vel[2 * i + lane], gain = p.gains[2 * i + lane];
        gain = (v * g < 0.f) ? gain + 0.2f : gain * 0.8f;
        gain = fmaxf(gain, p.min_gain);
        v = p.mom * v - p.lr * (gain * g);
        p.gains[2 * i + lane] = gain;
        p.vel[2 * i + lane] = v;
        reinterpret_cast<float*>(p.yout)[2 * i + lane] = y + v;
    }
}

__global__ __launch_bounds__(1024) void tsne_sum_k(const float* __restrict__ v, int n, float* __restrict__ out) {
    __shared__ float red[32];
    float s = 0.f;
    for (int k = threadIdx.x; k < n; k += 1024) s += v[k];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

int launch_repulse(const float* y, int N, int splits, float* part, float* zblk, hipStream_t st) {
    const int chunk = cdiv(cdiv(N, splits), 4) * 4;
    const dim3 grid(cdiv(N, TS_THR), splits);
    GGAN_LAUNCH("tsne_repulse", 12.0 * N * (double)N, 8.0 * N * splits, tsne_repulse_k, grid, dim3(TS_THR), 0, st,
                reinterpret_cast<const float2*>(y), N, chunk, part, zblk);
    return 0;
}

int check_embedding_args(const char* fn, const int* ptr, const int32_t* col, const float* val, const float* y, int N, int splits,
                         const float* part, const float* zblk) {
    if (!(ptr && col && val && y && part && zblk)) { set_error("%s: null pointer", fn); return -1; }
    if (N < 2) { set_error("%s: N must be at least 2", fn); return -1; }
    if (splits < 1 || splits > TS_SPLITS_MAX) { set_error("%s: splits must be 1 .. %d", fn, TS_SPLITS_MAX); return -1; }
    if ((uintptr_t)y % 8) { set_error("%s: misaligned embedding", fn); return -1; }
    return 0;
}

StepParams step_params(const int* ptr, const int32_t* col, const float* val, const float* y, int N, int splits, const float* part,
                       const float* zblk) {
    StepParams p;
    memset(&p, 0, sizeof(p));
    p.ptr = ptr; p.col = col; p.val = val; p.yin = reinterpret_cast<const float2*>(y);
    p.part = part; p.zblk = zblk;
    p.N = N; p.splits = splits; p.nz = splits * cdiv(N, TS_THR);
    return p;
}

}  // namespace

extern "C" {

int ggan_tsne_sqnorms(const float* x, int N, int D, float* norms, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && norms, "null pointer");
    GGAN_CHECK_ARG(N > 0 && D > 0, "bad shape");
    GGAN_LAUNCH("tsne_sqnorm", 2.0 * N * D, 4.0 * N * D, tsne_sqnorm_k, dim3(cdiv(N, TS_WAVES)), dim3(TS_THR), 0, (hipStream_t)stream, x, N, D,
                norms);
    return 0;
}

int ggan_tsne_neighbours(const float* x, const float* norms, int N, int D, int row0, int rows, int K, float* dots, int32_t* idx, float* dist,
                         void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && norms && dots && idx && dist, "null pointer");
    GGAN_CHECK_ARG(N >= 2 && D > 0, "bad shape (N must be at least 2)");
    GGAN_CHECK_ARG(K >= 1 && K <= TS_KMAX, "K must be 1 .. GGAN_TSNE_MAX_K");
    GGAN_CHECK_ARG(K < N, "K must be below N (a point is not its own neighbour)");
    GGAN_CHECK_ARG(rows > 0 && row0 >= 0 && row0 + rows <= N, "row block outside the data");
    GGAN_CHECK_ARG((double)N * K < 2147483648.0 && (double)rows * N < 2147483648.0, "too large (a row block is indexed with 31 bits, as ggan_gemm's operands are)");
    const int rc = ggan_gemm(0, 1, rows, N, D, x + (size_t)row0 * D, x, nullptr, dots, GGAN_ACT_NONE, 0.f, ws, ws_bytes, stream);
    if (rc) return rc;
    int idx_bits = 1;
    while ((1 << idx_bits) < N) ++idx_bits;
    GGAN_LAUNCH("tsne_select", 0, 4.0 * rows * (double)N * 47, tsne_select_k, dim3(rows), dim3(TS_THR), 0, (hipStream_t)stream, dots, norms, N,
                row0, K, idx_bits, idx, dist);
    return 0;
}

int ggan_tsne_affinities(const float* dist, int N, int K, float perplexity, int steps, float tol, float* p_cond, float* beta,
                         ggan_stream_t stream) {
    GGAN_CHECK_ARG(dist && p_cond && beta, "null pointer");
    GGAN_CHECK_ARG(N >= 2, "N must be at least 2");
    GGAN_CHECK_ARG(K >= 1 && K <= TS_KMAX && K < N, "K must be 1 .. GGAN_TSNE_MAX_K and below N");
    GGAN_CHECK_ARG(perplexity > 0.f && perplexity < (float)N, "perplexity must be positive and below N");
    GGAN_CHECK_ARG(steps >= 1 && steps <= 1000 && tol >= 0.f, "bad search bound");
    GGAN_LAUNCH("tsne_affinity", 0, 8.0 * N * K, tsne_affinity_k, dim3(cdiv(N, TS_WAVES)), dim3(TS_THR), 0, (hipStream_t)stream, dist, N, K,
                logf(perplexity), steps, tol, p_cond, beta);
    return 0;
}

int ggan_tsne_symmetrise(const int32_t* idx, const float* p_cond, int N, int K, int* ptr, int32_t* col, float* val, int* scratch,
                         ggan_stream_t stream) {
    GGAN_CHECK_ARG(idx && p_cond && ptr && col && val && scratch, "null pointer");
    GGAN_CHECK_ARG(N >= 2, "N must be at least 2");
    GGAN_CHECK_ARG(K >= 1 && K <= TS_KMAX && K < N, "K must be 1 .. GGAN_TSNE_MAX_K and below N");
    GGAN_CHECK_ARG((double)N * K < 1073741824.0, "too large");
    hipStream_t st = (hipStream_t)stream;
    const int NK = N * K;
    int *cnt = scratch, *cursor = scratch + N, *edges = scratch + 2 * N;       // scratch: 2 N + N K ints
    if (hipMemsetAsync(scratch, 0, (size_t)2 * N * sizeof(int), st) != hipSuccess) {
        set_error("%s: memset failed", __func__);
        return -2;
    }
    GGAN_LAUNCH("tsne_rev_count", 0, 4.0 * NK, tsne_rev_count_k, dim3(cdiv(NK, TS_THR)), dim3(TS_THR), 0, st, idx, NK, cnt);
    GGAN_LAUNCH("tsne_scan", 0, 8.0 * N, tsne_scan_k, dim3(1), dim3(1024), 0, st, cnt, N, K, ptr);
    GGAN_LAUNCH("tsne_rev_fill", 0, 8.0 * NK, tsne_rev_fill_k, dim3(cdiv(NK, TS_THR)), dim3(TS_THR), 0, st, idx, NK, K, ptr, cursor, edges);
    GGAN_LAUNCH("tsne_sym", 0, 16.0 * NK, tsne_sym_k, dim3(cdiv(N, TS_WAVES)), dim3(TS_THR), 0, st, idx, p_cond, ptr, edges, N, K,
                0.5f / (float)N, col, val);
    return 0;
}

int ggan_tsne_gradient(const int* ptr, const int32_t* col, const float* val, const float* y, int N, int splits, float* part, float* zblk,
                       float* attr, float* rep, float* z, ggan_stream_t stream) {
    if (check_embedding_args(__func__, ptr, col, val, y, N, splits, part, zblk)) return -1;
    GGAN_CHECK_ARG(attr && rep && z, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = launch_repulse(y, N, splits, part, zblk, st)) return rc;
    StepParams p = step_params(ptr, col, val, y, N, splits, part, zblk);
    p.attr = attr; p.rep = rep; p.z = z;
    GGAN_LAUNCH("tsne_terms", 0, 0, tsne_step_k<1>, dim3(cdiv(N, TS_WAVES)), dim3(TS_THR), 0, st, p);
    return 0;
}

int ggan_tsne_kl(const int* ptr, const int32_t* col, const float* val, const float* y, int N, int splits, float* part, float* zblk,
                 float* klrow, float* kl, ggan_stream_t stream) {
    if (check_embedding_args(__func__, ptr, col, val, y, N, splits, part, zblk)) return -1;
    GGAN_CHECK_ARG(klrow && kl, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = launch_repulse(y, N, splits, part, zblk, st)) return rc;
    StepParams p = step_params(ptr, col, val, y, N, splits, part, zblk);
    p.klrow = klrow;
    GGAN_LAUNCH("tsne_kl_rows", 0, 0, tsne_step_k<2>, dim3(cdiv(N, TS_WAVES)), dim3(TS_THR), 0, st, p);
    GGAN_LAUNCH("tsne_sum", 0, 4.0 * N, tsne_sum_k, dim3(1), dim3(1024), 0, st, klrow, N, kl);
    return 0;
}

int ggan_tsne_iterate(const int* ptr, const int32_t* col, const float* val, float* ya, float* yb, float* vel, float* gains, int N, int splits,
                      float* part, float* zblk, int it0, int it1, int exploration_iters, float early_exaggeration, float momentum0,
                      float momentum1, float learning_rate, float min_gain, ggan_stream_t stream) {
    if (check_embedding_args(__func__, ptr, col, val, ya, N, splits, part, zblk)) return -1;
    GGAN_CHECK_ARG(yb && vel && gains && yb != ya && (uintptr_t)yb % 8 == 0, "null, aliased or misaligned buffer");
    GGAN_CHECK_ARG(it0 >= 0 && it1 >= it0 && it1 - it0 <= 1000000, "bad iteration range");
    hipStream_t st = (hipStream_t)stream;
    StepParams p = step_params(ptr, col, val, ya, N, splits, part, zblk);
    p.vel = vel; p.gains = gains; p.lr = learning_rate; p.min_gain = min_gain;
    for (int it = it0; it < it1; ++it) {
        float* in = ((it - it0) & 1) ? yb : ya;
        float* out = ((it - it0) & 1) ? ya : yb;
        if (const int rc = launch_repulse(in, N, splits, part, zblk, st)) return rc;
        p.yin = reinterpret_cast<const float2*>(in);
        p.yout = reinterpret_cast<float2*>(out);
        p.exag = it < exploration_iters ? early_exaggeration : 1.f;
        p.mom = it < exploration_iters ? momentum0 : momentum1;
        GGAN_LAUNCH("tsne_step", 0, 0, tsne_step_k<0>, dim3(cdiv(N, TS_WAVES)), dim3(TS_THR), 0, st, p);
    }
    return 0;
}

}  // extern "C"
