// Set-level mixture-of-RBF kernel sums between two row sets (tflib/objs/mmd.py:20-67 at dev-set sizes): for X[m,d], Y[n,d]
//   S_xx = sum_{i != j} k(x_i, x_j),  S_yy likewise,  S_xy = sum_{i,j} k(x_i, y_j),  k(a,b) = sum_s wt_s exp(-||a-b||^2 / (2 sigma_s^2))
// from which both MMD^2 estimators follow (include/ggan.h).  ggan_mix_rbf_mmd2_fwd (losses.hip) forms direct differences on one
// scalar workgroup per row and stops at m + n = 512; here the Gram product runs on v_mfma_f32_32x32x2_f32 and nothing of size
// (m+n)^2 ever reaches memory.
//
// The two sets are ONE row list Z = [X; Y] of T = m + n rows, cut into blocks of 128.  A tile is a pair of blocks (a, b): 128x128
// dot products g_ij from LDS-staged k-major operand tiles (both operands are k-contiguous in memory, as op(B) of gemm.hip with
// tb = 1), 2x2 waves of 64x64, four 32x32 accumulators per wave.  The epilogue forms max(n_i + n_j - 2 g_ij, 0) from the row norms
// of a pre-pass, the mixture of exponentials, and adds the value to the sum its PAIR belongs to -- decided per element from
// (i < m, j < m), so a tile may straddle the X / Y boundary or hang over the end of Z.
//
// Symmetry: k(z_i, z_j) = k(z_j, z_i), so of the nb x nb tiles only one of (a, b) / (b, a) is computed.  Block a visits
// b = (a + t) mod nb for t = 0 .. nb/2 (the last step, when nb is even, only from the lower half of the blocks): every unordered pair of
// blocks exactly once, and every block the same number of tiles.  A visited element stands for both orders of its pair: it counts twice
// in S_xx / S_yy and once in S_xy; on the diagonal tile (t = 0) only i < j is counted, which also drops i == j.
//
// Reduction: workgroup (a, s) walks the steps t = s, s + S, ... of block a, accumulates each tile in float per thread (<= 64 values),
// the tiles in double, and leaves ONE partial triple; the last stage adds the nb * S triples in a fixed order in double.  No atomics: two
// calls on the same input give the same bits.  S is chosen so that nb * S is about 2048 workgroups, so the workspace (T norms + nb * S
// triples) is linear in m + n.
#include "common.h"
#include "set_rows.h"
using namespace ggan;

namespace {

constexpr int kMaxSigmas = 8;

struct SetParams : RowSets {       // (set_rows.h: the row list, its loads and the norm pre-pass)
    double* part;                  // [nb * S][3]
    int ns;
    int nb, S;
    float g2[kMaxSigmas];          // log2(e) / (2 sigma^2): exp(-gamma D) = exp2(-g2 D)
    float wt[kMaxSigmas];
};

// is step t of block a a tile to compute (see the head of the file)
__device__ __forceinline__ bool step_valid(int a, int t, int nb) { return 2 * t < nb || (2 * t == nb && 2 * a < nb) || t == 0; }

// NS: the number of kernel widths (their constants then live in scalar registers for the whole epilogue; a run-time count made every
// element's loop re-read them from the argument block).  VEC: see load4_raw.  Two workgroups per CU, as the sweeps of knn_sets.hip: without
// the bound the allocator takes a whole SIMD's registers for NS >= 2 and one wave per SIMD is left.
template <int NS, bool VEC>
__global__ __launch_bounds__(256, 2) void set_sums_k(const SetParams P) {
    warm_kernarg(P);
    __shared__ __attribute__((aligned(16))) float As[2][KS * LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][KS * LD];
    __shared__ float nA[BT], nB[BT];
    __shared__ double red[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = blockIdx.x, s = blockIdx.y;
    double dxx = 0.0, dyy = 0.0, dxy = 0.0;
    float g2[NS], wt[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) { g2[q] = P.g2[q]; wt[q] = P.wt[q]; }

    // the steps of this workgroup: t = s, s + S, ... as far as they are tiles to compute (uniform over the workgroup)
    const int nt = P.nb / 2 + 1;
    auto next_step = [&](int t) {
        while (t < nt && !step_valid(a, t, P.nb)) t += P.S;
        return t;
    };
    const int r0a = a * BT;
    float4 ra[2], rb[2];
    int t = next_step(s);
    if (t < nt) load_step<VEC>(P, r0a, ((a + t) % P.nb) * BT, 0, ra, rb);
    while (t < nt) {
        const int r0b = ((a + t) % P.nb) * BT;
        if (tid < BT) nA[tid] = r0a + tid < P.T ? P.norms[r0a + tid] : 0.f;
        else nB[tid - BT] = r0b + tid - BT < P.T ? P.norms[r0b + tid - BT] : 0.f;
        const int tn = next_step(t + P.S);
        f32x16 acc[2][2];
        gram_tile<VEC>(P, r0a, r0b, tn < nt, r0a, ((a + tn) % P.nb) * BT, As, Bs, ra, rb, acc);

        float fxx = 0.f, fyy = 0.f, fxy = 0.f;
        const bool diag = t == 0;
        for_each_acc([&](int il, int jl, int bi, int bj, int r) {
            const int i = r0a + il, j = r0b + jl;
            const bool on = i < P.T && j < P.T && (!diag || i < j);
            const float dist = gram_dist(nA[il], nB[jl], acc[bi][bj][r]);
            float kv = 0.f;
#pragma unroll
            for (int q = 0; q < NS; ++q) kv = fmaf(wt[q], __builtin_amdgcn_exp2f(-g2[q] * dist), kv);
            kv = on ? kv : 0.f;
            const bool ix = i < P.m, jx = j < P.m;
            fxx += (ix && jx) ? 2.f * kv : 0.f;
            fyy += (!ix && !jx) ? 2.f * kv : 0.f;
            fxy += (ix != jx) ? kv : 0.f;
        });
        dxx += (double)fxx; dyy += (double)fyy; dxy += (double)fxy;
        __syncthreads();                                   // nA / nB are rewritten by the next tile
        t = tn;
    }

    // the workgroup's triple: lanes by the wave's butterfly, the four waves in wave order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        dxx += __shfl_xor(dxx, o, 64);
        dyy += __shfl_xor(dyy, o, 64);
        dxy += __shfl_xor(dxy, o, 64);
    }
    if (lane == 0) { red[wave][0] = dxx; red[wave][1] = dyy; red[wave][2] = dxy; }
    __syncthreads();
    if (tid < 3) P.part[((size_t)a * P.S + s) * 3 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// last stage: thread i adds triples i, i + 256, ... in that order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void set_final_k(const double* __restrict__ part, int count, double* __restrict__ sums3) {
    __shared__ double sm[256];
    const int tid = threadIdx.x;
    for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int i = tid; i < count; i += 256) v += part[(size_t)i * 3 + c];
        sm[tid] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) sm[tid] += sm[tid + o];
            __syncthreads();
        }
        if (tid == 0) sums3[c] = sm[0];
        __syncthreads();
    }
}

// mmd's own splits, of the nt = nb / 2 + 1 steps of a block (the symmetric half: see the head of the file)
inline int mmd_splits_of(int nb) {
    const int nt = nb / 2 + 1;
    int S = (kTargetWgs + nb - 1) / nb;
    if (S > nt) S = nt;
    return S < 1 ? 1 : S;
}

}  // namespace

extern "C" {

size_t ggan_mix_rbf_sums_workspace(int m, int n) {
    if (m < 1 || n < 1 || m > kMaxRows || n > kMaxRows) return 0;
    const int nb = blocks_of((long)m + n);
    return norms_bytes((long)m + n) + (size_t)nb * mmd_splits_of(nb) * 3 * sizeof(double);
}

int ggan_mix_rbf_sums(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                      double* sums3, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(X && Y && sigmas && sums3 && ws, "null pointer");
    GGAN_CHECK_ARG(m >= 1 && n >= 1 && m <= kMaxRows && n <= kMaxRows, "1 <= m, n <= 131072");
    GGAN_CHECK_ARG(d >= 1, "d < 1");
    GGAN_CHECK_ARG(ns >= 1 && ns <= kMaxSigmas, "1 <= ns <= 8");
    GGAN_CHECK_ARG(ws_bytes >= ggan_mix_rbf_sums_workspace(m, n), "workspace too small (ggan_mix_rbf_sums_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)sums3 & 7) == 0, "workspace must be 16-byte, sums3 8-byte aligned");
    for (int i = 0; i < ns; ++i) GGAN_CHECK_ARG(sigmas[i] > 0.f, "sigma <= 0");
    SetParams P;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = rows_setup(P, "mmd_set_norms", X, Y, m, n, d, ws, st)) return rc;
    P.ns = ns;
    P.nb = blocks_of(P.T);
    P.S = mmd_splits_of(P.nb);
    for (int i = 0; i < kMaxSigmas; ++i) {
        P.g2[i] = i < ns ? (float)(1.4426950408889634 / (2.0 * (double)sigmas[i] * (double)sigmas[i])) : 0.f;
        P.wt[i] = i < ns ? (wts ? wts[i] : 1.f) : 0.f;
    }
    P.part = (double*)((char*)ws + norms_bytes(P.T));
    // tiles computed: nb diagonal ones and nb (nb - 1) / 2 pairs
    const double tiles = 0.5 * (double)P.nb * (P.nb + 1);
    if (const int rc = dispatch_k_vec(ns, P.vec, [&](auto NS, auto VEC) {
            if (trace_sets_on()) trace_sets("mmd_set_sums", decltype(NS)::value, decltype(VEC)::value, P, nullptr, P.nb, P.S, dim3(P.nb, P.S));
            GGAN_LAUNCH("mmd_set_sums", tile_flops(tiles, d), tile_bytes(tiles, d), (set_sums_k<decltype(NS)::value, decltype(VEC)::value>),
                        dim3(P.nb, P.S), dim3(256), 0, st, P);
            return 0;
        }))
        return rc;
    GGAN_LAUNCH("mmd_set_final", 0, 24.0 * P.nb * P.S, set_final_k, dim3(1), dim3(256), 0, st, (const double*)P.part, P.nb * P.S, sums3);
    return 0;
}

}  // extern "C"
