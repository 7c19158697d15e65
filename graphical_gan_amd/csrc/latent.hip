// Latent-space glue of the gmgan scripts: the HyperGenerator mix, the mixture-of-Gaussians latent with its straight-through
// variants, the test-set posterior pass with its cluster accuracy, and the noise generator of one session.run.
#include "common.h"
#include "pointwise.h"
using namespace ggan;

namespace {

// out[b][d] = sum_j k[b][j] * mu[j][d] + noise[b][d]: HyperGenerator of the gmgan scripts, tf.add(tf.matmul(tf.cast(hyper_k, tf.float32), com_mu),
// hyper_noise) (gmgan_inference_cifar10.py:150-153), as ONE pointwise launch instead of a 30-deep GEMM launch and an addition launch at the head of
// the Generator chain.  The fmaf chain in j order is what the MFMA GEMM computes; with one-hot rows it is the selected mean exactly.
__global__ void mix_mean_k(const float* __restrict__ k, const float* __restrict__ mu, const float* __restrict__ noise, float* __restrict__ out,
                           int B, int K, int D4) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * D4) return;
    const int b = idx / D4, d4 = idx - b * D4;
    const float* kr = k + (size_t)b * K;
    const float4* m = reinterpret_cast<const float4*>(mu) + d4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < K; ++j) {
        const float kv = kr[j];
        const float4 mv = m[(size_t)j * D4];
        acc.x = fmaf(kv, mv.x, acc.x); acc.y = fmaf(kv, mv.y, acc.y); acc.z = fmaf(kv, mv.z, acc.z); acc.w = fmaf(kv, mv.w, acc.w);
    }
    const float4 nv = reinterpret_cast<const float4*>(noise)[idx];
    acc.x += nv.x; acc.y += nv.y; acc.z += nv.z; acc.w += nv.w;
    reinterpret_cast<float4*>(out)[idx] = acc;
}

// ---- mixture-of-Gaussians latent glue of the gmgan scripts (gmgan_inference_cifar10.py:156-173, MODE_K = 'CONCRETE'):
//        logits[b, j] = -.5 * sum_d (z[b, d] - mu[j, d])^2 + log_pi
//        k[b, :]      = softmax((logits[b, :] - log(-log(u[b, :] + 1e-20) + 1e-20)) / temp)          (Gumbel-softmax relaxation)
//      a dozen [B, K] / [B, K, D] pointwise launches in the TF graph, one here: a workgroup per batch row, a wave per
//      component for the distance (lanes over d, shuffle reduce), the softmax over the K values in LDS. ----
constexpr int kGmmMaxK = 256;

__global__ __launch_bounds__(256) void gmm_latent_fwd_k(const float* __restrict__ z, const float* __restrict__ mu,
                                                        const float* __restrict__ u, float* __restrict__ logits, float* __restrict__ k,
                                                        int K, int D, float log_pi, float inv_temp) {
    __shared__ float sv[kGmmMaxK];
    __shared__ float red[32];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* zb = z + (size_t)b * D;
    for (int j = wave; j < K; j += 4) {
        const float* mj = mu + (size_t)j * D;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float t = zb[d] - mj[d];
            s = fmaf(t, t, s);
        }
        s = wave_sum(s);
        if (lane == 0) {
            const float lg = -0.5f * s + log_pi;
            if (logits) logits[(size_t)b * K + j] = lg;
            const float g = -logf(-logf(u[(size_t)b * K + j] + 1e-20f) + 1e-20f);
            sv[j] = (lg + g) * inv_temp;
        }
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = threadIdx.x; j < K; j += 256) m = fmaxf(m, sv[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float e = 0.f;
    for (int j = threadIdx.x; j < K; j += 256) {
        const float t = expf(sv[j] - m);
        sv[j] = t;
        e += t;
    }
    const float tot = block_sum(e, red + 8);
    const float inv = 1.f / tot;
    for (int j = threadIdx.x; j < K; j += 256) k[(size_t)b * K + j] = sv[j] * inv;
}

// Backward in ONE launch: blocks [0, B) own a batch row (-> dz), blocks [B, B + K) own a component (-> dmu, a sum over the batch
// in row order: deterministic).  dlog[b, j] = gl[b, j] + k[b, j] * (gk[b, j] - sum_i gk[b, i] * k[b, i]) / temp.
__global__ __launch_bounds__(256) void gmm_latent_bwd_k(const float* __restrict__ z, const float* __restrict__ mu,
                                                        const float* __restrict__ kk, const float* __restrict__ gl,
                                                        const float* __restrict__ gk, float* __restrict__ dz, float* __restrict__ dmu,
                                                        int B, int K, int D, float inv_temp) {
    __shared__ float sv[kGmmMaxK];
    __shared__ float red[32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < B) {
        const int b = blockIdx.x;
        float dot = 0.f;
        if (gk)
            for (int j = threadIdx.x; j < K; j += 256) dot += gk[(size_t)b * K + j] * kk[(size_t)b * K + j];
        dot = block_sum(dot, red);
        for (int j = threadIdx.x; j < K; j += 256) {
            float v = gl ? gl[(size_t)b * K + j] : 0.f;
            if (gk) v += kk[(size_t)b * K + j] * (gk[(size_t)b * K + j] - dot) * inv_temp;
            sv[j] = v;
        }
        __syncthreads();
        if (dz) {
            // dz[b, d] = -sum_j dlog[j] * (z[b, d] - mu[j, d])
            for (int d = threadIdx.x; d < D; d += 256) {
                const float zv = z[(size_t)b * D + d];
                float acc = 0.f;
                for (int j = 0; j < K; ++j) acc = fmaf(sv[j], zv - mu[(size_t)j * D + d], acc);
                dz[(size_t)b * D + d] = -acc;
            }
        }
        return;
    }
    if (!dmu) return;
    const int j = blockIdx.x - B;
    // dlog[b, j] for every b (one wave per row: the softmax-backward dot product is a K-long reduction), then
    // dmu[j, d] = sum_b dlog[b, j] * (z[b, d] - mu[j, d])
    float* col = sv;                       // B <= kGmmMaxK values
    for (int b = wave; b < B; b += 4) {
        float dot = 0.f;
        if (gk)
            for (int i = lane; i < K; i += 64) dot += gk[(size_t)b * K + i] * kk[(size_t)b * K + i];
        dot = wave_sum(dot);
        if (lane == 0) {
            float v = gl ? gl[(size_t)b * K + j] : 0.f;
            if (gk) v += kk[(size_t)b * K + j] * (gk[(size_t)b * K + j] - dot) * inv_temp;
            col[b] = v;
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
        const float mv = mu[(size_t)j * D + d];
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc = fmaf(col[b], z[(size_t)b * D + d] - mv, acc);
        dmu[(size_t)j * D + d] = acc;
    }
}


// ---- the straight-through MODE_K values of the same HyperExtractor (gmgan_inference_cifar10.py:164-171, include/ggan.h GGAN_MODE_K_*):
//        STRAIGHT_THROUGHT_CONCRETE  s = the softmax above, h = one_hot(argmax s), k = (h - s) + s, s kept in `soft` for the backward
//        STRAIGHT_THROUGHT           h = one_hot(argmax logits), k = (h - logits) + logits              (no noise, no temperature)
//      The same launch shape as gmm_latent_fwd_k plus a block argmax (first index on a tie).  k is TF's float32
//      stop_gradient(h - v) + v, a subtraction then an addition (no fast-math in this build: the order holds): exactly 0 where h = 0,
//      fl(fl(1 - v) + v) at the argmax, which may miss 1 by an ulp of v (v = logits ~ -D under ST: ~1e-5).  (The CONCRETE kernels above
//      stay as they are: folding them into these templates compiled them to reordered instructions.) ----
enum { kModeKConcrete = 0, kModeKStc = 1, kModeKSt = 2 };            // include/ggan.h GGAN_MODE_K_*

// (value, index) argmax over the workgroup, the larger value or on a tie the smaller index (tf.argmax / np.argmax); best / arg:
// this thread's candidate, found over ascending indices with `>`.  Every thread returns the result.
__device__ __forceinline__ int block_argmax_first(float best, int arg, float* bv /* 4 */, int* bi /* 4 */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(arg, o, 64);
        if (ov > best || (ov == best && oi < arg)) { best = ov; arg = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = arg; }
    __syncthreads();
    best = bv[0];
    arg = bi[0];
    for (int w = 1; w < 4; ++w)
        if (bv[w] > best || (bv[w] == best && bi[w] < arg)) { best = bv[w]; arg = bi[w]; }
    return arg;
}

template <int MODE>
__global__ __launch_bounds__(256) void gmm_latent_st_fwd_k(const float* __restrict__ z, const float* __restrict__ mu,
                                                           const float* __restrict__ u, float* __restrict__ logits, float* __restrict__ k,
                                                           float* __restrict__ soft, int K, int D, float log_pi, float inv_temp) {
    __shared__ float sv[kGmmMaxK];
    __shared__ float red[32];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* zb = z + (size_t)b * D;
    for (int j = wave; j < K; j += 4) {
        const float* mj = mu + (size_t)j * D;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float t = zb[d] - mj[d];
            s = fmaf(t, t, s);
        }
        s = wave_sum(s);
        if (lane == 0) {
            const float lg = -0.5f * s + log_pi;
            if (logits) logits[(size_t)b * K + j] = lg;
            if constexpr (MODE == kModeKSt) {
                sv[j] = lg;
            } else {
                const float g = -logf(-logf(u[(size_t)b * K + j] + 1e-20f) + 1e-20f);
                sv[j] = (lg + g) * inv_temp;
            }
        }
    }
    __syncthreads();
    if constexpr (MODE == kModeKStc) {
        float m = -INFINITY;
        for (int j = threadIdx.x; j < K; j += 256) m = fmaxf(m, sv[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        float e = 0.f;
        for (int j = threadIdx.x; j < K; j += 256) {
            const float t = expf(sv[j] - m);
            sv[j] = t;
            e += t;
        }
        const float inv = 1.f / block_sum(e, red + 8);
        for (int j = threadIdx.x; j < K; j += 256) {          // (each thread rewrites only the j it reads below: no barrier)
            const float p = sv[j] * inv;                       // (the bits gmm_latent_fwd_k writes as k)
            soft[(size_t)b * K + j] = p;
            sv[j] = p;
        }
    }
    // argmax over sv (the float32 softmax output under STC, the logits under ST): ascending j per thread, `>` keeps the first
    float best = -INFINITY;
    int arg = 0x7FFFFFFF;
    for (int j = threadIdx.x; j < K; j += 256)
        if (sv[j] > best) { best = sv[j]; arg = j; }
    const int hot = block_argmax_first(best, arg, bv, bi);
    for (int j = threadIdx.x; j < K; j += 256) {
        const float v = sv[j], h = j == hot ? 1.f : 0.f;
        k[(size_t)b * K + j] = (h - v) + v;
    }
}

// Backward of STRAIGHT_THROUGHT: k = stop_gradient(h - logits) + logits hands dk to the logits unchanged,
// dlog[b, j] = gl[b, j] + gk[b, j]; then dz / dmu as in gmm_latent_bwd_k (blocks [0, B) rows, [B, B + K) components, dmu summed
// over the batch in row order: deterministic).  STRAIGHT_THROUGHT_CONCRETE needs no kernel of its own: it is gmm_latent_bwd_k on
// the saved soft s.
__global__ __launch_bounds__(256) void gmm_latent_st_bwd_k(const float* __restrict__ z, const float* __restrict__ mu,
                                                           const float* __restrict__ gl, const float* __restrict__ gk,
                                                           float* __restrict__ dz, float* __restrict__ dmu, int B, int K, int D) {
    __shared__ float sv[kGmmMaxK];
    if ((int)blockIdx.x < B) {
        const int b = blockIdx.x;
        for (int j = threadIdx.x; j < K; j += 256) {
            float v = gl ? gl[(size_t)b * K + j] : 0.f;
            if (gk) v += gk[(size_t)b * K + j];
            sv[j] = v;
        }
        __syncthreads();
        if (dz) {
            for (int d = threadIdx.x; d < D; d += 256) {
                const float zv = z[(size_t)b * D + d];
                float acc = 0.f;
                for (int j = 0; j < K; ++j) acc = fmaf(sv[j], zv - mu[(size_t)j * D + d], acc);
                dz[(size_t)b * D + d] = -acc;
            }
        }
        return;
    }
    if (!dmu) return;
    const int j = blockIdx.x - B;
    float* col = sv;                       // B <= kGmmMaxK values
    for (int b = threadIdx.x; b < B; b += 256) {
        float v = gl ? gl[(size_t)b * K + j] : 0.f;
        if (gk) v += gk[(size_t)b * K + j];
        col[b] = v;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
        const float mv = mu[(size_t)j * D + d];
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc = fmaf(col[b], z[(size_t)b * D + d] - mv, acc);
        dmu[(size_t)j * D + d] = acc;
    }
}


// ---- the test-set pass of the gmgan scripts (gmgan_inference_mnist.py:338,511-529): q_k_probs = softmax(q_k_logits) -- no Gumbel
//      noise, no temperature --, the row argmax (the sample's cluster) and the running column argmax over the whole test set (the
//      sample that labels each cluster).  A workgroup per row; the logits are summed exactly as gmm_latent_fwd_k sums them (same
//      bits).  Column argmax across launches: one 64-bit atomicMax per (row, component) on (p bits << 32 | ~row): p >= 0, so the
//      float's bits order like the float, and the complemented row makes the LOWEST row win a tie (np.argmax(prob_c, axis=0)). ----
__global__ __launch_bounds__(256) void gmm_posterior_assign_k(const float* __restrict__ z, const float* __restrict__ mu, float log_pi,
                                                              int K, int D, int row0, float* __restrict__ probs,
                                                              int32_t* __restrict__ assign, unsigned long long* __restrict__ colbest) {
    extern __shared__ float sv[];          // K values
    __shared__ float red[32];
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* zb = z + (size_t)b * D;
    for (int j = wave; j < K; j += 4) {
        const float* mj = mu + (size_t)j * D;
        float s = 0.f;
        for (int d = lane; d < D; d += 64) {
            const float t = zb[d] - mj[d];
            s = fmaf(t, t, s);
        }
        s = wave_sum(s);
        if (lane == 0) sv[j] = -0.5f * s + log_pi;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = threadIdx.x; j < K; j += 256) m = fmaxf(m, sv[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float e = 0.f;
    for (int j = threadIdx.x; j < K; j += 256) {
        const float t = expf(sv[j] - m);
        sv[j] = t;
        e += t;
    }
    const float inv = 1.f / block_sum(e, red + 8);
    const unsigned grow = (unsigned)(row0 + b);
    const unsigned long long low = 0xFFFFFFFFull - grow;
    float best = -1.f;
    int arg = 0;
    for (int j = threadIdx.x; j < K; j += 256) {
        const float p = sv[j] * inv;
        if (probs) probs[(size_t)b * K + j] = p;
        if (p > best) { best = p; arg = j; }            // (ascending j per thread: the first index wins a tie)
        atomicMax(colbest + j, ((unsigned long long)__float_as_uint(p) << 32) | low);
    }
    // row argmax: larger p, on a tie the smaller index (np.argmax)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(arg, o, 64);
        if (ov > best || (ov == best && oi < arg)) { best = ov; arg = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = arg; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (bv[w] > best || (bv[w] == best && bi[w] < arg)) { best = bv[w]; arg = bi[w]; }
        assign[grow] = arg;
    }
}

// Label propagation and the match count of gmgan_inference_mnist.py:518-528 in one workgroup: label_of[j] = labels[row of colbest[j]],
// correct = #{b : label_of[assign[b]] == labels[b]} (an integer: the same on every run).
__global__ __launch_bounds__(256) void cluster_accuracy_k(const int32_t* __restrict__ assign, const int32_t* __restrict__ labels,
                                                          const unsigned long long* __restrict__ colbest, int N, int K,
                                                          int32_t* __restrict__ correct) {
    extern __shared__ int label_of[];      // K values
    __shared__ int red[4];
    for (int j = threadIdx.x; j < K; j += 256) {
        const unsigned row = 0xFFFFFFFFu - (unsigned)(colbest[j] & 0xFFFFFFFFull);
        label_of[j] = row < (unsigned)N ? labels[row] : (-2147483647 - 1);      // (an unwritten column: a label nothing carries)
    }
    __syncthreads();
    int n = 0;
    for (int b = threadIdx.x; b < N; b += 256) {
        const int a = assign[b];
        n += (a >= 0 && a < K && label_of[a] == labels[b]) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) correct[0] = red[0] + red[1] + red[2] + red[3];
}


// ---- all the noise of one session.run in ONE launch (the TF graph draws p_z ~ N(0,1), k ~ Cat(1/K) as a one-hot, Gumbel U, the GP
//      alpha and the dequantisation noise with separate random ops: gmgan_inference_cifar10.py:115-120,344-346).  Counter-based
//      generator (Philox4x32-10, key = seed, counter = (element group, tensor, draw number)); the draw number lives in device
//      memory and is advanced by the last workgroup to arrive, so a captured graph produces fresh noise on every replay. ----
struct NoiseTable {
    float* dst[GGAN_NOISE_MAX];
    unsigned n[GGAN_NOISE_MAX];
    int kind[GGAN_NOISE_MAX];      // 0 normal(a, b) = a + b*N(0,1); 1 uniform (a, b) for a = 0, else [a, b]; 2 one-hot rows of width K (n = rows * K)
    float a[GGAN_NOISE_MAX], b[GGAN_NOISE_MAX];
    int K[GGAN_NOISE_MAX];
    int slot[GGAN_NOISE_MAX];      // the tensor's ordinal within the step's draw (part of the counter): its index
    int step[GGAN_NOISE_MAX];      // draw number = state + step (always 0: one session.run per launch)
    int count, advance;
};

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// (0, 1): 2^-25 .. 1 - 2^-24.  16777215 + 0.5 is no float32 and rounds to 2^24, so the top word would give exactly 1; the fminf moves
// that one value and no other.
__device__ __forceinline__ float u01(unsigned x) { return fminf(((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f), 0.99999994f); }

__global__ __launch_bounds__(256) void noise_fill_k(const NoiseTable t, unsigned long long* __restrict__ state) {
    const int tb = blockIdx.y, ti = t.slot[tb];
    const unsigned long long seed = state[0], draw0 = state[1], draw = draw0 + (unsigned long long)t.step[tb];
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    float* dst = t.dst[tb];
    const unsigned n = t.n[tb];
    const int kind = t.kind[tb];
    for (unsigned g = blockIdx.x * 256 + threadIdx.x; g * 4 < n; g += gridDim.x * 256) {
        unsigned r[4];
        float v[4];
        if (kind == 2) {
            // element e of a one-hot row: the row's component index comes from a draw keyed by the ROW
            const int K = t.K[tb];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned e = g * 4 + q, row = e / (unsigned)K, col = e - row * (unsigned)K;
                philox4x32_10(row, (unsigned)ti | 0x80000000u, (unsigned)draw, (unsigned)(draw >> 32), k0, k1, r);
                const unsigned idx = min((unsigned)(u01(r[0]) * (float)K), (unsigned)K - 1u);
                v[q] = col == idx ? 1.f : 0.f;
            }
        } else {
            philox4x32_10(g, (unsigned)ti, (unsigned)draw, (unsigned)(draw >> 32), k0, k1, r);
            if (kind == 0) {            // Box-Muller, two pairs
                const float r0 = sqrtf(-2.f * logf(u01(r[0]))), r1 = sqrtf(-2.f * logf(u01(r[2])));
                float s0, c0, s1, c1;
                sincosf(6.28318530718f * u01(r[1]), &s0, &c0);
                sincosf(6.28318530718f * u01(r[3]), &s1, &c1);
                v[0] = t.a[tb] + t.b[tb] * r0 * c0; v[1] = t.a[tb] + t.b[tb] * r0 * s0;
                v[2] = t.a[tb] + t.b[tb] * r1 * c1; v[3] = t.a[tb] + t.b[tb] * r1 * s1;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = t.a[tb] + (t.b[tb] - t.a[tb]) * u01(r[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (g * 4 + q < n) dst[g * 4 + q] = v[q];
    }
    // every workgroup has read `draw` before it arrives here; the last one advances it.  (No fence: nothing is PUBLISHED to the
    // other workgroups -- the arrival count only orders "all have read draw" before "draw is overwritten", and every thread's use
    // of `draw` precedes its workgroup's barrier.  A __threadfence() per workgroup cost 16 us on the 512-workgroup launches.)
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long total = (unsigned long long)gridDim.x * gridDim.y;
        const unsigned long long prev = atomicAdd(&state[2], 1ull);
        if (prev == total - 1) {
            state[1] = draw0 + (unsigned long long)t.advance;
            state[2] = 0;
        }
    }
}

}  // namespace

extern "C" {

int ggan_mix_mean(const float* k, const float* mu, const float* noise, float* out, int B, int K, int D, ggan_stream_t stream) {
    GGAN_CHECK_ARG(k && mu && noise && out && B > 0 && K > 0 && D > 0, "bad argument");
    GGAN_CHECK_ARG((D & 3) == 0 && !(((uintptr_t)mu | (uintptr_t)noise | (uintptr_t)out) & 15), "D a multiple of 4, 16-byte aligned buffers");
    const int n = B * (D / 4);
    GGAN_LAUNCH("mix_mean", 2.0 * B * K * D, 4.0 * (2.0 * B * D + (double)K * D), mix_mean_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, k,
                mu, noise, out, B, K, D / 4);
    return 0;
}

int ggan_gmm_latent_fwd(const float* z, const float* mu, const float* gumbel_u, float* logits, float* k, int B, int K, int D,
                        float log_pi, float temp, ggan_stream_t stream) {
    GGAN_CHECK_ARG(z && mu && gumbel_u && k, "null pointer");
    GGAN_CHECK_ARG(B > 0 && K > 0 && K <= kGmmMaxK && D > 0 && temp > 0.f, "bad shape");
    GGAN_LAUNCH("gmm_latent_fwd", 3.0 * B * K * D, 0, gmm_latent_fwd_k, dim3(B), dim3(256), 0, (hipStream_t)stream, z, mu, gumbel_u, logits, k,
                K, D, log_pi, 1.f / temp);
    return 0;
}

int ggan_gmm_latent_bwd(const float* z, const float* mu, const float* k, const float* g_logits, const float* g_k, float* dz,
                        float* dmu, int B, int K, int D, float temp, ggan_stream_t stream) {
    GGAN_CHECK_ARG(z && mu && k && (g_logits || g_k) && (dz || dmu), "null pointer");
    GGAN_CHECK_ARG(B > 0 && B <= kGmmMaxK && K > 0 && K <= kGmmMaxK && D > 0 && temp > 0.f, "bad shape");
    GGAN_LAUNCH("gmm_latent_bwd", 4.0 * B * K * D, 0, gmm_latent_bwd_k, dim3(B + (dmu ? K : 0)), dim3(256), 0, (hipStream_t)stream, z, mu, k,
                g_logits, g_k, dz, dmu, B, K, D, 1.f / temp);
    return 0;
}

int ggan_gmm_latent_st_fwd(const float* z, const float* mu, const float* gumbel_u, float* logits, float* k, float* soft, int B, int K,
                           int D, float log_pi, float temp, int mode, ggan_stream_t stream) {
    GGAN_CHECK_ARG(mode == GGAN_MODE_K_STC || mode == GGAN_MODE_K_ST, "mode is not a straight-through MODE_K");
    GGAN_CHECK_ARG(z && mu && k && (mode == GGAN_MODE_K_ST || (gumbel_u && soft)), "null pointer");
    GGAN_CHECK_ARG(B > 0 && K > 0 && K <= kGmmMaxK && D > 0 && (mode == GGAN_MODE_K_ST || temp > 0.f), "bad shape");
    if (mode == GGAN_MODE_K_STC) {
        GGAN_LAUNCH("gmm_latent_stc_fwd", 3.0 * B * K * D, 0, gmm_latent_st_fwd_k<kModeKStc>, dim3(B), dim3(256), 0, (hipStream_t)stream, z,
                    mu, gumbel_u, logits, k, soft, K, D, log_pi, 1.f / temp);
    } else {
        GGAN_LAUNCH("gmm_latent_st_fwd", 3.0 * B * K * D, 0, gmm_latent_st_fwd_k<kModeKSt>, dim3(B), dim3(256), 0, (hipStream_t)stream, z,
                    mu, nullptr, logits, k, nullptr, K, D, log_pi, 1.f);
    }
    return 0;
}

int ggan_gmm_latent_st_bwd(const float* z, const float* mu, const float* soft, const float* g_logits, const float* g_k, float* dz,
                           float* dmu, int B, int K, int D, float temp, int mode, ggan_stream_t stream) {
    GGAN_CHECK_ARG(mode == GGAN_MODE_K_STC || mode == GGAN_MODE_K_ST, "mode is not a straight-through MODE_K");
    GGAN_CHECK_ARG(z && mu && (mode == GGAN_MODE_K_ST || soft) && (g_logits || g_k) && (dz || dmu), "null pointer");
    GGAN_CHECK_ARG(B > 0 && B <= kGmmMaxK && K > 0 && K <= kGmmMaxK && D > 0 && (mode == GGAN_MODE_K_ST || temp > 0.f), "bad shape");
    if (mode == GGAN_MODE_K_STC)          // the CONCRETE backward on the soft assignment the forward kept
        return ggan_gmm_latent_bwd(z, mu, soft, g_logits, g_k, dz, dmu, B, K, D, temp, stream);
    GGAN_LAUNCH("gmm_latent_st_bwd", 2.0 * B * K * D, 0, gmm_latent_st_bwd_k, dim3(B + (dmu ? K : 0)), dim3(256), 0, (hipStream_t)stream, z,
                mu, g_logits, g_k, dz, dmu, B, K, D);
    return 0;
}

int ggan_gmm_posterior_assign(const float* z, const float* mu, float log_pi, int B, int K, int D, int row0, float* probs,
                              int32_t* assign, uint64_t* colbest, ggan_stream_t stream) {
    GGAN_CHECK_ARG(z && mu && assign && colbest, "null pointer");
    GGAN_CHECK_ARG(B > 0 && K > 0 && K <= GGAN_POSTERIOR_MAX_K && D > 0 && row0 >= 0 && (long long)row0 + B <= 0x7FFFFFFFll, "bad shape");
    GGAN_LAUNCH("gmm_posterior_assign", 3.0 * B * K * D, 4.0 * ((double)B * D + (double)K * D + (probs ? (double)B * K : 0.0)),
                gmm_posterior_assign_k, dim3(B), dim3(256), (size_t)K * sizeof(float), (hipStream_t)stream, z, mu, log_pi, K, D, row0,
                probs, assign, (unsigned long long*)colbest);
    return 0;
}

int ggan_cluster_accuracy(const int32_t* assign, const int32_t* labels, const uint64_t* colbest, int N, int K, int32_t* correct,
                          ggan_stream_t stream) {
    GGAN_CHECK_ARG(assign && labels && colbest && correct, "null pointer");
    GGAN_CHECK_ARG(N > 0 && K > 0 && K <= GGAN_POSTERIOR_MAX_K, "bad shape");
    GGAN_LAUNCH("cluster_accuracy", 0, 8.0 * N + 12.0 * K, cluster_accuracy_k, dim3(1), dim3(256), (size_t)K * sizeof(int), (hipStream_t)stream,
                assign, labels, (const unsigned long long*)colbest, N, K, correct);
    return 0;
}

int ggan_noise_fill(float* const* dsts, const size_t* sizes, const int* kinds, const float* a, const float* b, const int* widths,
                    int count, uint64_t* state, ggan_stream_t stream) {
    GGAN_CHECK_ARG(dsts && sizes && kinds && a && b && widths && state, "null pointer");
    GGAN_CHECK_ARG(count > 0 && count <= GGAN_NOISE_MAX, "count out of range");
    NoiseTable t;
    size_t mx = 0, tot = 0;
    for (int i = 0; i < count; ++i) {
        GGAN_CHECK_ARG(dsts[i] && sizes[i] > 0 && sizes[i] < 0x7FFFFFFFull && kinds[i] >= 0 && kinds[i] <= 2, "bad noise spec");
        GGAN_CHECK_ARG(kinds[i] != 2 || (widths[i] > 0 && sizes[i] % (size_t)widths[i] == 0), "one-hot rows need a width dividing the size");
        t.dst[i] = dsts[i]; t.n[i] = (unsigned)sizes[i]; t.kind[i] = kinds[i]; t.a[i] = a[i]; t.b[i] = b[i]; t.K[i] = widths[i];
        t.slot[i] = i;
        t.step[i] = 0;
        if (sizes[i] > mx) mx = sizes[i];
        tot += sizes[i];
    }
    t.count = count;
    t.advance = 1;
    int gx = (int)cdivz(mx, (size_t)1024);
    if (gx < 1) gx = 1;
    if (gx > 256) gx = 256;
    GGAN_LAUNCH("noise_fill", 0, 4.0 * tot, noise_fill_k, dim3(gx, count), dim3(256), 0, (hipStream_t)stream, t, (unsigned long long*)state);
    return 0;
}

}  // extern "C"
