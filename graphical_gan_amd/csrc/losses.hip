// The costs of the training step: BCE / Wasserstein (mean) terms, reconstruction distances, the gradient penalty, the
// training MMD^2 between two sets of codes and the aggregated-posterior divergences.  Single-workgroup or workgroup-per-row
// reductions, every sum in a fixed order.
#include "common.h"
#include "cost_head.h"
#include "pointwise.h"
using namespace ggan;

namespace {

// ---- losses (single block: n is a minibatch of logits).  The expressions and their order: cost_head.h ------------------------
__global__ void bce_fwd_k(const float* __restrict__ x, float z, float weight, float* __restrict__ loss, int n,
                          int accumulate) {
    __shared__ float sm[32];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += bce_value(x[i], z);
    s = block_sum(s, sm);
    if (threadIdx.x == 0) store_weighted_mean(loss, weight, s, (float)n, accumulate);
}

__global__ void bce_bwd_k(const float* __restrict__ x, float z, float weight, const float* __restrict__ gloss,
                          float* __restrict__ gx, int n) {
    const float g = gloss[0] * weight / (float)n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) gx[i] = bce_grad(g, x[i], z);
}

// all terms of one cost in ONE launch: loss = sum_i w_i * mean(bce(x_i, z_i)) (or mean(x_i): the Wasserstein costs)
struct BceTable {
    const float* x[GGAN_BCE_MAX];
    float* gx[GGAN_BCE_MAX];   // optional: the gradient for a unit upstream gradient (bce_multi_bwd_k / mean_bwd_k with gloss == 1)
    float z[GGAN_BCE_MAX];
    float w[GGAN_BCE_MAX];
    int n[GGAN_BCE_MAX];
    int count;
};

// the cost of a table on this workgroup, terms in order: the same summation order as one accumulating launch per term
__device__ __forceinline__ float table_cost(const BceTable& t, bool mean, float* sm) {
    float tot = 0.f;
    for (int k = 0; k < t.count; ++k) {
        const float* x = t.x[k];
        const float z = t.z[k];
        float* gx = t.gx[k];
        const float w = t.w[k];
        const int n = t.n[k];
        tot = cost_add_term(tot, k, mean, x, n, z, w, gx, blockDim.x, true, sm);
    }
    return tot;
}

__global__ void bce_multi_fwd_k(BceTable t, float* __restrict__ loss) {
    __shared__ float sm[32];
    const float tot = table_cost(t, false, sm);
    if (threadIdx.x == 0) loss[0] = tot;
}

// bce_multi_fwd_k with unit-seed gradients AND the row-local part of the critic head's backward (head_out_bwd_k, gemm.hip) in one
// launch: the logits of a cost are the output of ONE critic head (terms = consecutive row ranges of its logits), the cost's
// gradient for a unit upstream gradient is row-local, so  gh[r,c] = g[r] * w_out[c] * lrelu'(h[r,c]),  d_wout[c] = sum_r g[r] h[r,c]
// and d_bout = sum_r g[r]  need nothing but the logits.  Workgroup 0 is bce_multi_fwd_k (loss, g); workgroups 1.. are head_out_bwd_k
// with g[r] formed on the fly into LDS.  Saves the head kernel's launch on the critical chain of every BCE step (tail GEMM ->
// logits -> cost -> head backward -> products).
struct BceHead {
    const float* h;
    const float* w_out;
    float* gh;
    float* d_wout;
    float* d_bout;
    float alpha;
    int M, H;
    int k0, k1;             // its terms [k0, k1) of the table: consecutive row ranges of its logits
    int first;              // its first workgroup
};
struct BceHeads { BceHead hd[GGAN_BCE_HEADS]; int count; };

__global__ __launch_bounds__(256) void bce_head_bwd_k(BceTable t, float* __restrict__ loss, const BceHeads hs) {
    __shared__ float sm[32];
    __shared__ float red[16][16];
    __shared__ float gs_[GGAN_HEAD_BCE_MAX_ROWS];
    if (blockIdx.x == 0) {
        const float tot = table_cost(t, false, sm);
        if (threadIdx.x == 0) loss[0] = tot;
        return;
    }
    const int hi = (hs.count > 1 && (int)blockIdx.x >= hs.hd[1].first) ? 1 : 0;
    const BceHead& hd = hs.hd[hi];
    // (the head's fields now, not at the call below: their loads then overlap the loop that forms g)
    const float* __restrict__ h = hd.h;
    const float* __restrict__ w_out = hd.w_out;
    float* __restrict__ gh = hd.gh;
    float* __restrict__ d_wout = hd.d_wout;
    float* __restrict__ d_bout = hd.d_bout;
    const float alpha = hd.alpha;
    const int M = hd.M, H = hd.H;
    // g of every row (the head's terms are consecutive row ranges of its logits, in order)
    {
        int r0 = 0;
        for (int k = hd.k0; k < hd.k1; ++k) {
            const float g = unit_seed(t.w[k], t.n[k]), z = t.z[k];
            for (int i = threadIdx.x; i < t.n[k]; i += blockDim.x) gs_[r0 + i] = bce_grad(g, t.x[k][i], z);
            r0 += t.n[k];
        }
    }
    __syncthreads();
    const int tid = threadIdx.x, c = ((int)blockIdx.x - hd.first) * 16 + (tid & 15);
    head_columns<true>(gs_, h, w_out, alpha, gh, d_wout, d_bout, (int)blockIdx.x == hd.first, M, H, c, tid, tid >> 4, true, red);
}

__global__ void bce_multi_bwd_k(BceTable t, const float* __restrict__ gloss) {
    const int k = blockIdx.y;
    const int n = t.n[k];
    const float g = gloss[0] * t.w[k] / (float)n, z = t.z[k];
    const float* x = t.x[k];
    float* gx = t.gx[k];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) gx[i] = bce_grad(g, x[i], z);
}

// reconstruction distances of tflib/utils/distance.py: mean(|x-y|^p), p = 1 | 2, one workgroup (n <= a few 100 K)
__global__ void dist_fwd_k(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out, size_t n, int p,
                           float weight, int accumulate) {
    __shared__ float sm[32];
    float s = 0.f;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float d = x[i] - y[i];
        s += p == 2 ? d * d : fabsf(d);
    }
    s = block_sum(s, sm);
    if (threadIdx.x == 0) store_weighted_mean(out, weight, s, (float)n, accumulate);
}

__global__ void dist_bwd_k(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ gout,
                           float* __restrict__ gx, float* __restrict__ gy, size_t n, int p, float weight) {
    const float g = gout[0] * weight / (float)n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float d = x[i] - y[i];
        const float v = g * (p == 2 ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)));
        if (gx) gx[i] = v;
        if (gy) gy[i] = -v;
    }
}

__global__ void mean_fwd_k(const float* __restrict__ x, float weight, float* __restrict__ loss, int n, int accumulate) {
    __shared__ float sm[32];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += x[i];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) store_weighted_mean(loss, weight, s, (float)n, accumulate);
}

__global__ void mean_multi_fwd_k(BceTable t, float* __restrict__ loss) {
    __shared__ float sm[32];
    const float tot = table_cost(t, true, sm);
    if (threadIdx.x == 0) loss[0] = tot;
}

__global__ void mean_bwd_k(const float* __restrict__ gloss, float weight, float* __restrict__ gx, int n) {
    const float g = gloss[0] * weight / (float)n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) gx[i] = g;
}

// one block per sample row: slopes[b] = ||g[b,:]||_2
__global__ void gp_slopes_k(const float* __restrict__ g, float* __restrict__ slopes, int D) {
    __shared__ float sm[32];
    const float* row = g + (size_t)blockIdx.x * D;
    float s = 0.f;
    for (int i = threadIdx.x; i < D; i += blockDim.x) s += row[i] * row[i];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) slopes[blockIdx.x] = sqrtf(s);
}

__global__ void gp_pen_k(const float* __restrict__ slopes, float* __restrict__ pen, int B, float lam) {
    __shared__ float sm[32];
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        float d = slopes[i] - 1.f;
        s += d * d;
    }
    s = block_sum(s, sm);
    if (threadIdx.x == 0) pen[0] = lam * (s / (float)B);
}

// gp_slopes_k + gp_pen_k + gp_bwd_k for a unit upstream gradient in ONE launch: a workgroup per row computes its norm, writes the
// row of d(pen)/dg, and the LAST workgroup to arrive (counter in `arrive`, left zero) forms the penalty from all slopes with the same
// fixed-order block sum as gp_pen_k -- deterministic.
__global__ void gp_fwd_grad_k(const float* __restrict__ g, float* __restrict__ slopes, float* __restrict__ pen, float* __restrict__ gg,
                              int32_t* __restrict__ arrive, int B, int D, float lam) {
    __shared__ float sm[32];
    __shared__ int last;
    const int b = blockIdx.x;
    const float* row = g + (size_t)b * D;
    float s = 0.f;
    for (int i = threadIdx.x; i < D; i += blockDim.x) s += row[i] * row[i];
    s = block_sum(s, sm);
    const float sl = sqrtf(s);
    const float coef = lam * 2.f * (sl - 1.f) / ((float)B * sl);
    float* orow = gg + (size_t)b * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) orow[i] = coef * row[i];
    if (threadIdx.x == 0) {
        __hip_atomic_store(slopes + b, sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = atomicAdd(arrive, 1) == B - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    float t = 0.f;
    for (int i = threadIdx.x; i < B; i += blockDim.x) {
        const float d = __hip_atomic_load(slopes + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1.f;
        t += d * d;
    }
    t = block_sum(t, sm);
    if (threadIdx.x == 0) {
        pen[0] = lam * (t / (float)B);
        arrive[0] = 0;
    }
}

__global__ void gp_bwd_k(const float* __restrict__ g, const float* __restrict__ slopes, const float* __restrict__ gpen,
                         float* __restrict__ gg, int B, int D, float lam) {
    const int b = blockIdx.x;
    const float s = slopes[b];
    const float coef = gpen[0] * lam * 2.f * (s - 1.f) / ((float)B * s);
    const float* row = g + (size_t)b * D;
    float* orow = gg + (size_t)b * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) orow[i] = coef * row[i];
}

// ---- biased MMD^2 with a mixture of RBF kernels between two sets of codes (MODE vegan-mmd: tflib/objs/mmd.py:20-71,
//      mix_rbf_mmd2(q_z, p_z), sigmas 2..80): k(a, b) = sum_s wt_s exp(-gamma_s ||a-b||^2), gamma_s = 1/(2 sigma_s^2),
//      mmd2 = mean k(X,X) + mean k(Y,Y) - 2 mean k(X,Y).  The TF graph builds three Gram matrices and 18 exp maps; here the
//      pairwise distances are formed on the fly.  One workgroup per row of Z = [X; Y] computes that row's weighted kernel sum
//      (forward: into a per-row partial, summed in row order by the last stage) or its gradient row (backward). ----
constexpr int kMmdMaxSigmas = 8;
struct MmdParams {
    const float* X;
    const float* Y;
    int m, n, d, ns;
    float gamma[kMmdMaxSigmas], wt[kMmdMaxSigmas];
    int unbiased;      // mmd.py:53-61: the diagonal of the same-set blocks is left out, the means are over m (m - 1) and n (n - 1) pairs
};

__device__ __forceinline__ const float* mmd_row(const MmdParams& P, int r) { return r < P.m ? P.X + (size_t)r * P.d : P.Y + (size_t)(r - P.m) * P.d; }

// coefficient of k(z_r, z_j) in mmd2 seen from row r: 1/m^2 (both in X), 1/n^2 (both in Y), -1/(mn) (mixed: each unordered mixed
// pair is visited from both sides, which makes the -2/(mn) of the definition)
__device__ __forceinline__ float mmd_coef(const MmdParams& P, int r, int j) {
    const bool rx = r < P.m, jx = j < P.m;
    if (P.unbiased && rx == jx) {
        if (r == j) return 0.f;
        return rx ? 1.f / ((float)P.m * (float)(P.m - 1)) : 1.f / ((float)P.n * (float)(P.n - 1));
    }
    if (rx && jx) return 1.f / ((float)P.m * (float)P.m);
    if (!rx && !jx) return 1.f / ((float)P.n * (float)P.n);
    return -1.f / ((float)P.m * (float)P.n);
}

__global__ __launch_bounds__(256) void mmd2_rows_k(const MmdParams P, float* __restrict__ partial) {
    __shared__ float sm[32];
    const int r = blockIdx.x, tot = P.m + P.n;
    const float* zr = mmd_row(P, r);
    float acc = 0.f;
    for (int j = threadIdx.x; j < tot; j += 256) {
        const float* zj = mmd_row(P, j);
        float dist = 0.f;
        for (int k = 0; k < P.d; ++k) {
            const float t = zr[k] - zj[k];
            dist = fmaf(t, t, dist);
        }
        float kv = 0.f;
        for (int s2 = 0; s2 < P.ns; ++s2) kv += P.wt[s2] * expf(-P.gamma[s2] * dist);
        acc += mmd_coef(P, r, j) * kv;
    }
    const float t = block_sum(acc, sm);
    if (threadIdx.x == 0) partial[r] = t;
}

__global__ __launch_bounds__(256) void mmd2_final_k(const float* __restrict__ partial, int tot, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float s2 = 0.f;
        for (int r = 0; r < tot; ++r) s2 += partial[r];          // row order: deterministic
        out[0] = s2;
    }
}

// gradient row r: sum_j 2 * coef(r, j) * (-2 G_rj) (z_r - z_j) with G_rj = sum_s wt_s gamma_s exp(-gamma_s D_rj)
// (the factor 2: the pair (r, j) enters the double sum as (r, j) and as (j, r))
__global__ __launch_bounds__(256) void mmd2_bwd_k(const MmdParams P, const float* __restrict__ gout, float* __restrict__ dX,
                                                  float* __restrict__ dY) {
    __shared__ float cf[512];
    const int r = blockIdx.x, tot = P.m + P.n;
    const float* zr = mmd_row(P, r);
    const float go = gout[0];
    for (int j = threadIdx.x; j < tot; j += 256) {
        const float* zj = mmd_row(P, j);
        float dist = 0.f;
        for (int k = 0; k < P.d; ++k) {
            const float t = zr[k] - zj[k];
            dist = fmaf(t, t, dist);
        }
        float gv = 0.f;
        for (int s2 = 0; s2 < P.ns; ++s2) gv += P.wt[s2] * P.gamma[s2] * expf(-P.gamma[s2] * dist);
        cf[j] = -4.f * mmd_coef(P, r, j) * gv * go;
    }
    __syncthreads();
    float* dst = r < P.m ? (dX ? dX + (size_t)r * P.d : nullptr) : (dY ? dY + (size_t)(r - P.m) * P.d : nullptr);
    if (!dst) return;
    for (int k = threadIdx.x; k < P.d; k += 256) {
        const float zv = zr[k];
        float acc = 0.f;
        for (int j = 0; j < tot; ++j) acc = fmaf(cf[j], zv - mmd_row(P, j)[k], acc);
        dst[k] = acc;
    }
}

// ---- tflib/objs/kl_aggregated.py: KL / inverse KL / JSD between the aggregated posterior (equal-weight mixture of the minibatch's nx
// diagonal Gaussians) and the N(0, I) prior on nz Monte-Carlo samples.  kind 0 kl (samples from q), 1 ikl (samples from p), 2 jsd
// (both: rows [0, nz) from q, [nz, 2nz) from p).  One block per sample; every reduction in a fixed order.
struct AggP {
    const float *mu, *sd, *k, *eps_q, *z_p;
    int kind, nx, nz, d, n_coms;
};
#define GGAN_LOG2PI 1.8378770664093453f

__device__ __forceinline__ float block_max(float v, float* smem) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) smem[wid] = v;
    __syncthreads();
    float t = smem[0];
    for (int i = 1; i < nw; ++i) t = fmaxf(t, smem[i]);
    return t;
}

__global__ __launch_bounds__(128) void agg_div_fwd_k(const AggP P, float* __restrict__ Z, float* __restrict__ A, float* __restrict__ Bv,
                                                      float* __restrict__ T) {
    extern __shared__ float zs[];          // d
    __shared__ float red[20];
    const int i = blockIdx.x, nx = P.nx, d = P.d;
    const bool qs = P.kind == 0 || (P.kind == 2 && i < P.nz);
    const int ip = P.kind == 2 ? i - P.nz : i;
    float part = 0.f;
    for (int dd = threadIdx.x; dd < d; dd += blockDim.x) {
        float z;
        if (qs) {                           // mixture_gaussian (:6-16): k @ mu + (k @ std) * eps, k one-hot
            float m = 0.f, sg = 0.f;
            for (int j = 0; j < nx; ++j) {
                const float kk = P.k[(size_t)i * nx + j];
                m = fmaf(kk, P.mu[(size_t)j * d + dd], m);
                sg = fmaf(kk, P.sd[(size_t)j * d + dd], sg);
            }
            z = fmaf(sg, P.eps_q[(size_t)i * d + dd], m);
        } else {
            z = P.z_p[(size_t)ip * d + dd];
        }
        zs[dd] = z;
        Z[(size_t)i * d + dd] = z;
        part += z * z + GGAN_LOG2PI;
    }
    const float b = -0.5f * block_sum(part, red);       // log N(z; 0, I)   (also orders the zs writes before the reads below)
    float lmax = -3.0e38f;
    for (int j = threadIdx.x; j < nx; j += blockDim.x) {
        float acc = 0.f;
        for (int dd = 0; dd < d; ++dd) {
            const float sg = P.sd[(size_t)j * d + dd], r = (zs[dd] - P.mu[(size_t)j * d + dd]) / sg;
            acc += r * r + GGAN_LOG2PI + 2.f * logf(sg);
        }
        const float a = -0.5f * acc;
        A[(size_t)i * nx + j] = a;
        lmax = fmaxf(lmax, a);
    }
    // (as the reference: log q is shifted by ITS row maximum (:26-29), the mixture m by the maximum over its own terms (:41-44) -- a
    // common shift would underflow sum exp(a_j) to 0 wherever the prior term dominates)
    const float mq = block_max(lmax, red);
    float se = 0.f;
    for (int j = threadIdx.x; j < nx; j += blockDim.x) se += expf(A[(size_t)i * nx + j] - mq);
    const float Sq = block_sum(se, red);
    if (threadIdx.x == 0) {
        const float lq = mq + logf(Sq) - logf((float)nx);
        float t;
        if (P.kind == 0) t = lq - b;
        else if (P.kind == 1) t = b - lq;
        else {
            const float mm = fmaxf(mq, b);
            const float lm = mm + logf(Sq * expf(mq - mm) + (float)P.n_coms * expf(b - mm)) - logf((float)(nx + P.n_coms));
            t = qs ? 0.5f * (lq - lm) : 0.5f * (b - lm);
        }
        T[i] = t;
        Bv[i] = b;
    }
}

__global__ void agg_div_final_k(const float* __restrict__ T, int ns, int nz, float* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < ns; ++i) s += T[i];           // sample order: deterministic
        out[0] = s / (float)nz;
    }
}

// stage A (block per sample): W[i][j] = dL/da_ij, GZ[i][:] = dL/dz_i for the samples drawn from q (they depend on mu / std)
__global__ __launch_bounds__(128) void agg_div_bwd_samples_k(const AggP P, const float* __restrict__ Z, const float* __restrict__ A,
                                                              const float* __restrict__ Bv, const float* __restrict__ gout,
                                                              float* __restrict__ W, float* __restrict__ GZ) {
    extern __shared__ float ws[];          // nx
    __shared__ float red[20];
    const int i = blockIdx.x, nx = P.nx, d = P.d;
    const bool qs = P.kind == 0 || (P.kind == 2 && i < P.nz);
    const float b = Bv[i], gs = gout[0] / (float)P.nz;
    float lmax = -3.0e38f;
    for (int j = threadIdx.x; j < nx; j += blockDim.x) lmax = fmaxf(lmax, A[(size_t)i * nx + j]);
    const float mq = block_max(lmax, red);
    float se = 0.f;
    for (int j = threadIdx.x; j < nx; j += blockDim.x) se += expf(A[(size_t)i * nx + j] - mq);
    const float Sq = block_sum(se, red);
    const float mm = P.kind == 2 ? fmaxf(mq, b) : mq;                       // shift of the mixture m (jsd)
    const float pe = (float)P.n_coms * expf(b - mm), M = Sq * expf(mq - mm) + pe;
    for (int j = threadIdx.x; j < nx; j += blockDim.x) {
        const float a = A[(size_t)i * nx + j], rq = expf(a - mq) / Sq;      // responsibility under q
        float w;
        if (P.kind == 0) w = rq;
        else if (P.kind == 1) w = -rq;
        else {
            const float rm = expf(a - mm) / M;                                // ... under m
            w = qs ? 0.5f * (rq - rm) : -0.5f * rm;
        }
        w *= gs;
        ws[j] = w;
        W[(size_t)i * nx + j] = w;
    }
    __syncthreads();
    if (!qs) return;
    const float v = gs * (P.kind == 0 ? -1.f : -0.5f * pe / M);      // dL/db; db/dz = -z
    for (int dd = threadIdx.x; dd < d; dd += blockDim.x) {
        const float z = Z[(size_t)i * d + dd];
        float acc = -v * z;
        for (int j = 0; j < nx; ++j) {
            const float sg = P.sd[(size_t)j * d + dd];
            acc -= ws[j] * (z - P.mu[(size_t)j * d + dd]) / (sg * sg);
        }
        GZ[(size_t)i * d + dd] = acc;
    }
}

// stage B (block per component j): the direct terms of every sample, then the samples drawn from this component (through z)
__global__ __launch_bounds__(128) void agg_div_bwd_comps_k(const AggP P, int ns, const float* __restrict__ Z, const float* __restrict__ W,
                                                            const float* __restrict__ GZ, float* __restrict__ gmu, float* __restrict__ gsd) {
    const int j = blockIdx.x, nx = P.nx, d = P.d;
    const int nq = P.kind == 1 ? 0 : P.nz;
    for (int dd = threadIdx.x; dd < d; dd += blockDim.x) {
        const float m = P.mu[(size_t)j * d + dd], sg = P.sd[(size_t)j * d + dd], i2 = 1.f / (sg * sg);
        float gm = 0.f, gsg = 0.f;
        for (int i = 0; i < ns; ++i) {
            const float w = W[(size_t)i * nx + j], r = Z[(size_t)i * d + dd] - m;
            gm = fmaf(w, r * i2, gm);
            gsg = fmaf(w, r * r * i2 / sg - 1.f / sg, gsg);
        }
        for (int i = 0; i < nq; ++i) {
            const float kk = P.k[(size_t)i * nx + j];
            if (kk != 0.f) {
                const float gz = kk * GZ[(size_t)i * d + dd];
                gm += gz;
                gsg = fmaf(gz, P.eps_q[(size_t)i * d + dd], gsg);
            }
        }
        gmu[(size_t)j * d + dd] = gm;
        gsd[(size_t)j * d + dd] = gsg;
    }
}

}  // namespace

extern "C" {

int ggan_bce_logits_fwd(const float* x, float label, float weight, float* loss, int n, int accumulate, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && loss && n > 0, "bad argument");
    GGAN_LAUNCH("bce_logits_fwd", 0, 4.0 * n, bce_fwd_k, dim3(1), dim3(256), 0, (hipStream_t)stream, x, label, weight, loss, n, accumulate);
    return 0;
}

int ggan_bce_logits_bwd(const float* x, float label, float weight, const float* gloss, float* gx, int n, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && gloss && gx && n > 0, "bad argument");
    GGAN_LAUNCH("bce_logits_bwd", 0, 8.0 * n, bce_bwd_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, label, weight, gloss, gx, n);
    return 0;
}

static int bce_table(BceTable& t, const float* const* xs, float* const* gxs, const float* labels, const float* weights,
                     const int* ns, int count, int* max_n) {
    *max_n = 0;
    for (int i = 0; i < count; ++i) {
        if (!xs[i] || ns[i] <= 0 || (gxs && !gxs[i])) return -1;
        t.x[i] = xs[i]; t.gx[i] = gxs ? gxs[i] : nullptr; t.z[i] = labels[i]; t.w[i] = weights[i]; t.n[i] = ns[i];
        if (ns[i] > *max_n) *max_n = ns[i];
    }
    t.count = count;
    return 0;
}

int ggan_bce_logits_multi_fwd(const float* const* xs, const float* labels, const float* weights, const int* ns, int count,
                              float* loss, ggan_stream_t stream) {
    GGAN_CHECK_ARG(xs && labels && weights && ns && loss, "null pointer");
    GGAN_CHECK_ARG(count > 0 && count <= GGAN_BCE_MAX, "count out of range");
    BceTable t;
    int mx;
    GGAN_CHECK_ARG(bce_table(t, xs, nullptr, labels, weights, ns, count, &mx) == 0, "bad term");
    GGAN_LAUNCH("bce_logits_fwd", 0, 4.0 * mx * count, bce_multi_fwd_k, dim3(1), dim3(256), 0, (hipStream_t)stream, t, loss);
    return 0;
}

int ggan_bce_logits_multi_fwd_grad(const float* const* xs, const float* labels, const float* weights, const int* ns, int count,
                                   float* loss, float* const* gxs, ggan_stream_t stream) {
    GGAN_CHECK_ARG(xs && labels && weights && ns && loss && gxs, "null pointer");
    GGAN_CHECK_ARG(count > 0 && count <= GGAN_BCE_MAX, "count out of range");
    BceTable t;
    int mx;
    GGAN_CHECK_ARG(bce_table(t, xs, gxs, labels, weights, ns, count, &mx) == 0, "bad term");
    GGAN_LAUNCH("bce_logits_fwd_grad", 0, 8.0 * mx * count, bce_multi_fwd_k, dim3(1), dim3(256), 0, (hipStream_t)stream, t, loss);
    return 0;
}

int ggan_bce_heads_bwd(const float* const* xs, const float* labels, const float* weights, const int* ns, int count, float* loss,
                       float* const* gxs, int nheads, const int* head_terms, const int* Ms, const int* Hs, const float* const* hs,
                       const float* const* w_outs, const float* alphas, float* const* ghs, float* const* d_wouts,
                       float* const* d_bouts, ggan_stream_t stream) {
    GGAN_CHECK_ARG(xs && labels && weights && ns && loss && gxs && head_terms && Ms && Hs && hs && w_outs && alphas && ghs, "null pointer");
    GGAN_CHECK_ARG(count > 0 && count <= GGAN_BCE_MAX && nheads >= 1 && nheads <= GGAN_BCE_HEADS, "count out of range");
    BceTable t;
    int mx;
    GGAN_CHECK_ARG(bce_table(t, xs, gxs, labels, weights, ns, count, &mx) == 0, "bad term");
    BceHeads H;
    memset(&H, 0, sizeof(H));
    H.count = nheads;
    int k = 0, wg = 1;
    for (int a = 0; a < nheads; ++a) {
        BceHead& d = H.hd[a];
        GGAN_CHECK_ARG(hs[a] && w_outs[a] && ghs[a] && Ms[a] > 0 && Ms[a] <= GGAN_HEAD_BCE_MAX_ROWS && Hs[a] > 0 && head_terms[a] > 0 &&
                       k + head_terms[a] <= count, "bad head");
        d.h = hs[a]; d.w_out = w_outs[a]; d.gh = ghs[a]; d.d_wout = d_wouts ? d_wouts[a] : nullptr; d.d_bout = d_bouts ? d_bouts[a] : nullptr;
        d.alpha = alphas[a]; d.M = Ms[a]; d.H = Hs[a]; d.k0 = k; d.k1 = k + head_terms[a]; d.first = wg;
        int rows = 0;
        for (int i = d.k0; i < d.k1; ++i) {
            GGAN_CHECK_ARG(xs[i] == xs[d.k0] + rows, "a head's terms must be consecutive row ranges of one logits vector");
            rows += ns[i];
        }
        GGAN_CHECK_ARG(rows == d.M, "a head's terms must cover its rows");
        k = d.k1;
        wg += cdiv(d.H, 16);
    }
    GGAN_CHECK_ARG(k == count, "every term belongs to a head");
    GGAN_LAUNCH("bce_head_bwd", 0, 0, bce_head_bwd_k, dim3(wg), dim3(256), 0, (hipStream_t)stream, t, loss, H);
    return 0;
}

int ggan_bce_head_bwd(const float* const* xs, const float* labels, const float* weights, const int* ns, int count, float* loss,
                      float* const* gxs, int M, int H, const float* h, const float* w_out, float alpha, float* gh, float* d_wout,
                      float* d_bout, ggan_stream_t stream) {
    return ggan_bce_heads_bwd(xs, labels, weights, ns, count, loss, gxs, 1, &count, &M, &H, &h, &w_out, &alpha, &gh, &d_wout, &d_bout, stream);
}

int ggan_bce_logits_multi_bwd(const float* const* xs, const float* labels, const float* weights, const int* ns, int count,
                              const float* gloss, float* const* gxs, ggan_stream_t stream) {
    GGAN_CHECK_ARG(xs && labels && weights && ns && gloss && gxs, "null pointer");
    GGAN_CHECK_ARG(count > 0 && count <= GGAN_BCE_MAX, "count out of range");
    BceTable t;
    int mx;
    GGAN_CHECK_ARG(bce_table(t, xs, gxs, labels, weights, ns, count, &mx) == 0, "bad term");
    GGAN_LAUNCH("bce_logits_bwd", 0, 8.0 * mx * count, bce_multi_bwd_k, dim3(cdiv(mx, 256), count), dim3(256), 0,
                (hipStream_t)stream, t, gloss);
    return 0;
}

int ggan_dist_fwd(const float* x, const float* y, float* out, size_t n, int p, float weight, int accumulate, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && y && out && n > 0 && (p == 1 || p == 2), "bad argument");
    GGAN_LAUNCH("dist_fwd", 0, 8.0 * n, dist_fwd_k, dim3(1), dim3(1024), 0, (hipStream_t)stream, x, y, out, n, p, weight, accumulate);
    return 0;
}

int ggan_dist_bwd(const float* x, const float* y, const float* gout, float* gx, float* gy, size_t n, int p, float weight,
                  ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && y && gout && (gx || gy) && n > 0 && (p == 1 || p == 2), "bad argument");
    GGAN_LAUNCH("dist_bwd", 0, 16.0 * n, dist_bwd_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, x, y, gout, gx, gy, n, p, weight);
    return 0;
}

int ggan_mean_fwd(const float* x, float weight, float* loss, int n, int accumulate, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && loss && n > 0, "bad argument");
    GGAN_LAUNCH("mean_fwd", 0, 4.0 * n, mean_fwd_k, dim3(1), dim3(256), 0, (hipStream_t)stream, x, weight, loss, n, accumulate);
    return 0;
}

int ggan_mean_multi_fwd_grad(const float* const* xs, const float* weights, const int* ns, int count, float* loss, float* const* gxs,
                             ggan_stream_t stream) {
    GGAN_CHECK_ARG(xs && weights && ns && loss, "null pointer");
    GGAN_CHECK_ARG(count > 0 && count <= GGAN_BCE_MAX, "count out of range");
    BceTable t;
    int mx;
    float zeros[GGAN_BCE_MAX] = {0.f};
    GGAN_CHECK_ARG(bce_table(t, xs, gxs, zeros, weights, ns, count, &mx) == 0, "bad term");
    GGAN_LAUNCH("mean_multi_fwd", 0, 8.0 * mx * count, mean_multi_fwd_k, dim3(1), dim3(256), 0, (hipStream_t)stream, t, loss);
    return 0;
}

int ggan_mean_bwd(const float* gloss, float weight, float* gx, int n, ggan_stream_t stream) {
    GGAN_CHECK_ARG(gloss && gx && n > 0, "bad argument");
    GGAN_LAUNCH("mean_bwd", 0, 4.0 * n, mean_bwd_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, gloss, weight, gx, n);
    return 0;
}

int ggan_gp_penalty_fwd(const float* g, float* slopes, float* pen, int B, int D, float lam, ggan_stream_t stream) {
    GGAN_CHECK_ARG(g && slopes && pen && B > 0 && D > 0, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    GGAN_LAUNCH("gp_slopes", 0, 4.0 * B * D, gp_slopes_k, dim3(B), dim3(256), 0, s, g, slopes, D);
    GGAN_LAUNCH("gp_penalty", 0, 4.0 * B, gp_pen_k, dim3(1), dim3(256), 0, s, slopes, pen, B, lam);
    return 0;
}

int ggan_gp_penalty_fwd_grad(const float* g, float* slopes, float* pen, float* gg_unit, int32_t* arrive, int B, int D, float lam,
                             ggan_stream_t stream) {
    GGAN_CHECK_ARG(g && slopes && pen && gg_unit && arrive && B > 0 && D > 0, "bad argument");
    GGAN_LAUNCH("gp_fwd_grad", 0, 8.0 * B * D, gp_fwd_grad_k, dim3(B), dim3(256), 0, (hipStream_t)stream, g, slopes, pen, gg_unit, arrive, B, D,
                lam);
    return 0;
}

int ggan_gp_penalty_bwd(const float* g, const float* slopes, const float* gpen, float* gg, int B, int D, float lam, ggan_stream_t stream) {
    GGAN_CHECK_ARG(g && slopes && gpen && gg && B > 0 && D > 0, "bad argument");
    GGAN_LAUNCH("gp_penalty_bwd", 0, 8.0 * B * D, gp_bwd_k, dim3(B), dim3(256), 0, (hipStream_t)stream, g, slopes, gpen, gg, B, D, lam);
    return 0;
}

static int mmd_params(MmdParams& P, const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                      int unbiased) {
    if (!(X && Y && sigmas) || m <= 0 || n <= 0 || d <= 0 || ns <= 0 || ns > kMmdMaxSigmas || m + n > 512) return -1;
    if (unbiased && (m < 2 || n < 2)) return -1;
    P.X = X; P.Y = Y; P.m = m; P.n = n; P.d = d; P.ns = ns; P.unbiased = unbiased;
    for (int i = 0; i < ns; ++i) {
        P.gamma[i] = 1.f / (2.f * sigmas[i] * sigmas[i]);
        P.wt[i] = wts ? wts[i] : 1.f;
    }
    return 0;
}

// the biased and the unbiased estimator differ in the flag mmd_coef reads and in a launch label (fn: the entry point, for its error)
static int mmd2_fwd(const char* fn, const char* rows_label, int unbiased, const float* X, const float* Y, int m, int n, int d, const float* sigmas,
                    const float* wts, int ns, float* out, float* row_scratch, ggan_stream_t stream) {
    MmdParams P;
    if (!(mmd_params(P, X, Y, m, n, d, sigmas, wts, ns, unbiased) == 0 && out && row_scratch)) {
        set_error("%s: %s", fn, "bad argument");
        return -1;
    }
    GGAN_LAUNCH(rows_label, 3.0 * (m + n) * (m + n) * d, 0, mmd2_rows_k, dim3(m + n), dim3(256), 0, (hipStream_t)stream, P, row_scratch);
    GGAN_LAUNCH("mmd2_final", 0, 0, mmd2_final_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)row_scratch, m + n, out);
    return 0;
}

static int mmd2_bwd(const char* fn, const char* label, int unbiased, const float* X, const float* Y, int m, int n, int d, const float* sigmas,
                    const float* wts, int ns, const float* gout, float* dX, float* dY, ggan_stream_t stream) {
    MmdParams P;
    if (!(mmd_params(P, X, Y, m, n, d, sigmas, wts, ns, unbiased) == 0 && gout && (dX || dY))) {
        set_error("%s: %s", fn, "bad argument");
        return -1;
    }
    GGAN_LAUNCH(label, 5.0 * (m + n) * (m + n) * d, 0, mmd2_bwd_k, dim3(m + n), dim3(256), 0, (hipStream_t)stream, P, gout, dX, dY);
    return 0;
}

int ggan_mix_rbf_mmd2_fwd(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                          float* out, float* row_scratch, ggan_stream_t stream) {
    return mmd2_fwd(__func__, "mmd2_rows", 0, X, Y, m, n, d, sigmas, wts, ns, out, row_scratch, stream);
}

int ggan_mix_rbf_mmd2_bwd(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                          const float* gout, float* dX, float* dY, ggan_stream_t stream) {
    return mmd2_bwd(__func__, "mmd2_bwd", 0, X, Y, m, n, d, sigmas, wts, ns, gout, dX, dY, stream);
}

int ggan_mix_rbf_mmd2_unbiased_fwd(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                                   float* out, float* row_scratch, ggan_stream_t stream) {
    return mmd2_fwd(__func__, "mmd2u_rows", 1, X, Y, m, n, d, sigmas, wts, ns, out, row_scratch, stream);
}

int ggan_mix_rbf_mmd2_unbiased_bwd(const float* X, const float* Y, int m, int n, int d, const float* sigmas, const float* wts, int ns,
                                   const float* gout, float* dX, float* dY, ggan_stream_t stream) {
    return mmd2_bwd(__func__, "mmd2u_bwd", 1, X, Y, m, n, d, sigmas, wts, ns, gout, dX, dY, stream);
}

static int agg_params(AggP& P, int kind, const float* mu, const float* sd, const float* k_onehot, const float* eps_q, const float* z_p, int nx,
                      int nz, int d, int n_coms) {
    if (kind < 0 || kind > 2 || !mu || !sd || nx <= 0 || nz <= 0 || d <= 0 || n_coms <= 0 || d > 8192 || nx > 8192) return -1;
    if (kind != 1 && (!k_onehot || !eps_q)) return -1;
    if (kind != 0 && !z_p) return -1;
    P.mu = mu; P.sd = sd; P.k = k_onehot; P.eps_q = eps_q; P.z_p = z_p;
    P.kind = kind; P.nx = nx; P.nz = nz; P.d = d; P.n_coms = n_coms;
    return 0;
}

int ggan_agg_div_fwd(int kind, const float* mu, const float* sd, const float* k_onehot, const float* eps_q, const float* z_p, int nx, int nz,
                     int d, int n_coms, float* out, float* Z, float* A, float* Bv, float* T, ggan_stream_t stream) {
    AggP P;
    GGAN_CHECK_ARG(agg_params(P, kind, mu, sd, k_onehot, eps_q, z_p, nx, nz, d, n_coms) == 0 && out && Z && A && Bv && T, "bad argument");
    const int ns = kind == 2 ? 2 * nz : nz;
    GGAN_LAUNCH("agg_div_fwd", 8.0 * ns * nx * d, 0, agg_div_fwd_k, dim3(ns), dim3(128), d * sizeof(float), (hipStream_t)stream, P, Z, A, Bv, T);
    GGAN_LAUNCH("agg_div_final", 0, 0, agg_div_final_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (const float*)T, ns, nz, out);
    return 0;
}

int ggan_agg_div_bwd(int kind, const float* mu, const float* sd, const float* k_onehot, const float* eps_q, int nx, int nz, int d, int n_coms,
                     const float* Z, const float* A, const float* Bv, const float* gout, float* W, float* GZ, float* gmu, float* gsd,
                     ggan_stream_t stream) {
    AggP P;
    GGAN_CHECK_ARG(agg_params(P, kind, mu, sd, k_onehot, eps_q, Z /* unused */, nx, nz, d, n_coms) == 0 && Z && A && Bv && gout && W && GZ && gmu &&
                       gsd, "bad argument");
    const int ns = kind == 2 ? 2 * nz : nz;
    GGAN_LAUNCH("agg_div_bwd_samples", 6.0 * ns * nx * d, 0, agg_div_bwd_samples_k, dim3(ns), dim3(128), nx * sizeof(float), (hipStream_t)stream, P,
                Z, A, Bv, gout, W, GZ);
    GGAN_LAUNCH("agg_div_bwd_comps", 8.0 * ns * nx * d, 0, agg_div_bwd_comps_k, dim3(nx), dim3(128), 0, (hipStream_t)stream, P, ns, Z,
                (const float*)W, (const float*)GZ, gmu, gsd);
    return 0;
}

}  // extern "C"
