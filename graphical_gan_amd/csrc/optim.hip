// The optimizer tail of the training step: Adam (TF flavour), RMSProp, the evaluation-only weight average and its swap,
// gradient packing and packing fused with Adam.  HBM-bound, float4-vectorised where every side is aligned.
#include "common.h"
#include "pointwise.h"
using namespace ggan;

namespace {

// ---- Adam (TF flavour) ------------------------------------------------------------------------
// the bias-corrected step size of update number `ordinal` (1 for the first)
__device__ __forceinline__ float adam_lr_t(float ordinal, float lr, float b1, float b2) {
    return lr * sqrtf(1.f - powf(b2, ordinal)) / (1.f - powf(b1, ordinal));
}

// one element's update, the three statements as tests/_optim_dispatch.py counts their roundings (contraction is per expression)
struct AdamCoef { float gscale, b1, b2, lr_t, eps; };
__device__ __forceinline__ void adam1(float& th, float g, float& m, float& v, const AdamCoef& c) {
    const float gscale = c.gscale, b1 = c.b1, b2 = c.b2, lr_t = c.lr_t, eps = c.eps;
    float gg = g * gscale;
    m = b1 * m + (1.f - b1) * gg;
    v = b2 * v + (1.f - b2) * gg * gg;
    th = th - lr_t * m / (sqrtf(v) + eps);
}

// PRE: step[0] already holds this update's ordinal (the gradient-pack kernel of the same optimizer step incremented it)
template <bool PRE>
__global__ void adam_k(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, size_t n, const int32_t* __restrict__ step, float lr, float b1,
                       float b2, float eps, float gscale) {
    const float t = (float)(step[0] + (PRE ? 0 : 1));
    const AdamCoef A{gscale, b1, b2, adam_lr_t(t, lr, b1, b2), eps};
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    size_t n4 = n >> 2;
    float4* th4 = reinterpret_cast<float4*>(theta);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (size_t j = i; j < n4; j += stride) {
        float4 th = th4[j], gg4 = g4[j], mm = m4[j], vv = v4[j];
        adam1(th.x, gg4.x, mm.x, vv.x, A); adam1(th.y, gg4.y, mm.y, vv.y, A);
        adam1(th.z, gg4.z, mm.z, vv.z, A); adam1(th.w, gg4.w, mm.w, vv.w, A);
        th4[j] = th; m4[j] = mm; v4[j] = vv;
    }
    for (size_t j = (n4 << 2) + i; j < n; j += stride) {
        float th = theta[j], mm = m[j], vv = v[j];
        adam1(th, g[j], mm, vv, A);
        theta[j] = th; m[j] = mm; v[j] = vv;
    }
}

__global__ void adam_advance_k(int32_t* step) { step[0] += 1; }

// tf.train.RMSPropOptimizer (momentum 0, centered=False): ms = decay*ms + (1-decay)*g^2; theta -= lr*g/sqrt(ms+eps);
// then (optionally) the weight clipping of the original WGAN, tf.clip_by_value(var, lo, hi)
__global__ void rmsprop_k(float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ ms, size_t n, float lr,
                          float decay, float eps, float gscale, float lo, float hi) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float gg = g[i] * gscale;
        const float m = decay * ms[i] + (1.f - decay) * gg * gg;
        ms[i] = m;
        theta[i] = fminf(fmaxf(theta[i] - lr * gg / sqrtf(m + eps), lo), hi);
    }
}

// ---- exponential moving average of the weights (evaluation only) ---------------------------------
// No call site in the reference: the semantics are those of TensorFlow 1's documented tf.train.ExponentialMovingAverage(decay,
// num_updates): d_t = min(decay, (1 + t) / (10 + t)); shadow -= (1 - d_t) * (shadow - theta), with t = step[0], the ordinal of the
// update just applied (the optimizer's device-side counter, already advanced).  theta is only read.
__global__ void ema_k(float* __restrict__ shadow, const float* __restrict__ theta, size_t n, const int32_t* __restrict__ step,
                      float decay) {
    const float t = (float)step[0];
    const float w = 1.f - fminf(decay, (1.f + t) / (10.f + t));
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    size_t n4 = n >> 2;
    float4* s4 = reinterpret_cast<float4*>(shadow);
    const float4* th4 = reinterpret_cast<const float4*>(theta);
    for (size_t j = i; j < n4; j += stride) {
        float4 s = s4[j];
        const float4 th = th4[j];
        s.x -= w * (s.x - th.x); s.y -= w * (s.y - th.y);
        s.z -= w * (s.z - th.z); s.w -= w * (s.w - th.w);
        s4[j] = s;
    }
    for (size_t j = (n4 << 2) + i; j < n; j += stride) shadow[j] -= w * (shadow[j] - theta[j]);
}

// a <-> b in one pass (the averaged weights visit the live storage for an evaluation: captured graphs bake theta's address)
__global__ void swap_k(float* __restrict__ a, float* __restrict__ b, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    size_t n4 = n >> 2;
    float4* a4 = reinterpret_cast<float4*>(a);
    float4* b4 = reinterpret_cast<float4*>(b);
    for (size_t j = i; j < n4; j += stride) {
        const float4 va = a4[j], vb = b4[j];
        a4[j] = vb; b4[j] = va;
    }
    for (size_t j = (n4 << 2) + i; j < n; j += stride) {
        const float va = a[j], vb = b[j];
        a[j] = vb; b[j] = va;
    }
}

struct PackTable {
    const float* src[GGAN_PACK_MAX];
    size_t size[GGAN_PACK_MAX];
    size_t off[GGAN_PACK_MAX];
    size_t pstride[GGAN_PACK_MAX];   // floats between the partial slabs of source k
    int parts[GGAN_PACK_MAX];        // number of slabs to sum (1 = plain copy)
    const float* src2[GGAN_PACK_MAX];  // optional SECOND gradient contribution of the same tensor (a parameter used by two passes of a
    size_t pstride2[GGAN_PACK_MAX];    // step, e.g. the critic's main pass and its gradient-penalty pass), added after the first
    int parts2[GGAN_PACK_MAX];
    int count;
    int32_t* bump;                   // optional: counter incremented once per launch (the optimizer's step ordinal)
    int first[GGAN_PACK_MAX + 1];    // pack_adam_k: first workgroup of tensor k (1-D grid of kPackChunk-float chunks)
};
constexpr int kPackChunk = 4096;
__host__ __device__ inline int pack_chunk(int slabs) { return slabs > 4 ? 1024 : kPackChunk; }

// element i of a packed gradient: the slabs of s in slab order (0.f where a tensor has no first source), then those of s2
__device__ __forceinline__ float slab_sum(const float* s, int np, size_t ps, const float* s2, int np2, size_t ps2, size_t i) {
    float a = 0.f;
    if (s) {
        a = s[i];
        for (int p = 1; p < np; ++p) a += s[(size_t)p * ps + i];
    }
    for (int p = 0; p < np2; ++p) a += s2[(size_t)p * ps2 + i];
    return a;
}

// ... four at a time on the float4 path (s is there): a is slab 0 of s, already loaded; the same order
__device__ __forceinline__ float4 slab_sum4(float4 a, const float* s, int np, size_t ps, const float* s2, int np2, size_t ps2, size_t i) {
#pragma unroll 8
    for (int p = 1; p < np; ++p) {      // (unrolled: the slab loads are independent, only the adds are ordered)
        const float4 b = reinterpret_cast<const float4*>(s + (size_t)p * ps)[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
#pragma unroll 8
    for (int p = 0; p < np2; ++p) {
        const float4 b = reinterpret_cast<const float4*>(s2 + (size_t)p * ps2)[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    return a;
}

// blockIdx.y = tensor, blockIdx.x grid-strides inside it (16-byte accesses when every side is aligned); a source made of
// several split-K slabs is summed in slab order on the way
__global__ void pack_k(PackTable t, float* __restrict__ flat) {
    const int k = blockIdx.y;
    const float* s = t.src[k];
    const float* s2 = t.src2[k];
    float* d = flat + t.off[k];
    const size_t n = t.size[k];
    const int np = t.parts[k], np2 = s2 ? t.parts2[k] : 0;
    const size_t ps = t.pstride[k], ps2 = t.pstride2[k];
    const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (t.bump && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) t.bump[0] += 1;
    if (s && ((((uintptr_t)s) | ((uintptr_t)d) | ((uintptr_t)s2)) & 15) == 0 && (np == 1 || (ps & 3) == 0) && (np2 <= 1 || (ps2 & 3) == 0)) {
        const size_t n4 = n >> 2;
        float4* d4 = reinterpret_cast<float4*>(d);
        for (size_t i = i0; i < n4; i += stride) d4[i] = slab_sum4(reinterpret_cast<const float4*>(s)[i], s, np, ps, s2, np2, ps2, i);
        for (size_t i = (n4 << 2) + i0; i < n; i += stride) d[i] = slab_sum(s, np, ps, s2, np2, ps2, i);
    } else {
        for (size_t i = i0; i < n; i += stride) d[i] = slab_sum(s, np, ps, s2, np2, ps2, i);
    }
}

// pack_k and adam_k<true> in one pass (single-replica steps: nothing happens to the packed gradient between the two): a
// parameter's gradient is summed from its sources exactly as pack_k does, written to the flat gradient buffer (it stays
// inspectable) and applied at once -- the flat gradient is not read back, and one launch of the step's tail is gone.
// The update's ordinal is step[0] + 1 for every workgroup; the LAST workgroup to finish advances step[0] (arrival counter, left
// at zero), so no workgroup can see the advanced value.
__global__ void pack_adam_k(PackTable t, float* __restrict__ flat, float* __restrict__ theta, float* __restrict__ m,
                            float* __restrict__ v, int32_t* __restrict__ arrive, float lr, float b1, float b2, float eps,
                            float gscale) {
    // 1-D grid: workgroups [first[k], first[k+1]) own 4096-float chunks of tensor k (only workgroups with work exist: every one of
    // them pays a same-address atomic at the end, and those are served one at a time)
    int k = 0;
    while (k + 1 < t.count && (int)blockIdx.x >= t.first[k + 1]) ++k;
    const float* s = t.src[k];
    const float* s2 = t.src2[k];
    const size_t off = t.off[k];
    float* d = flat + off;
    float* th = theta + off;
    float* mp = m + off;
    float* vp = v + off;
    const size_t n = t.size[k];
    const int np = t.parts[k], np2 = s2 ? t.parts2[k] : 0;
    const size_t ps = t.pstride[k], ps2 = t.pstride2[k];
    // (a tensor summed from many slabs gets one float4 per thread: its loads are the long chain)
    const int chunk = pack_chunk(t.parts[k] + (s2 ? t.parts2[k] : 0));
    const size_t base = (size_t)((int)blockIdx.x - t.first[k]) * chunk;
    const float tt = (float)(t.bump[0] + 1);
    const AdamCoef A{gscale, b1, b2, adam_lr_t(tt, lr, b1, b2), eps};
    auto one = [&](size_t i) {
        const float a = slab_sum(s, np, ps, s2, np2, ps2, i);
        d[i] = a;
        float x = th[i], mm = mp[i], vv = vp[i];
        adam1(x, a, mm, vv, A);
        th[i] = x; mp[i] = mm; vp[i] = vv;
    };
    if (s && ((((uintptr_t)s) | ((uintptr_t)d) | ((uintptr_t)s2)) & 15) == 0 && (np == 1 || (ps & 3) == 0) && (np2 <= 1 || (ps2 & 3) == 0)) {
        const size_t n4 = n >> 2;
        // every load of the chunk first (the four float4 groups of a thread, 16 independent loads in flight), then the arithmetic
        // and the stores: written as "load, update, store" per group the stores of one group ordered the loads of the next behind
        // them (the buffers may alias as far as the compiler knows) -- four memory round trips per thread instead of one
        constexpr int NQ = kPackChunk / 4 / kBlock;
        float4 X[NQ], Mq[NQ], Vq[NQ], Aq[NQ];
        bool ok[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const size_t i = base / 4 + threadIdx.x + (size_t)q * kBlock;
            ok[q] = i < n4 && q * kBlock * 4 < chunk;
            if (ok[q]) {
                X[q] = reinterpret_cast<const float4*>(th)[i]; Mq[q] = reinterpret_cast<const float4*>(mp)[i];
                Vq[q] = reinterpret_cast<const float4*>(vp)[i]; Aq[q] = reinterpret_cast<const float4*>(s)[i];
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (!ok[q]) continue;
            const size_t i = base / 4 + threadIdx.x + (size_t)q * kBlock;
            float4 x = X[q], mm = Mq[q], vv = Vq[q];
            const float4 a = slab_sum4(Aq[q], s, np, ps, s2, np2, ps2, i);
            reinterpret_cast<float4*>(d)[i] = a;
            adam1(x.x, a.x, mm.x, vv.x, A); adam1(x.y, a.y, mm.y, vv.y, A);
            adam1(x.z, a.z, mm.z, vv.z, A); adam1(x.w, a.w, mm.w, vv.w, A);
            reinterpret_cast<float4*>(th)[i] = x; reinterpret_cast<float4*>(mp)[i] = mm; reinterpret_cast<float4*>(vp)[i] = vv;
        }
        // (the 1..3 elements behind the last whole float4: the workgroup that owns the end of the tensor)
        if (base + chunk >= n && (n4 << 2) + threadIdx.x < n) one((n4 << 2) + threadIdx.x);
    } else {
        for (int q = 0; q < kPackChunk / kBlock; ++q) {
            const size_t i = base + threadIdx.x + (size_t)q * kBlock;
            if (i >= n || q * kBlock >= chunk) break;
            one(i);
        }
    }
    // arrival in two levels (same-address atomics are served one at a time, ~13 ns each, and the workgroups of this one-round
    // launch all finish together): 32 group counters 4 KB apart, the last workgroup of each group reports to counter 0
    // (arrive == NULL: this launch applies PART of an update -- the ordinal stays step[0] + 1 for the launch that completes it)
    if (!arrive) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int grp = blockIdx.x & 31, members = ((int)gridDim.x - grp + 31) >> 5, groups = gridDim.x < 32 ? (int)gridDim.x : 32;
        int32_t* c = arrive + (size_t)(1 + grp) * GGAN_PACK_ARRIVE_STRIDE;
        if (atomicAdd(c, 1) == members - 1) {
            c[0] = 0;
            __threadfence();
            if (atomicAdd(arrive, 1) == groups - 1) {
                arrive[0] = 0;
                t.bump[0] += 1;
            }
        }
    }
}

}  // namespace

extern "C" {

int ggan_adam_step(float* theta, const float* g, float* m, float* v, size_t n, const int32_t* step, float lr,
                   float beta1, float beta2, float eps, float grad_scale, ggan_stream_t stream) {
    GGAN_CHECK_ARG(theta && g && m && v && step, "null pointer");
    if (n == 0) return 0;
    GGAN_CHECK_ARG(aligned16(theta) && aligned16(g) && aligned16(m) && aligned16(v), "buffers must be 16-byte aligned");
    GGAN_LAUNCH("adam_step", 0, 28.0 * n, adam_k<false>, dim3(grid_for(n, 8)), dim3(kBlock), 0, (hipStream_t)stream, theta, g, m, v, n, step, lr, beta1, beta2, eps, grad_scale);
    return 0;
}

int ggan_adam_step_counted(float* theta, const float* g, float* m, float* v, size_t n, const int32_t* step, float lr,
                           float beta1, float beta2, float eps, float grad_scale, ggan_stream_t stream) {
    GGAN_CHECK_ARG(theta && g && m && v && step, "null pointer");
    if (n == 0) return 0;
    GGAN_CHECK_ARG(aligned16(theta) && aligned16(g) && aligned16(m) && aligned16(v), "buffers must be 16-byte aligned");
    GGAN_LAUNCH("adam_step", 0, 28.0 * n, adam_k<true>, dim3(grid_for(n, 8)), dim3(kBlock), 0, (hipStream_t)stream, theta, g, m, v, n, step, lr, beta1, beta2, eps, grad_scale);
    return 0;
}

int ggan_rmsprop_step(float* theta, const float* g, float* ms, size_t n, float lr, float decay, float eps, float grad_scale,
                      float clip_lo, float clip_hi, ggan_stream_t stream) {
    GGAN_CHECK_ARG(theta && g && ms, "null pointer");
    GGAN_CHECK_ARG(clip_lo <= clip_hi, "empty clip interval");
    if (n == 0) return 0;
    GGAN_LAUNCH("rmsprop_step", 0, 20.0 * n, rmsprop_k, dim3(grid_for(n, 8)), dim3(kBlock), 0, (hipStream_t)stream, theta, g, ms, n, lr,
                decay, eps, grad_scale, clip_lo, clip_hi);
    return 0;
}

int ggan_ema_step(float* shadow, const float* theta, size_t n, const int32_t* step, float decay, ggan_stream_t stream) {
    GGAN_CHECK_ARG(shadow && theta && step, "null pointer");
    GGAN_CHECK_ARG(decay >= 0.f && decay < 1.f, "decay must lie in [0, 1)");
    GGAN_CHECK_ARG(shadow != theta, "shadow and theta are the same buffer");
    GGAN_CHECK_ARG(shadow + n <= theta || theta + n <= shadow, "the buffers overlap");
    if (n == 0) return 0;
    GGAN_CHECK_ARG(aligned16(shadow) && aligned16(theta), "buffers must be 16-byte aligned");
    GGAN_LAUNCH("ema_step", 0, 12.0 * n, ema_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, shadow, theta, n, step, decay);
    return 0;
}

int ggan_swap(float* a, float* b, size_t n, ggan_stream_t stream) {
    GGAN_CHECK_ARG(a && b, "null pointer");
    GGAN_CHECK_ARG(a + n <= b || b + n <= a, "the buffers overlap");
    if (n == 0) return 0;
    GGAN_CHECK_ARG(aligned16(a) && aligned16(b), "buffers must be 16-byte aligned");
    GGAN_LAUNCH("swap", 0, 16.0 * n, swap_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, a, b, n);
    return 0;
}

int ggan_adam_advance(int32_t* step, ggan_stream_t stream) {
    GGAN_CHECK_ARG(step, "null pointer");
    GGAN_LAUNCH("adam_advance", 0, 8, adam_advance_k, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
    return 0;
}

// The PackTable of the ABI's arrays (absent arrays: one slab, no second source).  mx: the longest tensor, tot: floats read over all
// slabs, all: floats written.  -1: a slab count below 1.
struct PackSizes { size_t mx, tot, all; };
static int pack_table(PackTable& t, PackSizes& z, const float* const* srcs, const size_t* sizes, const size_t* offsets, const int* parts,
                      const size_t* strides, const float* const* srcs2, const int* parts2, const size_t* strides2, int count, int32_t* bump) {
    z.mx = z.tot = z.all = 0;
    for (int i = 0; i < count; ++i) {
        t.src[i] = srcs[i]; t.size[i] = sizes[i]; t.off[i] = offsets[i];
        t.parts[i] = parts ? parts[i] : 1;
        t.pstride[i] = strides ? strides[i] : 0;
        t.src2[i] = srcs2 ? srcs2[i] : nullptr;
        t.parts2[i] = (srcs2 && parts2) ? parts2[i] : 1;
        t.pstride2[i] = (srcs2 && strides2) ? strides2[i] : 0;
        if (t.parts[i] < 1 || t.parts2[i] < 1) return -1;
        if (sizes[i] > z.mx) z.mx = sizes[i];
        z.tot += sizes[i] * (size_t)(t.parts[i] + (t.src2[i] ? t.parts2[i] : 0));
        z.all += sizes[i];
    }
    t.count = count;
    t.bump = bump;
    return 0;
}

int ggan_pack_parts2(const float* const* srcs, const size_t* sizes, const size_t* offsets, const int* parts, const size_t* strides,
                     const float* const* srcs2, const int* parts2, const size_t* strides2, int count, float* flat, int32_t* bump,
                     ggan_stream_t stream) {
    GGAN_CHECK_ARG(srcs && sizes && offsets && flat, "null pointer");
    GGAN_CHECK_ARG(count > 0 && count <= GGAN_PACK_MAX, "count out of range");
    PackTable t;
    PackSizes z;
    GGAN_CHECK_ARG(pack_table(t, z, srcs, sizes, offsets, parts, strides, srcs2, parts2, strides2, count, bump) == 0, "parts must be >= 1");
    const size_t mx = z.mx, tot = z.tot;
    int gx = (int)cdivz(mx, (size_t)kBlock * 16);
    if (gx < 1) gx = 1;
    if (gx > 512) gx = 512;
    GGAN_LAUNCH("pack", 0, 4.0 * tot + 4.0 * mx, pack_k, dim3(gx, count), dim3(kBlock), 0, (hipStream_t)stream, t, flat);
    return 0;
}

int ggan_pack_adam(const float* const* srcs, const size_t* sizes, const size_t* offsets, const int* parts, const size_t* strides,
                   const float* const* srcs2, const int* parts2, const size_t* strides2, int count, float* flat, float* theta,
                   float* m, float* v, int32_t* step, int32_t* arrive, float lr, float beta1, float beta2, float eps,
                   float grad_scale, ggan_stream_t stream) {
    GGAN_CHECK_ARG(srcs && sizes && offsets && flat && theta && m && v && step, "null pointer");
    GGAN_CHECK_ARG(count > 0 && count <= GGAN_PACK_MAX, "count out of range");
    // (the kernel decides float4 or scalar from flat + off and the sources alone: theta, m and v must be congruent to flat)
    GGAN_CHECK_ARG(aligned16(flat) && aligned16(theta) && aligned16(m) && aligned16(v), "buffers must be 16-byte aligned");
    PackTable t;
    PackSizes z;
    GGAN_CHECK_ARG(pack_table(t, z, srcs, sizes, offsets, parts, strides, srcs2, parts2, strides2, count, step) == 0, "parts must be >= 1");
    int nb = 0;
    for (int i = 0; i < count; ++i) {
        t.first[i] = nb;
        nb += (int)cdivz(sizes[i] > 0 ? sizes[i] : 1, (size_t)pack_chunk(t.parts[i] + (t.src2[i] ? t.parts2[i] : 0)));
    }
    t.first[count] = nb;
    GGAN_LAUNCH("pack_adam", 0, 4.0 * z.tot + 28.0 * z.all, pack_adam_k, dim3(nb), dim3(kBlock), 0, (hipStream_t)stream, t, flat, theta,
                m, v, arrive, lr, beta1, beta2, eps, grad_scale);
    return 0;
}

int ggan_pack_parts(const float* const* srcs, const size_t* sizes, const size_t* offsets, const int* parts,
                    const size_t* strides, int count, float* flat, int32_t* bump, ggan_stream_t stream) {
    return ggan_pack_parts2(srcs, sizes, offsets, parts, strides, nullptr, nullptr, nullptr, count, flat, bump, stream);
}

int ggan_pack(const float* const* srcs, const size_t* sizes, const size_t* offsets, int count, float* flat, ggan_stream_t stream) {
    return ggan_pack_parts(srcs, sizes, offsets, nullptr, nullptr, count, flat, nullptr, stream);
}

}  // extern "C"
