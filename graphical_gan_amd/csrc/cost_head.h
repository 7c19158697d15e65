// The arithmetic of the critic's cost and of the critic head around it, written once (losses.hip, gemm.hip).  The fused launches of
// the step's critical chain (head_out_fwd_bce_k, bce_head_bwd_k, the head_tail_wg workgroups of the grouped products) are held
// bit-equal to the unfused ones by the tests: every kernel that forms one of these values forms it through the helper here, so the
// expression and its order exist in one place.  Each helper says which expression it is and which order it keeps.
#pragma once
#include "common.h"

namespace ggan {
namespace {

// sigmoid cross-entropy of one logit v against the label z: max(v, 0) - v z + log(1 + exp(-|v|)), added left to right
__device__ __forceinline__ float bce_value(float v, float z) { return fmaxf(v, 0.f) - v * z + log1pf(expf(-fabsf(v))); }

// d(w * mean)/d(element) for a unit upstream gradient: a term's weight over its length, the product before the division
__device__ __forceinline__ float unit_seed(float w, int n) { return 1.f * w / (float)n; }

// d(bce_value)/dv scaled by g (unit_seed, or gloss * w / n): g * (sigmoid(v) - z), the sigmoid as 1 / (1 + exp(-v))
__device__ __forceinline__ float bce_grad(float g, float v, float z) { return g * (1.f / (1.f + expf(-v)) - z); }

// a term's share of a cost: w * (s / n), the division first
__device__ __forceinline__ float weighted_mean(float w, float s, float n) { return w * (s / n); }

// ... stored by the single-term launches, which may add to what is there (the terms of a cost, one accumulating launch each)
__device__ __forceinline__ void store_weighted_mean(float* out, float w, float s, float n, int accumulate) {
    const float r = weighted_mean(w, s, n);
    out[0] = accumulate ? out[0] + r : r;
}

// One term of a cost on one workgroup, added to the running total: s = sum_i value(x[i]) per thread over i = threadIdx.x, + stride, ...,
// block_sum, r = w * (s / n); term k = 0 IS the total (tot = r, not 0 + r), later ones are added in term order -- the summation
// order of one accumulating launch per term.  value: x[i] itself (mean: the Wasserstein costs) or bce_value(x[i], z).  gx (optional):
// the term's gradient for a unit upstream gradient, stored on the way.  Threads with on == false (beyond the 256 of an eight-wave
// launch) only keep block_sum's barriers company: they contribute exact zeros.  sm: block_sum's scratch.
template <class Stride>
__device__ __forceinline__ float cost_add_term(float tot, int k, bool mean, const float* x, int n, float z, float w, float* gx,
                                               Stride stride, bool on, float* sm) {
    const float g = unit_seed(w, n);
    float s = 0.f;
    if (on)
        for (int i = threadIdx.x; i < n; i += stride) {
            const float v = x[i];
            s += mean ? v : bce_value(v, z);
            if (gx) gx[i] = mean ? g : bce_grad(g, v, z);
        }
    s = block_sum(s, sm);
    const float r = weighted_mean(w, s, (float)n);
    return k ? tot + r : r;
}

// the 16 row groups of column cl, combined as a fixed balanced tree (deterministic, and the same tree in every head kernel)
__device__ __forceinline__ float combine16(const float (*red)[16], int cl) {
    return (((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) + ((red[4][cl] + red[5][cl]) + (red[6][cl] + red[7][cl]))) +
           (((red[8][cl] + red[9][cl]) + (red[10][cl] + red[11][cl])) + ((red[12][cl] + red[13][cl]) + (red[14][cl] + red[15][cl])));
}

// The critic head's backward over column c = 16 * (its workgroup) + (tid & 15), row group rg = tid / 16 of 16:  gh[r,c] = g[r] * w_out[c] * lrelu'(h[r,c]) (GH only),
// d_wout[c] = sum_r g[r] h[r,c] as an fmaf chain over the rows rg, rg + 16, ... of each of 16 row groups, d_bout = sum_r g[r] by the
// workgroup with `first`; the row groups meet in combine16's order.  16 columns x 16 row groups (measured against 64 x 4 and 32 x 8:
// the launch is a chain of L2 round trips per thread, not bandwidth -- 8 rows per thread at 128 rows, all of their loads in flight
// at once, hence the unroll).  g: global memory or LDS.  Threads with on == false contribute nothing and store nothing.
template <bool GH>
__device__ __forceinline__ void head_columns(const float* g, const float* h, const float* w_out, float alpha, float* gh, float* d_wout,
                                             float* d_bout, bool first, int M, int H, int c, int tid, int rg, bool on, float (*red)[16]) {
    const int cl = tid & 15;
    float acc = 0.f, gs = 0.f;
    if (on && c < H) {
        float w = 0.f;
        if constexpr (GH) w = w_out[c];
#pragma unroll 8
        for (int r = rg; r < M; r += 16) {
            const float gr = g[r], hv = h[(size_t)r * H + c];
            if constexpr (GH) gh[(size_t)r * H + c] = gr * w * (hv > 0.f ? 1.f : alpha);
            acc = fmaf(gr, hv, acc);
            gs += gr;
        }
    }
    if (on) red[rg][cl] = acc;
    __syncthreads();
    if (on && rg == 0 && c < H && d_wout) d_wout[c] = combine16(red, cl);
    if (first && d_bout) {
        __syncthreads();
        if (on && cl == 0) red[rg][0] = gs;
        __syncthreads();
        if (tid == 0) d_bout[0] = combine16(red, 0);
    }
}

// The critic head's forward for four columns c .. c + 3 of one row (o = row * H + c): the split-K slabs of the first Linear added in
// slab order, + b, LeakyReLU as max(alpha t, t), h stored, and the row's dot product with w_out continued four deep (w first).
// (Slab order: deterministic.  Unrolled: the slab loads are independent, only the adds are ordered -- rolled, the 16 slabs of the
// K = 4608 tail were 16 serial L2 round trips, most of head_out_fwd_k's 8 us.)  v, ww: what was stored and the weights, for a caller
// that goes on to the backward.
__device__ __forceinline__ float head_fwd_unit(const float* part, int SK, size_t slab, size_t o, const float* b, const float* w_out,
                                               int c, float alpha, float* h, float dot, float4& v, float4& ww) {
    v = *reinterpret_cast<const float4*>(part + o);
#pragma unroll 8
    for (int s = 1; s < SK; ++s) {
        const float4 u = *reinterpret_cast<const float4*>(part + (size_t)s * slab + o);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    const float4 bb = *reinterpret_cast<const float4*>(b + c);
    ww = *reinterpret_cast<const float4*>(w_out + c);
    v.x = fmaxf(alpha * (v.x + bb.x), v.x + bb.x); v.y = fmaxf(alpha * (v.y + bb.y), v.y + bb.y);
    v.z = fmaxf(alpha * (v.z + bb.z), v.z + bb.z); v.w = fmaxf(alpha * (v.w + bb.w), v.w + bb.w);
    *reinterpret_cast<float4*>(h + o) = v;
    return fmaf(v.x, ww.x, fmaf(v.y, ww.y, fmaf(v.z, ww.z, fmaf(v.w, ww.w, dot))));
}

}  // namespace
}  // namespace ggan
