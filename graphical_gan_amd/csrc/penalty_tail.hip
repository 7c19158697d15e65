// The critic tail of the wali-gp penalty pass, Linear([a1 | a2] -> H) -> LeakyReLU -> Linear(H -> 1), differentiated w.r.t. its input:
// d D / d h[n, j] = u[n] * w_out[j] * lrelu'(h[n, j]).  Composed from plain ops that was a 1-wide product for logits nobody reads, a
// K = 1 "product" (u[M,1] w_out^T) and an act_bwd pass: three launches on the critical chain of every critic step for one pointwise
// result.  The kernel here is what they amount to, bit for bit.  (The second-order phase's column sum d_wout stays with the
// composition's act_bwd + N = 1 product: a kernel that summed the rows in another order changed the last bits of that gradient, and
// with them the weights a long run ends at.)
#include "common.h"
using namespace ggan;

namespace {

// one element of the seed: the K = 1 product's value (an accumulator that starts at +0, so a product of -0 leaves as +0), then the
// LeakyReLU derivative exactly as act_grad applies it
__device__ __forceinline__ float seed1(float s, float w, float r, float alpha) {
    const float g = s * w + 0.f;
    return act_grad(g, r, GGAN_ACT_LRELU, alpha);
}

// gpre[n, j] = (u ? u[n] : 1) * w_out[j] * lrelu'(h[n, j]); total4 = M * H / 4 float4 groups, H4 = H / 4 (H a multiple of 4, 16-byte
// aligned buffers)
__global__ void head_seed_fwd4_k(const float* __restrict__ u, const float* __restrict__ h, const float* __restrict__ w_out,
                                 float* __restrict__ gpre, unsigned total4, unsigned H4, float alpha) {
    const unsigned stride = gridDim.x * blockDim.x;
    const float4* h4 = reinterpret_cast<const float4*>(h);
    const float4* w4 = reinterpret_cast<const float4*>(w_out);
    float4* o4 = reinterpret_cast<float4*>(gpre);
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += stride) {
        const unsigned n = i / H4, j4 = i - n * H4;
        const float s = u ? u[n] : 1.f;
        const float4 w = w4[j4], r = h4[i];
        float4 o;
        o.x = seed1(s, w.x, r.x, alpha); o.y = seed1(s, w.y, r.y, alpha);
        o.z = seed1(s, w.z, r.z, alpha); o.w = seed1(s, w.w, r.w, alpha);
        o4[i] = o;
    }
}

// any H, any alignment: one element per step
__global__ void head_seed_fwd1_k(const float* __restrict__ u, const float* __restrict__ h, const float* __restrict__ w_out,
                                 float* __restrict__ gpre, unsigned total, unsigned H, float alpha) {
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned n = i / H, j = i - n * H;
        gpre[i] = seed1(u ? u[n] : 1.f, w_out[j], h[i], alpha);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int ggan_head_seed_fwd(int M, int H, const float* u, const float* h, const float* w_out, float alpha, float* gpre, ggan_stream_t stream) {
    GGAN_CHECK_ARG(h && w_out && gpre, "null pointer");
    GGAN_CHECK_ARG(M >= 1 && H >= 1 && (double)M * H < 2147483648.0, "bad shape");
    const unsigned total = (unsigned)M * (unsigned)H;
    if ((H & 3) == 0 && aligned16(h) && aligned16(w_out) && aligned16(gpre)) {
        const unsigned total4 = total / 4;
        const int grid = (int)((total4 + 255) / 256 < 2048 ? (total4 + 255) / 256 : 2048);
        GGAN_LAUNCH("head_seed_fwd", 1.0 * total, 8.0 * total, head_seed_fwd4_k, dim3(grid), dim3(256), 0, (hipStream_t)stream, u, h, w_out, gpre,
                    total4, (unsigned)(H / 4), alpha);
        return 0;
    }
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    GGAN_LAUNCH("head_seed_fwd", 1.0 * total, 8.0 * total, head_seed_fwd1_k, dim3(grid), dim3(256), 0, (hipStream_t)stream, u, h, w_out, gpre, total,
                (unsigned)H, alpha);
    return 0;
}

}  // extern "C"
