// HBM-bound pointwise / reduction kernels of the training step: activations, bias, input scaling, axpby,
// interpolation, the column / channel reductions, the reparameterisation.
// All are grid-stride, float4-vectorised where the layout allows, wave-shuffle reductions.
#include "common.h"
#include "conv.h"
#include "pointwise.h"
using namespace ggan;

namespace {

// ---------------------------------------------------------------------------------------------
__global__ void act_fwd_k(const float* __restrict__ x, float* __restrict__ y, size_t n, int act, float alpha) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    size_t n4 = n >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    float4* y4 = reinterpret_cast<float4*>(y);
    for (size_t j = i; j < n4; j += stride) {
        float4 v = x4[j];
        v.x = act_apply(v.x, act, alpha); v.y = act_apply(v.y, act, alpha);
        v.z = act_apply(v.z, act, alpha); v.w = act_apply(v.w, act, alpha);
        y4[j] = v;
    }
    for (size_t j = (n4 << 2) + i; j < n; j += stride) y[j] = act_apply(x[j], act, alpha);
}

__global__ void act_bwd_k(const float* __restrict__ gy, const float* __restrict__ ref, float* __restrict__ gx,
                          size_t n, int act, float alpha) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    size_t n4 = n >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(gy);
    const float4* r4 = reinterpret_cast<const float4*>(ref);
    float4* o4 = reinterpret_cast<float4*>(gx);
    for (size_t j = i; j < n4; j += stride) {
        float4 g = g4[j], r = r4[j], o;
        o.x = act_grad(g.x, r.x, act, alpha); o.y = act_grad(g.y, r.y, act, alpha);
        o.z = act_grad(g.z, r.z, act, alpha); o.w = act_grad(g.w, r.w, act, alpha);
        o4[j] = o;
    }
    for (size_t j = (n4 << 2) + i; j < n; j += stride) gx[j] = act_grad(gy[j], ref[j], act, alpha);
}

// act_bwd + the bias gradient of the layer in one pass: workgroup (c, s) handles channel c of the images [s*ipb, (s+1)*ipb),
// writes gx = gy * act'(ref) and its partial sum to parts[s*C + c] (slab s of a "parts" gradient: the pack kernel or a split-K
// reduce adds the slabs in order -- deterministic, no second reduction launch).  Replaces act_bwd + chansum_part + chansum_final
// in the backward of a Deconv2D / Conv2D whose bias does not feed a BatchNorm.
__global__ __launch_bounds__(256) void act_bwd_chansum_k(const float* __restrict__ gy, const float* __restrict__ ref, float* __restrict__ gx,
                                                         float* __restrict__ parts, int N, int C, int HW, int ipb, int act, float alpha) {
    __shared__ float red[4];
    const int c = blockIdx.x, sidx = blockIdx.y, tid = threadIdx.x;
    const int n0 = sidx * ipb, n1 = min(n0 + ipb, N);
    float acc = 0.f;
    const int hw4 = HW >> 2;
    for (int n = n0; n < n1; ++n) {
        const size_t base = ((size_t)n * C + c) * HW;
        if ((HW & 3) == 0) {
            const float4* g4 = reinterpret_cast<const float4*>(gy + base);
            const float4* r4 = reinterpret_cast<const float4*>(ref + base);
            float4* o4 = reinterpret_cast<float4*>(gx + base);
            for (int j = tid; j < hw4; j += 256) {
                const float4 g = g4[j], r = r4[j];
                float4 o;
                o.x = act_grad(g.x, r.x, act, alpha); o.y = act_grad(g.y, r.y, act, alpha);
                o.z = act_grad(g.z, r.z, act, alpha); o.w = act_grad(g.w, r.w, act, alpha);
                o4[j] = o;
                acc += (o.x + o.y) + (o.z + o.w);
            }
        } else {
            for (int j = tid; j < HW; j += 256) {
                const float o = act_grad(gy[base + j], ref[base + j], act, alpha);
                gx[base + j] = o;
                acc += o;
            }
        }
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) parts[(size_t)sidx * C + c] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void bias_add_k(const float* __restrict__ x, const float* __restrict__ bias, float* __restrict__ y,
                           size_t total, int C, int HW) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = i; j < total; j += stride) {
        int c = (int)((j / (size_t)HW) % (size_t)C);
        y[j] = x[j] + bias[c];
    }
}

__global__ void cast_scale_k(const int32_t* __restrict__ x, const float* __restrict__ noise, float* __restrict__ y,
                             size_t n, float div, float mul) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = i; j < n; j += stride) {
        // reference op order: 2*((float(x)/255.)-.5)  (gmgan_inference_cifar10.py:342)
        float v = mul * (((float)x[j] / div) - 0.5f);
        if (noise) v += noise[j];
        y[j] = v;
    }
}

__global__ void cast_scale_ring_k(const int32_t* __restrict__ ring, int nslots, const int32_t* __restrict__ ctr_a,
                                  const int32_t* __restrict__ ctr_b, int offset, const float* __restrict__ noise,
                                  float* __restrict__ y, size_t n, float div, float mul) {
    // (nothing in this launch writes the counters: every workgroup sees the same slot)
    long long c = (long long)offset + (ctr_a ? *ctr_a : 0) + (ctr_b ? *ctr_b : 0);
    const int slot = (int)(((c % nslots) + nslots) % nslots);
    const int32_t* x = ring + (size_t)slot * n;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = i; j < n; j += stride) {
        float v = mul * (((float)x[j] / div) - 0.5f);
        if (noise) v += noise[j];
        y[j] = v;
    }
}

__global__ void axpby_k(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out,
                        size_t n, float a, float b, float c) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = i; j < n; j += stride) out[j] = a * x[j] + (y ? b * y[j] : 0.f) + c;
}

__global__ void row_lerp_k(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ alpha,
                           float* __restrict__ out, int rows, int cols) {
    size_t total = (size_t)rows * cols;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t j = i; j < total; j += stride) {
        float a = alpha[j / (size_t)cols];
        out[j] = x[j] + a * (y[j] - x[j]);
    }
}
// (32-bit indices and the row by one v_mul_hi: the 64-bit division above is ~100 instructions per element)
__global__ void row_lerp32_k(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ alpha,
                             float* __restrict__ out, unsigned total, int cols, FastDiv dc) {
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
        const float a = alpha[fdiv(j, dc)];
        out[j] = x[j] + a * (y[j] - x[j]);
    }
}

// ---- reductions -------------------------------------------------------------------------------
// column sums of a [rows, cols] matrix: one thread per column chunk, lanes along columns (coalesced)
__global__ void colsum_k(const float* __restrict__ x, float* __restrict__ out, int rows, int cols) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += x[(size_t)r * cols + c];
    out[c] = s;
}

// tall matrices (the patch-matrix layers of Conv3D: 10^5..10^6 rows): block (column tile of 64, slab p) sums a contiguous range of rows
// with 4 row lanes, the lanes are added through LDS in a fixed order, part[c*P + p]; chansum_final_k adds the slabs in order.
__global__ void __launch_bounds__(256) colsum_part_k(const float* __restrict__ x, float* __restrict__ part, int rows, int cols,
                                                     int rows_per_slab, int P) {
    __shared__ float sm[4][64];
    const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6, c = blockIdx.x * 64 + lc, p = blockIdx.y;
    const int r0 = p * rows_per_slab, r1 = min(rows, r0 + rows_per_slab);
    float s = 0.f;
    if (c < cols)
        for (int r = r0 + lr; r < r1; r += 4) s += x[(size_t)r * cols + c];
    sm[lr][lc] = s;
    __syncthreads();
    if (lr == 0 && c < cols) part[(size_t)c * P + p] = (sm[0][lc] + sm[1][lc]) + (sm[2][lc] + sm[3][lc]);
}

// per-channel sum over (n, hw) of NCHW: block (c, p) sums images p, p+P, ... of channel c (each image-channel plane is HW
// contiguous floats: float4 loads when HW % 4 == 0) into part[c*P + p]; launched with P = 1 (one block per channel).
__global__ void chansum_part_k(const float* __restrict__ x, float* __restrict__ part, int N, int C, int HW, int P) {
    __shared__ float sm[32];
    const int c = blockIdx.x, p = blockIdx.y;
    float s = 0.f;
    if ((HW & 3) == 0) {
        const int hw4 = HW >> 2;
        for (int n = p; n < N; n += P) {
            const float4* pl = reinterpret_cast<const float4*>(x + ((size_t)n * C + c) * HW);
            for (int i = threadIdx.x; i < hw4; i += blockDim.x) {
                const float4 v = pl[i];
                s += (v.x + v.y) + (v.z + v.w);
            }
        }
    } else {
        for (int n = p; n < N; n += P) {
            const float* pl = x + ((size_t)n * C + c) * HW;
            for (int i = threadIdx.x; i < HW; i += blockDim.x) s += pl[i];
        }
    }
    s = block_sum(s, sm);
    if (threadIdx.x == 0) part[(size_t)c * P + p] = s;
}

// one wave per channel: lane l adds partials l, l+64, ... (coalesced), the 64 lane sums are combined by a fixed butterfly --
// deterministic, and the chain is P/64 long instead of P (one thread per channel took 50-60 us for the ~1000 partials of a tall sum)
__global__ void __launch_bounds__(256) chansum_final_k(const float* __restrict__ part, float* __restrict__ out, int C, int P) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;
    float s = 0.f;
    for (int p = lane; p < P; p += 64) s += part[(size_t)c * P + p];
    s = wave_sum(s);
    if (lane == 0) out[c] = s;
}

// ---- stochastic encoder head (TYPE_Q = 'learn_std', gan_inference_cifar10.py:173-188): std = exp(log_std), z = mean + eps * std ----------
__global__ void reparam_fwd_k(const float* __restrict__ mean, const float* __restrict__ log_std, const float* __restrict__ eps,
                              float* __restrict__ z, float* __restrict__ sd, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float s = expf(log_std[i]);
        sd[i] = s;
        z[i] = fmaf(eps[i], s, mean[i]);
    }
}

__global__ void reparam_bwd_k(const float* __restrict__ gz, const float* __restrict__ gsd, const float* __restrict__ eps,
                              const float* __restrict__ sd, float* __restrict__ gmean, float* __restrict__ glog, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float a = gz ? gz[i] : 0.f, b = gsd ? gsd[i] : 0.f;
        gmean[i] = a;
        glog[i] = (a * eps[i] + b) * sd[i];
    }
}

// ---- two row-major matrices side by side: [A | A2] <-> P (ggan::stage_cols; the mixture scripts' Linear on concat([z, k], 1)) -----------
// JOIN: P[r, c] = c < split ? A[r, c] : A2[r, c - split];  !JOIN: the inverse (P is read, A and A2 are written).  One element per thread.
template <bool JOIN>
__global__ void __launch_bounds__(kBlock) stage_cols_k(float* __restrict__ A, float* __restrict__ A2, float* __restrict__ P, int R, int C,
                                                       int split) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (size_t)R * C) return;
    const int r = (int)(i / (size_t)C), c = (int)(i - (size_t)r * C);
    float* q = c < split ? A + (size_t)r * split + c : A2 + (size_t)r * (C - split) + (c - split);
    if (JOIN) P[i] = *q;
    else *q = P[i];
}

}  // namespace

namespace ggan {

int stage_cols(bool join, float* A, float* A2, float* P, int R, int C, int split, hipStream_t s) {
    GGAN_CHECK_ARG(A && A2 && P && R > 0 && split > 0 && split < C, "bad argument");
    const size_t n = (size_t)R * C;
    GGAN_CHECK_ARG(cdivz(n, kBlock) < 0x7FFFFFFFull, "matrix too large");
    const dim3 grid((unsigned)cdivz(n, kBlock));
    if (join) {
        GGAN_LAUNCH("stage_cols<join>", 0, 8.0 * n, stage_cols_k<true>, grid, dim3(kBlock), 0, s, A, A2, P, R, C, split);
    } else {
        GGAN_LAUNCH("stage_cols<deal>", 0, 8.0 * n, stage_cols_k<false>, grid, dim3(kBlock), 0, s, A, A2, P, R, C, split);
    }
    return 0;
}

}  // namespace ggan

extern "C" {

int ggan_act_fwd(const float* x, float* y, size_t n, int act, float alpha, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && y, "null pointer");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    GGAN_CHECK_ARG(aligned16(x) && aligned16(y), "buffers must be 16-byte aligned");
    GGAN_LAUNCH("act_fwd", 0, 8.0 * n, act_fwd_k, dim3(grid_for(n, 16)), dim3(kBlock), 0, s, x, y, n, act, alpha);
    return 0;
}

int ggan_act_bwd(const float* gy, const float* ref, float* gx, size_t n, int act, float alpha, ggan_stream_t stream) {
    GGAN_CHECK_ARG(gy && ref && gx, "null pointer");
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    GGAN_CHECK_ARG(aligned16(gy) && aligned16(ref) && aligned16(gx), "buffers must be 16-byte aligned");
    GGAN_LAUNCH("act_bwd", 0, 12.0 * n, act_bwd_k, dim3(grid_for(n, 16)), dim3(kBlock), 0, s, gy, ref, gx, n, act, alpha);
    return 0;
}

int ggan_act_bwd_chansum(const float* gy, const float* ref, float* gx, float* parts, int parts_cap, int* n_parts, int N, int C, int HW,
                         int act, float alpha, ggan_stream_t stream) {
    GGAN_CHECK_ARG(gy && ref && gx && parts && n_parts, "null pointer");
    GGAN_CHECK_ARG(N > 0 && C > 0 && HW > 0 && parts_cap >= C, "bad shape");
    GGAN_CHECK_ARG(aligned16(gy) && aligned16(ref) && aligned16(gx), "buffers must be 16-byte aligned");
    // enough workgroups to cover the chip, at most one slab per image and at most parts_cap / C slabs
    int S = (512 + C - 1) / C;
    if (S > N) S = N;
    if (S > parts_cap / C) S = parts_cap / C;
    if (S > 64) S = 64;
    if (S < 1) S = 1;
    const int ipb = (N + S - 1) / S;
    S = (N + ipb - 1) / ipb;
    *n_parts = S;
    GGAN_LAUNCH("act_bwd_chansum", 0, 12.0 * N * C * HW, act_bwd_chansum_k, dim3(C, S), dim3(256), 0, (hipStream_t)stream, gy, ref, gx, parts,
                N, C, HW, ipb, act, alpha);
    return 0;
}

int ggan_bias_add(const float* x, const float* bias, float* y, int N, int C, int HW, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && bias && y && N > 0 && C > 0 && HW > 0, "bad argument");
    size_t total = (size_t)N * C * HW;
    GGAN_LAUNCH("bias_add", 0, 8.0 * total, bias_add_k, dim3(grid_for(total)), dim3(kBlock), 0, (hipStream_t)stream, x, bias, y, total, C, HW);
    return 0;
}

int ggan_cast_scale_i32(const int32_t* x, const float* noise, float* y, size_t n, float div, float mul, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && y, "null pointer");
    if (n == 0) return 0;
    GGAN_LAUNCH("cast_scale_i32", 0, 8.0 * n, cast_scale_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, x, noise, y, n, div, mul);
    return 0;
}

int ggan_cast_scale_ring_i32(const int32_t* ring, int nslots, const int32_t* ctr_a, const int32_t* ctr_b, int offset,
                             const float* noise, float* y, size_t n, float div, float mul, ggan_stream_t stream) {
    GGAN_CHECK_ARG(ring && y && nslots > 0, "bad argument");
    if (n == 0) return 0;
    GGAN_LAUNCH("cast_scale_ring_i32", 0, 8.0 * n, cast_scale_ring_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, ring,
                nslots, ctr_a, ctr_b, offset, noise, y, n, div, mul);
    return 0;
}

int ggan_axpby(const float* x, const float* y, float* out, size_t n, float a, float b, float c, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && out, "null pointer");
    if (n == 0) return 0;
    GGAN_LAUNCH("axpby", 0, 12.0 * n, axpby_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, x, y, out, n, a, b, c);
    return 0;
}

int ggan_row_lerp(const float* x, const float* y, const float* alpha, float* out, int rows, int cols, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && y && alpha && out && rows > 0 && cols > 0, "bad argument");
    size_t n = (size_t)rows * cols;
    if ((double)n * cols < 4.0e9) {
        GGAN_LAUNCH("row_lerp<32>", 0, 12.0 * n, row_lerp32_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, x, y, alpha, out, (unsigned)n, cols,
                    make_fastdiv((uint32_t)cols));
        return 0;
    }
    GGAN_LAUNCH("row_lerp<64>", 0, 12.0 * n, row_lerp_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, x, y, alpha, out, rows, cols);
    return 0;
}

int ggan_colsum(const float* x, float* out, int rows, int cols, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && out && rows > 0 && cols > 0, "bad argument");
    GGAN_LAUNCH("colsum", 0, 4.0 * rows * cols, colsum_k, dim3(cdiv(cols, 64)), dim3(64), 0, (hipStream_t)stream, x, out, rows, cols);
    return 0;
}

int ggan_colsum_tall(const float* x, float* out, int rows, int cols, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && out && rows > 0 && cols > 0, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int tiles = cdiv(cols, 64);
    int P = cdiv(1024, tiles);                       // ~1024 workgroups, at least 64 rows per slab
    if (P > rows / 64) P = rows / 64;
    ws = ws_scratch(ws, ws_bytes);
    if (P < 2 || !ws || (size_t)cols * P * sizeof(float) > ws_bytes) return ggan_colsum(x, out, rows, cols, stream);
    const int rows_per_slab = cdiv(rows, P);
    float* part = (float*)ws;
    GGAN_LAUNCH("colsum_tall", 0, 4.0 * rows * cols, colsum_part_k, dim3(tiles, P), dim3(256), 0, s, x, part, rows, cols, rows_per_slab, P);
    GGAN_LAUNCH("chansum_final", 0, 4.0 * cols * P, chansum_final_k, dim3(cdiv(cols, 4)), dim3(256), 0, s, (const float*)part, out, cols, P);
    return 0;
}

int ggan_chansum(const float* x, float* out, int N, int C, int HW, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(x && out && N > 0 && C > 0 && HW > 0, "bad argument");
    hipStream_t s = (hipStream_t)stream;
    // stage 1 over ~1024 workgroups (C x P, each sums every P-th image plane of one channel), stage 2 adds the P
    // partials per channel in a fixed order: chip-wide bandwidth, deterministic, scratch supplied by the caller
    int P = 1024 / C;
    if (P > N) P = N;
    ws = ws_scratch(ws, ws_bytes);
    if (!ws || (size_t)C * P * sizeof(float) > ws_bytes) P = 1;
    if (P <= 1) {
        const int threads = (size_t)N * HW >= 16384 ? 1024 : 256;
        GGAN_LAUNCH("chansum<one>", 0, 4.0 * N * C * HW, chansum_part_k, dim3(C, 1), dim3(threads), 0, s, x, out, N, C, HW, 1);
        return 0;
    }
    const int threads = HW >= 1024 ? 256 : (HW >= 256 ? 128 : 64);
    float* part = (float*)ws;
    GGAN_LAUNCH("chansum<part>", 0, 4.0 * N * C * HW, chansum_part_k, dim3(C, P), dim3(threads), 0, s, x, part, N, C, HW, P);
    GGAN_LAUNCH("chansum_final", 0, 4.0 * C * P, chansum_final_k, dim3(cdiv(C, 4)), dim3(256), 0, s, (const float*)part, out, C, P);
    return 0;
}

int ggan_reparam_fwd(const float* mean, const float* log_std, const float* eps, float* z, float* std_out, size_t n, ggan_stream_t stream) {
    GGAN_CHECK_ARG(mean && log_std && eps && z && std_out, "null pointer");
    if (n == 0) return 0;
    GGAN_LAUNCH("reparam_fwd", 0, 20.0 * n, reparam_fwd_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, mean, log_std, eps, z, std_out, n);
    return 0;
}

int ggan_reparam_bwd(const float* gz, const float* gstd, const float* eps, const float* std_in, float* gmean, float* glog_std, size_t n,
                     ggan_stream_t stream) {
    GGAN_CHECK_ARG((gz || gstd) && eps && std_in && gmean && glog_std, "null pointer");
    if (n == 0) return 0;
    GGAN_LAUNCH("reparam_bwd", 0, 24.0 * n, reparam_bwd_k, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, gz, gstd, eps, std_in, gmean,
                glog_std, n);
    return 0;
}

}  // extern "C"
