// Reconstruction fidelity of image pairs (include/ggan.h):
//   ggan_ssim_pairs  mse[i] = mean (ua - ub)^2,  ssim[i] = mean over channels and valid window positions of the structural similarity
// (Wang, Bovik, Sheikh, Simoncelli 2004) under the separable 11x11 Gaussian window of sigma 1.5, u = scale * x + shift the unit-scale pixel.
//
// One workgroup per (image, channel) plane.  Both planes are staged into LDS once -- 16-byte loads where both plane addresses allow, a
// scalar path otherwise --, so every input value is read from HBM exactly once; the unit-scale map is applied on the way in.  A second walk
// over the LDS image, in ONE thread assignment whichever path staged it, gives the plane sums of ua, ub and (ua - ub)^2: the mse, and the two
// plane means the moments are centred by.  sxx = E[x^2] - mx^2 cancels in fp32 on bright flat regions, where C2 = 8.1e-4 is all that stands
// in the denominator (0.98 + 1e-3 noise: 1.4e-5 off); variance and covariance are shift-invariant, so the five window moments are taken of
// x - mean(x), y - mean(y) and the means are added back for mx, my alone (1.2e-7 off).
//
// The horizontal 11-tap pass runs LDS to LDS for the five moments (x, y, xx, yy, xy), one output per thread, consecutive lanes on
// consecutive columns; the vertical pass runs in registers: a thread owns one column and four output rows, reads the 14 row-filtered
// values of a moment once and forms its four outputs from them.  The SSIM map never leaves the CU.  The row-filtered moments are kept for
// a BAND of output rows plus a 10-row halo: at 64 x 64 the whole map would take 69 KB beside the 32 KB of the planes and leave one
// workgroup per CU; bands of 16 rows take 28 KB, 60 KB in all, two workgroups per CU and no opt-in to large LDS, for 94 instead of 64
// filtered rows.  Smaller planes fit in one band.  The workgroup is 64, 128 or 256 threads by the work a band holds.
//
// Per-thread sums are combined by wave shuffle, then across the waves through LDS in wave order, into two floats per plane; a second small
// launch adds the c planes of an image in index order and divides.  No floating-point atomics; every order is fixed by (h, w) alone, so
// two calls give the same bits and an image's values depend neither on its neighbours nor on n.  The products that decide whether a set
// against itself scores exactly 1 are written with the unfused intrinsics: a contraction would round the two sides of the ratio apart.
#include "common.h"
#include <math.h>
using namespace ggan;

namespace {

constexpr int kTaps = 11, kHalo = kTaps - 1;
constexpr int kMaxRows = 131072, kMaxC = 4, kMinSide = kTaps, kMaxSide = 64;
constexpr int kLdsFloats = 16000;          // planes + row-filtered moments of a band: 64000 B, two workgroups per CU
constexpr int kVRows = 4;                  // output rows a thread of the vertical pass owns
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct SsimParams {
    const float* A;
    const float* B;
    float* part;                           // [planes][2]: sum of (ua - ub)^2, sum of the SSIM map
    int h, w, ho, wo, hw, hw4;             // hw4: hw rounded up to a multiple of 4 (the second plane starts 16-byte aligned)
    int band;                              // output rows per band
    float sa, ha, sb, hb;
    float g[kTaps];
};

// three block sums at once, valid in every thread: wave shuffle, then the waves in index order
__device__ __forceinline__ void block_sum3(float& a, float& b, float& c, float (*red)[4]) {
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) { red[0][wid] = a; red[1][wid] = b; red[2][wid] = c; }
    __syncthreads();
    float ta = 0.f, tb = 0.f, tc = 0.f;
    for (int i = 0; i < nw; ++i) { ta += red[0][i]; tb += red[1][i]; tc += red[2][i]; }
    a = ta; b = tb; c = tc;
}

__global__ __launch_bounds__(256) void ssim_planes_k(const SsimParams P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float red[3][4];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int w = P.w, wo = P.wo, hw = P.hw;
    float* pa = lds;
    float* pb = lds + P.hw4;
    float* hm = pb + P.hw4;                                // [5][band + 10][wo]
    const int hstride = (P.band + kHalo) * wo;
    const float* a = P.A + (size_t)blockIdx.x * hw;
    const float* b = P.B + (size_t)blockIdx.x * hw;

    // ---- stage both planes, in unit scale
    if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
        const int n4 = hw >> 2;
        for (int i = tid; i < n4; i += nt) {
            const float4 va = reinterpret_cast<const float4*>(a)[i], vb = reinterpret_cast<const float4*>(b)[i];
            float4 ua, ub;
            ua.x = __builtin_fmaf(P.sa, va.x, P.ha); ua.y = __builtin_fmaf(P.sa, va.y, P.ha);
            ua.z = __builtin_fmaf(P.sa, va.z, P.ha); ua.w = __builtin_fmaf(P.sa, va.w, P.ha);
            ub.x = __builtin_fmaf(P.sb, vb.x, P.hb); ub.y = __builtin_fmaf(P.sb, vb.y, P.hb);
            ub.z = __builtin_fmaf(P.sb, vb.z, P.hb); ub.w = __builtin_fmaf(P.sb, vb.w, P.hb);
            reinterpret_cast<float4*>(pa)[i] = ua;
            reinterpret_cast<float4*>(pb)[i] = ub;
        }
        for (int i = 4 * n4 + tid; i < hw; i += nt) {
            pa[i] = __builtin_fmaf(P.sa, a[i], P.ha);
            pb[i] = __builtin_fmaf(P.sb, b[i], P.hb);
        }
    } else {
        for (int i = tid; i < hw; i += nt) {
            pa[i] = __builtin_fmaf(P.sa, a[i], P.ha);
            pb[i] = __builtin_fmaf(P.sb, b[i], P.hb);
        }
    }
    __syncthreads();

    // ---- plane sums from the LDS image: one assignment of elements to threads whichever path staged them
    float s_a = 0.f, s_b = 0.f, s_d = 0.f;
    for (int i = tid; i < hw; i += nt) {
        const float xa = pa[i], xb = pb[i], d = xa - xb;
        s_a += xa;
        s_b += xb;
        s_d = __builtin_fmaf(d, d, s_d);
    }
    block_sum3(s_a, s_b, s_d, red);
    const float ca = s_a / (float)hw, cb = s_b / (float)hw;

    float acc = 0.f;                                       // this thread's share of the SSIM map
    for (int r0 = 0; r0 < P.ho; r0 += P.band) {
        const int rows_out = min(P.band, P.ho - r0), hrows = rows_out + kHalo;
        // ---- horizontal pass, LDS to LDS: the five moments of the centred values, rows r0 .. r0 + hrows - 1
        for (int it = tid; it < hrows * wo; it += nt) {
            const int r = it / wo, j = it - r * wo;
            const float* xa = pa + (r0 + r) * w + j;
            const float* xb = pb + (r0 + r) * w + j;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float x = xa[k] - ca, y = xb[k] - cb;
                const float gx = __fmul_rn(P.g[k], x), gy = __fmul_rn(P.g[k], y);
                m0 += gx;
                m1 += gy;
                m2 = __builtin_fmaf(gx, x, m2);
                m3 = __builtin_fmaf(gy, y, m3);
                m4 = __builtin_fmaf(gx, y, m4);
            }
            float* o = hm + r * wo + j;
            o[0] = m0; o[hstride] = m1; o[2 * hstride] = m2; o[3 * hstride] = m3; o[4 * hstride] = m4;
        }
        __syncthreads();
        // ---- vertical pass in registers: column j, output rows 4 q .. 4 q + 3 of the band
        const int groups = (rows_out + kVRows - 1) / kVRows;
        for (int it = tid; it < groups * wo; it += nt) {
            const int q = it / wo, j = it - q * wo, rq = q * kVRows;
            float out[5][kVRows];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                float v[kVRows + kHalo];
#pragma unroll
                for (int k = 0; k < kVRows + kHalo; ++k) v[k] = rq + k < hrows ? hm[m * hstride + (rq + k) * wo + j] : 0.f;
#pragma unroll
                for (int o = 0; o < kVRows; ++o) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < kTaps; ++k) s = __builtin_fmaf(P.g[k], v[o + k], s);
                    out[m][o] = s;
                }
            }
#pragma unroll
            for (int o = 0; o < kVRows; ++o) {
                if (rq + o >= rows_out) break;
                const float dx = out[0][o], dy = out[1][o];
                const float mx = ca + dx, my = cb + dy;
                const float sxx = __fsub_rn(out[2][o], __fmul_rn(dx, dx));
                const float syy = __fsub_rn(out[3][o], __fmul_rn(dy, dy));
                const float sxy = __fsub_rn(out[4][o], __fmul_rn(dx, dy));
                const float num = __fmul_rn(__fadd_rn(__fmul_rn(2.f, __fmul_rn(mx, my)), kC1), __fadd_rn(__fmul_rn(2.f, sxy), kC2));
                const float den = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my)), kC1),
                                            __fadd_rn(__fadd_rn(sxx, syy), kC2));
                acc += __fdiv_rn(num, den);
            }
        }
        __syncthreads();                                   // the next band rewrites hm
    }
    float z0 = 0.f, z1 = 0.f;
    block_sum3(acc, z0, z1, red);
    if (tid == 0) {
        P.part[2 * (size_t)blockIdx.x] = s_d;
        P.part[2 * (size_t)blockIdx.x + 1] = acc;
    }
}

// image i: its c planes in index order
__global__ __launch_bounds__(256) void ssim_images_k(const float* __restrict__ part, int n, int c, int hw, int valid, float* __restrict__ mse,
                                                     float* __restrict__ ssim) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sd = 0.f, ss = 0.f;
    for (int ch = 0; ch < c; ++ch) {
        sd += part[2 * ((size_t)i * c + ch)];
        ss += part[2 * ((size_t)i * c + ch) + 1];
    }
    mse[i] = sd / (float)(c * hw);
    ssim[i] = ss / (float)(c * valid);
}

inline bool args_ok(int n, int c, int h, int w) {
    return n >= 1 && n <= kMaxRows && c >= 1 && c <= kMaxC && h >= kMinSide && h <= kMaxSide && w >= kMinSide && w <= kMaxSide;
}

// output rows per band: all of them where the row-filtered moments fit beside the planes, else a multiple of the vertical pass's row group
inline int band_of(int h, int w) {
    const int ho = h - kHalo, wo = w - kHalo, hw4 = (h * w + 3) & ~3;
    int band = (kLdsFloats - 2 * hw4) / (5 * wo) - kHalo;
    if (band >= ho) return ho;
    return band >= kVRows ? band / kVRows * kVRows : band;
}

}  // namespace

extern "C" {

size_t ggan_ssim_pairs_workspace(int n, int c, int h, int w) {
    if (!args_ok(n, c, h, w)) return 0;
    return (size_t)n * c * 2 * sizeof(float);
}

int ggan_ssim_pairs(const float* A, const float* B, int n, int c, int h, int w, float scale_a, float shift_a, float scale_b, float shift_b,
                    float* mse, float* ssim, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(A && B && mse && ssim && ws, "null pointer");
    GGAN_CHECK_ARG(n >= 1 && n <= kMaxRows, "1 <= n <= 131072");
    GGAN_CHECK_ARG(c >= 1 && c <= kMaxC, "1 <= c <= 4");
    GGAN_CHECK_ARG(h >= kMinSide && h <= kMaxSide && w >= kMinSide && w <= kMaxSide, "11 <= h, w <= 64");
    GGAN_CHECK_ARG(std::isfinite(scale_a) && std::isfinite(shift_a) && std::isfinite(scale_b) && std::isfinite(shift_b),
                   "the unit-scale maps must be finite");
    GGAN_CHECK_ARG(ws_bytes >= ggan_ssim_pairs_workspace(n, c, h, w), "workspace too small (ggan_ssim_pairs_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 3) == 0, "workspace must be 4-byte aligned");
    SsimParams P;
    P.A = A; P.B = B; P.part = (float*)ws;
    P.h = h; P.w = w; P.ho = h - kHalo; P.wo = w - kHalo; P.hw = h * w; P.hw4 = (P.hw + 3) & ~3;
    P.band = band_of(h, w);
    GGAN_CHECK_ARG(P.band >= 1, "no band of output rows fits in LDS");
    P.sa = scale_a; P.ha = shift_a; P.sb = scale_b; P.hb = shift_b;
    double g[kTaps], sum = 0.0;                            // the window: exp(-k^2 / (2 sigma^2)), sigma 1.5, normalised to sum 1
    for (int k = 0; k < kTaps; ++k) sum += g[k] = exp(-0.5 * (k - 5) * (k - 5) / (1.5 * 1.5));
    for (int k = 0; k < kTaps; ++k) P.g[k] = (float)(g[k] / sum);
    const int items = (P.band + kHalo) * P.wo;             // the horizontal pass of a full band
    const int threads = items >= 192 ? 256 : items >= 96 ? 128 : 64;
    const size_t lds = (size_t)(2 * P.hw4 + 5 * (P.band + kHalo) * P.wo) * sizeof(float);
    const int planes = n * c;
    hipStream_t st = (hipStream_t)stream;
    const double taps = (double)planes * (P.ho + kHalo * cdiv(P.ho, P.band)) * P.wo * kTaps * 10.0 + (double)planes * P.ho * P.wo * kTaps * 10.0;
    GGAN_LAUNCH("ssim_planes", taps, 8.0 * planes * P.hw, ssim_planes_k, dim3(planes), dim3(threads), lds, st, P);
    GGAN_LAUNCH("ssim_images", 0, 8.0 * planes, ssim_images_k, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float*)P.part, n, c, P.hw,
                P.ho * P.wo, mse, ssim);
    return 0;
}

}  // extern "C"
