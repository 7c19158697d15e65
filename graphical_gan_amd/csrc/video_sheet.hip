// The frame sheets of the state-space scripts' video passes (ssgan_inference_moving_mnist.py:568-618): float frames -> the bytes of
// the PNG sheet and the palette indices of the GIF stack, both from ONE read of each pixel.
//
//   sheet [rows*H, LEN*W, C]      vis(): save_images(x, size=(rows, LEN)) -- sequence r is a row of LEN frames
//   gif   [LEN, nh*H, nw*W]       save_gifs(x, size=None): frame t tiles sequence r at grid cell (r / nw, r % nw); one palette index per
//                                 pixel: the grey byte (C = 1) or the 6x6x6 cube index 36 r6 + 6 g6 + b6, r6 = (5 r + 127) / 255 (C = 3)
//
// A lane owns four pixels along W: one 16-byte load per channel plane, one 4-byte (C = 1) or 12-byte (C = 3: the HWC bytes of its four
// pixels, built in registers) store to the sheet and one 4-byte store to the index plane; neighbouring lanes read and write
// neighbouring addresses within a frame line.  Nothing is reused, so there is no LDS and no second pass: the kernel is bounded by the
// 4 C bytes it reads and the C + 1 bytes it writes per pixel.
#include "common.h"
using namespace ggan;

namespace {

constexpr int VS_THR = 256;

struct SheetParams {
    const float* gen;      // [n][LEN][C][H][W] in [-1, 1], or null (a data-only sheet)
    const float* data;     // [n][LEN][C*H*W] as the feed holds it, or null
    uint8_t* sheet;
    uint8_t* gif;
    int LEN, H, W4, nh, nw;   // W4 = W / 4; nh x nw: the cells of one index plane
    int interleave;        // row 2i = data i, row 2i + 1 = generated i
    unsigned total;        // rows * LEN * H * W4 lane items
    float a, b, d;
};

typedef unsigned int u32x3 __attribute__((ext_vector_type(3), aligned(4)));

// q = trunc(v) clamped to 0..255 (a NaN becomes 0)
__device__ __forceinline__ unsigned to_byte(float v) { return (unsigned)(int)fminf(fmaxf(v, 0.f), 255.f); }

// every product is rounded to float32 on its own, in the written order: ((x + 1) * a) * b -- what numpy does with a float32 array
__device__ __forceinline__ unsigned gen_byte(float x, float a, float b) { return to_byte(__fmul_rn(__fmul_rn(__fadd_rn(x, 1.f), a), b)); }
__device__ __forceinline__ unsigned data_byte(float x, float d) { return to_byte(__fmul_rn(x, d)); }

template <int C>
__global__ __launch_bounds__(VS_THR) void video_sheet_k(SheetParams p) {
    const unsigned idx = blockIdx.x * VS_THR + threadIdx.x;
    if (idx >= p.total) return;
    const int w4 = idx % p.W4;
    unsigned rest = idx / p.W4;
    const int h = rest % p.H;
    rest /= p.H;
    const int t = rest % p.LEN;
    const int r = rest / p.LEN;                       // the sheet's row: one sequence
    const int W = 4 * p.W4;
    const bool from_data = p.interleave ? !(r & 1) : (p.gen == nullptr);
    const int i = p.interleave ? (r >> 1) : r;        // the sequence within its source
    const float* src = (from_data ? p.data : p.gen) + ((size_t)(i * p.LEN + t) * C) * p.H * W + (size_t)h * W + 4 * w4;
    unsigned q[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)c * p.H * W);
        const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) q[c][k] = from_data ? data_byte(x[k], p.d) : gen_byte(x[k], p.a, p.b);
    }
    const size_t line = (size_t)(r * p.H + h) * ((size_t)p.LEN * W) + (size_t)t * W + 4 * w4;      // pixels in front of this lane's four
    const int gj = r / p.nw, gi = r % p.nw;          // the sequence's cell in every frame of the index stack
    const size_t plane_w = (size_t)p.nw * W;
    uint8_t* gdst = p.gif + ((size_t)t * p.nh + gj) * p.H * plane_w + (size_t)h * plane_w + (size_t)gi * W + 4 * w4;
    if (C == 1) {
        const unsigned pk = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[0][3] << 24);
        *reinterpret_cast<unsigned*>(p.sheet + line) = pk;
        *reinterpret_cast<unsigned*>(gdst) = pk;
    } else {
        unsigned by[12], ix = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned cube = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                by[3 * k + c] = q[c][k];
                cube = cube * 6 + (5 * q[c][k] + 127) / 255;
            }
            ix |= cube << (8 * k);
        }
        u32x3 o;
        o.x = by[0] | (by[1] << 8) | (by[2] << 16) | (by[3] << 24);
        o.y = by[4] | (by[5] << 8) | (by[6] << 16) | (by[7] << 24);
        o.z = by[8] | (by[9] << 8) | (by[10] << 16) | (by[11] << 24);
        *reinterpret_cast<u32x3*>(p.sheet + 3 * line) = o;
        *reinterpret_cast<unsigned*>(gdst) = ix;
    }
}

}  // namespace

extern "C" {

int ggan_video_sheet_u8(const float* gen, const float* data, uint8_t* sheet, uint8_t* gif, int n, int rows, int LEN, int C, int H, int W,
                        int nh, int nw, int interleave, float a, float b, float d, ggan_stream_t stream) {
    GGAN_CHECK_ARG(sheet && gif, "null output");
    GGAN_CHECK_ARG(C == 1 || C == 3, "C must be 1 (grey) or 3 (RGB)");
    GGAN_CHECK_ARG(!interleave || data, "interleaved rows need a data source");
    GGAN_CHECK_ARG(interleave ? gen != nullptr : (gen != nullptr) != (data != nullptr),
                   "one source (generated frames or data), or both with interleave");
    GGAN_CHECK_ARG(n > 0 && LEN > 0 && H > 0 && W > 0 && W % 4 == 0, "bad shape (W must be a multiple of 4)");
    GGAN_CHECK_ARG(rows == (interleave ? 2 * n : n), "rows does not match n");
    GGAN_CHECK_ARG(nh > 0 && nw > 0 && (long long)nh * nw == rows, "nh * nw must be rows");
    GGAN_CHECK_ARG((double)rows * LEN * C * H * W < 2147483648.0, "sheet too large");
    GGAN_CHECK_ARG(((uintptr_t)gen | (uintptr_t)data) % 16 == 0 && ((uintptr_t)sheet | (uintptr_t)gif) % 4 == 0, "misaligned pointer");
    SheetParams p;
    p.gen = gen; p.data = data; p.sheet = sheet; p.gif = gif;
    p.LEN = LEN; p.H = H; p.W4 = W / 4; p.nh = nh; p.nw = nw; p.interleave = interleave ? 1 : 0;
    p.total = (unsigned)((size_t)rows * LEN * H * (W / 4));
    p.a = a; p.b = b; p.d = d;
    const double px = (double)rows * LEN * H * W;
    const dim3 grid((p.total + VS_THR - 1) / VS_THR);
    if (C == 1) {
        GGAN_LAUNCH("video_sheet_u8", 0, px * (4.0 + 2.0), video_sheet_k<1>, grid, dim3(VS_THR), 0, (hipStream_t)stream, p);
    } else {
        GGAN_LAUNCH("video_sheet_u8", 0, px * (12.0 + 4.0), video_sheet_k<3>, grid, dim3(VS_THR), 0, (hipStream_t)stream, p);
    }
    return 0;
}

}  // extern "C"
