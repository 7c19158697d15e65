// What the set-level Gram-tile kernels share (mmd_sets.hip, knn_sets.hip, knn_lists.hip): the row list Z = [X; Y] of two row-major fp32
// sets, its branch-free clamped loads, the tile constants, the squared-norm pre-pass and the 128 x 128 Gram tile of the k-NN sweeps.
#pragma once
#include "common.h"

namespace ggan {
namespace {

constexpr int BT = 128;            // rows of Z per block: a tile is BT x BT
constexpr int KS = 16;             // k per main-loop step
constexpr int LD = BT + 4;         // LDS tile row (floats): 4 * LD = 16 (mod 64), the four k-quads of a staging wave hit disjoint banks
constexpr int kMaxRows = 131072;

struct RowSets {
    const float* X;
    const float* Y;
    const float* norms;            // [T] squared row norms of Z
    int m, T, d;
    int vec;                       // float4 loads legal on every row (d % 4 == 0 and both bases 16-byte aligned)
};

__device__ __forceinline__ const float* z_row(const RowSets& P, int r) {
    return r < P.m ? P.X + (size_t)r * P.d : P.Y + (size_t)(r - P.m) * P.d;
}

// four consecutive k of row r of Z (zeros beyond T or d), without a branch: the address is clamped into the row list and into the row, the
// value dropped afterwards -- every load of a step can then be in flight at once (guarded loads compile to "load; wait" chains).
// VEC (d % 4 == 0 and both bases 16-byte aligned, so every row is): one 16-byte load; k is a multiple of 4, so k < d means k + 3 < d.
// !VEC (rows of odd d are not 16-byte aligned): four dword loads, each with its own range test.
template <bool VEC>
__device__ __forceinline__ float4 load4(const RowSets& P, int r, int k) {
    const float* row = z_row(P, min(r, P.T - 1));
    const bool rok = r < P.T;
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(row + min(k, P.d - 4));
        const bool ok = rok && k < P.d;
        return make_float4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
    }
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float t = row[min(k + j, P.d - 1)];
        v[j] = (rok && k + j < P.d) ? t : 0.f;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// squared norms: one wave per row, lane-strided fma chains combined by the wave's butterfly (a fixed order)
__global__ __launch_bounds__(256) void set_norms_k(const RowSets P, float* __restrict__ norms) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= P.T) return;
    const float* z = z_row(P, r);
    float s = 0.f;
    for (int k = lane; k < P.d; k += 64) s = fmaf(z[k], z[k], s);
    s = wave_sum(s);
    if (lane == 0) norms[r] = s;
}

// staging: unit u of a thread is 4 consecutive k of one tile row; 4 lanes cover the 16 k of a row (64 contiguous bytes)
template <bool VEC>
__device__ __forceinline__ void load_step(const RowSets& P, int r0a, int r0b, int k0, float4 (&xa)[2], float4 (&xb)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int unit = threadIdx.x + 256 * u, row = unit >> 2, k = k0 + (unit & 3) * 4;
        xa[u] = load4<VEC>(P, r0a + row, k);
        xb[u] = load4<VEC>(P, r0b + row, k);
    }
}
__device__ __forceinline__ void store_step(float* As, float* Bs, const float4 (&xa)[2], const float4 (&xb)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int unit = threadIdx.x + 256 * u, row = unit >> 2, kq = unit & 3;
        float* da = &As[(kq * 4) * LD + row];
        float* db = &Bs[(kq * 4) * LD + row];
        da[0] = xa[u].x; da[LD] = xa[u].y; da[2 * LD] = xa[u].z; da[3 * LD] = xa[u].w;
        db[0] = xb[u].x; db[LD] = xb[u].y; db[2 * LD] = xb[u].z; db[3 * LD] = xb[u].w;
    }
}

// one tile: acc = Z[r0a .. r0a + 128) Z[r0b .. r0b + 128)^T (set_sums_k's main loop).  On entry ra / rb hold the tile's first step; on
// exit, if `next`, the first step of tile (n0a, n0b), in flight during the caller's epilogue.  Ends behind a barrier.
template <bool VEC>
__device__ __forceinline__ void gram_tile(const RowSets& P, int r0a, int r0b, bool next, int n0a, int n0b, float (&As)[2][KS * LD],
                                          float (&Bs)[2][KS * LD], float4 (&ra)[2], float4 (&rb)[2], f32x16 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1, half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    store_step(As[0], Bs[0], ra, rb);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < P.d; k0 += KS) {
        const bool more = k0 + KS < P.d;
        if (more) load_step<VEC>(P, r0a, r0b, k0 + KS, ra, rb);        // in flight while the MFMA block runs
        const float* Ab = As[buf];
        const float* Bb = Bs[buf];
#pragma unroll
        for (int kk = 0; kk < KS / 2; ++kk) {
            const int k = 2 * kk + half;
            const float a0 = Ab[k * LD + wm * 64 + l31], a1 = Ab[k * LD + wm * 64 + 32 + l31];
            const float b0 = Bb[k * LD + wn * 64 + l31], b1 = Bb[k * LD + wn * 64 + 32 + l31];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) store_step(As[buf ^ 1], Bs[buf ^ 1], ra, rb);
        __syncthreads();
        buf ^= 1;
    }
    if (next) load_step<VEC>(P, n0a, n0b, 0, ra, rb);
}

inline size_t norms_bytes(long rows) { return ((size_t)rows * sizeof(float) + 15) & ~(size_t)15; }

}  // namespace
}  // namespace ggan
