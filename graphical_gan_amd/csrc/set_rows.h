// What the set-level Gram-tile kernels share (mmd_sets.hip, knn_sets.hip): the row list Z = [X; Y] of two row-major fp32 sets, its
// branch-free clamped loads, the tile constants and the squared-norm pre-pass.
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

inline size_t norms_bytes(long rows) { return ((size_t)rows * sizeof(float) + 15) & ~(size_t)15; }

}  // namespace
}  // namespace ggan
