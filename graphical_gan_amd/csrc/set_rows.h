// What the set-level Gram-tile kernels share (mmd_sets.hip, knn_sets.hip, knn_lists.hip, parzen_sets.hip): the row list Z = [X; Y] of two
// row-major fp32 sets, its branch-free clamped loads, the tile constants, the squared-norm pre-pass, the 128 x 128 Gram tile, the walk over
// a lane's accumulators, the query / candidate sweep with its sorted K-smallest lists, and the host preamble of the five entry points.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "common.h"

namespace ggan {
namespace {

constexpr int BT = 128;            // rows of Z per block: a tile is BT x BT
constexpr int KS = 16;             // k per main-loop step
constexpr int LD = BT + 4;         // LDS tile row (floats): 4 * LD = 16 (mod 64), the four k-quads of a staging wave hit disjoint banks
constexpr int kMaxRows = 131072;
constexpr int kTargetWgs = 2048;

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

// four consecutive k of row r of Z (zeros beyond T or d), without a branch: the address is clamped into the row list and into the row
// (load4_raw), the value dropped afterwards (load4_keep) -- every load of a step can then be in flight at once (guarded loads compile to
// "load; wait" chains).
// VEC (d % 4 == 0 and both bases 16-byte aligned, so every row is): one 16-byte load; k is a multiple of 4, so k < d means k + 3 < d.
// !VEC (rows of odd d are not 16-byte aligned): four dword loads, each with its own range test.
template <bool VEC>
__device__ __forceinline__ float4 load4_raw(const RowSets& P, int r, int k) {
    const float* row = z_row(P, min(r, P.T - 1));
    if (VEC) return *reinterpret_cast<const float4*>(row + min(k, P.d - 4));
    return make_float4(row[min(k, P.d - 1)], row[min(k + 1, P.d - 1)], row[min(k + 2, P.d - 1)], row[min(k + 3, P.d - 1)]);
}
template <bool VEC>
__device__ __forceinline__ float4 load4_keep(const RowSets& P, int r, int k, float4 t) {
    const bool rok = r < P.T;
    if (VEC) {
        const bool ok = rok && k < P.d;
        return make_float4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
    }
    return make_float4((rok && k < P.d) ? t.x : 0.f, (rok && k + 1 < P.d) ? t.y : 0.f, (rok && k + 2 < P.d) ? t.z : 0.f,
                       (rok && k + 3 < P.d) ? t.w : 0.f);
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

// staging: unit u of a thread is 4 consecutive k of one tile row; 4 lanes cover the 16 k of a row (64 contiguous bytes).  The scheduling
// barrier keeps all loads of the step ahead of the first wait: left alone, the scheduler now and then saves registers by waiting for one
// load before it issues the next (seen in single instances, whichever epilogue follows), and a step then costs four latencies, not one.
template <bool VEC>
__device__ __forceinline__ void load_step(const RowSets& P, int r0a, int r0b, int k0, float4 (&xa)[2], float4 (&xb)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int unit = threadIdx.x + 256 * u, row = unit >> 2, k = k0 + (unit & 3) * 4;
        xa[u] = load4_raw<VEC>(P, r0a + row, k);
        xb[u] = load4_raw<VEC>(P, r0b + row, k);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int unit = threadIdx.x + 256 * u, row = unit >> 2, k = k0 + (unit & 3) * 4;
        xa[u] = load4_keep<VEC>(P, r0a + row, k, xa[u]);
        xb[u] = load4_keep<VEC>(P, r0b + row, k, xb[u]);
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

// one tile, the main loop of all five kernels: acc = Z[r0a .. r0a + 128) Z[r0b .. r0b + 128)^T, 2 x 2 waves of 64 x 64, four 32x32x2
// accumulators per wave.  On entry ra / rb hold the tile's first step (loaded ahead: before the first tile, or behind the last tile's k
// loop); on exit, if `next`, the first step of tile (n0a, n0b), in flight during the caller's epilogue.  Ends behind a barrier.
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
            // one schedule for every instance: the four fragment reads of a k pair, then its four MFMAs.  Left alone, the scheduler
            // picks one of three interleavings per instance (all reads of the step first, or reads next to their MFMAs in two
            // ways), so which K or NS is fast is a matter of luck
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
        if (more) store_step(As[buf ^ 1], Bs[buf ^ 1], ra, rb);
        __syncthreads();
        buf ^= 1;
    }
    if (next) load_step<VEC>(P, n0a, n0b, 0, ra, rb);
}

// The accumulator layout, stated once: register r of acc[bi][bj] of lane l is g[row (r & 3) + 8 (r >> 2) + 4 (l >> 5)][column l & 31] of
// the 32x32 block (bi, bj) of the 64 x 64 tile of wave (wm, wn) = (wave & 1, wave >> 1).  Rows are the a side of gram_tile, columns its
// b side: a lane owns ONE b row per block column -- two per tile -- and sees 32 a rows of each.
__device__ __forceinline__ int acc_row(int bi, int r) {
    return ((threadIdx.x >> 6) & 1) * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * ((threadIdx.x >> 5) & 1);
}
__device__ __forceinline__ int acc_col(int bj) { return (threadIdx.x >> 7) * 64 + bj * 32 + (threadIdx.x & 31); }
// f(il, jl, bi, bj, r) for the 64 accumulators acc[bi][bj][r] of the lane: il / jl the tile-local a / b row; block columns outermost
template <class F>
__device__ __forceinline__ void for_each_acc(F&& f) {
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        const int jl = acc_col(bj);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int r = 0; r < 16; ++r) f(acc_row(bi, r), jl, bi, bj, r);
    }
}
// the squared distance of two rows from their squared norms and their dot product, never negative
__device__ __forceinline__ float gram_dist(float ni, float nj, float g) { return fmaxf(ni + nj - 2.f * g, 0.f); }

// ---- the query / candidate sweep (knn_sets.hip, knn_lists.hip, parzen_sets.hip) ------------------------------------------------------------
// Queries are the rows [0, nq) of Z, candidates the rows [c0, c0 + nc).  The QUERY rows are gram_tile's b side, so that a lane owns two
// queries for the whole sweep; grid (query blocks, S): workgroup (b, s) takes the candidate blocks s, s + S, ...
struct SweepParams : RowSets {
    int nq, nc, c0;
    int nbc, S;                    // candidate blocks, splits of them
};

// The walk of one workgroup: the LDS tiles, the first-step prefetch, per tile the staged norms (0 for a ghost row beyond the set), the
// Gram tile with the next one's first step behind it, the caller's epilogue and the barrier before the staged values are rewritten.
// NX = 1: one further value per candidate, extra[candidate], is staged under the norms' ghost rule and rides along in cand[1].
// tile(r0c, acc, ni, nj, cand): r0c the tile's first candidate; ni[bi][r] / nj[bj] the norms of the candidate / the query of accumulator
// acc[bi][bj][r], read from LDS once per tile, ahead of the walk; cand[1][il] the extra value of tile-local candidate il.
template <bool VEC, int NX, class Tile>
__device__ __forceinline__ void sweep_tiles(const SweepParams& P, const float* extra, Tile&& tile) {
    __shared__ __attribute__((aligned(16))) float As[2][KS * LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][KS * LD];
    __shared__ float cand[1 + NX][BT], nQ[BT];
    const int tid = threadIdx.x, r0q = blockIdx.x * BT, s = blockIdx.y;
    float4 ra[2], rb[2];
    if (s < P.nbc) load_step<VEC>(P, P.c0 + s * BT, r0q, 0, ra, rb);
    for (int c = s; c < P.nbc; c += P.S) {
        const int r0c = c * BT, cn = c + P.S;
        if (tid < BT) {
            const bool ok = r0c + tid < P.nc;
            cand[0][tid] = ok ? P.norms[P.c0 + r0c + tid] : 0.f;
            if (NX) cand[NX][tid] = ok ? extra[r0c + tid] : 0.f;
        } else {
            nQ[tid - BT] = r0q + tid - BT < P.nq ? P.norms[r0q + tid - BT] : 0.f;
        }
        f32x16 acc[2][2];
        gram_tile<VEC>(P, P.c0 + r0c, r0q, cn < P.nbc, P.c0 + cn * BT, r0q, As, Bs, ra, rb, acc);
        const float nj[2] = {nQ[acc_col(0)], nQ[acc_col(1)]};
        float ni[2][16];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int r = 0; r < 16; ++r) ni[bi][r] = cand[0][acc_row(bi, r)];
        tile(r0c, acc, ni, nj, cand);
        __syncthreads();                                   // cand / nQ are rewritten by the next tile
    }
}

// ---- the K smallest of a stream, as an ascending list in registers (K a template argument, every index a compile-time constant) ------------
// T is float (distances) or a 64-bit key (distance bits << 32 | index); min / max by overload.  Equal values are kept: a multiset.
typedef unsigned long long nkey;
__device__ __forceinline__ float lmin(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float lmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ nkey lmin(nkey a, nkey b) { return a < b ? a : b; }
__device__ __forceinline__ nkey lmax(nkey a, nkey b) { return a < b ? b : a; }
__device__ __forceinline__ float other_half(float v) { return __shfl_xor(v, 32, 64); }
__device__ __forceinline__ nkey other_half(nkey v) {
    const unsigned lo = __shfl_xor((unsigned)v, 32, 64), hi = __shfl_xor((unsigned)(v >> 32), 32, 64);
    return ((nkey)hi << 32) | lo;
}
// what an empty slot holds, above every real entry: +inf, or the key ~0 (a real key's upper word is at most the bit pattern of +inf)
template <class T> __device__ __forceinline__ T list_top();
template <> __device__ __forceinline__ float list_top<float>() { return INFINITY; }
template <> __device__ __forceinline__ nkey list_top<nkey>() { return ~(nkey)0; }

// v into the ascending list L of the K smallest values seen so far: tested against the K-th first; then every slot takes the median of
// its lower neighbour, itself and v (the lower neighbour is never the larger of the two)
template <int K, class T>
__device__ __forceinline__ void list_insert(T (&L)[K], T v) {
    if (v < L[K - 1]) {
#pragma unroll
        for (int q = K - 1; q > 0; --q) L[q] = lmax(L[q - 1], lmin(L[q], v));
        L[0] = lmin(L[0], v);
    }
}
template <int K, class T>
__device__ __forceinline__ void list_clear(T (&L)[K]) {
#pragma unroll
    for (int q = 0; q < K; ++q) L[q] = list_top<T>();
}

// behind a sweep, once per workgroup: the lists L[bj] of a lane's two queries -> the workgroup's list of every query of the block, as
// split s of part [S][K][nq].  Lanes l and l ^ 32 own the same queries (other candidates) and take each other's list; waves (0, wn) and
// (1, wn) own the same 64 queries and meet in LDS, where thread ql < 128 merges the pair of query ql.
template <int K, class T>
__device__ __forceinline__ void lists_store(T (&L)[2][K], T* part, int nq) {
    __shared__ T mg[4][64][K];                           // the waves' lists, one per owned query
    const int tid = threadIdx.x, wave = tid >> 6, r0q = blockIdx.x * BT, s = blockIdx.y;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        T o[K];
#pragma unroll
        for (int q = 0; q < K; ++q) o[q] = other_half(L[bj][q]);
#pragma unroll
        for (int q = 0; q < K; ++q) list_insert<K>(L[bj], o[q]);
        if ((tid & 32) == 0) {
#pragma unroll
            for (int q = 0; q < K; ++q) mg[wave][bj * 32 + (tid & 31)][q] = L[bj][q];
        }
    }
    __syncthreads();
    if (tid < BT) {
        const int w0 = 2 * (tid >> 6), ql = tid & 63, j = r0q + tid;
        T a[K];
#pragma unroll
        for (int q = 0; q < K; ++q) a[q] = mg[w0][ql][q];
#pragma unroll
        for (int q = 0; q < K; ++q) list_insert<K>(a, mg[w0 + 1][ql][q]);
        if (j < nq) {
#pragma unroll
            for (int q = 0; q < K; ++q) part[((size_t)s * K + q) * nq + j] = a[q];
        }
    }
}
// row j of n: the S partial lists of part [S][K][n] merged into L
template <int K, class T>
__device__ __forceinline__ void lists_merge_splits(const T* __restrict__ part, int n, int S, int j, T (&L)[K]) {
    list_clear(L);
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int q = 0; q < K; ++q) list_insert<K>(L, part[((size_t)s * K + q) * n + j]);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------
inline size_t norms_bytes(long rows) { return ((size_t)rows * sizeof(float) + 15) & ~(size_t)15; }
inline int blocks_of(long rows) { return (int)((rows + BT - 1) / BT); }
inline bool rows_ok(int n) { return n >= 1 && n <= kMaxRows; }
// splits of the candidate blocks: about kTargetWgs workgroups, so that a small query set still fills the chip
inline int splits_of(int nbq, int nbc) {
    int S = (kTargetWgs + nbq - 1) / nbq;
    if (S > nbc) S = nbc;
    return S < 1 ? 1 : S;
}

// the row list Z = [X; Y] (Y == nullptr: Z = X alone, m rows) with its norms at the head of ws, computed by set_norms_k under `name`
inline int rows_setup(RowSets& P, const char* name, const float* X, const float* Y, int m, int n, int d, void* ws, hipStream_t st) {
    P.X = X; P.Y = Y ? Y : X; P.m = m; P.T = Y ? m + n : m; P.d = d;
    P.vec = (d % 4 == 0) && ((uintptr_t)P.X & 15) == 0 && ((uintptr_t)P.Y & 15) == 0;
    float* norms = (float*)ws;
    P.norms = norms;
    GGAN_LAUNCH(name, 2.0 * P.T * d, 4.0 * P.T * d, set_norms_k, dim3(cdiv(P.T, 4)), dim3(256), 0, st, P, norms);
    return 0;
}
inline double tile_flops(double tiles, int d) { return tiles * 2.0 * BT * BT * d; }
inline double tile_bytes(double tiles, int d) { return tiles * 2.0 * BT * d * 4.0; }

struct SweepLaunch {
    dim3 grid;                     // (query blocks, S)
    double flops, bytes;           // of the sweep kernel
    void* part;                    // the workspace behind the norms: the op's partials
};
// Z = [Q; C], the queries first, the candidates behind them (C == nullptr: the m rows of Q against themselves): fills P, launches the
// norms under `name`
inline int sweep_setup(SweepParams& P, SweepLaunch& L, const char* name, const float* Q, const float* C, int m, int n, int d, void* ws,
                       hipStream_t st) {
    if (const int rc = rows_setup(P, name, Q, C, m, n, d, ws, st)) return rc;
    P.nq = m; P.nc = C ? n : m; P.c0 = C ? m : 0;
    P.nbc = blocks_of(P.nc);
    const int nbq = blocks_of(m);
    P.S = splits_of(nbq, P.nbc);
    const double tiles = (double)nbq * P.nbc;
    L.grid = dim3(nbq, P.S);
    L.flops = tile_flops(tiles, d);
    L.bytes = tile_bytes(tiles, d);
    L.part = (char*)ws + norms_bytes(P.T);
    return 0;
}

// GGAN_TRACE_SETS=1: one stderr line per launch of a Gram-sweep kernel with what its name cannot show -- the template instance (k: K or NS,
// Parzen's run-time ns, 0 where the kernel has none; vec: the loader), the width, the row and block counts, the splits and the grid.
// W == nullptr: the symmetric walk of mmd_sets.hip over the nb blocks of Z (rows m, T); else a query / candidate sweep (rows nq, nc, c0;
// blocks grid.x, nbc).  Diagnostic only (tests/test_sets_dispatch_gpu.py reads the lines); looked up per launch on the host, like
// GGAN_TRACE_GEMM.
inline bool trace_sets_on() { return getenv("GGAN_TRACE_SETS") != nullptr; }
inline void trace_sets(const char* name, int k, bool vec, const RowSets& P, const SweepParams* W, int nb, int S, dim3 grid) {
    fprintf(stderr, "[ggan] sets %s k=%d vec=%d d=%d", name, k, (int)vec, P.d);
    if (W) fprintf(stderr, " nq=%d nc=%d c0=%d nbq=%u nbc=%d", W->nq, W->nc, W->c0, grid.x, W->nbc);
    else fprintf(stderr, " m=%d T=%d nb=%d", P.m, P.T, nb);
    fprintf(stderr, " S=%d grid=(%u,%u)\n", S, grid.x, grid.y);
}
inline void trace_sweep(const char* name, int k, bool vec, const SweepParams& P, dim3 grid) {
    trace_sets(name, k, vec, P, &P, 0, P.S, grid);
}

// f(std::bool_constant<VEC>) -> status for the run-time vec; f(std::integral_constant<int, K>, std::bool_constant<VEC>) with 1 <= k <= 8
template <class F>
inline int dispatch_vec(bool vec, F&& f) {
    return vec ? f(std::true_type{}) : f(std::false_type{});
}
template <int K = 1, class F>
inline int dispatch_k_vec(int k, bool vec, F&& f) {
    if constexpr (K > 8) {
        set_error("dispatch_k_vec: k = %d outside 1 .. 8 (the caller checks the range)", k);
        return -1;
    } else {
        if (k != K) return dispatch_k_vec<K + 1>(k, vec, f);
        return dispatch_vec(vec, [&](auto VEC) { return f(std::integral_constant<int, K>{}, VEC); });
    }
}

}  // namespace
}  // namespace ggan
