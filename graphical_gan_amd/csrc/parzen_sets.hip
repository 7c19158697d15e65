// Parzen-window log-sums across two row sets (include/ggan.h):
//   ggan_parzen_lse  lse[s, i] = log sum_j exp(-D(q_i, s_j) / (2 sigma_s^2)),  D(a, b) = max(|a|^2 + |b|^2 - 2 a.b, 0)
// the per-row term of the Gaussian Parzen-window log-likelihood (Breuleux et al. 2011; Goodfellow et al. 2014) for up to 16 bandwidths
// in one sweep.  At image bandwidths every exponent lies thousands below zero -- a plain sum of kernel values is log 0 --, so the row
// sums are carried SHIFTED: per query one running minimum distance m (the arg-min does not depend on sigma, so one m serves all of them)
// and ns sums  A_s = sum_j exp(-(D_j - m) / (2 sigma_s^2)),  each term in (0, 1] and the nearest candidate's exactly 1.  When a tile
// lowers m to m', the sums are rescaled by exp(-(m - m') / (2 sigma_s^2)) first.  The result log A_s - m / (2 sigma_s^2) is finite for
// every finite input, and equals -D_min / (2 sigma_s^2) where only the nearest candidate survives in fp32.
//
// The sweep is knn_sets.hip's, ONE pass over the Gram tiles: 128 x 128 tiles (set_rows.h), the QUERY rows on the MFMA's N side, so a lane
// owns one query per 32-wide block column -- two per 64 x 64 wave tile -- for the whole sweep and sees 32 candidates of each per tile;
// grid (query blocks, S splits of the candidate blocks).  The epilogue turns the 64 accumulators into distances IN PLACE (a ghost row of
// a ragged tile, decided by index, becomes +inf, whose term is exp2(-inf) = 0), takes the tile's minimum per owned query, rescales, and
// then walks the bandwidths: one subtract, one multiply, one exp2 and one add per distance and bandwidth; the sums wait in LDS.  The pairs
// (m, A[ns]) of the lanes, waves and splits that share a query are combined by the same rescaling, always in one fixed order: wave 0
// before wave 1, lane half 0 before half 1, split 0 .. S - 1.  No floating-point atomics: two calls give the same bits, and the value
// for one bandwidth does not depend on which others ride along.
#include "common.h"
#include "set_rows.h"
using namespace ggan;

namespace {

constexpr int kMaxSigmas = 16;

struct ParzenParams : SweepParams {    // (set_rows.h: Z = [Q; S], queries and candidates, the splits)
    float* part;                   // partials [S][1 + ns][nq]: slot 0 the minimum distance, slot 1 + s the shifted sum of bandwidth s
    int ns;
    float c2[kMaxSigmas];          // -log2(e) / (2 sigma_s^2): exp(-x / (2 sigma^2)) = exp2(c2 x)
};

// the factor that moves a sum shifted by `from` to the shift `to` <= from; from == to (both +inf included: no candidate met yet) is 1
__device__ __forceinline__ float reshift(float c2, float from, float to) { return __builtin_amdgcn_exp2f(c2 * (from == to ? 0.f : from - to)); }

template <bool VEC>
__global__ __launch_bounds__(256, 2) void parzen_lse_k(const ParzenParams P) {
    warm_kernarg(P);
    // the running sums live in LDS, not in registers: 64 accumulators are live in the epilogue, and 2 x 16 sums on top of them spill.
    // Slot [g][bj][tid] belongs to thread tid alone during the sweep (consecutive lanes, consecutive banks), one read and one write per
    // tile, bandwidth and owned query -- against 2 d reads per tile of the main loop.
    __shared__ float Asum[kMaxSigmas][2][256];
    __shared__ float Msh[2][256];                          // the threads' minima, for the combination behind the sweep
    const int tid = threadIdx.x, r0q = blockIdx.x * BT, s = blockIdx.y;
    float mn[2] = {INFINITY, INFINITY};
    for (int g = 0; g < P.ns; ++g) { Asum[g][0][tid] = 0.f; Asum[g][1][tid] = 0.f; }

    sweep_tiles<VEC, 0>(P, nullptr, [&](int r0c, f32x16 (&acc)[2][2], const float (&ni)[2][16], const float (&nj)[2], const float (&)[1][BT]) {
        // accumulators -> distances in place, +inf for a ghost candidate; the tile's minimum per owned query
        float t[2] = {INFINITY, INFINITY};
        for_each_acc([&](int il, int jl, int bi, int bj, int r) {
            const float dist = gram_dist(ni[bi][r], nj[bj], acc[bi][bj][r]);
            acc[bi][bj][r] = r0c + il < P.nc ? dist : INFINITY;
            t[bj] = fminf(t[bj], acc[bi][bj][r]);
        });
        float old[2], sh[2];
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            old[bj] = mn[bj];
            mn[bj] = fminf(mn[bj], t[bj]);
            sh[bj] = mn[bj] == INFINITY ? 0.f : mn[bj];    // only ghosts so far: every term below is exp2(-inf) = 0
        }
        for (int g = 0; g < P.ns; ++g) {
            const float c2 = P.c2[g];
#pragma unroll
            for (int bj = 0; bj < 2; ++bj) {
                float a = Asum[g][bj][tid] * reshift(c2, old[bj], mn[bj]);
#pragma unroll
                for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) a += __builtin_amdgcn_exp2f(c2 * (acc[bi][bj][r] - sh[bj]));
                }
                Asum[g][bj][tid] = a;
            }
        }
    });
    Msh[0][tid] = mn[0];
    Msh[1][tid] = mn[1];
    __syncthreads();
    // query ql of the block is owned by four threads -- waves (0, wn) and (1, wn), lanes l and l ^ 32 of each, 32 candidates of a tile
    // each --: thread ql < 128 combines their pairs, wave 0 half 0 first, and writes the workgroup's partial
    if (tid < BT) {
        const int j = r0q + tid, bj = (tid >> 5) & 1, t0 = 128 * (tid >> 6) + (tid & 31);     // wave (0, wn), half 0
        if (j < P.nq) {
            const float m0 = Msh[bj][t0], m1 = Msh[bj][t0 + 32], m2 = Msh[bj][t0 + 64], m3 = Msh[bj][t0 + 96];
            const float m = fminf(fminf(m0, m1), fminf(m2, m3));
            P.part[((size_t)s * (1 + P.ns)) * P.nq + j] = m;
            for (int g = 0; g < P.ns; ++g) {
                const float c2 = P.c2[g];
                float v = __fmul_rn(Asum[g][bj][t0], reshift(c2, m0, m));
                v += __fmul_rn(Asum[g][bj][t0 + 32], reshift(c2, m1, m));
                v += __fmul_rn(Asum[g][bj][t0 + 64], reshift(c2, m2, m));
                v += __fmul_rn(Asum[g][bj][t0 + 96], reshift(c2, m3, m));
                P.part[((size_t)s * (1 + P.ns) + 1 + g) * P.nq + j] = v;
            }
        }
    }
}

// row j: the S partials under the row's overall minimum, split 0 first; lse = log A - m / (2 sigma^2)
__global__ __launch_bounds__(256) void parzen_final_k(const ParzenParams P, float* __restrict__ lse) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= P.nq) return;
    const size_t slot = (size_t)P.nq, split = (size_t)(1 + P.ns) * P.nq;
    float m = INFINITY;
    for (int s = 0; s < P.S; ++s) m = fminf(m, P.part[s * split + j]);
    for (int g = 0; g < P.ns; ++g) {
        const float c2 = P.c2[g];
        float a = 0.f;
        for (int s = 0; s < P.S; ++s) a += __fmul_rn(P.part[s * split + (1 + g) * slot + j], reshift(c2, P.part[s * split + j], m));
        lse[(size_t)g * P.nq + j] = logf(a) + 0.6931471805599453f * (c2 * m);     // c2 m = -log2(e) m / (2 sigma^2)
    }
}

}  // namespace

extern "C" {

size_t ggan_parzen_lse_workspace(int m, int n, int ns) {
    if (!rows_ok(m) || !rows_ok(n) || ns < 1 || ns > kMaxSigmas) return 0;
    return norms_bytes((long)m + n) + (size_t)splits_of(blocks_of(m), blocks_of(n)) * (1 + ns) * m * sizeof(float);
}

int ggan_parzen_lse(const float* Q, const float* S, int m, int n, int d, const float* sigmas, int ns, float* lse, void* ws,
                    size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(Q && S && sigmas && lse && ws, "null pointer");
    GGAN_CHECK_ARG(rows_ok(m) && rows_ok(n), "1 <= m, n <= 131072");
    GGAN_CHECK_ARG(d >= 1, "d < 1");
    GGAN_CHECK_ARG(ns >= 1 && ns <= kMaxSigmas, "1 <= ns <= 16");
    for (int g = 0; g < ns; ++g) GGAN_CHECK_ARG(std::isfinite(sigmas[g]) && sigmas[g] > 0.f, "sigma must be finite and positive");
    GGAN_CHECK_ARG(ws_bytes >= ggan_parzen_lse_workspace(m, n, ns), "workspace too small (ggan_parzen_lse_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    ParzenParams P;
    SweepLaunch L;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = sweep_setup(P, L, "parzen_norms", Q, S, m, n, d, ws, st)) return rc;
    P.part = (float*)L.part;
    P.ns = ns;
    for (int g = 0; g < kMaxSigmas; ++g) {
        const double sg = g < ns ? (double)sigmas[g] : 1.0;
        P.c2[g] = (float)(-1.4426950408889634 / (2.0 * sg * sg));
    }
    if (const int rc = dispatch_vec(P.vec, [&](auto VEC) {
            if (trace_sets_on()) trace_sweep("parzen_lse", ns, decltype(VEC)::value, P, L.grid);
            GGAN_LAUNCH("parzen_lse", L.flops, L.bytes, parzen_lse_k<decltype(VEC)::value>, L.grid, dim3(256), 0, st, P);
            return 0;
        }))
        return rc;
    GGAN_LAUNCH("parzen_final", 0, 4.0 * P.S * (1 + ns) * m, parzen_final_k, dim3(cdiv(m, 256)), dim3(256), 0, st, P, lse);
    return 0;
}

}  // extern "C"
