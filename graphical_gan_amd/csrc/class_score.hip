// A classifier's loss and the score of its posteriors (include/ggan.h):
//   ggan_softmax_xent_fwd_grad  mean softmax cross-entropy of logits [B, C] against int labels, its gradient, the number of rows whose argmax
//                               is their label;
//   ggan_class_score            the inception-score formula exp(mean_i KL(p_i || pbar)) per split of the rows of logits [N, C], with the mean
//                               and the population std over the splits and the two entropies it is made of.
// Both are one sweep plus one finishing workgroup.  In the sweep ONE WAVEFRONT takes a row and ONE LANE a class (C <= 64): the row's maximum
// and its sum of exponentials are xor-butterflies over the wave -- a fixed tree, the same value in every lane -- in fp32; whatever is added
// ACROSS rows is fp64: a wave adds its rows in row order, the four waves of a workgroup are added in wave order, the workgroups' partials by
// the finishing workgroup in a fixed order.  log p is always the log-softmax (x - max) - log(sum), never the log of a probability.  Nothing
// depends on the launch shape and there is no floating-point atomic: two calls give the same bits.
#include <math.h>
#include "common.h"
using namespace ggan;

namespace {

constexpr int kMaxC = GGAN_CLS_MAX_CLASSES, kMaxS = GGAN_CLS_MAX_SPLITS;
constexpr int kMaxB = 65536, kMaxN = 1 << 20;
constexpr int kWaves = 4;                  // waves of a sweep workgroup
constexpr int kXR = 64;                    // rows per workgroup of softmax_xent_k: 16 per wave
constexpr int kSR = GGAN_CLS_ROW_BLOCK;    // rows per workgroup of class_score_k: 64 per wave
static_assert(kMaxC == 64, "one lane per class");
static_assert(kMaxS <= 64, "the finishing workgroup keeps one score per split in LDS");

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// what both sweeps need of one row, lane = class: x the logit (-inf in the lanes past C), m the row's maximum, e = exp(x - m) (0 past C),
// s the sum of e, the row's non-finite flag
struct Row {
    float x, m, e, s;
    bool bad;
};
__device__ __forceinline__ Row load_row(const float* __restrict__ row, int C, int lane) {
    Row r;
    const bool in = lane < C;
    r.x = in ? row[lane] : -INFINITY;
    r.bad = __ballot(in && !isfinite(r.x)) != 0ull;
    r.m = wave_max(r.x);
    r.e = in ? expf(r.x - r.m) : 0.f;
    r.s = wave_sum(r.e);
    return r;
}

// ---- softmax cross-entropy -------------------------------------------------------------------------------------------------------------
// workgroup b: rows [b kXR, min((b + 1) kXR, B)), wave w the rows b kXR + w, + kWaves, ...; part[b] = the sum of its rows' losses (fp64),
// hit[b] the rows whose argmax is their label, flag[b] the status bits met
__global__ __launch_bounds__(64 * kWaves) void softmax_xent_k(const float* __restrict__ logits, const int* __restrict__ labels, int B, int C,
                                                              float* __restrict__ dlogits, double* __restrict__ part, int* __restrict__ hit,
                                                              int* __restrict__ flag) {
    __shared__ double ls[kWaves];
    __shared__ int hs[kWaves], fs[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r1 = min((blockIdx.x + 1) * kXR, B);
    const float fB = (float)B;
    double loss = 0.0;
    int hits = 0, bits = 0;
    for (int r = blockIdx.x * kXR + w; r < r1; r += kWaves) {
        const Row t = load_row(logits + (size_t)r * C, C, lane);
        const int y = labels[r];
        const bool y_ok = y >= 0 && y < C;
        if (t.bad) bits |= GGAN_CLS_NONFINITE;
        if (!y_ok) bits |= GGAN_CLS_BAD_LABEL;
        // the lowest class among the maxima (no arithmetic: a comparison with a value that IS one of the inputs); a row of NaN has none
        const unsigned long long top = __ballot(lane < C && t.x == t.m);
        const int arg = top ? __ffsll((long long)top) - 1 : 0;
        hits += (y_ok && arg == y) ? 1 : 0;
        const float xy = __shfl(t.x, y_ok ? y : 0, 64);         // (a label out of range is never an index)
        loss += (double)(logf(t.s) - (y_ok ? xy - t.m : 0.f));
        if (lane < C) dlogits[(size_t)r * C + lane] = (t.e / t.s - ((y_ok && lane == y) ? 1.f : 0.f)) / fB;
    }
    if (lane == 0) { ls[w] = loss; hs[w] = hits; fs[w] = bits; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double l = 0.0;
        int h = 0, f = 0;
        for (int i = 0; i < kWaves; ++i) { l += ls[i]; h += hs[i]; f |= fs[i]; }
        part[blockIdx.x] = l;
        hit[blockIdx.x] = h;
        flag[blockIdx.x] = f;
    }
}

// one workgroup: thread t adds the partials t, t + 256, ... in that order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void softmax_xent_final_k(const double* __restrict__ part, const int* __restrict__ hit,
                                                            const int* __restrict__ flag, int nblk, int B, float* __restrict__ loss,
                                                            int* __restrict__ hits, int* __restrict__ status) {
    __shared__ double ls[256];
    __shared__ int hs[256], fs[256];
    const int tid = threadIdx.x;
    double l = 0.0;
    int h = 0, f = 0;
    for (int b = tid; b < nblk; b += 256) { l += part[b]; h += hit[b]; f |= flag[b]; }
    ls[tid] = l; hs[tid] = h; fs[tid] = f;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { ls[tid] += ls[tid + o]; hs[tid] += hs[tid + o]; fs[tid] |= fs[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        loss[0] = fs[0] ? __builtin_nanf("") : (float)(ls[0] / (double)B);
        hits[0] = hs[0];
        status[0] = fs[0];
    }
}

// ---- class score ---------------------------------------------------------------------------------------------------------------------------
// split s covers the rows [s N / S, (s + 1) N / S) (integer division)
__device__ __host__ __forceinline__ int split_start(int s, int N, int S) { return (int)(((long long)s * N) / S); }

// workgroup (j, s): rows start_s + j kSR ... of split s (none: zeros), wave w the rows + w, + kWaves, ...; part[(s nchunk + j)(C + 1) + c] =
// sum_i p_ic for c < C and, at c = C, sum_i sum_c p_ic log p_ic (each row's sum in fp32 over the wave, the rows in fp64)
__global__ __launch_bounds__(64 * kWaves) void class_score_k(const float* __restrict__ logits, int N, int C, int S, int nchunk,
                                                             double* __restrict__ part, int* __restrict__ flag) {
    __shared__ double cs[kWaves][kMaxC + 1];
    __shared__ int fs[kWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x, s = blockIdx.y;
    const int r0 = split_start(s, N, S) + j * kSR, r1 = min(r0 + kSR, split_start(s + 1, N, S));
    double col = 0.0, plp = 0.0;
    int bits = 0;
    for (int r = r0 + w; r < r1; r += kWaves) {
        const Row t = load_row(logits + (size_t)r * C, C, lane);
        if (t.bad) bits |= GGAN_CLS_NONFINITE;
        const float p = t.e / t.s;
        const float lp = (t.x - t.m) - logf(t.s);
        col += (double)p;
        plp += (double)wave_sum(lane < C ? p * lp : 0.f);        // (p = 0 where the exponential underflowed, lp is finite: 0, not NaN)
    }
    if (lane < C) cs[w][lane] = col;
    if (lane == 0) { cs[w][kMaxC] = plp; fs[w] = bits; }
    __syncthreads();
    double* out = part + ((size_t)s * nchunk + j) * (C + 1);
    if (w == 0 && lane < C) out[lane] = ((cs[0][lane] + cs[1][lane]) + cs[2][lane]) + cs[3][lane];
    if (w == 1 && lane == 0) {                                  // (not a 65th lane of wave 0: C may be 64)
        out[C] = ((cs[0][kMaxC] + cs[1][kMaxC]) + cs[2][kMaxC]) + cs[3][kMaxC];
        flag[(size_t)s * nchunk + j] = (fs[0] | fs[1]) | (fs[2] | fs[3]);
    }
}

// one workgroup; wave w finishes the splits w, w + kWaves, ... (lane = class, a split's chunks in chunk order), then wave 0 the whole set
__global__ __launch_bounds__(64 * kWaves) void class_score_final_k(const double* __restrict__ part, const int* __restrict__ flag, int N, int C,
                                                                   int S, int nchunk, float* __restrict__ scores, float* __restrict__ stats,
                                                                   int* __restrict__ status) {
    __shared__ double cs[kMaxS][kMaxC];      // column sums per split
    __shared__ double sc[kMaxS], pl[kMaxS];  // score and sum p log p per split
    __shared__ int fs[64 * kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int f = 0;
    for (int b = tid; b < S * nchunk; b += 64 * kWaves) f |= flag[b];
    fs[tid] = f;
    for (int s = w; s < S; s += kWaves) {
        const double* ps = part + (size_t)s * nchunk * (C + 1);
        double col = 0.0, plp = 0.0;
        for (int j = 0; j < nchunk; ++j) {
            if (lane < C) col += ps[(size_t)j * (C + 1) + lane];
            plp += ps[(size_t)j * (C + 1) + C];
        }
        const double n = (double)(split_start(s + 1, N, S) - split_start(s, N, S));
        const double pb = col / n;
        const double hbar = -wave_sum_f64((lane < C && pb > 0.0) ? pb * log(pb) : 0.0);
        if (lane < C) cs[s][lane] = col;
        if (lane == 0) { sc[s] = exp(hbar + plp / n); pl[s] = plp; }
    }
    __syncthreads();
    if (w != 0) return;
    for (int i = 1; i < kWaves; ++i) f |= fs[lane + 64 * i];
    f |= fs[lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f |= __shfl_xor(f, o, 64);
    double col = 0.0, plp = 0.0, mean = 0.0, var = 0.0;
    for (int s = 0; s < S; ++s) {
        if (lane < C) col += cs[s][lane];
        plp += pl[s];
        mean += sc[s];
    }
    mean /= (double)S;
    for (int s = 0; s < S; ++s) var += (sc[s] - mean) * (sc[s] - mean);
    const double pb = col / (double)N;
    const double hbar = -wave_sum_f64((lane < C && pb > 0.0) ? pb * log(pb) : 0.0);
    const float nan = __builtin_nanf("");
    if (lane < S) scores[lane] = f ? nan : (float)sc[lane];
    if (lane == 0) {
        stats[0] = f ? nan : (float)mean;
        stats[1] = f ? nan : (float)sqrt(var / (double)S);
        stats[2] = f ? nan : (float)(-plp / (double)N);
        stats[3] = f ? nan : (float)hbar;
        status[0] = f;
    }
}

inline bool xent_ok(int B, int C) { return B >= 1 && B <= kMaxB && C >= 2 && C <= kMaxC; }
inline bool score_ok(int N, int C, int S) { return S >= 1 && S <= kMaxS && N >= S && N <= kMaxN && C >= 2 && C <= kMaxC; }
// chunks of kSR rows in the longest split, ceil(N / S) rows
inline int score_chunks(int N, int S) { return cdiv(cdiv(N, S), kSR); }

}  // namespace

extern "C" {

size_t ggan_softmax_xent_workspace(int B, int classes) {
    if (!xent_ok(B, classes)) return 0;
    const size_t nb = cdiv(B, kXR);
    return align16(nb * sizeof(double)) + 2 * align16(nb * sizeof(int));
}

int ggan_softmax_xent_fwd_grad(const float* logits, const int32_t* labels, int B, int classes, float* loss, float* dlogits, int32_t* hits,
                               int32_t* status, void* ws, size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(logits && labels && loss && dlogits && hits && status && ws, "null pointer");
    GGAN_CHECK_ARG(xent_ok(B, classes), "1 <= B <= 65536, 2 <= classes <= 64");
    GGAN_CHECK_ARG(ws_bytes >= ggan_softmax_xent_workspace(B, classes), "workspace too small (ggan_softmax_xent_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    const int nb = cdiv(B, kXR);
    double* part = (double*)ws;
    int* hit = (int*)((char*)ws + align16((size_t)nb * sizeof(double)));
    int* flag = (int*)((char*)hit + align16((size_t)nb * sizeof(int)));
    hipStream_t st = (hipStream_t)stream;
    GGAN_LAUNCH("softmax_xent", 8.0 * B * classes, 8.0 * B * classes + 4.0 * B, softmax_xent_k, dim3(nb), dim3(64 * kWaves), 0, st, logits,
                (const int*)labels, B, classes, dlogits, part, hit, flag);
    GGAN_LAUNCH("softmax_xent_final", 1.0 * nb, 16.0 * nb, softmax_xent_final_k, dim3(1), dim3(256), 0, st, (const double*)part,
                (const int*)hit, (const int*)flag, nb, B, loss, (int*)hits, (int*)status);
    return 0;
}

size_t ggan_class_score_workspace(int N, int classes, int splits) {
    if (!score_ok(N, classes, splits)) return 0;
    const size_t nb = (size_t)splits * score_chunks(N, splits);
    return align16(nb * (classes + 1) * sizeof(double)) + align16(nb * sizeof(int));
}

int ggan_class_score(const float* logits, int N, int classes, int splits, float* scores, float* stats, int32_t* status, void* ws,
                     size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(logits && scores && stats && status && ws, "null pointer");
    GGAN_CHECK_ARG(score_ok(N, classes, splits), "1 <= splits <= 64, splits <= N <= 1048576, 2 <= classes <= 64");
    GGAN_CHECK_ARG(ws_bytes >= ggan_class_score_workspace(N, classes, splits), "workspace too small (ggan_class_score_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    const int nchunk = score_chunks(N, splits);
    const size_t nb = (size_t)splits * nchunk;
    double* part = (double*)ws;
    int* flag = (int*)((char*)ws + align16(nb * (classes + 1) * sizeof(double)));
    hipStream_t st = (hipStream_t)stream;
    GGAN_LAUNCH("class_score", 10.0 * N * classes, 4.0 * N * classes, class_score_k, dim3(nchunk, splits), dim3(64 * kWaves), 0, st, logits, N,
                classes, splits, nchunk, part, flag);
    GGAN_LAUNCH("class_score_final", 1.0 * nb * classes, 8.0 * nb * (classes + 1), class_score_final_k, dim3(1), dim3(64 * kWaves), 0, st,
                (const double*)part, (const int*)flag, N, classes, splits, nchunk, scores, stats, (int*)status);
    return 0;
}

}  // extern "C"
