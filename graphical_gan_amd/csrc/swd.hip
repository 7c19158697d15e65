// Sliced Wasserstein distance between two sets of projected rows (include/ggan.h): per direction l, W_p^p between the empirical measures of
// column l of PX [m, L] and of column l of PY [n, L] -- in one dimension the optimal plan is the sorted order, so a direction costs two sorts
// and the quantile integral.
//   swd_transpose_k  PX, PY -> XT [L, m], YT [L, n] in the workspace, through a 32 x 32 LDS tile: the stride-L column becomes a contiguous row
//                    (scalar loads: no alignment and no multiple of anything is assumed of L or of the pointers)
//   swd_sort_k       one workgroup per direction: both columns padded with +inf to powers of two (a real inf is found while loading and raises
//                    the status before anything is computed from a key), a bitonic network on each with its compare-exchanges on registers,
//                    the sorted columns in LDS, then the integral over the merged breakpoints with integer weights, everything behind
//                    the float32 keys in fp64
//   swd_final_k      mean and max over the directions in index order in fp64, the root
// No floating-point atomic; every sum runs in an order fixed by sorted position: the result depends on the multiset of each column only, and
// two calls give the same bits.
#include <math.h>
#include "common.h"
using namespace ggan;

namespace {

constexpr int kMaxRows = GGAN_SWD_MAX_ROWS;
constexpr int kMaxDirs = GGAN_SWD_MAX_DIRS;
constexpr int kMinPad = 64;            // a padded column is at least one wave wide: the in-wave stages then never meet an idle lane
constexpr int kKeys = 16;              // keys a thread holds in registers, from 1024 keys a column on (below: a column is one wave's)
constexpr int kSortThreads = 1024;     // at most: kMaxRows / kKeys
constexpr int kTile = 32;
static_assert(kMaxRows == kKeys * kSortThreads && kMaxRows == 16384 && (kMaxRows & (kMaxRows - 1)) == 0, "two padded columns of kMaxRows floats are the 128 KiB the sort kernel asks for");
static_assert((size_t)kMaxRows * kMaxRows <= (1u << 28), "the integer weights of the integral fit an int");

inline bool shape_ok(int m, int n, int L) { return m >= 1 && m <= kMaxRows && n >= 1 && n <= kMaxRows && L >= 1 && L <= kMaxDirs; }
inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
// the padded length of a column of n keys: the next power of two, at least kMinPad
__host__ __device__ inline int padded(int n) {
    int p = kMinPad;
    while (p < n) p <<= 1;
    return p;
}

// ---- transpose ----------------------------------------------------------------------------------------------------------------------------
// blockIdx.z picks the set; tile (blockIdx.y: rows, blockIdx.x: directions).  32 x 8 threads; reads run along l, writes along the row index.
__global__ __launch_bounds__(256) void swd_transpose_k(const float* __restrict__ PX, const float* __restrict__ PY, int m, int n, int L,
                                                       float* __restrict__ XT, float* __restrict__ YT) {
    __shared__ float tile[kTile][kTile + 1];
    const float* __restrict__ src = blockIdx.z ? PY : PX;
    float* __restrict__ dst = blockIdx.z ? YT : XT;
    const int rows = blockIdx.z ? n : m;
    const int r0 = blockIdx.y * kTile, l0 = blockIdx.x * kTile;
    if (r0 >= rows) return;                    // (the same for the whole workgroup, in front of the barrier)
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < kTile; k += 8) {
        const int r = r0 + ty + k, l = l0 + tx;
        if (r < rows && l < L) tile[ty + k][tx] = src[(size_t)r * L + l];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTile; k += 8) {
        const int l = l0 + ty + k, r = r0 + tx;
        if (r < rows && l < L) dst[(size_t)l * rows + r] = tile[tx][ty + k];
    }
}

// ---- sort -----------------------------------------------------------------------------------------------------------------------------------
// A bitonic network on a column of P keys in LDS, P = 64 KPT << LW: merge widths k = 2 .. P, partner distances j = k / 2 .. 1 inside each,
// ascending where (i & k) == 0.  Who holds which key follows the distance, so that most stages never touch LDS:
//   the low layout   thread (wave w, lane) holds the KPT keys i = lane | s << 6 | w * 64 KPT: distances below 64 are another lane of the same
//                    wave (__shfl_xor), distances 64 .. 32 KPT another register of the same thread.  Every width up to 64 KPT runs here
//                    without a barrier, and so do the distances below 64 KPT of every wider merge;
//   the high layout  thread g holds the 1 << LW keys i = g | s * 64 KPT: the distances 64 KPT .. P / 2 of the wider merges are registers of
//                    one thread again.
// A merge wider than 64 KPT is one pass in the high layout and one in the low layout, an LDS round trip and a barrier each; in both layouts
// consecutive threads take consecutive keys.  Comparisons only: keys are moved, never computed, and a NaN leaves the order undefined and
// changes nothing else -- the trip counts depend on P alone.

// one compare-exchange of two keys a thread holds, `lo` the one of the lower index
__device__ __forceinline__ void exchange(float& lo, float& hi, bool up) {
    const float a = lo, b = hi;
    const bool sw = up ? (a > b) : (a < b);
    lo = sw ? b : a;
    hi = sw ? a : b;
}

// ... and of a key with its partner's copy from another lane: the lower index of an ascending pair keeps the smaller key
__device__ __forceinline__ float keep(float v, float o, bool take_min) { return take_min ? (o < v ? o : v) : (o > v ? o : v); }

// the stages of merge width k with partner distance below 64 KPT, on the keys i = base | s << 6 of the low layout
template <int KPT>
__device__ __forceinline__ void low_stages(float (&v)[KPT], int base, int lane, int k) {
#pragma unroll
    for (int jb = KPT >> 1; jb >= 1; jb >>= 1) {             // distance 64 jb: register s against register s | jb
        if (64 * jb < k) {
#pragma unroll
            for (int s = 0; s < KPT; ++s)
                if (!(s & jb)) exchange(v[s], v[s | jb], ((base | (s << 6)) & k) == 0);
        }
    }
#pragma unroll
    for (int j = 32; j >= 1; j >>= 1) {                      // distance j: lane against lane ^ j
        if (j < k) {
#pragma unroll
            for (int s = 0; s < KPT; ++s) {
                const float o = __shfl_xor(v[s], j, 64);
                v[s] = keep(v[s], o, (((base | (s << 6)) & k) == 0) == ((lane & j) == 0));
            }
        }
    }
}

// the stages of merge width k with partner distance 64 KPT and above, on the keys i = g | s * 64 KPT of the high layout, by all the threads
template <int KPT, int LW>
__device__ __forceinline__ void high_stages(float* S, int tid, int nthreads, int k) {
    constexpr int G = 64 * KPT, N = 1 << LW;
    for (int g = tid; g < G; g += nthreads) {
        float u[N];
#pragma unroll
        for (int s = 0; s < N; ++s) u[s] = S[g + s * G];
#pragma unroll
        for (int jb = N >> 1; jb >= 1; jb >>= 1) {
            if (G * jb < k) {
#pragma unroll
                for (int s = 0; s < N; ++s)
                    if (!(s & jb)) exchange(u[s], u[s | jb], ((s * G) & k) == 0);
            }
        }
#pragma unroll
        for (int s = 0; s < N; ++s) S[g + s * G] = u[s];
    }
}

// column src[0 .. n) -> sorted in S[0 .. P), P = 64 KPT << LW >= n, the tail +inf; `bad` collects a non-finite key.  The first 64 << LW
// threads hold keys in the low layout, the others only help in the high layout; every thread meets every barrier.
template <int KPT, int LW>
__device__ __forceinline__ void sort_column(const float* __restrict__ src, int n, float* S, int tid, int nthreads, bool& bad) {
    constexpr int P = (64 * KPT) << LW;
    const bool on = tid < (64 << LW);          // (whole waves)
    const int lane = tid & 63, base = lane | ((tid >> 6) * (64 * KPT));
    float v[KPT];
    if (on) {
#pragma unroll
        for (int s = 0; s < KPT; ++s) {
            const int i = base | (s << 6);
            v[s] = i < n ? src[i] : INFINITY;
            bad |= i < n && !isfinite(v[s]);
        }
#pragma nounroll
        for (int k = 2; k <= 64 * KPT; k <<= 1) low_stages<KPT>(v, base, lane, k);
#pragma unroll
        for (int s = 0; s < KPT; ++s) S[base | (s << 6)] = v[s];
    }
    __syncthreads();
#pragma nounroll
    for (int k = 128 * KPT; k <= P; k <<= 1) {
        high_stages<KPT, LW>(S, tid, nthreads, k);
        __syncthreads();
        if (on) {
#pragma unroll
            for (int s = 0; s < KPT; ++s) v[s] = S[base | (s << 6)];
            low_stages<KPT>(v, base, lane, k);
#pragma unroll
            for (int s = 0; s < KPT; ++s) S[base | (s << 6)] = v[s];
        }
        __syncthreads();
    }
}

// the threads of a workgroup: one per kKeys keys of the longer padded column, at least a wave
__host__ __device__ inline int sort_threads(int m, int n) {
    const int P = padded(m > n ? m : n);
    return P / kKeys < 64 ? 64 : P / kKeys;
}

// dynamic LDS: the two padded columns
__host__ __device__ inline size_t sort_lds(int m, int n) { return ((size_t)padded(m) + padded(n)) * sizeof(float); }

// One workgroup per direction.  The trip counts of the network depend on the padded sizes alone, so non-finite keys go through it like any
// others; the flag is then made once, published through LDS and read by every thread, so the one early return is uniform and every barrier
// sits in uniform control flow.  Nothing is computed from the keys in front of it.
__global__ __launch_bounds__(kSortThreads) void swd_sort_k(const float* __restrict__ XT, const float* __restrict__ YT, int m, int n, int p,
                                                           double* __restrict__ per, int* __restrict__ status) {
    extern __shared__ float swd_sh[];
    __shared__ double red[kSortThreads / 64];
    __shared__ int sh_bad;
    const int tid = threadIdx.x, T = blockDim.x, l = blockIdx.x;
    float* a = swd_sh;
    float* b = swd_sh + padded(m);
    if (tid == 0) sh_bad = 0;
    bool bad = false;
#pragma nounroll
    for (int set = 0; set < 2; ++set) {
        const float* __restrict__ src = set ? YT + (size_t)l * n : XT + (size_t)l * m;
        const int cnt = set ? n : m;
        float* S = set ? b : a;
        switch (padded(cnt)) {                 // (the same for every thread)
            case 64: sort_column<1, 0>(src, cnt, S, tid, T, bad); break;
            case 128: sort_column<2, 0>(src, cnt, S, tid, T, bad); break;
            case 256: sort_column<4, 0>(src, cnt, S, tid, T, bad); break;
            case 512: sort_column<8, 0>(src, cnt, S, tid, T, bad); break;
            case 1024: sort_column<kKeys, 0>(src, cnt, S, tid, T, bad); break;
            case 2048: sort_column<kKeys, 1>(src, cnt, S, tid, T, bad); break;
            case 4096: sort_column<kKeys, 2>(src, cnt, S, tid, T, bad); break;
            case 8192: sort_column<kKeys, 3>(src, cnt, S, tid, T, bad); break;
            default: sort_column<kKeys, 4>(src, cnt, S, tid, T, bad); break;
        }
    }
    if (bad) atomicOr(&sh_bad, 1);
    __syncthreads();
    if (sh_bad) {                              // (the same for every thread)
        if (tid == 0) {
            per[l] = __builtin_nan("");
            atomicOr(status, GGAN_SWD_NONFINITE);
        }
        return;
    }

    // ---- the integral: point i of the longer column owns [i ns, (i + 1) ns) in units of 1 / (m n), point j of the shorter [j nl, (j + 1) nl);
    // the pieces of point i are j = floor(i ns / nl) .. ceil((i + 1) ns / nl) - 1, at most two where ns <= nl.  Differences of float32 keys are
    // exact in fp64; the weights are integers below 2^28
    const bool swap = n > m;
    const float* lg = swap ? b : a;
    const float* sh = swap ? a : b;
    const int nl = swap ? n : m, ns = swap ? m : n;
    double acc = 0.0;
    for (int i = tid; i < nl; i += T) {
        const int lo = i * ns, hi = lo + ns;
        const double v = (double)lg[i];
        for (int j = lo / nl; j * nl < hi; ++j) {
            const int w = min(hi, (j + 1) * nl) - max(lo, j * nl);
            const double d = v - (double)sh[j];
            acc += (double)w * (p == 1 ? fabs(d) : d * d);
        }
    }
    // a fixed tree: the butterfly inside a wave, then the waves in wave order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < (T >> 6); ++w) t += red[w];
        per[l] = t / ((double)m * (double)n);
    }
}

// ---- mean, max, root ----------------------------------------------------------------------------------------------------------------------
// one workgroup.  The directions are staged in LDS; thread 0 adds them in index order with the rounding error of every addition carried along
// (two-sum), so the mean is the rounded exact sum whatever L is, and takes the max.  A raised status turns every output into NaN.
__global__ __launch_bounds__(256) void swd_final_k(double* __restrict__ per, int L, int p, double* __restrict__ out, const int* __restrict__ status) {
    __shared__ double sm[kMaxDirs];
    const int tid = threadIdx.x;
    const bool bad = *status != 0;             // (one word, written by the launches in front: the same for every thread)
    for (int l = tid; l < L; l += 256) {
        if (bad) per[l] = __builtin_nan("");
        else sm[l] = per[l];
    }
    __syncthreads();
    if (tid == 0) {
        if (bad) {
            out[0] = out[1] = __builtin_nan("");
            return;
        }
        double s = 0.0, c = 0.0, mx = 0.0;
        for (int l = 0; l < L; ++l) {
            const double x = sm[l], t = __dadd_rn(s, x), z = __dadd_rn(t, -s);
            c = __dadd_rn(c, __dadd_rn(__dadd_rn(s, -__dadd_rn(t, -z)), __dadd_rn(x, -z)));
            s = t;
            mx = fmax(mx, x);
        }
        const double mean = __dadd_rn(s, c) / (double)L;
        out[0] = p == 1 ? mean : sqrt(mean);
        out[1] = p == 1 ? mx : sqrt(mx);
    }
}

}  // namespace

extern "C" {

size_t ggan_swd_workspace(int m, int n, int L) {
    if (!shape_ok(m, n, L)) return 0;
    return align16((size_t)L * m * sizeof(float)) + align16((size_t)L * n * sizeof(float));
}

int ggan_swd(const float* PX, const float* PY, int m, int n, int L, int p, double* per, double* out, int32_t* status, void* ws,
             size_t ws_bytes, ggan_stream_t stream) {
    GGAN_CHECK_ARG(PX && PY && per && out && status && ws, "null pointer");
    GGAN_CHECK_ARG(m >= 1 && m <= kMaxRows && n >= 1 && n <= kMaxRows, "1 <= m, n <= 16384 rows");
    GGAN_CHECK_ARG(L >= 1 && L <= kMaxDirs, "1 <= L <= 4096 directions");
    GGAN_CHECK_ARG(p == 1 || p == 2, "p must be 1 or 2");
    GGAN_CHECK_ARG(ws_bytes >= ggan_swd_workspace(m, n, L), "workspace too small (ggan_swd_workspace)");
    GGAN_CHECK_ARG(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
    GGAN_CHECK_ARG((((uintptr_t)per | (uintptr_t)out) & 7) == 0, "per and out must be 8-byte aligned");
    // two full columns take 128 KiB of the CU's 160 KiB, above the 64 KiB default; the request is the largest this entry can make
    const int kMaxShmem = (int)sort_lds(kMaxRows, kMaxRows);
    static std::atomic<unsigned long long> once{0};
    if (first_on_device(once) &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(swd_sort_k), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShmem) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: the device refuses %d bytes of dynamic LDS", __func__, kMaxShmem);
        return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int), st) != hipSuccess) {
        set_error("%s: memset failed", __func__);
        return -2;
    }
    float* XT = (float*)ws;
    float* YT = (float*)((char*)ws + align16((size_t)L * m * sizeof(float)));
    const double bytes = 4.0 * L * ((double)m + n);
    GGAN_LAUNCH("swd_transpose", 0, 2.0 * bytes, swd_transpose_k, dim3(cdiv(L, kTile), cdiv(m > n ? m : n, kTile), 2), dim3(256), 0, st, PX, PY,
                m, n, L, XT, YT);
    const int T = sort_threads(m, n);
    GGAN_LAUNCH("swd_sort", 3.0 * L * ((double)m + n), bytes, swd_sort_k, dim3(L), dim3(T), sort_lds(m, n), st, (const float*)XT,
                (const float*)YT, m, n, p, per, (int*)status);
    GGAN_LAUNCH("swd_final", 1.0 * L, 8.0 * L, swd_final_k, dim3(1), dim3(256), 0, st, per, L, p, out, (const int*)status);
    return 0;
}

}  // extern "C"
