// The stored energies and state indices of a multistate run on the device (include/remd_hip_energy_store.h).
//
//   effective energy   one thread per iteration: the R occupied energies in ascending r, then (with weights) the R occupied log
//                      weights in ascending r and the log-sum-exp over the S states in ascending s.  One fixed order per iteration.
//   u_ln gather        a strided transposition [t][r][s] -> [s][r][j]: tiles of ES_TILE selected iterations x ES_TILE states go
//                      through the LDS, read contiguously along s and written contiguously along j.  The tile is padded to
//                      ES_TILE + 1 words of 64 bits per row: the transposed read of lane l then starts at bank 2 l of 64, no two
//                      lanes of a 32-lane half on one bank.  The two unsampled rows are a pass of their own (16 bytes per column).
//   counting           N_l and the transition counts: integers only.  Every workgroup takes ES_COUNT_CHUNK (iteration, replica)
//                      pairs; for S <= ES_HIST_MAX_S it counts them in a 32-bit LDS histogram (a cell holds at most ES_COUNT_CHUNK,
//                      see the static_assert) and adds the cells that are not zero to the 64-bit result, above that it adds every
//                      pair straight to the 64-bit result.
//   several series     the passes of timeseries.hip for K series and one origin: sums per (series, chunk of ES_SERIES_CHUNK
//                      samples), merged by one thread in the order (series, chunk); one thread walks the lags of a batch.
//
// No floating-point atomics anywhere.  Every index that can pass 2^31 is 64 bits wide.
#include "remd_internal.h"
#include "../../include/remd_hip_energy_store.h"
#include <cmath>
#include <limits>

#define ES_BLOCK          256
#define ES_TILE           32
#define ES_TILE_ROWS      8                       // blockDim.y of the gather: a thread moves ES_TILE / ES_TILE_ROWS words each way
#define ES_COUNT_CHUNK    8192                    // (iteration, replica) pairs per workgroup of the counting passes
#define ES_HIST_MAX_S     64                      // the LDS histogram of the transition counts has S x S cells: 16 KiB at 64
#define ES_SERIES_CHUNK   2048                    // samples per workgroup of the series passes: 8 per thread
#define ES_FIRST_BATCH    8
#define ES_PARTIAL_CAP    (int64_t(1) << 22)      // doubles of per-chunk partials at most (32 MiB)

static_assert((uint64_t)ES_COUNT_CHUNK < (uint64_t(1) << 32), "a 32-bit LDS counter must hold every pair of a workgroup's chunk");
static_assert(ES_HIST_MAX_S * ES_HIST_MAX_S * sizeof(uint32_t) <= 64 * 1024, "the LDS histogram must fit a workgroup's LDS");

typedef unsigned long long es_u64;

// ---- effective energy ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ES_BLOCK) void es_effective_kernel(const double* __restrict__ energies, const int32_t* __restrict__ states,
                                                                const double* __restrict__ log_weights, const double* __restrict__ f_l,
                                                                int64_t T, int R, int S, double* __restrict__ u_n)
{
    const int64_t t = (int64_t)blockIdx.x * ES_BLOCK + threadIdx.x;
    if (t >= T) return;
    const int32_t* st = states + t * R;
    const double* e = energies + t * R * (int64_t)S;
    double u = 0.0;
    for (int r = 0; r < R; r++) u += e[(int64_t)r * S + st[r]];
    if (log_weights) {
        const double* lw = log_weights + t * S;
        double w = 0.0;
        for (int r = 0; r < R; r++) w += lw[st[r]];
        double m = -std::numeric_limits<double>::infinity();
        for (int s = 0; s < S; s++) m = fmax(m, -f_l[s] + lw[s]);
        if (!isfinite(m)) m = 0.0;
        double sum = 0.0;
        for (int s = 0; s < S; s++) sum += exp((-f_l[s] + lw[s]) - m);
        u = u + (-w + (log(sum) + m));
    }
    u_n[t] = u;
}

// ---- u_ln gather -----------------------------------------------------------------------------------------------------------------
// grid: (tiles of j) x (tiles of s) x R, flattened into x; block (ES_TILE, ES_TILE_ROWS)
__global__ __launch_bounds__(ES_TILE * ES_TILE_ROWS) void es_gather_kernel(const es_u64* __restrict__ energies, const int64_t* __restrict__ iterations,
                                                                          int64_t n_sel, int R, int S, int first, es_u64* __restrict__ u_ln)
{
    __shared__ es_u64 tile[ES_TILE][ES_TILE + 1];
    const int64_t j_tiles = (n_sel + ES_TILE - 1) / ES_TILE;
    const int s_tiles = (S + ES_TILE - 1) / ES_TILE;
    int64_t b = blockIdx.x;
    const int64_t j0 = (b % j_tiles) * ES_TILE; b /= j_tiles;
    const int s0 = (int)(b % s_tiles) * ES_TILE;
    const int r = (int)(b / s_tiles);
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int jj = ty; jj < ES_TILE; jj += ES_TILE_ROWS) {
        const int64_t j = j0 + jj;
        const int s = s0 + tx;
        if (j < n_sel && s < S) tile[jj][tx] = energies[(iterations[j] * R + r) * (int64_t)S + s];
    }
    __syncthreads();
    const int64_t cols = (int64_t)R * n_sel;
    for (int ss = ty; ss < ES_TILE; ss += ES_TILE_ROWS) {
        const int s = s0 + ss;
        const int64_t j = j0 + tx;
        if (s < S && j < n_sel) u_ln[(int64_t)(first + s) * cols + (int64_t)r * n_sel + j] = tile[tx][ss];
    }
}

// one thread per column: the two unsampled rows
__global__ __launch_bounds__(ES_BLOCK) void es_gather_unsampled_kernel(const es_u64* __restrict__ unsampled, const int64_t* __restrict__ iterations,
                                                                       int64_t n_sel, int R, int S, es_u64* __restrict__ u_ln)
{
    const int64_t cols = (int64_t)R * n_sel;
    const int64_t c = (int64_t)blockIdx.x * ES_BLOCK + threadIdx.x;
    if (c >= cols) return;
    const int64_t r = c / n_sel, j = c % n_sel;
    const es_u64* u = unsampled + (iterations[j] * R + r) * 2;
    u_ln[c] = u[0];
    u_ln[(int64_t)(S + 1) * cols + c] = u[1];
}

// ---- counting --------------------------------------------------------------------------------------------------------------------
// the cells of a workgroup's histogram that are not zero, added to the 64-bit result
__device__ __forceinline__ void es_flush(const uint32_t* hist, int cells, es_u64* __restrict__ out)
{
    __syncthreads();
    for (int c = threadIdx.x; c < cells; c += ES_BLOCK)
        if (hist[c]) atomicAdd(&out[c], (es_u64)hist[c]);
}

// pair p of [0, n_sel * R) is (selection p / R, replica p % R)
template <int HIST>
__global__ __launch_bounds__(ES_BLOCK) void es_state_count_kernel(const int32_t* __restrict__ states, const int64_t* __restrict__ iterations,
                                                                  int64_t n_pairs, int R, int S, es_u64* __restrict__ N_s)
{
    __shared__ uint32_t hist[HIST ? ES_HIST_MAX_S : 1];
    if (HIST) {
        for (int c = threadIdx.x; c < S; c += ES_BLOCK) hist[c] = 0;
        __syncthreads();
    }
    const int64_t p0 = (int64_t)blockIdx.x * ES_COUNT_CHUNK;
    const int64_t hi = p0 + ES_COUNT_CHUNK < n_pairs ? p0 + ES_COUNT_CHUNK : n_pairs;
    for (int64_t p = p0 + threadIdx.x; p < hi; p += ES_BLOCK) {
        const int s = states[iterations[p / R] * R + p % R];
        if (HIST) atomicAdd(&hist[s], 1u); else atomicAdd(&N_s[s], (es_u64)1);
    }
    if (HIST) es_flush(hist, S, N_s);
}

// pair p of [0, n_pairs) is (iteration t_begin + p / R, replica p % R): `from` points at states[t_begin][0], the next iteration is R on
template <int HIST>
__global__ __launch_bounds__(ES_BLOCK) void es_transition_kernel(const int32_t* __restrict__ from, int64_t n_pairs, int R, int S,
                                                                 es_u64* __restrict__ n_ij)
{
    __shared__ uint32_t hist[HIST ? ES_HIST_MAX_S * ES_HIST_MAX_S : 1];
    if (HIST) {
        for (int c = threadIdx.x; c < S * S; c += ES_BLOCK) hist[c] = 0;
        __syncthreads();
    }
    const int64_t p0 = (int64_t)blockIdx.x * ES_COUNT_CHUNK;
    const int64_t hi = p0 + ES_COUNT_CHUNK < n_pairs ? p0 + ES_COUNT_CHUNK : n_pairs;
    for (int64_t p = p0 + threadIdx.x; p < hi; p += ES_BLOCK) {
        const int64_t cell = (int64_t)from[p] * S + from[p + R];
        if (HIST) atomicAdd(&hist[cell], 1u); else atomicAdd(&n_ij[cell], (es_u64)1);
    }
    if (HIST) es_flush(hist, S * S, n_ij);
}

// ---- several series --------------------------------------------------------------------------------------------------------------
// lanes by __shfl_down, then the four waves in wave order: one fixed order (as ts_block_sum of timeseries.hip)
__device__ __forceinline__ double es_block_sum(double v, double* sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ int64_t es_lag(int64_t t0, int64_t inc0, int fast, int b)
{
    return fast ? t0 + (int64_t)b * inc0 + (int64_t)b * (b - 1) / 2 : t0 + b;
}
__device__ __forceinline__ int64_t es_increment(int64_t inc0, int fast, int b) { return fast ? inc0 + b : 1; }

struct es_walk { double mu, sigma2, g; int64_t last; int done, status; };

// grid (chunks, K): partial[k * chunks + c] = sum over chunk c of series k of A (SQUARED = 0) or (A - mu)^2 (SQUARED = 1)
template <int SQUARED>
__global__ __launch_bounds__(ES_BLOCK) void es_series_moment_kernel(const double* __restrict__ A, int64_t N, const es_walk* __restrict__ w,
                                                                    double* __restrict__ partial)
{
    __shared__ double sh[4];
    const int64_t n0 = (int64_t)blockIdx.x * ES_SERIES_CHUNK;
    const int64_t hi = n0 + ES_SERIES_CHUNK < N ? n0 + ES_SERIES_CHUNK : N;
    const double* a = A + (int64_t)blockIdx.y * N;
    const double m = SQUARED ? w->mu : 0.0;
    double acc = 0.0;
    for (int64_t n = n0 + threadIdx.x; n < hi; n += ES_BLOCK) {
        const double d = a[n] - m;
        acc += SQUARED ? d * d : d;
    }
    const double t = es_block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// one thread: the K * chunks partials in the order (series, chunk)
template <int SQUARED>
__global__ void es_series_moment_merge_kernel(const double* __restrict__ partial, int64_t n_partial, double count, es_walk* __restrict__ w)
{
    double sum = 0.0;
    for (int64_t i = 0; i < n_partial; i++) sum += partial[i];
    const double v = sum / count;
    if (!SQUARED) {
        w->mu = v; w->g = 1.0; w->last = 0; w->done = 0; w->status = 0;
    } else {
        w->sigma2 = v;
        if (v == 0.0) { w->g = std::numeric_limits<double>::quiet_NaN(); w->done = 1; w->status = 1; }
    }
}

struct es_batch {
    const double* A; int64_t N; int K; int64_t chunks;                   // chunks of a whole series
    int64_t t0, inc0; int fast, B, mintime;
    double* partial;                                                     // [B][K][chunks]
    double* lagsum;                                                      // [B]
    es_walk* w;
};

// grid (chunks, B, K)
__global__ __launch_bounds__(ES_BLOCK) void es_series_lag_kernel(es_batch a)
{
    __shared__ double sh[4];
    const int64_t t = es_lag(a.t0, a.inc0, a.fast, blockIdx.y);
    if (t >= a.N - 1) return;                                            // the walk stops before this lag
    const int64_t end = a.N - t;                                         // n + t < N for every n below it
    const int64_t n0 = (int64_t)blockIdx.x * ES_SERIES_CHUNK;
    if (n0 >= end) return;
    const int64_t hi = n0 + ES_SERIES_CHUNK < end ? n0 + ES_SERIES_CHUNK : end;
    const double* s = a.A + (int64_t)blockIdx.z * a.N;
    const double m = a.w->mu;
    double acc = 0.0;
    for (int64_t n = n0 + threadIdx.x; n < hi; n += ES_BLOCK) acc += (s[n] - m) * (s[n + t] - m);
    const double v = es_block_sum(acc, sh);
    if (threadIdx.x == 0) a.partial[((int64_t)blockIdx.y * a.K + blockIdx.z) * a.chunks + blockIdx.x] = v;
}

// one thread per lag of the batch: the series in order, of each the chunks [0, (N - t - 1) / chunk] in order
__global__ __launch_bounds__(64) void es_series_lag_merge_kernel(es_batch a)
{
    const int b = threadIdx.x;
    if (b >= a.B) return;
    const int64_t t = es_lag(a.t0, a.inc0, a.fast, b);
    double sum = 0.0;
    if (t < a.N - 1) {
        const int64_t chunks = (a.N - t - 1) / ES_SERIES_CHUNK + 1;
        for (int k = 0; k < a.K; k++)
            for (int64_t c = 0; c < chunks; c++) sum += a.partial[((int64_t)b * a.K + k) * a.chunks + c];
    }
    a.lagsum[b] = sum;
}

// one thread: the loop of analysis.statistical_inefficiency_multiple over the lags of this batch
__global__ void es_series_walk_kernel(es_batch a)
{
    es_walk w = *a.w;
    int done = 0;
    for (int b = 0; b < a.B; b++) {
        const int64_t t = es_lag(a.t0, a.inc0, a.fast, b);
        if (t >= a.N - 1) { done = 1; break; }
        const double C = a.lagsum[b] / ((double)a.K * (double)(a.N - t) * w.sigma2);
        if (C <= 0.0 && t > a.mintime) { done = 1; break; }
        w.g += 2.0 * C * (1.0 - (double)t / (double)a.N) * (double)es_increment(a.inc0, a.fast, b);
        w.last = t;
    }
    w.done = done;
    *a.w = w;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#define ES_CHECK(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return remd_hip_fail(nullptr, #expr, _e); } while (0)

// a stream and the two events that time the launches on it
struct es_timer {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ms = 0.0;
    int open(int dev)
    {
        device = dev;
        ES_CHECK(hipStreamCreate(&stream));
        ES_CHECK(hipEventCreate(&ev0));
        ES_CHECK(hipEventCreate(&ev1));
        return 0;
    }
    int begin() { ES_CHECK(hipEventRecord(ev0, stream)); return 0; }
    // waits for the launches since begin() and adds their time to ms
    int end()
    {
        ES_CHECK(hipGetLastError());
        ES_CHECK(hipEventRecord(ev1, stream));
        ES_CHECK(hipStreamSynchronize(stream));
        float t = 0.0f;
        ES_CHECK(hipEventElapsedTime(&t, ev0, ev1));
        ms += t;
        return 0;
    }
    ~es_timer()
    {
        hipSetDevice(device);
        if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); }
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
    }
};

struct remd_energy_store_ctx {
    int64_t T = 0;
    int R = 0, S = 0, U = 0;
    bool timed = false;
    es_timer tm;
    dev_array<double> energies, unsampled, log_weights, f_l, u_n, u_ln;
    dev_array<int32_t> states;
    dev_array<int64_t> iterations;
    dev_array<es_u64> counts;
};

static int es_device(const char* who, int device)
{
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return remd_fail(nullptr, -2, std::string(who) + ": no HIP device available (" + hipGetErrorString(e) + ")");
    if (device < 0 || device >= n) return remd_fail(nullptr, -1, std::string(who) + ": bad device index");
    ES_CHECK(hipSetDevice(device));
    return 0;
}

static int es_series(int device, int32_t K, int64_t N, const double* A_kn, int fast, int mintime, int32_t first_batch, double* g,
                     int32_t* status, int64_t* last_lag, double* ms, int64_t* chunk)
{
    const char* who = "remd_series_inefficiency_multiple";
    if (K < 1) return remd_fail(nullptr, -1, std::string(who) + ": K must be at least 1");
    if (K > 65535) return remd_fail(nullptr, -1, std::string(who) + ": K must be at most 65535");
    if (N < 2) return remd_fail(nullptr, -1, std::string(who) + ": N must be at least 2");
    if (mintime < 0) return remd_fail(nullptr, -1, std::string(who) + ": mintime must not be negative");
    if (first_batch < 1 || first_batch > REMD_SERIES_MAX_BATCH)
        return remd_fail(nullptr, -1, std::string(who) + ": first_batch must be 1 ... " + std::to_string(REMD_SERIES_MAX_BATCH));
    if (!A_kn || !g || !status) return remd_fail(nullptr, -1, std::string(who) + ": A_kn, g or status is NULL");
    const int64_t total = (int64_t)K * N;
    for (int64_t i = 0; i < total; i++)
        if (!std::isfinite(A_kn[i]))
            return remd_fail(nullptr, -1, std::string(who) + ": non-finite sample " + std::to_string(i % N) + " of series " + std::to_string(i / N));
    REMD_TRY(es_device(who, device));
    es_timer tm;
    REMD_TRY(tm.open(device));
    const int64_t chunks = (N - 1) / ES_SERIES_CHUNK + 1;
    const int64_t per_lag = (int64_t)K * chunks;
    dev_array<double> A, partial, lagsum;
    dev_array<es_walk> walk;
    REMD_TRY(A.alloc(nullptr, (size_t)total));
    REMD_TRY(partial.alloc(nullptr, (size_t)std::max<int64_t>(ES_PARTIAL_CAP, per_lag)));
    REMD_TRY(lagsum.alloc(nullptr, REMD_SERIES_MAX_BATCH));
    REMD_TRY(walk.alloc(nullptr, 1));
    ES_CHECK(hipMemcpy(A, A_kn, sizeof(double) * (size_t)total, hipMemcpyHostToDevice));

    const dim3 mgrid((unsigned)chunks, (unsigned)K);
    REMD_TRY(tm.begin());
    hipLaunchKernelGGL(es_series_moment_kernel<0>, mgrid, dim3(ES_BLOCK), 0, tm.stream, A.get(), N, walk.get(), partial.get());
    hipLaunchKernelGGL(es_series_moment_merge_kernel<0>, dim3(1), dim3(1), 0, tm.stream, partial.get(), per_lag, (double)total, walk.get());
    hipLaunchKernelGGL(es_series_moment_kernel<1>, mgrid, dim3(ES_BLOCK), 0, tm.stream, A.get(), N, walk.get(), partial.get());
    hipLaunchKernelGGL(es_series_moment_merge_kernel<1>, dim3(1), dim3(1), 0, tm.stream, partial.get(), per_lag, (double)total, walk.get());
    REMD_TRY(tm.end());

    es_walk w;
    ES_CHECK(hipMemcpy(&w, walk, sizeof(es_walk), hipMemcpyDeviceToHost));
    int64_t t0 = 1, inc0 = 1;
    int ramp = first_batch;
    while (!w.done && t0 < N - 1) {
        const int B = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(ramp, REMD_SERIES_MAX_BATCH), ES_PARTIAL_CAP / per_lag));
        es_batch a;
        a.A = A; a.N = N; a.K = K; a.chunks = chunks; a.t0 = t0; a.inc0 = inc0; a.fast = fast; a.B = B; a.mintime = mintime;
        a.partial = partial; a.lagsum = lagsum; a.w = walk;
        const int64_t lag_chunks = (N - t0 - 1) / ES_SERIES_CHUNK + 1;                 // of the batch's first lag, the most
        REMD_TRY(tm.begin());
        hipLaunchKernelGGL(es_series_lag_kernel, dim3((unsigned)lag_chunks, (unsigned)B, (unsigned)K), dim3(ES_BLOCK), 0, tm.stream, a);
        hipLaunchKernelGGL(es_series_lag_merge_kernel, dim3(1), dim3(64), 0, tm.stream, a);
        hipLaunchKernelGGL(es_series_walk_kernel, dim3(1), dim3(1), 0, tm.stream, a);
        REMD_TRY(tm.end());
        ES_CHECK(hipMemcpy(&w, walk, sizeof(es_walk), hipMemcpyDeviceToHost));          // the one read-back of a batch
        for (int b = 0; b < B; b++) { t0 += inc0; if (fast) inc0++; }
        ramp = std::min(2 * ramp, REMD_SERIES_MAX_BATCH);
    }
    *status = w.status;
    *g = w.status ? w.g : std::max(w.g, 1.0);
    if (last_lag) *last_lag = w.last;
    if (ms) *ms = tm.ms;
    if (chunk) *chunk = ES_SERIES_CHUNK;
    return 0;
}

extern "C" {

int remd_energy_store_create(int device, int64_t T, int32_t R, int32_t S, int32_t U, const double* energies, const double* unsampled,
                             const int32_t* states, remd_energy_store* out)
{
    const char* who = "remd_energy_store_create";
    if (!out) return remd_fail(nullptr, -1, std::string(who) + ": out is NULL");
    *out = nullptr;
    if (T < 1) return remd_fail(nullptr, -1, std::string(who) + ": T must be at least 1");
    if (R < 1) return remd_fail(nullptr, -1, std::string(who) + ": R must be at least 1");
    if (S < 1) return remd_fail(nullptr, -1, std::string(who) + ": S must be at least 1");
    if (U != 0 && U != 2) return remd_fail(nullptr, -1, std::string(who) + ": U must be 0 or 2");
    if (!energies || !states || (U && !unsampled)) return remd_fail(nullptr, -1, std::string(who) + ": energies, states or unsampled is NULL");
    const int64_t pairs = T * R;
    for (int64_t p = 0; p < pairs; p++)
        if (states[p] < 0 || states[p] >= S)
            return remd_fail(nullptr, -1, std::string(who) + ": states[" + std::to_string(p / R) + "][" + std::to_string(p % R) + "] = " +
                                          std::to_string(states[p]) + " is outside 0 ... S - 1 = " + std::to_string(S - 1));
    REMD_TRY(es_device(who, device));
    std::unique_ptr<remd_energy_store_ctx> st(new remd_energy_store_ctx());
    st->T = T; st->R = R; st->S = S; st->U = U;
    REMD_TRY(st->tm.open(device));
    REMD_TRY(st->energies.alloc(nullptr, (size_t)pairs * S));
    REMD_TRY(st->states.alloc(nullptr, (size_t)pairs));
    ES_CHECK(hipMemcpy(st->energies, energies, sizeof(double) * (size_t)pairs * S, hipMemcpyHostToDevice));
    ES_CHECK(hipMemcpy(st->states, states, sizeof(int32_t) * (size_t)pairs, hipMemcpyHostToDevice));
    if (U) {
        REMD_TRY(st->unsampled.alloc(nullptr, (size_t)pairs * U));
        ES_CHECK(hipMemcpy(st->unsampled, unsampled, sizeof(double) * (size_t)pairs * U, hipMemcpyHostToDevice));
    }
    *out = st.release();
    return 0;
}

void remd_energy_store_destroy(remd_energy_store store) { delete store; }

int remd_energy_store_effective_energy(remd_energy_store st, const double* log_weights, const double* f_l, double* u_n)
{
    const char* who = "remd_energy_store_effective_energy";
    if (!st) return remd_fail(nullptr, -1, std::string(who) + ": the store is NULL");
    if (!u_n) return remd_fail(nullptr, -1, std::string(who) + ": u_n is NULL");
    if ((log_weights == nullptr) != (f_l == nullptr))
        return remd_fail(nullptr, -1, std::string(who) + ": log_weights and f_l go together: pass both or neither");
    ES_CHECK(hipSetDevice(st->tm.device));
    const int64_t T = st->T;
    REMD_TRY(st->u_n.grow(nullptr, (size_t)T));
    if (log_weights) {
        REMD_TRY(st->log_weights.grow(nullptr, (size_t)T * st->S));
        REMD_TRY(st->f_l.grow(nullptr, (size_t)st->S));
        ES_CHECK(hipMemcpy(st->log_weights, log_weights, sizeof(double) * (size_t)T * st->S, hipMemcpyHostToDevice));
        ES_CHECK(hipMemcpy(st->f_l, f_l, sizeof(double) * (size_t)st->S, hipMemcpyHostToDevice));
    }
    st->tm.ms = 0.0; st->timed = false;
    REMD_TRY(st->tm.begin());
    hipLaunchKernelGGL(es_effective_kernel, dim3((unsigned)((T + ES_BLOCK - 1) / ES_BLOCK)), dim3(ES_BLOCK), 0, st->tm.stream, st->energies.get(),
                       st->states.get(), log_weights ? st->log_weights.get() : nullptr, log_weights ? st->f_l.get() : nullptr, T, st->R, st->S,
                       st->u_n.get());
    REMD_TRY(st->tm.end());
    st->timed = true;
    ES_CHECK(hipMemcpy(u_n, st->u_n, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost));
    return 0;
}

int remd_energy_store_gather_u_ln(remd_energy_store st, int64_t n_sel, const int64_t* iterations, double* u_ln, int64_t* N_l)
{
    const char* who = "remd_energy_store_gather_u_ln";
    if (!st) return remd_fail(nullptr, -1, std::string(who) + ": the store is NULL");
    if (n_sel < 0) return remd_fail(nullptr, -1, std::string(who) + ": n_sel must not be negative");
    if (!N_l || (n_sel > 0 && (!iterations || !u_ln))) return remd_fail(nullptr, -1, std::string(who) + ": iterations, u_ln or N_l is NULL");
    for (int64_t j = 0; j < n_sel; j++)
        if (iterations[j] < 0 || iterations[j] >= st->T)
            return remd_fail(nullptr, -1, std::string(who) + ": iterations[" + std::to_string(j) + "] = " + std::to_string(iterations[j]) +
                                          " is outside 0 ... T - 1 = " + std::to_string(st->T - 1));
    const int R = st->R, S = st->S, first = st->U / 2, rows = S + st->U;
    for (int l = 0; l < rows; l++) N_l[l] = 0;
    if (n_sel == 0) return 0;
    const int64_t cols = (int64_t)R * n_sel;
    const int64_t tiles = ((n_sel + ES_TILE - 1) / ES_TILE) * ((S + ES_TILE - 1) / ES_TILE) * R;
    const int64_t count_groups = (cols + ES_COUNT_CHUNK - 1) / ES_COUNT_CHUNK;
    if (tiles > 0x7fffffff || (cols + ES_BLOCK - 1) / ES_BLOCK > 0x7fffffff)
        return remd_fail(nullptr, -1, std::string(who) + ": the selection is too large for one launch");
    ES_CHECK(hipSetDevice(st->tm.device));
    REMD_TRY(st->iterations.grow(nullptr, (size_t)n_sel));
    REMD_TRY(st->u_ln.grow(nullptr, (size_t)rows * cols));
    REMD_TRY(st->counts.grow(nullptr, (size_t)S * S));
    ES_CHECK(hipMemcpy(st->iterations, iterations, sizeof(int64_t) * (size_t)n_sel, hipMemcpyHostToDevice));
    ES_CHECK(hipMemsetAsync(st->counts, 0, sizeof(es_u64) * (size_t)S, st->tm.stream));
    st->tm.ms = 0.0; st->timed = false;
    REMD_TRY(st->tm.begin());
    hipLaunchKernelGGL(es_gather_kernel, dim3((unsigned)tiles), dim3(ES_TILE, ES_TILE_ROWS), 0, st->tm.stream, (const es_u64*)st->energies.get(),
                       st->iterations.get(), n_sel, R, S, first, (es_u64*)st->u_ln.get());
    if (st->U)
        hipLaunchKernelGGL(es_gather_unsampled_kernel, dim3((unsigned)((cols + ES_BLOCK - 1) / ES_BLOCK)), dim3(ES_BLOCK), 0, st->tm.stream,
                           (const es_u64*)st->unsampled.get(), st->iterations.get(), n_sel, R, S, (es_u64*)st->u_ln.get());
    if (S <= ES_HIST_MAX_S)
        hipLaunchKernelGGL(es_state_count_kernel<1>, dim3((unsigned)count_groups), dim3(ES_BLOCK), 0, st->tm.stream, st->states.get(),
                           st->iterations.get(), cols, R, S, st->counts.get());
    else
        hipLaunchKernelGGL(es_state_count_kernel<0>, dim3((unsigned)count_groups), dim3(ES_BLOCK), 0, st->tm.stream, st->states.get(),
                           st->iterations.get(), cols, R, S, st->counts.get());
    REMD_TRY(st->tm.end());
    st->timed = true;
    ES_CHECK(hipMemcpy(u_ln, st->u_ln, sizeof(double) * (size_t)rows * cols, hipMemcpyDeviceToHost));
    static_assert(sizeof(es_u64) == sizeof(int64_t), "the counters are read back as int64_t");
    ES_CHECK(hipMemcpy(N_l + first, st->counts, sizeof(int64_t) * (size_t)S, hipMemcpyDeviceToHost));
    return 0;
}

int remd_energy_store_transition_counts(remd_energy_store st, int64_t t_begin, int64_t t_end, int64_t* n_ij)
{
    const char* who = "remd_energy_store_transition_counts";
    if (!st) return remd_fail(nullptr, -1, std::string(who) + ": the store is NULL");
    if (!n_ij) return remd_fail(nullptr, -1, std::string(who) + ": n_ij is NULL");
    if (t_begin < 0 || t_end > st->T || t_begin > t_end)
        return remd_fail(nullptr, -1, std::string(who) + ": the range [" + std::to_string(t_begin) + ", " + std::to_string(t_end) +
                                      ") is outside 0 ... T = " + std::to_string(st->T));
    const int R = st->R, S = st->S;
    const size_t cells = (size_t)S * S;
    if (t_end - t_begin < 2) {
        for (size_t c = 0; c < cells; c++) n_ij[c] = 0;
        return 0;
    }
    const int64_t n_pairs = (t_end - 1 - t_begin) * R;
    const int64_t groups = (n_pairs + ES_COUNT_CHUNK - 1) / ES_COUNT_CHUNK;
    if (groups > 0x7fffffff) return remd_fail(nullptr, -1, std::string(who) + ": the range is too large for one launch");
    ES_CHECK(hipSetDevice(st->tm.device));
    REMD_TRY(st->counts.grow(nullptr, cells));
    ES_CHECK(hipMemsetAsync(st->counts, 0, sizeof(es_u64) * cells, st->tm.stream));
    st->tm.ms = 0.0; st->timed = false;
    REMD_TRY(st->tm.begin());
    const int32_t* from = st->states.get() + t_begin * R;
    if (S <= ES_HIST_MAX_S)
        hipLaunchKernelGGL(es_transition_kernel<1>, dim3((unsigned)groups), dim3(ES_BLOCK), 0, st->tm.stream, from, n_pairs, R, S, st->counts.get());
    else
        hipLaunchKernelGGL(es_transition_kernel<0>, dim3((unsigned)groups), dim3(ES_BLOCK), 0, st->tm.stream, from, n_pairs, R, S, st->counts.get());
    REMD_TRY(st->tm.end());
    st->timed = true;
    ES_CHECK(hipMemcpy(n_ij, st->counts, sizeof(int64_t) * cells, hipMemcpyDeviceToHost));
    return 0;
}

int remd_energy_store_chunks(remd_energy_store st, int64_t* effective_chunk, int64_t* gather_tile, int64_t* count_chunk, int32_t* hist_max_states)
{
    if (!st || !effective_chunk || !gather_tile || !count_chunk || !hist_max_states)
        return remd_fail(nullptr, -1, "remd_energy_store_chunks: the store or an output is NULL");
    *effective_chunk = ES_BLOCK; *gather_tile = ES_TILE; *count_chunk = ES_COUNT_CHUNK; *hist_max_states = ES_HIST_MAX_S;
    return 0;
}

int remd_energy_store_last_ms(remd_energy_store st, double* ms)
{
    if (!st || !ms) return remd_fail(nullptr, -1, "remd_energy_store_last_ms: the store or ms is NULL");
    if (!st->timed) return remd_fail(nullptr, -1, "remd_energy_store_last_ms: no pass has run on this store yet");
    *ms = st->tm.ms;
    return 0;
}

int remd_series_inefficiency_multiple(int device, int32_t K, int64_t N, const double* A_kn, int fast, int mintime, double* g,
                                      int32_t* status, int64_t* last_lag)
{
    return es_series(device, K, N, A_kn, fast ? 1 : 0, mintime, ES_FIRST_BATCH, g, status, last_lag, nullptr, nullptr);
}

int remd_series_inefficiency_multiple_batched(int device, int32_t K, int64_t N, const double* A_kn, int fast, int mintime,
                                              int32_t first_batch, double* g, int32_t* status, int64_t* last_lag, double* ms, int64_t* chunk)
{
    return es_series(device, K, N, A_kn, fast ? 1 : 0, mintime, first_batch, g, status, last_lag, ms, chunk);
}

}
