// The statistical inefficiency of the suffixes of a timeseries on the device (include/remd_hip_timeseries.h).  All f64.
//
//   moments      workgroups per (origin, chunk of samples): sum A over the suffix, merged per origin in chunk order -> mean; then the
//                same for sum (A - mean)^2 -> sigma2.  Two passes, as the host takes them.
//   lag batch    workgroups per (origin, lag of the batch, chunk of n): sum (A[n] - mean)(A[n + t] - mean) over the chunk; one thread
//                per (origin, lag) merges the chunks in chunk order; one thread per origin walks the lags of the batch in order,
//                applies the stopping rule and carries (g, done, last lag) to the next batch
//
// Chunk c is the samples [c * TS_CHUNK, (c + 1) * TS_CHUNK) whatever the origin and the lag, clipped to the range a sum runs over,
// and thread i of a workgroup always takes the samples c * TS_CHUNK + i, + 256, ...: a sum has one fixed order, set by (A, origin,
// lag) alone.  No floating-point atomics.
//
// Until it stops, every origin visits the same lags (1, 2, 3, ... or 1, 2, 4, 7, ...), so the lag and the increment a batch starts
// at are the host's, one pair for all origins, and a batch is (first lag, first increment, number of lags).
#include "remd_internal.h"
#include "../../include/remd_hip_timeseries.h"
#include <cmath>
#include <limits>

#define TS_BLOCK        256
#define TS_CHUNK        2048                    // samples per workgroup: 8 per thread
#define TS_FIRST_BATCH  8                       // lags of the first batch; doubled per batch up to REMD_TIMESERIES_MAX_BATCH
#define TS_PARTIAL_CAP  (int64_t(1) << 22)      // doubles of per-chunk partials at most (32 MiB)
#define TS_GROUP_MAX    32768                   // origins of one pass over the series at most (a grid dimension)

// lanes by __shfl_down, then the four waves in wave order: one fixed order; every thread gets the result
__device__ __forceinline__ double ts_block_sum(double v, double* sh)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// lag b of a batch that starts at lag t0 with increment inc0, and the increment that goes with it
__device__ __forceinline__ int64_t ts_lag(int64_t t0, int64_t inc0, int fast, int b)
{
    return fast ? t0 + (int64_t)b * inc0 + (int64_t)b * (b - 1) / 2 : t0 + b;
}
__device__ __forceinline__ int64_t ts_increment(int64_t inc0, int fast, int b) { return fast ? inc0 + b : 1; }

// ---- moments --------------------------------------------------------------------------------------------------------------------
// grid (chunks from the origin's own first chunk on, origins): partial[x * S + s] = sum over chunk ∩ [t_s, N) of A (SQUARED = 0) or
// of (A - mean_s)^2 (SQUARED = 1)
template <int SQUARED>
__global__ __launch_bounds__(TS_BLOCK) void ts_moment_kernel(const double* __restrict__ A, int64_t N, const int64_t* __restrict__ origin,
                                                             const double* __restrict__ mean, double* __restrict__ partial)
{
    __shared__ double sh[4];
    const int s = blockIdx.y;
    const int64_t ts = origin[s];
    const int64_t n0 = (ts / TS_CHUNK + blockIdx.x) * TS_CHUNK;
    if (n0 >= N) return;                                                 // (the whole workgroup: this origin has fewer chunks)
    const int64_t hi = n0 + TS_CHUNK < N ? n0 + TS_CHUNK : N;
    const double m = SQUARED ? mean[s] : 0.0;
    double acc = 0.0;
    for (int64_t n = n0 + threadIdx.x; n < hi; n += TS_BLOCK)
        if (n >= ts) {
            const double d = A[n] - m;
            acc += SQUARED ? d * d : d;
        }
    const double t = ts_block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * gridDim.y + s] = t;
}

// one thread per origin adds its chunks in chunk order.  SQUARED = 0: the mean, and the walk's state at its start; SQUARED = 1: sigma2,
// and a suffix without variance is marked and done
template <int SQUARED>
__global__ void ts_moment_merge_kernel(const double* __restrict__ partial, int64_t N, const int64_t* __restrict__ origin, int S,
                                       double* __restrict__ mean, double* __restrict__ sigma2, double* __restrict__ g,
                                       int* __restrict__ done, int* __restrict__ status, int64_t* __restrict__ last_lag)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int64_t ts = origin[s];
    const int64_t chunks = (N - 1) / TS_CHUNK - ts / TS_CHUNK + 1;
    double sum = 0.0;
    for (int64_t k = 0; k < chunks; k++) sum += partial[k * S + s];
    const double v = sum / (double)(N - ts);
    if (!SQUARED) {
        mean[s] = v; g[s] = 1.0; done[s] = 0; status[s] = 0; last_lag[s] = 0;
    } else {
        sigma2[s] = v;
        if (v == 0.0) { g[s] = std::numeric_limits<double>::quiet_NaN(); done[s] = 1; status[s] = 1; }
    }
}

// ---- lag batches ----------------------------------------------------------------------------------------------------------------
struct ts_batch {
    const double* A; int64_t N;
    const int64_t* origin; const double* mean; const double* sigma2;      // per origin of the group
    const int* active; int n_active;                                     // the origins that have not stopped
    int64_t t0, inc0; int fast, B, mintime;
    double* partial;                                                     // [chunk from the origin's first][active][B]
    double* lagsum;                                                      // [active][B]
    double* g; int* done; int64_t* last_lag;
};

// grid (chunks, B, active)
__global__ __launch_bounds__(TS_BLOCK) void ts_lag_kernel(ts_batch a)
{
    __shared__ double sh[4];
    const int s = a.active[blockIdx.z];
    const int64_t ts = a.origin[s];
    const int64_t t = ts_lag(a.t0, a.inc0, a.fast, blockIdx.y);
    if (t >= a.N - ts - 1) return;                                       // the walk stops before this lag
    const int64_t end = a.N - t;                                         // n + t < N for every n below it
    const int64_t n0 = (ts / TS_CHUNK + blockIdx.x) * TS_CHUNK;
    if (n0 >= end) return;
    const int64_t hi = n0 + TS_CHUNK < end ? n0 + TS_CHUNK : end;
    const double m = a.mean[s];
    double acc = 0.0;
    for (int64_t n = n0 + threadIdx.x; n < hi; n += TS_BLOCK)
        if (n >= ts) acc += (a.A[n] - m) * (a.A[n + t] - m);
    const double v = ts_block_sum(acc, sh);
    if (threadIdx.x == 0) a.partial[((int64_t)blockIdx.x * a.n_active + blockIdx.z) * a.B + blockIdx.y] = v;
}

// one thread per (active origin, lag): the chunks [t_s / chunk, (N - t - 1) / chunk] in order, each of which the lag kernel wrote
__global__ __launch_bounds__(TS_BLOCK) void ts_lag_merge_kernel(ts_batch a)
{
    const int64_t idx = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x;
    if (idx >= (int64_t)a.n_active * a.B) return;
    const int s = a.active[idx / a.B];
    const int64_t ts = a.origin[s];
    const int64_t t = ts_lag(a.t0, a.inc0, a.fast, (int)(idx % a.B));
    double sum = 0.0;
    if (t < a.N - ts - 1) {
        const int64_t chunks = (a.N - t - 1) / TS_CHUNK - ts / TS_CHUNK + 1;
        for (int64_t k = 0; k < chunks; k++) sum += a.partial[k * a.n_active * a.B + idx];
    }
    a.lagsum[idx] = sum;
}

// one thread per active origin: the loop of analysis.statistical_inefficiency over the lags of this batch
__global__ void ts_walk_kernel(ts_batch a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_active) return;
    const int s = a.active[i];
    const int64_t Ns = a.N - a.origin[s];
    const double sigma2 = a.sigma2[s];
    double g = a.g[s];
    int64_t last = a.last_lag[s];
    int done = 0;
    for (int b = 0; b < a.B; b++) {
        const int64_t t = ts_lag(a.t0, a.inc0, a.fast, b);
        if (t >= Ns - 1) { done = 1; break; }
        const double C = a.lagsum[(int64_t)i * a.B + b] / ((double)(Ns - t) * sigma2);
        if (C <= 0.0 && t > a.mintime) { done = 1; break; }
        g += 2.0 * C * (1.0 - (double)t / (double)Ns) * (double)ts_increment(a.inc0, a.fast, b);
        last = t;
    }
    a.g[s] = g; a.last_lag[s] = last; a.done[s] = done;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct remd_timeseries_ctx {
    int device = 0;
    int64_t N = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    double ms = 0.0;                        // kernels of the last call
    dev_array<double> A, mean, sigma2, g, partial, lagsum;
    dev_array<int64_t> origin, last_lag;
    dev_array<int> done, status, active;
    ~remd_timeseries_ctx()
    {
        hipSetDevice(device);
        if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); }
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
    }
};

#define TS_CHECK(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return remd_hip_fail(nullptr, #expr, _e); } while (0)

// the launches between ts_begin and ts_end are timed; ts_end waits for them
static int ts_begin(remd_timeseries ts) { TS_CHECK(hipEventRecord(ts->ev0, ts->stream)); return 0; }
static int ts_end(remd_timeseries ts)
{
    TS_CHECK(hipGetLastError());
    TS_CHECK(hipEventRecord(ts->ev1, ts->stream));
    TS_CHECK(hipStreamSynchronize(ts->stream));
    float t = 0.0f;
    TS_CHECK(hipEventElapsedTime(&t, ts->ev0, ts->ev1));
    ts->ms += t;
    return 0;
}

// g, status and last lag of the S origins of one group (S <= TS_GROUP_MAX, S * chunks of the series <= TS_PARTIAL_CAP where that can be)
static int ts_group(remd_timeseries ts, int S, const int64_t* origin, int fast, int mintime, double* g, int32_t* status, int64_t* last_lag)
{
    const int64_t N = ts->N;
    const int64_t all_chunks = (N - 1) / TS_CHUNK + 1;
    const size_t cap = (size_t)std::max<int64_t>(TS_PARTIAL_CAP, (int64_t)S * all_chunks);
    REMD_TRY(ts->partial.grow(nullptr, cap));
    REMD_TRY(ts->lagsum.grow(nullptr, (size_t)S * REMD_TIMESERIES_MAX_BATCH));
    REMD_TRY(ts->origin.grow(nullptr, S));
    REMD_TRY(ts->last_lag.grow(nullptr, S));
    REMD_TRY(ts->mean.grow(nullptr, S));
    REMD_TRY(ts->sigma2.grow(nullptr, S));
    REMD_TRY(ts->g.grow(nullptr, S));
    REMD_TRY(ts->done.grow(nullptr, S));
    REMD_TRY(ts->status.grow(nullptr, S));
    REMD_TRY(ts->active.grow(nullptr, S));
    TS_CHECK(hipMemcpyAsync(ts->origin, origin, sizeof(int64_t) * S, hipMemcpyHostToDevice, ts->stream));
    TS_CHECK(hipStreamSynchronize(ts->stream));

    // moments: mean, then sigma2 around it
    int64_t first = origin[0];
    for (int s = 1; s < S; s++) first = std::min(first, origin[s]);
    const dim3 mgrid((unsigned)(all_chunks - first / TS_CHUNK), (unsigned)S);
    const dim3 sgrid((unsigned)((S + 63) / 64));
    REMD_TRY(ts_begin(ts));
    hipLaunchKernelGGL(ts_moment_kernel<0>, mgrid, dim3(TS_BLOCK), 0, ts->stream, ts->A.get(), N, ts->origin.get(), ts->mean.get(), ts->partial.get());
    hipLaunchKernelGGL(ts_moment_merge_kernel<0>, sgrid, dim3(64), 0, ts->stream, ts->partial.get(), N, ts->origin.get(), S, ts->mean.get(),
                       ts->sigma2.get(), ts->g.get(), ts->done.get(), ts->status.get(), ts->last_lag.get());
    hipLaunchKernelGGL(ts_moment_kernel<1>, mgrid, dim3(TS_BLOCK), 0, ts->stream, ts->A.get(), N, ts->origin.get(), ts->mean.get(), ts->partial.get());
    hipLaunchKernelGGL(ts_moment_merge_kernel<1>, sgrid, dim3(64), 0, ts->stream, ts->partial.get(), N, ts->origin.get(), S, ts->mean.get(),
                       ts->sigma2.get(), ts->g.get(), ts->done.get(), ts->status.get(), ts->last_lag.get());
    REMD_TRY(ts_end(ts));

    std::vector<int> done(S), active;
    TS_CHECK(hipMemcpy(done.data(), ts->done, sizeof(int) * S, hipMemcpyDeviceToHost));
    int64_t t0 = 1, inc0 = 1;
    int ramp = TS_FIRST_BATCH;
    for (;;) {
        // the origins that go on, and the longest suffix among them
        active.clear();
        int64_t lo = N;
        for (int s = 0; s < S; s++)
            if (!done[s] && t0 < N - origin[s] - 1) { active.push_back(s); lo = std::min(lo, origin[s]); }
        if (active.empty()) break;
        const int n_active = (int)active.size();
        const int64_t chunks = (N - t0 - 1) / TS_CHUNK - lo / TS_CHUNK + 1;          // of the batch's first lag, the most
        const int64_t fit = TS_PARTIAL_CAP / ((int64_t)n_active * chunks);
        const int B = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(ramp, REMD_TIMESERIES_MAX_BATCH), fit));
        TS_CHECK(hipMemcpyAsync(ts->active, active.data(), sizeof(int) * n_active, hipMemcpyHostToDevice, ts->stream));
        TS_CHECK(hipStreamSynchronize(ts->stream));
        ts_batch a;
        a.A = ts->A; a.N = N; a.origin = ts->origin; a.mean = ts->mean; a.sigma2 = ts->sigma2; a.active = ts->active; a.n_active = n_active;
        a.t0 = t0; a.inc0 = inc0; a.fast = fast; a.B = B; a.mintime = mintime;
        a.partial = ts->partial; a.lagsum = ts->lagsum; a.g = ts->g; a.done = ts->done; a.last_lag = ts->last_lag;
        const int64_t pairs = (int64_t)n_active * B;
        REMD_TRY(ts_begin(ts));
        hipLaunchKernelGGL(ts_lag_kernel, dim3((unsigned)chunks, (unsigned)B, (unsigned)n_active), dim3(TS_BLOCK), 0, ts->stream, a);
        hipLaunchKernelGGL(ts_lag_merge_kernel, dim3((unsigned)((pairs + TS_BLOCK - 1) / TS_BLOCK)), dim3(TS_BLOCK), 0, ts->stream, a);
        hipLaunchKernelGGL(ts_walk_kernel, dim3((unsigned)((n_active + 63) / 64)), dim3(64), 0, ts->stream, a);
        REMD_TRY(ts_end(ts));
        TS_CHECK(hipMemcpy(done.data(), ts->done, sizeof(int) * S, hipMemcpyDeviceToHost));      // the one read-back of a batch
        for (int b = 0; b < B; b++) { t0 += inc0; if (fast) inc0++; }
        ramp = std::min(2 * ramp, REMD_TIMESERIES_MAX_BATCH);
    }
    TS_CHECK(hipMemcpy(g, ts->g, sizeof(double) * S, hipMemcpyDeviceToHost));
    TS_CHECK(hipMemcpy(status, ts->status, sizeof(int32_t) * S, hipMemcpyDeviceToHost));
    if (last_lag) TS_CHECK(hipMemcpy(last_lag, ts->last_lag, sizeof(int64_t) * S, hipMemcpyDeviceToHost));
    for (int s = 0; s < S; s++)
        if (!status[s]) g[s] = std::max(g[s], 1.0);
    return 0;
}

extern "C" {

int remd_timeseries_create(int device, int64_t N, const double* A, remd_timeseries* out)
{
    if (!out) return remd_fail(nullptr, -1, "remd_timeseries_create: out is NULL");
    *out = nullptr;
    if (N < 2) return remd_fail(nullptr, -1, "remd_timeseries_create: N must be at least 2");
    if (!A) return remd_fail(nullptr, -1, "remd_timeseries_create: A is NULL");
    for (int64_t n = 0; n < N; n++)
        if (!std::isfinite(A[n])) return remd_fail(nullptr, -1, "remd_timeseries_create: non-finite sample " + std::to_string(n));
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return remd_fail(nullptr, -2, std::string("remd_timeseries_create: no HIP device available (") + hipGetErrorString(e) + ")");
    if (device < 0 || device >= n) return remd_fail(nullptr, -1, "remd_timeseries_create: bad device index");
    TS_CHECK(hipSetDevice(device));
    std::unique_ptr<remd_timeseries_ctx> ts(new remd_timeseries_ctx());
    ts->device = device; ts->N = N;
    TS_CHECK(hipStreamCreate(&ts->stream));
    TS_CHECK(hipEventCreate(&ts->ev0));
    TS_CHECK(hipEventCreate(&ts->ev1));
    REMD_TRY(ts->A.alloc(nullptr, (size_t)N));
    TS_CHECK(hipMemcpy(ts->A, A, sizeof(double) * (size_t)N, hipMemcpyHostToDevice));
    *out = ts.release();
    return 0;
}

void remd_timeseries_destroy(remd_timeseries ts) { delete ts; }

int remd_timeseries_inefficiency(remd_timeseries ts, int32_t S, const int64_t* origin, int fast, int mintime, double* g,
                                 int32_t* status, int64_t* last_lag)
{
    if (!ts) return remd_fail(nullptr, -1, "remd_timeseries_inefficiency: the timeseries is NULL");
    if (S < 1) return remd_fail(nullptr, -1, "remd_timeseries_inefficiency: S must be at least 1");
    if (mintime < 0) return remd_fail(nullptr, -1, "remd_timeseries_inefficiency: mintime must not be negative");
    if (!origin || !g || !status) return remd_fail(nullptr, -1, "remd_timeseries_inefficiency: origin, g or status is NULL");
    for (int s = 0; s < S; s++)
        if (origin[s] < 0 || origin[s] > ts->N - 2)
            return remd_fail(nullptr, -1, "remd_timeseries_inefficiency: origin[" + std::to_string(s) + "] = " + std::to_string(origin[s]) +
                                          " is outside 0 ... N - 2 = " + std::to_string(ts->N - 2));
    TS_CHECK(hipSetDevice(ts->device));
    ts->ms = 0.0;
    ts->timed = false;
    // groups of origins whose per-chunk partials of one lag fit the cap
    const int64_t all_chunks = (ts->N - 1) / TS_CHUNK + 1;
    const int group = (int)std::max<int64_t>(1, std::min<int64_t>(TS_GROUP_MAX, TS_PARTIAL_CAP / all_chunks));
    for (int s0 = 0; s0 < S; s0 += group) {
        const int n = std::min(group, S - s0);
        REMD_TRY(ts_group(ts, n, origin + s0, fast ? 1 : 0, mintime, g + s0, status + s0, last_lag ? last_lag + s0 : nullptr));
    }
    ts->timed = true;
    return 0;
}

int remd_timeseries_chunks(remd_timeseries ts, int64_t* chunk)
{
    if (!ts || !chunk) return remd_fail(nullptr, -1, "remd_timeseries_chunks: the timeseries or chunk is NULL");
    *chunk = TS_CHUNK;
    return 0;
}

int remd_timeseries_last_ms(remd_timeseries ts, double* ms)
{
    if (!ts || !ms) return remd_fail(nullptr, -1, "remd_timeseries_last_ms: the timeseries or ms is NULL");
    if (!ts->timed) return remd_fail(nullptr, -1, "remd_timeseries_last_ms: no pass has run on this timeseries yet");
    *ms = ts->ms;
    return 0;
}

}
