// The statistical inefficiency on the device: of the suffixes of one timeseries (include/remd_hip_timeseries.h) and of several series
// of one length taken together (remd_series_inefficiency_multiple of include/remd_hip_energy_store.h).  All f64.  One set of passes for
// K series of one length N and S origins, of which the entries reach K = 1 (any S) and S = 1 with origin 0 (any K):
//
//   moments      workgroups per (series, origin, chunk of samples): sum A over the suffix, merged per origin in the order (series,
//                chunk) -> mean; then the same for sum (A - mean)^2 -> sigma2.  Two passes, as the host takes them.
//   lag batch    workgroups per (series, origin, lag of the batch, chunk of n): sum (A[n] - mean)(A[n + t] - mean) over the chunk; one
//                thread per (origin, lag) merges in the order (series, chunk); one thread per origin walks the lags of the batch in
//                order, applies the stopping rule and carries (g, done, last lag) to the next batch
//
// Chunk c is the samples [c * TS_CHUNK, (c + 1) * TS_CHUNK) whatever the origin and the lag, clipped to the range a sum runs over,
// and thread i of a workgroup always takes the samples c * TS_CHUNK + i, + 256, ...: a sum has one fixed order, set by (A, origin,
// lag) alone.  No floating-point atomics.
//
// Until it stops, every origin visits the same lags (1, 2, 3, ... or 1, 2, 4, 7, ...), so the lag and the increment a batch starts
// at are the host's, one pair for all origins, and a batch is (first lag, first increment, number of lags).
#include "device_object.h"
#include "../../include/remd_hip_timeseries.h"
#include "../../include/remd_hip_energy_store.h"
#include <cmath>
#include <limits>

#define TS_BLOCK        256
#define TS_CHUNK        2048                    // samples per workgroup: 8 per thread
#define TS_FIRST_BATCH  8                       // lags of the first batch; doubled per batch up to REMD_TIMESERIES_MAX_BATCH
#define TS_PARTIAL_CAP  (int64_t(1) << 22)      // doubles of per-chunk partials at most (32 MiB)
#define TS_GROUP_MAX    32768                   // origins of one pass over the series at most (a grid dimension)

static_assert(REMD_SERIES_MAX_BATCH == REMD_TIMESERIES_MAX_BATCH, "both entries walk batches of one size");

// lag b of a batch that starts at lag t0 with increment inc0, and the increment that goes with it
__device__ __forceinline__ int64_t ts_lag(int64_t t0, int64_t inc0, int fast, int b)
{
    return fast ? t0 + (int64_t)b * inc0 + (int64_t)b * (b - 1) / 2 : t0 + b;
}
__device__ __forceinline__ int64_t ts_increment(int64_t inc0, int fast, int b) { return fast ? inc0 + b : 1; }

// Every kernel and the host loop are written once, for K series and S origins, and compiled twice.  SEVERAL = 0: one series (k = 0,
// K = 1 to the compiler), any origins.  SEVERAL = 1: K series and the one origin 0 (s = 0, t_s = 0 to the compiler; no origin or active
// list is read).  What folds away leaves the arithmetic of each case as it was when the two were separate files.

// ---- moments --------------------------------------------------------------------------------------------------------------------
// grid (chunks from the origin's own first chunk on, origins or series): partial[(k * chunks + c) * S + s] = sum over chunk ∩ [t_s, N)
// of series k of A (SQUARED = 0) or of (A - mean_s)^2 (SQUARED = 1)
template <int SQUARED, int SEVERAL>
__global__ __launch_bounds__(TS_BLOCK) void ts_moment_kernel(const double* __restrict__ A, int64_t N, const int64_t* __restrict__ origin,
                                                             const double* __restrict__ mean, double* __restrict__ partial)
{
    __shared__ double sh[4];
    const int s = SEVERAL ? 0 : blockIdx.y, k = SEVERAL ? blockIdx.y : 0;
    const int64_t ts = SEVERAL ? 0 : origin[s];
    const int64_t n0 = (ts / TS_CHUNK + blockIdx.x) * TS_CHUNK;
    if (n0 >= N) return;                                                 // (the whole workgroup: this origin has fewer chunks)
    const int64_t hi = n0 + TS_CHUNK < N ? n0 + TS_CHUNK : N;
    const double* a = A + (int64_t)k * N;
    const double m = SQUARED ? mean[s] : 0.0;
    double acc = 0.0;
    for (int64_t n = n0 + threadIdx.x; n < hi; n += TS_BLOCK)
        if (n >= ts) {
            const double d = a[n] - m;
            acc += SQUARED ? d * d : d;
        }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[((int64_t)k * gridDim.x + blockIdx.x) * (SEVERAL ? 1 : gridDim.y) + s] = t;
}

// one thread per origin adds the series in order, of each its chunks in chunk order (`stride` chunks per series).  SQUARED = 0: the
// mean, and the walk's state at its start; SQUARED = 1: sigma2, and a suffix without variance is marked and done
template <int SQUARED, int SEVERAL>
__global__ void ts_moment_merge_kernel(const double* __restrict__ partial, int series, int64_t N, int64_t stride,
                                       const int64_t* __restrict__ origin, int S, double* __restrict__ mean, double* __restrict__ sigma2,
                                       double* __restrict__ g, int* __restrict__ done, int* __restrict__ status, int64_t* __restrict__ last_lag)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int K = SEVERAL ? series : 1;
    const int64_t ts = SEVERAL ? 0 : origin[s];
    const int64_t chunks = (N - 1) / TS_CHUNK - ts / TS_CHUNK + 1;
    double sum = 0.0;
    for (int k = 0; k < K; k++)
        for (int64_t c = 0; c < chunks; c++) sum += partial[(k * stride + c) * S + s];
    const double v = sum / (double)((int64_t)K * (N - ts));
    if (!SQUARED) {
        mean[s] = v; g[s] = 1.0; done[s] = 0; status[s] = 0; last_lag[s] = 0;
    } else {
        sigma2[s] = v;
        if (v == 0.0) { g[s] = std::numeric_limits<double>::quiet_NaN(); done[s] = 1; status[s] = 1; }
    }
}

// ---- lag batches ----------------------------------------------------------------------------------------------------------------
struct ts_batch {
    const double* A; int K; int64_t N;
    const int64_t* origin; const double* mean; const double* sigma2;      // per origin of the group
    const int* active; int n_active;                                     // the origins that have not stopped
    int64_t t0, inc0; int fast, B, mintime;
    int64_t chunks;                                                      // of the batch's first lag and the longest suffix: the most
    double* partial;                                                     // ts_partial
    double* lagsum;                                                      // [active][B]
    double* g; int* done; int64_t* last_lag;
};

// where the sum of (series k, chunk c from the origin's first) goes for slot = active origin * B + lag of the batch.  Many origins:
// the chunk is the slowest index, so the merge threads read side by side.  Several series have one origin and at most 64 merge
// threads: each keeps a run of its own, [slot][series][chunk], and meets every cache line once (with the chunk slowest the merge of
// K = 24, N = 94 500 took 1.6 times as long)
template <int SEVERAL>
__device__ __forceinline__ int64_t ts_partial(const ts_batch& a, int k, int64_t c, int64_t slot)
{
    return SEVERAL ? (slot * a.K + k) * a.chunks + c : c * a.n_active * a.B + slot;
}

// grid (chunks, B, active origins or series)
template <int SEVERAL>
__global__ __launch_bounds__(TS_BLOCK) void ts_lag_kernel(ts_batch a)
{
    __shared__ double sh[4];
    const int i = SEVERAL ? 0 : blockIdx.z, k = SEVERAL ? blockIdx.z : 0;
    const int s = SEVERAL ? 0 : a.active[i];
    const int64_t ts = SEVERAL ? 0 : a.origin[s];
    const int64_t t = ts_lag(a.t0, a.inc0, a.fast, blockIdx.y);
    if (t >= a.N - ts - 1) return;                                       // the walk stops before this lag
    const int64_t end = a.N - t;                                         // n + t < N for every n below it
    const int64_t n0 = (ts / TS_CHUNK + blockIdx.x) * TS_CHUNK;
    if (n0 >= end) return;
    const int64_t hi = n0 + TS_CHUNK < end ? n0 + TS_CHUNK : end;
    const double* A = a.A + (int64_t)k * a.N;
    const double m = a.mean[s];
    double acc = 0.0;
    for (int64_t n = n0 + threadIdx.x; n < hi; n += TS_BLOCK)
        if (n >= ts) acc += (A[n] - m) * (A[n + t] - m);
    const double v = block_sum(acc, sh);
    if (threadIdx.x == 0) a.partial[ts_partial<SEVERAL>(a, k, blockIdx.x, (int64_t)i * a.B + blockIdx.y)] = v;
}

// one thread per (active origin, lag): the series in order, of each the chunks [t_s / chunk, (N - t - 1) / chunk] in order, each of
// which the lag kernel wrote
template <int SEVERAL>
__global__ __launch_bounds__(TS_BLOCK) void ts_lag_merge_kernel(ts_batch a)
{
    const int64_t idx = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x;
    if (idx >= (int64_t)a.n_active * a.B) return;
    const int K = SEVERAL ? a.K : 1;
    const int s = SEVERAL ? 0 : a.active[idx / a.B];
    const int64_t ts = SEVERAL ? 0 : a.origin[s];
    const int64_t t = ts_lag(a.t0, a.inc0, a.fast, (int)(idx % a.B));
    double sum = 0.0;
    if (t < a.N - ts - 1) {
        const int64_t chunks = (a.N - t - 1) / TS_CHUNK - ts / TS_CHUNK + 1;
        for (int k = 0; k < K; k++)
            for (int64_t c = 0; c < chunks; c++) sum += a.partial[ts_partial<SEVERAL>(a, k, c, idx)];
    }
    a.lagsum[idx] = sum;
}

// one thread per active origin: the loop of analysis.statistical_inefficiency (_multiple) over the lags of this batch
template <int SEVERAL>
__global__ void ts_walk_kernel(ts_batch a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_active) return;
    const int K = SEVERAL ? a.K : 1;
    const int s = SEVERAL ? 0 : a.active[i];
    const int64_t Ns = a.N - (SEVERAL ? 0 : a.origin[s]);
    const double sigma2 = a.sigma2[s];
    double g = a.g[s];
    int64_t last = a.last_lag[s];
    int done = 0;
    for (int b = 0; b < a.B; b++) {
        const int64_t t = ts_lag(a.t0, a.inc0, a.fast, b);
        if (t >= Ns - 1) { done = 1; break; }
        const double C = a.lagsum[(int64_t)i * a.B + b] / ((double)K * (double)(Ns - t) * sigma2);
        if (C <= 0.0 && t > a.mintime) { done = 1; break; }
        g += 2.0 * C * (1.0 - (double)t / (double)Ns) * (double)ts_increment(a.inc0, a.fast, b);
        last = t;
    }
    a.g[s] = g; a.last_lag[s] = last; a.done[s] = done;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct remd_timeseries_ctx {
    int K = 1;
    int64_t N = 0;
    bool timed = false;
    dev_array<double> A, partial, lagsum;
    dev_array<int64_t> state;               // per origin of a group: mean, sigma2, g, origin, last lag, then done, status, active
    device_timer tm;                        // ms: the kernels of the last call
};

// K series of length N on `device`, A [K][N]
static int ts_open(const char* who, int device, int K, int64_t N, const double* A, std::unique_ptr<remd_timeseries_ctx>& ts)
{
    REMD_TRY(select_device(who, device));
    ts.reset(new remd_timeseries_ctx());
    ts->K = K; ts->N = N;
    REMD_TRY(ts->tm.open(device));
    REMD_TRY(ts->A.alloc(nullptr, (size_t)K * (size_t)N));
    DEVICE_CHECK(hipMemcpy(ts->A, A, sizeof(double) * (size_t)K * (size_t)N, hipMemcpyHostToDevice));
    return 0;
}

// g, status and last lag of the S origins of one group (S <= TS_GROUP_MAX, S * chunks of the series <= TS_PARTIAL_CAP where that can
// be).  SEVERAL: the K series of ts taken together, S = 1 and the origin 0.  The result does not depend on first_batch
template <int SEVERAL>
static int ts_group(remd_timeseries ts, int S, const int64_t* origin, int fast, int mintime, int first_batch, double* g, int32_t* status,
                    int64_t* last_lag)
{
    const int64_t N = ts->N;
    const int K = SEVERAL ? ts->K : 1;
    const int64_t all_chunks = (N - 1) / TS_CHUNK + 1;
    REMD_TRY(ts->partial.grow(nullptr, (size_t)std::max<int64_t>(TS_PARTIAL_CAP, (int64_t)K * S * all_chunks)));
    REMD_TRY(ts->lagsum.grow(nullptr, (size_t)S * REMD_TIMESERIES_MAX_BATCH));
    static_assert(sizeof(double) == sizeof(int64_t) && 2 * sizeof(int) == sizeof(int64_t), "the per-origin state is cut from 64-bit words");
    REMD_TRY(ts->state.grow(nullptr, 5 * (size_t)S + (3 * (size_t)S + 1) / 2));
    double* d_mean = (double*)ts->state.get();
    double* d_sigma2 = d_mean + S;
    double* d_g = d_sigma2 + S;
    int64_t* d_origin = ts->state.get() + 3 * (size_t)S;
    int64_t* d_last = d_origin + S;
    int* d_done = (int*)(d_last + S);
    int* d_status = d_done + S;
    int* d_active = d_status + S;
    const hipStream_t stream = ts->tm.stream;
    if (!SEVERAL) {
        DEVICE_CHECK(hipMemcpyAsync(d_origin, origin, sizeof(int64_t) * S, hipMemcpyHostToDevice, stream));
        DEVICE_CHECK(hipStreamSynchronize(stream));
    }

    // moments: mean, then sigma2 around it
    int64_t first = origin[0];
    for (int s = 1; s < S; s++) first = std::min(first, origin[s]);
    const int64_t mchunks = all_chunks - first / TS_CHUNK;
    const dim3 mgrid((unsigned)mchunks, (unsigned)(SEVERAL ? K : S));
    const dim3 sgrid((unsigned)((S + 63) / 64));
    REMD_TRY(ts->tm.begin());
    hipLaunchKernelGGL((ts_moment_kernel<0, SEVERAL>), mgrid, dim3(TS_BLOCK), 0, stream, ts->A.get(), N, d_origin, d_mean, ts->partial.get());
    hipLaunchKernelGGL((ts_moment_merge_kernel<0, SEVERAL>), sgrid, dim3(64), 0, stream, ts->partial.get(), K, N, mchunks, d_origin, S, d_mean,
                       d_sigma2, d_g, d_done, d_status, d_last);
    hipLaunchKernelGGL((ts_moment_kernel<1, SEVERAL>), mgrid, dim3(TS_BLOCK), 0, stream, ts->A.get(), N, d_origin, d_mean, ts->partial.get());
    hipLaunchKernelGGL((ts_moment_merge_kernel<1, SEVERAL>), sgrid, dim3(64), 0, stream, ts->partial.get(), K, N, mchunks, d_origin, S, d_mean,
                       d_sigma2, d_g, d_done, d_status, d_last);
    REMD_TRY(ts->tm.end());

    std::vector<int> done(S), active, sent;
    DEVICE_CHECK(hipMemcpy(done.data(), d_done, sizeof(int) * S, hipMemcpyDeviceToHost));
    int64_t t0 = 1, inc0 = 1;
    int ramp = first_batch;
    for (;;) {
        // the origins that go on, and the longest suffix among them
        active.clear();
        int64_t lo = N;
        for (int s = 0; s < S; s++)
            if (!done[s] && t0 < N - origin[s] - 1) { active.push_back(s); lo = std::min(lo, origin[s]); }
        if (active.empty()) break;
        const int n_active = (int)active.size();
        const int64_t chunks = (N - t0 - 1) / TS_CHUNK - lo / TS_CHUNK + 1;          // of the batch's first lag, the most
        const int64_t fit = TS_PARTIAL_CAP / ((int64_t)K * n_active * chunks);
        const int B = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(ramp, REMD_TIMESERIES_MAX_BATCH), fit));
        if (!SEVERAL && active != sent) {
            DEVICE_CHECK(hipMemcpyAsync(d_active, active.data(), sizeof(int) * n_active, hipMemcpyHostToDevice, stream));
            DEVICE_CHECK(hipStreamSynchronize(stream));
            sent = active;
        }
        ts_batch a;
        a.A = ts->A; a.K = K; a.N = N; a.origin = d_origin; a.mean = d_mean; a.sigma2 = d_sigma2; a.active = d_active; a.n_active = n_active;
        a.t0 = t0; a.inc0 = inc0; a.fast = fast; a.B = B; a.mintime = mintime; a.chunks = chunks;
        a.partial = ts->partial; a.lagsum = ts->lagsum; a.g = d_g; a.done = d_done; a.last_lag = d_last;
        const int64_t pairs = (int64_t)n_active * B;
        REMD_TRY(ts->tm.begin());
        hipLaunchKernelGGL(ts_lag_kernel<SEVERAL>, dim3((unsigned)chunks, (unsigned)B, (unsigned)(SEVERAL ? K : n_active)), dim3(TS_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(ts_lag_merge_kernel<SEVERAL>, dim3((unsigned)((pairs + TS_BLOCK - 1) / TS_BLOCK)), dim3(TS_BLOCK), 0, stream, a);
        hipLaunchKernelGGL(ts_walk_kernel<SEVERAL>, dim3((unsigned)((n_active + 63) / 64)), dim3(64), 0, stream, a);
        REMD_TRY(ts->tm.end());
        DEVICE_CHECK(hipMemcpy(done.data(), d_done, sizeof(int) * S, hipMemcpyDeviceToHost));    // the one read-back of a batch
        for (int b = 0; b < B; b++) { t0 += inc0; if (fast) inc0++; }
        ramp = std::min(2 * ramp, REMD_TIMESERIES_MAX_BATCH);
    }
    DEVICE_CHECK(hipMemcpy(g, d_g, sizeof(double) * S, hipMemcpyDeviceToHost));
    DEVICE_CHECK(hipMemcpy(status, d_status, sizeof(int32_t) * S, hipMemcpyDeviceToHost));
    if (last_lag) DEVICE_CHECK(hipMemcpy(last_lag, d_last, sizeof(int64_t) * S, hipMemcpyDeviceToHost));
    for (int s = 0; s < S; s++)
        if (!status[s]) g[s] = std::max(g[s], 1.0);
    return 0;
}

// g, status and last lag of the K series A_kn [K][N] taken together (remd_series_inefficiency_multiple of energy_store.hip, which has
// checked the arguments); the first batch has first_batch lags.  ms (the kernels) and chunk (samples per workgroup) may be NULL
int series_inefficiency(const char* who, int device, int K, int64_t N, const double* A_kn, int fast, int mintime, int first_batch, double* g,
                        int32_t* status, int64_t* last_lag, double* ms, int64_t* chunk)
{
    std::unique_ptr<remd_timeseries_ctx> ts;
    REMD_TRY(ts_open(who, device, K, N, A_kn, ts));
    const int64_t origin = 0;
    REMD_TRY((K > 1 ? ts_group<1> : ts_group<0>)(ts.get(), 1, &origin, fast, mintime, first_batch, g, status, last_lag));
    if (ms) *ms = ts->tm.ms;
    if (chunk) *chunk = TS_CHUNK;
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
    std::unique_ptr<remd_timeseries_ctx> ts;
    REMD_TRY(ts_open("remd_timeseries_create", device, 1, N, A, ts));
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
    DEVICE_CHECK(hipSetDevice(ts->tm.device));
    ts->tm.ms = 0.0;
    ts->timed = false;
    // groups of origins whose per-chunk partials of one lag fit the cap
    const int64_t all_chunks = (ts->N - 1) / TS_CHUNK + 1;
    const int group = (int)std::max<int64_t>(1, std::min<int64_t>(TS_GROUP_MAX, TS_PARTIAL_CAP / all_chunks));
    for (int s0 = 0; s0 < S; s0 += group) {
        const int n = std::min(group, S - s0);
        REMD_TRY(ts_group<0>(ts, n, origin + s0, fast ? 1 : 0, mintime, TS_FIRST_BATCH, g + s0, status + s0, last_lag ? last_lag + s0 : nullptr));
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
    *ms = ts->tm.ms;
    return 0;
}

}
