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
//   several series     remd_series_inefficiency_multiple checks its arguments here; the passes are those of timeseries.hip, for K
//                      series and the one origin 0 (series_inefficiency, defined there).
//
// No floating-point atomics anywhere.  Every index that can pass 2^31 is 64 bits wide.
#include "device_object.h"
#include "../../include/remd_hip_energy_store.h"
#include <cmath>
#include <limits>

#define ES_BLOCK          256
#define ES_TILE           32
#define ES_TILE_ROWS      8                       // blockDim.y of the gather: a thread moves ES_TILE / ES_TILE_ROWS words each way
#define ES_COUNT_CHUNK    8192                    // (iteration, replica) pairs per workgroup of the counting passes
#define ES_HIST_MAX_S     64                      // the LDS histogram of the transition counts has S x S cells: 16 KiB at 64
#define ES_FIRST_BATCH    8                       // lags of the first batch of remd_series_inefficiency_multiple

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

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct remd_energy_store_ctx {
    int64_t T = 0;
    int R = 0, S = 0, U = 0;
    bool timed = false;
    dev_array<double> energies, unsampled, log_weights, f_l, u_n, u_ln;
    dev_array<int32_t> states;
    dev_array<int64_t> iterations;
    dev_array<es_u64> counts;
    device_timer tm;
};

// the passes of timeseries.hip at K series and the one origin 0 (defined there)
int series_inefficiency(const char* who, int device, int K, int64_t N, const double* A_kn, int fast, int mintime, int first_batch, double* g,
                        int32_t* status, int64_t* last_lag, double* ms, int64_t* chunk);

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
    return series_inefficiency(who, device, K, N, A_kn, fast, mintime, first_batch, g, status, last_lag, ms, chunk);
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
    REMD_TRY(select_device(who, device));
    std::unique_ptr<remd_energy_store_ctx> st(new remd_energy_store_ctx());
    st->T = T; st->R = R; st->S = S; st->U = U;
    REMD_TRY(st->tm.open(device));
    REMD_TRY(st->energies.alloc(nullptr, (size_t)pairs * S));
    REMD_TRY(st->states.alloc(nullptr, (size_t)pairs));
    DEVICE_CHECK(hipMemcpy(st->energies, energies, sizeof(double) * (size_t)pairs * S, hipMemcpyHostToDevice));
    DEVICE_CHECK(hipMemcpy(st->states, states, sizeof(int32_t) * (size_t)pairs, hipMemcpyHostToDevice));
    if (U) {
        REMD_TRY(st->unsampled.alloc(nullptr, (size_t)pairs * U));
        DEVICE_CHECK(hipMemcpy(st->unsampled, unsampled, sizeof(double) * (size_t)pairs * U, hipMemcpyHostToDevice));
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
    DEVICE_CHECK(hipSetDevice(st->tm.device));
    const int64_t T = st->T;
    REMD_TRY(st->u_n.grow(nullptr, (size_t)T));
    if (log_weights) {
        REMD_TRY(st->log_weights.grow(nullptr, (size_t)T * st->S));
        REMD_TRY(st->f_l.grow(nullptr, (size_t)st->S));
        DEVICE_CHECK(hipMemcpy(st->log_weights, log_weights, sizeof(double) * (size_t)T * st->S, hipMemcpyHostToDevice));
        DEVICE_CHECK(hipMemcpy(st->f_l, f_l, sizeof(double) * (size_t)st->S, hipMemcpyHostToDevice));
    }
    st->tm.ms = 0.0; st->timed = false;
    REMD_TRY(st->tm.begin());
    hipLaunchKernelGGL(es_effective_kernel, dim3((unsigned)((T + ES_BLOCK - 1) / ES_BLOCK)), dim3(ES_BLOCK), 0, st->tm.stream, st->energies.get(),
                       st->states.get(), log_weights ? st->log_weights.get() : nullptr, log_weights ? st->f_l.get() : nullptr, T, st->R, st->S,
                       st->u_n.get());
    REMD_TRY(st->tm.end());
    st->timed = true;
    DEVICE_CHECK(hipMemcpy(u_n, st->u_n, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost));
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
    DEVICE_CHECK(hipSetDevice(st->tm.device));
    REMD_TRY(st->iterations.grow(nullptr, (size_t)n_sel));
    REMD_TRY(st->u_ln.grow(nullptr, (size_t)rows * cols));
    REMD_TRY(st->counts.grow(nullptr, (size_t)S * S));
    DEVICE_CHECK(hipMemcpy(st->iterations, iterations, sizeof(int64_t) * (size_t)n_sel, hipMemcpyHostToDevice));
    DEVICE_CHECK(hipMemsetAsync(st->counts, 0, sizeof(es_u64) * (size_t)S, st->tm.stream));
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
    DEVICE_CHECK(hipMemcpy(u_ln, st->u_ln, sizeof(double) * (size_t)rows * cols, hipMemcpyDeviceToHost));
    static_assert(sizeof(es_u64) == sizeof(int64_t), "the counters are read back as int64_t");
    DEVICE_CHECK(hipMemcpy(N_l + first, st->counts, sizeof(int64_t) * (size_t)S, hipMemcpyDeviceToHost));
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
    DEVICE_CHECK(hipSetDevice(st->tm.device));
    REMD_TRY(st->counts.grow(nullptr, cells));
    DEVICE_CHECK(hipMemsetAsync(st->counts, 0, sizeof(es_u64) * cells, st->tm.stream));
    st->tm.ms = 0.0; st->timed = false;
    REMD_TRY(st->tm.begin());
    const int32_t* from = st->states.get() + t_begin * R;
    if (S <= ES_HIST_MAX_S)
        hipLaunchKernelGGL(es_transition_kernel<1>, dim3((unsigned)groups), dim3(ES_BLOCK), 0, st->tm.stream, from, n_pairs, R, S, st->counts.get());
    else
        hipLaunchKernelGGL(es_transition_kernel<0>, dim3((unsigned)groups), dim3(ES_BLOCK), 0, st->tm.stream, from, n_pairs, R, S, st->counts.get());
    REMD_TRY(st->tm.end());
    st->timed = true;
    DEVICE_CHECK(hipMemcpy(n_ij, st->counts, sizeof(int64_t) * cells, hipMemcpyDeviceToHost));
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
