// The MBAR problem on the device as mbar.hip (the passes at one f_k) and mbar_bootstrap.hip (the batched passes over resampled
// problems) share it: the uploaded matrix, the tables of the sampled states, the work arrays of either file and the timed stream.
#pragma once
#include "device_object.h"
#include "../../include/remd_hip_mbar.h"
#include <vector>

#define MBAR_BLOCK       256
#define MBAR_ROW_CHUNK   4096          // samples per workgroup of the row pass: 16 per thread
#define MBAR_TILE        64            // columns of the Gram matrix per tile edge
#define MBAR_TSTEP       16            // samples staged in LDS per step of the Gram pass
#define MBAR_LDS_STRIDE  (MBAR_TILE + 2)

// _logsumexp's guard: a non-finite maximum counts as 0
__device__ __forceinline__ double mbar_guard(double m) { return isfinite(m) ? m : 0.0; }

// one thread per state merges its pairs in chunk order.  as_log: out = sign * (ln S + M), else out = S
static __global__ void mbar_row_merge_kernel(const double2* __restrict__ pairs, int K, int chunks, int as_log, double sign, double* __restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const double2* p = pairs + (int64_t)k * chunks;
    double M = -INFINITY;
    for (int c = 0; c < chunks; c++) M = nanmax(M, p[c].x);
    M = mbar_guard(M);
    double S = 0.0;
    for (int c = 0; c < chunks; c++)
        if (p[c].y != 0.0) S += p[c].y * exp(mbar_guard(p[c].x) - M);      // (an empty chunk's scale may overflow: it adds nothing)
    out[k] = as_log ? sign * (log(S) + M) : S;
}

// what mbar_bootstrap.hip keeps between its calls: the multiplicities of the resident replicates and the work arrays of a batch
struct mbar_bootstrap_state {
    int b0 = 0, nb = 0;                     // replicates b0 .. b0 + nb - 1 are resident (nb = 0: none drawn)
    dev_array<uint32_t> counts;             // [nb][N]
    dev_array<int> state_start, state_samples;      // [Ks + 1], [N]: the samples of each sampled state, ascending
    dev_array<int> reps, row_state;                 // [nr] the replicates of a call, [rows] the state of each row of a row pass
    dev_array<int2> tiles;
    dev_array<double> f, log_den, col_partial, phi_sum, row_out, gram, gram_partial;     // f [nr][K], log_den [nr][N], ...
    dev_array<double2> pairs;
};

struct remd_mbar_ctx {
    int K = 0, Ks = 0;
    int64_t N = 0;
    double shift = 0.0;
    bool timed = false;                     // a pass has run: tm.ms holds its kernels
    std::vector<double> nk_all;             // [K]
    std::vector<int> srow;                  // [Ks]
    dev_array<double> u, nk, fs, f, log_den, col_partial, scalar, row_out, log_cA, gram, gram_partial, weights;
    dev_array<int> d_srow, col_state;
    dev_array<int2> tiles;
    dev_array<double2> pairs;
    mbar_bootstrap_state boot;
    device_timer tm;
};

// How a call of either file starts and ends, and its column pass; mbar_pmf.hip's calls go through the same ones.
// mbar.hip: every pointer is checked, f_k uploaded and the clock started; log_den on the device with its sum in scalar[0]; the clock
// stopped.  mbar_bootstrap.hip: a batched call is checked, reps[nr] and f_b[nr][K] uploaded, log_den[nr][N] sized and the clock
// started; log_den[nr][N] with sum_n c_n log_den_n per replicate in phi_sum[nr]; the clock stopped.
int mbar_begin(remd_mbar m, const char* who, const double* f_k, const void* out = (const void*)1, const void* out2 = (const void*)1);
int mbar_column_pass(remd_mbar m);
int mbar_end(remd_mbar m);
int boot_begin(remd_mbar m, const std::string& who, int nr, const int32_t* reps, const double* f_b);
int boot_column_pass(remd_mbar m, int nr);
int boot_end(remd_mbar m);
