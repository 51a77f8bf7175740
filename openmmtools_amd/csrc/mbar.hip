// The passes of the MBAR estimator on the device (include/remd_hip_mbar.h).  All f64; u_kn stays [K][N], sample index fastest.
//
//   column pass  one thread per sample over the sampled states: log_den_n, and its sum per workgroup -> fixed-order second stage
//   row pass     workgroups per (state, chunk of samples): a (max, scaled sum) pair each, merged per state in chunk order
//   Gram pass    workgroups per (64 x 64 tile of the lower triangle, chunk of samples): the weights are recomputed from u, f and
//                log_den into LDS, 16 samples at a time, and accumulated in a 4 x 4 register tile per thread with plain f64 FMAs;
//                the per-chunk partials are summed in chunk order by a second stage
//   augmented    remd_mbar_augmented_gram: the same three passes over K stored states + L perturbed states + I observables of one
//                call (the row pass of eq. 11 on u_ln, a row pass for ln <A>, the Gram tiles over the K + L + I columns)
//
// No floating-point atomics: every sum has one fixed order, set by (K, N) alone.
#include "mbar_ctx.h"
#include <cmath>
#include <limits>

#define MBAR_GRAM_MIN_CHUNK   256
#define MBAR_GRAM_MAX_CHUNKS  256
#define MBAR_GRAM_PARTIAL_CAP (int64_t(1) << 25)   // doubles of per-chunk partials at most (256 MiB)

enum { MBAR_ROW_SC = 0, MBAR_ROW_LOGCA = 1, MBAR_ROW_WSUM = 2 };

// ---- column pass ----------------------------------------------------------------------------------------------------------------
// fs[Ks], nk[Ks], srow[Ks]: f_k, N_k and the row of u of the sampled states
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_logden_kernel(const double* __restrict__ u, const double* __restrict__ fs,
                                                                 const double* __restrict__ nk, const int* __restrict__ srow, int Ks,
                                                                 int64_t N, double* __restrict__ log_den, double* __restrict__ partial)
{
    __shared__ double sh[4];
    const int64_t n = (int64_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    double ld = 0.0;
    if (n < N) {
        double m = -INFINITY;
        for (int j = 0; j < Ks; j++) m = nanmax(m, fs[j] - u[(int64_t)srow[j] * N + n]);
        m = mbar_guard(m);
        double s = 0.0;
        for (int j = 0; j < Ks; j++) s += nk[j] * exp((fs[j] - u[(int64_t)srow[j] * N + n]) - m);
        ld = log(s) + m;
        log_den[n] = ld;
    }
    const double t = block_sum(ld, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// out[0] = the sum of partial[n]: thread t takes t, t + 256, ... in order, then the block sum
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_sum_kernel(const double* __restrict__ partial, int64_t n, double* __restrict__ out)
{
    __shared__ double sh[4];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += MBAR_BLOCK) s += partial[i];
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) out[0] = t;
}

// ---- row pass -------------------------------------------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ double mbar_row_term(double uu, double ld, double fk, double shift)
{
    if (MODE == MBAR_ROW_SC) return -uu - ld;
    const double lw = (fk - uu) - ld;
    if (MODE == MBAR_ROW_LOGCA) return lw + log(uu - shift);
    return lw;
}

// grid (chunks, K): pairs[k * chunks + c] = (max of the terms, sum exp(term - guarded max)); MBAR_ROW_WSUM: (0, sum exp(term))
template <int MODE>
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_row_kernel(const double* __restrict__ u, const double* __restrict__ log_den,
                                                              const double* __restrict__ f, int64_t N, double shift,
                                                              double2* __restrict__ pairs)
{
    __shared__ double sh[4];
    const int k = blockIdx.y;
    const int64_t n0 = (int64_t)blockIdx.x * MBAR_ROW_CHUNK;
    const int64_t n1 = n0 + MBAR_ROW_CHUNK < N ? n0 + MBAR_ROW_CHUNK : N;
    const double* __restrict__ uk = u + (int64_t)k * N;
    const double fk = f[k];
    double mraw = 0.0, m = 0.0;
    if (MODE != MBAR_ROW_WSUM) {
        double mt = -INFINITY;
        for (int64_t n = n0 + threadIdx.x; n < n1; n += MBAR_BLOCK) mt = nanmax(mt, mbar_row_term<MODE>(uk[n], log_den[n], fk, shift));
        mraw = block_nanmax(mt, sh);
        m = mbar_guard(mraw);
    }
    double s = 0.0;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += MBAR_BLOCK) s += exp(mbar_row_term<MODE>(uk[n], log_den[n], fk, shift) - m);
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) pairs[(int64_t)k * gridDim.x + blockIdx.x] = make_double2(mraw, t);
}

// (mbar_row_merge_kernel: mbar_ctx.h)

// ---- Gram pass ------------------------------------------------------------------------------------------------------------------
struct mbar_gram_args {
    const double* u; const double* log_den; const double* f; const double* log_cA;
    const int* col_state;        // [C] the state of a column
    const int2* tiles;           // (ti, tj), ti >= tj
    int C, n_plain;              // columns >= n_plain carry the observable
    int64_t N, chunk;
    double shift;
    double* partial;             // [chunks][C][C], the lower triangle's tiles
};

__device__ __forceinline__ double mbar_column_value(const mbar_gram_args& a, int c, int64_t n, int64_t n1, double ld)
{
    if (c >= a.C || n >= n1) return 0.0;
    const int k = a.col_state[c];
    const double uu = a.u[(int64_t)k * a.N + n];
    double lw = (a.f[k] - uu) - ld;
    if (c >= a.n_plain) lw = (lw + log(uu - a.shift)) - a.log_cA[k];
    return exp(lw);
}

__global__ __launch_bounds__(MBAR_BLOCK) void mbar_gram_kernel(mbar_gram_args a)
{
    __shared__ double As[MBAR_TSTEP][MBAR_LDS_STRIDE];
    __shared__ double Bs[MBAR_TSTEP][MBAR_LDS_STRIDE];
    const int2 tile = a.tiles[blockIdx.x];
    const int i0 = tile.x * MBAR_TILE, j0 = tile.y * MBAR_TILE;
    const int64_t n0 = (int64_t)blockIdx.y * a.chunk;
    const int64_t n1 = n0 + a.chunk < a.N ? n0 + a.chunk : a.N;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int fs = t & (MBAR_TSTEP - 1), fc = t >> 4;             // the sample and the first column this thread stages
    const bool diagonal = i0 == j0;                               // both operands are the same columns: staged once
    const double (*Bp)[MBAR_LDS_STRIDE] = diagonal ? As : Bs;
    double acc[4][4];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    for (int64_t nb = n0; nb < n1; nb += MBAR_TSTEP) {
        const int64_t n = nb + fs;
        const double ld = n < n1 ? a.log_den[n] : 0.0;
        #pragma unroll
        for (int p = 0; p < 4; p++) {
            const int cl = fc + 16 * p;
            As[fs][cl] = mbar_column_value(a, i0 + cl, n, n1, ld);
            if (!diagonal) Bs[fs][cl] = mbar_column_value(a, j0 + cl, n, n1, ld);
        }
        __syncthreads();
        #pragma unroll
        for (int s = 0; s < MBAR_TSTEP; s++) {
            double av[4], bv[4];
            #pragma unroll
            for (int i = 0; i < 4; i++) { av[i] = As[s][ty * 4 + i]; bv[i] = Bp[s][tx * 4 + i]; }
            #pragma unroll
            for (int i = 0; i < 4; i++)
                #pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
    double* out = a.partial + (int64_t)blockIdx.y * a.C * a.C;
    for (int i = 0; i < 4; i++) {
        const int gi = i0 + ty * 4 + i;
        if (gi >= a.C) continue;
        for (int j = 0; j < 4; j++) {
            const int gj = j0 + tx * 4 + j;
            if (gj < a.C) out[(int64_t)gi * a.C + gj] = acc[i][j];
        }
    }
}

// one thread per entry of the lower triangle sums the partials in chunk order and writes both halves
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_gram_sum_kernel(const double* __restrict__ partial, int C, int chunks, double* __restrict__ gram)
{
    const int64_t idx = (int64_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (idx >= (int64_t)C * C) return;
    const int i = (int)(idx / C), j = (int)(idx % C);
    if (j > i) return;
    double s = 0.0;
    for (int c = 0; c < chunks; c++) s += partial[(int64_t)c * C * C + idx];
    gram[(int64_t)i * C + j] = s;
    gram[(int64_t)j * C + i] = s;
}

// ---- augmented columns (remd_mbar_augmented_gram) -------------------------------------------------------------------------------
// Column c of the augmented set: c < K a stored state, K <= c < K + L a perturbed state of the call, beyond that observable
// c - (K + L) on the weights of column obs_state[.].  States 0 .. K + L - 1 share f[K + L] (f_k, then f_l) and mbar_aug_row.
struct mbar_aug_args {
    const double* u; const double* u_ln; const double* A; const double* log_den; const double* f; const double* log_cA;
    const int* obs_state;        // [I]
    const int2* tiles;           // (ti, tj), ti >= tj
    int K, L, C;
    int64_t N, chunk;
    double* partial;             // [chunks][C][C], the lower triangle's tiles
};

__device__ __forceinline__ const double* mbar_aug_row(const double* __restrict__ u, const double* __restrict__ u_ln, int K, int64_t N, int s)
{
    return s < K ? u + (int64_t)s * N : u_ln + (int64_t)(s - K) * N;
}

// grid (chunks, I): pairs[i * chunks + c] = (max, sum exp(term - guarded max)) of  term = ln W_n,obs_state[i] + ln A_in
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_aug_logca_kernel(const double* __restrict__ u, const double* __restrict__ u_ln,
                                                                    const double* __restrict__ A, const double* __restrict__ log_den,
                                                                    const double* __restrict__ f, const int* __restrict__ obs_state,
                                                                    int K, int64_t N, double2* __restrict__ pairs)
{
    __shared__ double sh[4];
    const int i = blockIdx.y, s = obs_state[i];
    const int64_t n0 = (int64_t)blockIdx.x * MBAR_ROW_CHUNK;
    const int64_t n1 = n0 + MBAR_ROW_CHUNK < N ? n0 + MBAR_ROW_CHUNK : N;
    const double* __restrict__ us = mbar_aug_row(u, u_ln, K, N, s);
    const double* __restrict__ Ai = A + (int64_t)i * N;
    const double fs = f[s];
    double mt = -INFINITY;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += MBAR_BLOCK) mt = nanmax(mt, ((fs - us[n]) - log_den[n]) + log(Ai[n]));
    const double mraw = block_nanmax(mt, sh);
    const double m = mbar_guard(mraw);
    double sum = 0.0;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += MBAR_BLOCK) sum += exp((((fs - us[n]) - log_den[n]) + log(Ai[n])) - m);
    const double t = block_sum(sum, sh);
    if (threadIdx.x == 0) pairs[(int64_t)i * gridDim.x + blockIdx.x] = make_double2(mraw, t);
}

__device__ __forceinline__ double mbar_aug_column_value(const mbar_aug_args& a, int c, int64_t n, int64_t n1, double ld)
{
    if (c >= a.C || n >= n1) return 0.0;
    const int i = c - (a.K + a.L);
    const int s = i < 0 ? c : a.obs_state[i];
    double lw = (a.f[s] - mbar_aug_row(a.u, a.u_ln, a.K, a.N, s)[n]) - ld;
    if (i >= 0) lw = (lw + log(a.A[(int64_t)i * a.N + n])) - a.log_cA[i];
    return exp(lw);
}

// mbar_gram_kernel's tiles, staging and 4 x 4 register tile over the augmented columns
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_aug_gram_kernel(mbar_aug_args a)
{
    __shared__ double As[MBAR_TSTEP][MBAR_LDS_STRIDE];
    __shared__ double Bs[MBAR_TSTEP][MBAR_LDS_STRIDE];
    const int2 tile = a.tiles[blockIdx.x];
    const int i0 = tile.x * MBAR_TILE, j0 = tile.y * MBAR_TILE;
    const int64_t n0 = (int64_t)blockIdx.y * a.chunk;
    const int64_t n1 = n0 + a.chunk < a.N ? n0 + a.chunk : a.N;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int fs = t & (MBAR_TSTEP - 1), fc = t >> 4;
    const bool diagonal = i0 == j0;
    const double (*Bp)[MBAR_LDS_STRIDE] = diagonal ? As : Bs;
    double acc[4][4];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    for (int64_t nb = n0; nb < n1; nb += MBAR_TSTEP) {
        const int64_t n = nb + fs;
        const double ld = n < n1 ? a.log_den[n] : 0.0;
        #pragma unroll
        for (int p = 0; p < 4; p++) {
            const int cl = fc + 16 * p;
            As[fs][cl] = mbar_aug_column_value(a, i0 + cl, n, n1, ld);
            if (!diagonal) Bs[fs][cl] = mbar_aug_column_value(a, j0 + cl, n, n1, ld);
        }
        __syncthreads();
        #pragma unroll
        for (int s = 0; s < MBAR_TSTEP; s++) {
            double av[4], bv[4];
            #pragma unroll
            for (int i = 0; i < 4; i++) { av[i] = As[s][ty * 4 + i]; bv[i] = Bp[s][tx * 4 + i]; }
            #pragma unroll
            for (int i = 0; i < 4; i++)
                #pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
    double* out = a.partial + (int64_t)blockIdx.y * a.C * a.C;
    for (int i = 0; i < 4; i++) {
        const int gi = i0 + ty * 4 + i;
        if (gi >= a.C) continue;
        for (int j = 0; j < 4; j++) {
            const int gj = j0 + tx * 4 + j;
            if (gj < a.C) out[(int64_t)gi * a.C + gj] = acc[i][j];
        }
    }
}

// ---- weights --------------------------------------------------------------------------------------------------------------------
// 16 x 16 tiles through LDS: u is read along the samples, log_W_nk[N][K] written along the states
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_log_weights_kernel(const double* __restrict__ u, const double* __restrict__ log_den,
                                                                      const double* __restrict__ f, int K, int64_t N, double* __restrict__ out)
{
    __shared__ double tile[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t nb = (int64_t)blockIdx.x * 16;
    const int kb = blockIdx.y * 16;
    {
        const int64_t n = nb + tx; const int k = kb + ty;
        tile[ty][tx] = (n < N && k < K) ? (f[k] - u[(int64_t)k * N + n]) - log_den[n] : 0.0;
    }
    __syncthreads();
    {
        const int64_t n = nb + ty; const int k = kb + tx;
        if (n < N && k < K) out[n * K + k] = tile[tx][ty];
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// (remd_mbar_ctx: mbar_ctx.h)

static int64_t mbar_gram_chunk(int64_t N, int C)
{
    int64_t max_chunks = MBAR_GRAM_PARTIAL_CAP / ((int64_t)C * C);
    max_chunks = std::max<int64_t>(1, std::min<int64_t>(MBAR_GRAM_MAX_CHUNKS, max_chunks));
    int64_t chunk = (N + max_chunks - 1) / max_chunks;
    chunk = (chunk + MBAR_TSTEP - 1) / MBAR_TSTEP * MBAR_TSTEP;
    return std::max<int64_t>(MBAR_GRAM_MIN_CHUNK, chunk);
}

// every pointer of a call is checked before anything is copied; `out` and `out2` are the outputs that may not be NULL
int mbar_begin(remd_mbar m, const char* who, const double* f_k, const void* out, const void* out2)
{
    if (!m) return remd_fail(nullptr, -1, std::string(who) + ": the problem is NULL");
    if (!f_k) return remd_fail(nullptr, -1, std::string(who) + ": f_k is NULL");
    if (!out || !out2) return remd_fail(nullptr, -1, std::string(who) + ": an output array is NULL");
    DEVICE_CHECK(hipSetDevice(m->tm.device));
    std::vector<double> fs(m->Ks);
    for (int j = 0; j < m->Ks; j++) fs[j] = f_k[m->srow[j]];
    DEVICE_CHECK(hipMemcpyAsync(m->f, f_k, sizeof(double) * m->K, hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipMemcpyAsync(m->fs, fs.data(), sizeof(double) * m->Ks, hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipStreamSynchronize(m->tm.stream));            // (fs is a local)
    m->tm.ms = 0.0;
    return m->tm.begin();
}

int mbar_end(remd_mbar m)
{
    REMD_TRY(m->tm.end());
    m->timed = true;
    return 0;
}

// log_den on the device, its sum in scalar[0]
int mbar_column_pass(remd_mbar m)
{
    const int64_t blocks = (m->N + MBAR_BLOCK - 1) / MBAR_BLOCK;
    hipLaunchKernelGGL(mbar_logden_kernel, dim3((unsigned)blocks), dim3(MBAR_BLOCK), 0, m->tm.stream, m->u.get(), m->fs.get(), m->nk.get(),
                       m->d_srow.get(), m->Ks, m->N, m->log_den.get(), m->col_partial.get());
    hipLaunchKernelGGL(mbar_sum_kernel, dim3(1), dim3(MBAR_BLOCK), 0, m->tm.stream, m->col_partial.get(), blocks, m->scalar.get());
    DEVICE_CHECK(hipGetLastError());
    return 0;
}

static int mbar_phi(remd_mbar m, const double* f_k, double* phi)
{
    double sum = 0.0;
    DEVICE_CHECK(hipMemcpy(&sum, m->scalar, sizeof(double), hipMemcpyDeviceToHost));
    double dot = 0.0;
    for (int j = 0; j < m->Ks; j++) dot += m->nk_all[m->srow[j]] * f_k[m->srow[j]];
    *phi = sum - dot;
    return 0;
}

// the row pass over all K states into dst[K] (device)
static int mbar_row_pass(remd_mbar m, int mode, double* dst)
{
    const int chunks = (int)((m->N + MBAR_ROW_CHUNK - 1) / MBAR_ROW_CHUNK);
    const dim3 grid((unsigned)chunks, (unsigned)m->K);
    if (mode == MBAR_ROW_SC)
        hipLaunchKernelGGL(mbar_row_kernel<MBAR_ROW_SC>, grid, dim3(MBAR_BLOCK), 0, m->tm.stream, m->u.get(), m->log_den.get(), m->f.get(), m->N, m->shift, m->pairs.get());
    else if (mode == MBAR_ROW_LOGCA)
        hipLaunchKernelGGL(mbar_row_kernel<MBAR_ROW_LOGCA>, grid, dim3(MBAR_BLOCK), 0, m->tm.stream, m->u.get(), m->log_den.get(), m->f.get(), m->N, m->shift, m->pairs.get());
    else
        hipLaunchKernelGGL(mbar_row_kernel<MBAR_ROW_WSUM>, grid, dim3(MBAR_BLOCK), 0, m->tm.stream, m->u.get(), m->log_den.get(), m->f.get(), m->N, m->shift, m->pairs.get());
    hipLaunchKernelGGL(mbar_row_merge_kernel, dim3((unsigned)((m->K + 63) / 64)), dim3(64), 0, m->tm.stream, m->pairs.get(), m->K, chunks,
                       mode == MBAR_ROW_WSUM ? 0 : 1, mode == MBAR_ROW_SC ? -1.0 : 1.0, dst);
    DEVICE_CHECK(hipGetLastError());
    return 0;
}

// the Gram matrix of the columns `states` (the first n_plain plain weights, the rest observable-weighted) into m->gram [C][C]
static int mbar_gram_pass(remd_mbar m, const std::vector<int>& states, int n_plain)
{
    const int C = (int)states.size();
    const int T = (C + MBAR_TILE - 1) / MBAR_TILE;
    std::vector<int2> tiles;
    for (int ti = 0; ti < T; ti++) for (int tj = 0; tj <= ti; tj++) tiles.push_back(make_int2(ti, tj));
    const int64_t chunk = mbar_gram_chunk(m->N, C);
    const int chunks = (int)((m->N + chunk - 1) / chunk);
    REMD_TRY(m->col_state.grow(nullptr, C));
    REMD_TRY(m->tiles.grow(nullptr, tiles.size()));
    REMD_TRY(m->gram.grow(nullptr, (size_t)C * C));
    REMD_TRY(m->gram_partial.grow(nullptr, (size_t)chunks * C * C));
    DEVICE_CHECK(hipMemcpyAsync(m->col_state, states.data(), sizeof(int) * C, hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipMemcpyAsync(m->tiles, tiles.data(), sizeof(int2) * tiles.size(), hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipStreamSynchronize(m->tm.stream));            // (both sources are locals)
    mbar_gram_args a;
    a.u = m->u; a.log_den = m->log_den; a.f = m->f; a.log_cA = m->log_cA; a.col_state = m->col_state; a.tiles = m->tiles;
    a.C = C; a.n_plain = n_plain; a.N = m->N; a.chunk = chunk; a.shift = m->shift; a.partial = m->gram_partial;
    hipLaunchKernelGGL(mbar_gram_kernel, dim3((unsigned)tiles.size(), (unsigned)chunks), dim3(MBAR_BLOCK), 0, m->tm.stream, a);
    const int64_t entries = (int64_t)C * C;
    hipLaunchKernelGGL(mbar_gram_sum_kernel, dim3((unsigned)((entries + MBAR_BLOCK - 1) / MBAR_BLOCK)), dim3(MBAR_BLOCK), 0, m->tm.stream,
                       m->gram_partial.get(), C, chunks, m->gram.get());
    DEVICE_CHECK(hipGetLastError());
    return 0;
}

extern "C" {

int remd_mbar_create(int device, int K, int64_t N, const double* u_kn, const int64_t* N_k, remd_mbar* out)
{
    if (!out) return remd_fail(nullptr, -1, "remd_mbar_create: out is NULL");
    *out = nullptr;
    if (K < 1 || N < 1) return remd_fail(nullptr, -1, "remd_mbar_create: K and N must be at least 1");
    if (K > REMD_MBAR_MAX_STATES)
        return remd_fail(nullptr, -1, "remd_mbar_create: K = " + std::to_string(K) + " exceeds REMD_MBAR_MAX_STATES = " + std::to_string(REMD_MBAR_MAX_STATES));
    if (!u_kn || !N_k) return remd_fail(nullptr, -1, "remd_mbar_create: u_kn or N_k is NULL");
    int64_t total = 0;
    for (int k = 0; k < K; k++) {
        if (N_k[k] < 0 || N_k[k] > N) return remd_fail(nullptr, -1, "remd_mbar_create: N_k[" + std::to_string(k) + "] is negative or above N");
        total += N_k[k];
    }
    if (total != N) return remd_fail(nullptr, -1, "remd_mbar_create: sum N_k = " + std::to_string(total) + " is not N = " + std::to_string(N));
    double umin = std::numeric_limits<double>::infinity();
    bool has_nan = false;
    for (int k = 0; k < K; k++) {
        const double* row = u_kn + (int64_t)k * N;
        for (int64_t n = 0; n < N; n++) {
            if (N_k[k] > 0 && !std::isfinite(row[n]))
                return remd_fail(nullptr, -1, "remd_mbar_create: non-finite u_kn in sampled state " + std::to_string(k));
            if (row[n] != row[n]) has_nan = true;
            if (row[n] < umin) umin = row[n];
        }
    }
    REMD_TRY(select_device("remd_mbar_create", device));
    std::unique_ptr<remd_mbar_ctx> m(new remd_mbar_ctx());
    m->K = K; m->N = N;
    m->shift = (has_nan ? std::numeric_limits<double>::quiet_NaN() : umin) - 1.0;      // np.min keeps a NaN
    std::vector<double> nk;
    m->nk_all.resize(K);
    for (int k = 0; k < K; k++) {
        m->nk_all[k] = (double)N_k[k];
        if (N_k[k] > 0) { m->srow.push_back(k); nk.push_back((double)N_k[k]); }
    }
    m->Ks = (int)m->srow.size();
    REMD_TRY(m->tm.open(device));
    REMD_TRY(m->u.alloc(nullptr, (size_t)K * N));
    DEVICE_CHECK(hipMemcpy(m->u, u_kn, sizeof(double) * (size_t)K * N, hipMemcpyHostToDevice));
    REMD_TRY(m->nk.upload(nullptr, nk));
    REMD_TRY(m->d_srow.upload(nullptr, m->srow));
    REMD_TRY(m->fs.alloc(nullptr, m->Ks));
    REMD_TRY(m->f.alloc(nullptr, K));
    REMD_TRY(m->log_den.alloc(nullptr, N));
    REMD_TRY(m->col_partial.alloc(nullptr, (size_t)((N + MBAR_BLOCK - 1) / MBAR_BLOCK)));
    REMD_TRY(m->scalar.alloc(nullptr, 1));
    REMD_TRY(m->row_out.alloc(nullptr, K));
    REMD_TRY(m->log_cA.alloc(nullptr, K));
    REMD_TRY(m->pairs.alloc(nullptr, (size_t)K * (size_t)((N + MBAR_ROW_CHUNK - 1) / MBAR_ROW_CHUNK)));
    *out = m.release();
    return 0;
}

void remd_mbar_destroy(remd_mbar m) { delete m; }

int remd_mbar_log_denominator(remd_mbar m, const double* f_k, double* log_den, double* phi)
{
    REMD_TRY(mbar_begin(m, "remd_mbar_log_denominator", f_k));
    REMD_TRY(mbar_column_pass(m));
    REMD_TRY(mbar_end(m));
    if (log_den) DEVICE_CHECK(hipMemcpy(log_den, m->log_den, sizeof(double) * m->N, hipMemcpyDeviceToHost));
    if (phi) REMD_TRY(mbar_phi(m, f_k, phi));
    return 0;
}

int remd_mbar_self_consistent(remd_mbar m, const double* f_k, double* f_new)
{
    REMD_TRY(mbar_begin(m, "remd_mbar_self_consistent", f_k, f_new));
    REMD_TRY(mbar_column_pass(m));
    REMD_TRY(mbar_row_pass(m, MBAR_ROW_SC, m->row_out));
    REMD_TRY(mbar_end(m));
    DEVICE_CHECK(hipMemcpy(f_new, m->row_out, sizeof(double) * m->K, hipMemcpyDeviceToHost));
    return 0;
}

int remd_mbar_newton_parts(remd_mbar m, const double* f_k, double* W_sum, double* gram, double* phi)
{
    REMD_TRY(mbar_begin(m, "remd_mbar_newton_parts", f_k, W_sum, gram));
    REMD_TRY(mbar_column_pass(m));
    REMD_TRY(mbar_row_pass(m, MBAR_ROW_WSUM, m->row_out));
    REMD_TRY(mbar_gram_pass(m, m->srow, m->Ks));
    REMD_TRY(mbar_end(m));
    const int K = m->K, Ks = m->Ks;
    std::vector<double> ws(K), g((size_t)Ks * Ks);
    DEVICE_CHECK(hipMemcpy(ws.data(), m->row_out, sizeof(double) * K, hipMemcpyDeviceToHost));
    DEVICE_CHECK(hipMemcpy(g.data(), m->gram, sizeof(double) * g.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < K; k++) W_sum[k] = 0.0;
    for (int64_t i = 0; i < (int64_t)K * K; i++) gram[i] = 0.0;
    for (int a = 0; a < Ks; a++) {
        W_sum[m->srow[a]] = ws[m->srow[a]];
        for (int b = 0; b < Ks; b++) gram[(int64_t)m->srow[a] * K + m->srow[b]] = g[(size_t)a * Ks + b];
    }
    if (phi) REMD_TRY(mbar_phi(m, f_k, phi));
    return 0;
}

int remd_mbar_gram(remd_mbar m, const double* f_k, int with_observable, double* gram, double* log_cA)
{
    REMD_TRY(mbar_begin(m, "remd_mbar_gram", f_k, gram));
    const int K = m->K, C = with_observable ? 2 * K : K;
    std::vector<int> states(C);
    for (int c = 0; c < C; c++) states[c] = c % K;
    REMD_TRY(mbar_column_pass(m));
    if (with_observable) REMD_TRY(mbar_row_pass(m, MBAR_ROW_LOGCA, m->log_cA));
    REMD_TRY(mbar_gram_pass(m, states, K));
    REMD_TRY(mbar_end(m));
    DEVICE_CHECK(hipMemcpy(gram, m->gram, sizeof(double) * (size_t)C * C, hipMemcpyDeviceToHost));
    if (with_observable && log_cA) DEVICE_CHECK(hipMemcpy(log_cA, m->log_cA, sizeof(double) * K, hipMemcpyDeviceToHost));
    return 0;
}

int remd_mbar_augmented_gram(remd_mbar m, const double* f_k, int L, const double* u_ln, int I, const double* A_in, const int32_t* obs_state,
                             double* f_l, double* log_cA, double* gram)
{
    const std::string who = "remd_mbar_augmented_gram";
    if (!m) return remd_fail(nullptr, -1, who + ": the problem is NULL");
    if (L < 0 || I < 0) return remd_fail(nullptr, -1, who + ": L = " + std::to_string(L) + " or I = " + std::to_string(I) + " is negative");
    if (L == 0 && I == 0) return remd_fail(nullptr, -1, who + ": L and I are both 0 (remd_mbar_gram gives the plain Gram matrix)");
    const int K = m->K;
    const int64_t N = m->N, C64 = (int64_t)K + L + I;
    if (C64 > 2 * REMD_MBAR_MAX_STATES)
        return remd_fail(nullptr, -1, who + ": C = K + L + I = " + std::to_string(C64) + " exceeds 2 x REMD_MBAR_MAX_STATES = " + std::to_string(2 * REMD_MBAR_MAX_STATES));
    const int C = (int)C64;
    if ((L > 0 && (!u_ln || !f_l)) || (I > 0 && (!A_in || !obs_state || !log_cA)))
        return remd_fail(nullptr, -1, who + ": an array of a non-zero count is NULL");
    for (int l = 0; l < L; l++)
        for (int64_t n = 0; n < N; n++) {
            const double v = u_ln[(int64_t)l * N + n];
            if (v != v || v == -std::numeric_limits<double>::infinity())
                return remd_fail(nullptr, -1, who + ": u_ln of perturbed state " + std::to_string(l) + " holds a NaN or -inf");
        }
    for (int i = 0; i < I; i++) {
        if (obs_state[i] < 0 || obs_state[i] >= K + L)
            return remd_fail(nullptr, -1, who + ": obs_state[" + std::to_string(i) + "] = " + std::to_string(obs_state[i]) + " is outside 0 ... " + std::to_string(K + L - 1));
        for (int64_t n = 0; n < N; n++) {
            const double v = A_in[(int64_t)i * N + n];
            if (!(v > 0.0) || !std::isfinite(v))
                return remd_fail(nullptr, -1, who + ": A_in of observable " + std::to_string(i) + " holds a non-positive or non-finite value");
        }
    }
    if (!f_k) return remd_fail(nullptr, -1, who + ": f_k is NULL");
    if (!gram) return remd_fail(nullptr, -1, who + ": an output array is NULL");
    DEVICE_CHECK(hipSetDevice(m->tm.device));
    // the arrays of this call: freed when it returns
    const int row_chunks = (int)((N + MBAR_ROW_CHUNK - 1) / MBAR_ROW_CHUNK);
    dev_array<double> d_u_ln, d_A, d_f, d_log_cA;
    dev_array<int> d_obs;
    dev_array<double2> d_pairs;
    REMD_TRY(d_u_ln.alloc(nullptr, (size_t)L * N));
    REMD_TRY(d_A.alloc(nullptr, (size_t)I * N));
    REMD_TRY(d_f.alloc(nullptr, (size_t)K + L));
    REMD_TRY(d_log_cA.alloc(nullptr, (size_t)I));
    REMD_TRY(d_obs.alloc(nullptr, (size_t)I));
    REMD_TRY(d_pairs.alloc(nullptr, (size_t)std::max(L, I) * row_chunks));
    if (L) DEVICE_CHECK(hipMemcpy(d_u_ln, u_ln, sizeof(double) * (size_t)L * N, hipMemcpyHostToDevice));
    if (I) DEVICE_CHECK(hipMemcpy(d_A, A_in, sizeof(double) * (size_t)I * N, hipMemcpyHostToDevice));
    if (I) DEVICE_CHECK(hipMemcpy(d_obs, obs_state, sizeof(int) * (size_t)I, hipMemcpyHostToDevice));
    DEVICE_CHECK(hipMemset(d_f, 0, sizeof(double) * ((size_t)K + L)));
    DEVICE_CHECK(hipMemcpy(d_f, f_k, sizeof(double) * K, hipMemcpyHostToDevice));
    REMD_TRY(mbar_begin(m, who.c_str(), f_k));
    REMD_TRY(mbar_column_pass(m));
    std::vector<double> fl(L);
    if (L) {                                                 // eq. 11 on the rows of u_ln, into f[K ...]
        hipLaunchKernelGGL(mbar_row_kernel<MBAR_ROW_SC>, dim3((unsigned)row_chunks, (unsigned)L), dim3(MBAR_BLOCK), 0, m->tm.stream, d_u_ln.get(),
                           m->log_den.get(), d_f.get(), N, 0.0, d_pairs.get());
        hipLaunchKernelGGL(mbar_row_merge_kernel, dim3((unsigned)((L + 63) / 64)), dim3(64), 0, m->tm.stream, d_pairs.get(), L, row_chunks, 1, -1.0,
                           d_f.get() + K);
        DEVICE_CHECK(hipGetLastError());
        DEVICE_CHECK(hipMemcpyAsync(fl.data(), d_f.get() + K, sizeof(double) * L, hipMemcpyDeviceToHost, m->tm.stream));
        DEVICE_CHECK(hipStreamSynchronize(m->tm.stream));
        for (int l = 0; l < L; l++)
            if (!std::isfinite(fl[l])) {
                REMD_TRY(mbar_end(m));                       // (remd_mbar_last_ms then reports the passes this call did run)
                return remd_fail(nullptr, -1, who + ": perturbed state " + std::to_string(l) + " has no sample with a non-zero weight");
            }
    }
    if (I) {
        hipLaunchKernelGGL(mbar_aug_logca_kernel, dim3((unsigned)row_chunks, (unsigned)I), dim3(MBAR_BLOCK), 0, m->tm.stream, m->u.get(), d_u_ln.get(),
                           d_A.get(), m->log_den.get(), d_f.get(), d_obs.get(), K, N, d_pairs.get());
        hipLaunchKernelGGL(mbar_row_merge_kernel, dim3((unsigned)((I + 63) / 64)), dim3(64), 0, m->tm.stream, d_pairs.get(), I, row_chunks, 1, 1.0,
                           d_log_cA.get());
        DEVICE_CHECK(hipGetLastError());
    }
    const int T = (C + MBAR_TILE - 1) / MBAR_TILE;
    std::vector<int2> tiles;
    for (int ti = 0; ti < T; ti++) for (int tj = 0; tj <= ti; tj++) tiles.push_back(make_int2(ti, tj));
    const int64_t chunk = mbar_gram_chunk(N, C);
    const int chunks = (int)((N + chunk - 1) / chunk);
    REMD_TRY(m->tiles.grow(nullptr, tiles.size()));
    REMD_TRY(m->gram.grow(nullptr, (size_t)C * C));
    REMD_TRY(m->gram_partial.grow(nullptr, (size_t)chunks * C * C));
    DEVICE_CHECK(hipMemcpyAsync(m->tiles, tiles.data(), sizeof(int2) * tiles.size(), hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipStreamSynchronize(m->tm.stream));            // (the source is a local)
    mbar_aug_args a;
    a.u = m->u; a.u_ln = d_u_ln; a.A = d_A; a.log_den = m->log_den; a.f = d_f; a.log_cA = d_log_cA; a.obs_state = d_obs; a.tiles = m->tiles;
    a.K = K; a.L = L; a.C = C; a.N = N; a.chunk = chunk; a.partial = m->gram_partial;
    hipLaunchKernelGGL(mbar_aug_gram_kernel, dim3((unsigned)tiles.size(), (unsigned)chunks), dim3(MBAR_BLOCK), 0, m->tm.stream, a);
    const int64_t entries = (int64_t)C * C;
    hipLaunchKernelGGL(mbar_gram_sum_kernel, dim3((unsigned)((entries + MBAR_BLOCK - 1) / MBAR_BLOCK)), dim3(MBAR_BLOCK), 0, m->tm.stream,
                       m->gram_partial.get(), C, chunks, m->gram.get());
    DEVICE_CHECK(hipGetLastError());
    REMD_TRY(mbar_end(m));
    DEVICE_CHECK(hipMemcpy(gram, m->gram, sizeof(double) * (size_t)C * C, hipMemcpyDeviceToHost));
    for (int l = 0; l < L; l++) f_l[l] = fl[l];
    if (I) DEVICE_CHECK(hipMemcpy(log_cA, d_log_cA, sizeof(double) * I, hipMemcpyDeviceToHost));
    return 0;
}

int remd_mbar_log_weights(remd_mbar m, const double* f_k, double* log_W_nk)
{
    REMD_TRY(mbar_begin(m, "remd_mbar_log_weights", f_k, log_W_nk));
    REMD_TRY(m->weights.grow(nullptr, (size_t)m->N * m->K));
    REMD_TRY(mbar_column_pass(m));
    hipLaunchKernelGGL(mbar_log_weights_kernel, dim3((unsigned)((m->N + 15) / 16), (unsigned)((m->K + 15) / 16)), dim3(MBAR_BLOCK), 0, m->tm.stream,
                       m->u.get(), m->log_den.get(), m->f.get(), m->K, m->N, m->weights.get());
    DEVICE_CHECK(hipGetLastError());
    REMD_TRY(mbar_end(m));
    DEVICE_CHECK(hipMemcpy(log_W_nk, m->weights, sizeof(double) * (size_t)m->N * m->K, hipMemcpyDeviceToHost));
    return 0;
}

int remd_mbar_chunks(remd_mbar m, int C, int64_t* column_chunk, int64_t* row_chunk, int64_t* gram_chunk)
{
    if (!m || C < 1) return remd_fail(nullptr, -1, "remd_mbar_chunks: the problem is NULL or C < 1");
    if (column_chunk) *column_chunk = MBAR_BLOCK;
    if (row_chunk) *row_chunk = MBAR_ROW_CHUNK;
    if (gram_chunk) *gram_chunk = mbar_gram_chunk(m->N, C);
    return 0;
}

int remd_mbar_last_ms(remd_mbar m, double* ms)
{
    if (!m || !ms) return remd_fail(nullptr, -1, "remd_mbar_last_ms: the problem or ms is NULL");
    if (!m->timed) return remd_fail(nullptr, -1, "remd_mbar_last_ms: no pass has run on this problem yet");
    *ms = m->tm.ms;
    return 0;
}

}
