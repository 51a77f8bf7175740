// Bootstrap replicates of an MBAR problem on the device (include/remd_hip_mbar.h, remd_mbar_bootstrap_*).  A replicate is a vector of
// integer multiplicities c_n over the N stored samples, drawn per sampled state with Philox (REMD_STREAM_BOOTSTRAP of rng.h) and
// accumulated with integer atomics; every pass of mbar.hip is restated with c_n as the weight of sample n, for a batch of replicates
// each at its own f_b[K].  All f64, no floating-point atomics; the replicate is a grid dimension of every kernel.
//
//   draw         one thread per Philox call (two draws) of (replicate, sampled state)
//   column pass  one thread per sample and MBAR_BOOT_RB replicates: u[k][n] is loaded once for the group, whose f_b lie in LDS;
//                sum_n c_n log_den_n per workgroup and replicate, then a fixed-order second stage per replicate
//   row pass     workgroups per (chunk of samples, row, group of MBAR_BOOT_RB replicates): each u (and ln A) is loaded once for the
//                group, whose f_b are in registers; a (max, scaled sum) pair per (replicate, row, chunk) over the samples with
//                c_n > 0, merged by mbar_row_merge_kernel in chunk order
//   Gram pass    workgroups per (tile of the lower triangle, chunk of samples, replicate): the samples with c_n > 0 of a slab of 256
//                are compacted into LDS in ascending order (a ballot and a prefix count), then staged 16 at a time: c_n W_in in one
//                operand, W_jn in the other, accumulated in mbar.hip's 4 x 4 register tile
//
// A replicate's numbers are set by (K, N, seed, replicate) alone: the chunks do not depend on the batch, a replicate never shares
// a sum with another, and every sum has one fixed order.
#include "mbar_ctx.h"
#include "rng.h"
#include <cmath>
#include <limits>
#include <algorithm>

#define MBAR_BOOT_RB            4                         // replicates that share one load of u in the column and row passes
#define MBAR_BOOT_SLAB          256                       // samples compacted at a time in the Gram pass
#define MBAR_BOOT_GRAM_CHUNKS   32                        // chunks of the Gram pass at most: the replicates fill the device
#define MBAR_BOOT_PARTIAL_CAP   (int64_t(1) << 25)        // doubles of Gram partials per launch at most (256 MiB)

// ---- draw -----------------------------------------------------------------------------------------------------------------------
// grid (Philox calls of the largest state / 256, Ks, nb): draw j = 2a, 2a + 1 of state srow[y] for replicate b0 + z
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_boot_draw_kernel(uint64_t seed, const int* __restrict__ srow, const int* __restrict__ state_start,
                                                                    const int* __restrict__ state_samples, int64_t N, int b0,
                                                                    uint32_t* __restrict__ counts)
{
    const int j = blockIdx.y;
    const int start = state_start[j];
    const uint64_t nk = (uint64_t)(state_start[j + 1] - start);
    const uint64_t a = (uint64_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (2 * a >= nk) return;
    const philox4 w = remd_philox(seed, REMD_STREAM_BOOTSTRAP, (uint32_t)a, (uint32_t)srow[j], (uint64_t)(b0 + (int)blockIdx.z));
    uint32_t* __restrict__ c = counts + (int64_t)blockIdx.z * N;
    const uint64_t x0 = ((uint64_t)w.w[0] << 32) | w.w[1];
    atomicAdd(&c[state_samples[start + (int)__umul64hi(x0, nk)]], 1u);       // floor(x nk / 2^64) < nk
    if (2 * a + 1 < nk) {
        const uint64_t x1 = ((uint64_t)w.w[2] << 32) | w.w[3];
        atomicAdd(&c[state_samples[start + (int)__umul64hi(x1, nk)]], 1u);
    }
}

// ---- column pass ----------------------------------------------------------------------------------------------------------------
// grid (samples / 256, groups of MBAR_BOOT_RB replicates); LDS: the f of the group over the sampled states, [MBAR_BOOT_RB][Ks].
// log_den[r][n] at f[r][.], partial[r][block] = sum over the block of c_n log_den_n
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_boot_logden_kernel(const double* __restrict__ u, const double* __restrict__ f,
                                                                      const double* __restrict__ nk, const int* __restrict__ srow, int Ks, int K,
                                                                      int64_t N, const int* __restrict__ reps, int nr, int b0,
                                                                      const uint32_t* __restrict__ counts, double* __restrict__ log_den,
                                                                      double* __restrict__ partial)
{
    extern __shared__ double fsh[];
    __shared__ double sh[4];
    const int r0 = blockIdx.y * MBAR_BOOT_RB;
    for (int i = threadIdx.x; i < MBAR_BOOT_RB * Ks; i += MBAR_BLOCK) {
        const int q = i / Ks, j = i - q * Ks;
        fsh[i] = r0 + q < nr ? f[(int64_t)(r0 + q) * K + srow[j]] : 0.0;
    }
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    double m[MBAR_BOOT_RB], s[MBAR_BOOT_RB];
    #pragma unroll
    for (int q = 0; q < MBAR_BOOT_RB; q++) { m[q] = -INFINITY; s[q] = 0.0; }
    if (n < N) {
        for (int j = 0; j < Ks; j++) {
            const double uu = u[(int64_t)srow[j] * N + n];
            #pragma unroll
            for (int q = 0; q < MBAR_BOOT_RB; q++) m[q] = nanmax(m[q], fsh[q * Ks + j] - uu);
        }
        #pragma unroll
        for (int q = 0; q < MBAR_BOOT_RB; q++) m[q] = mbar_guard(m[q]);
        for (int j = 0; j < Ks; j++) {
            const double uu = u[(int64_t)srow[j] * N + n], w = nk[j];
            #pragma unroll
            for (int q = 0; q < MBAR_BOOT_RB; q++) s[q] += w * exp((fsh[q * Ks + j] - uu) - m[q]);
        }
    }
    #pragma unroll
    for (int q = 0; q < MBAR_BOOT_RB; q++) {
        const int r = r0 + q;
        if (r >= nr) break;                                               // (the same for every thread of the workgroup)
        double term = 0.0;
        if (n < N) {
            const double ld = log(s[q]) + m[q];
            log_den[(int64_t)r * N + n] = ld;
            const uint32_t c = counts[(int64_t)(reps[r] - b0) * N + n];
            if (c) term = (double)c * ld;
        }
        const double t = block_sum(term, sh);
        if (threadIdx.x == 0) partial[(int64_t)r * gridDim.x + blockIdx.x] = t;
    }
}

// grid (nr): out[r] = the sum of partial[r][.] in mbar_sum_kernel's order
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_boot_sum_kernel(const double* __restrict__ partial, int64_t n, double* __restrict__ out)
{
    __shared__ double sh[4];
    const double* __restrict__ p = partial + (int64_t)blockIdx.x * n;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += MBAR_BLOCK) s += p[i];
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// ---- row pass -------------------------------------------------------------------------------------------------------------------
// Row `row` of a pass is state s = row_state[row]: s < K a row of u, else row s - K of u_ln.  Its term at sample n for replicate r is
//   (f[r][s] - u_sn) - log_den[r][n]  (+ ln A[row][n] where A is given; f = NULL counts as 0: eq. 11)
// and its weight c_n of r.  pairs[(r * R + row) * chunks + chunk] = (max over c_n > 0, sum c_n exp(term - guarded max)), or with
// USE_MAX false (0, sum c_n exp(term)).
struct mbar_boot_row_args {
    const double* u; const double* u_ln; const double* A; const double* log_den; const double* f;
    const int* row_state; const int* reps; const uint32_t* counts;
    int K, R, nr, b0, fstride;
    int64_t N;
    double2* pairs;
};

// grid (chunks, R, groups of MBAR_BOOT_RB replicates)
template <bool USE_MAX>
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_boot_row_kernel(mbar_boot_row_args a)
{
    __shared__ double sh[4];
    const int row = blockIdx.y, s = a.row_state[row];
    const int64_t N = a.N;
    const int64_t n0 = (int64_t)blockIdx.x * MBAR_ROW_CHUNK;
    const int64_t n1 = n0 + MBAR_ROW_CHUNK < N ? n0 + MBAR_ROW_CHUNK : N;
    const double* __restrict__ us = s < a.K ? a.u + (int64_t)s * N : a.u_ln + (int64_t)(s - a.K) * N;
    const double* __restrict__ Ar = a.A ? a.A + (int64_t)row * N : nullptr;
    const int r0 = blockIdx.z * MBAR_BOOT_RB;
    double fq[MBAR_BOOT_RB];
    const double* ldq[MBAR_BOOT_RB];
    const uint32_t* cq[MBAR_BOOT_RB];
    #pragma unroll
    for (int q = 0; q < MBAR_BOOT_RB; q++) {
        const int r = r0 + q < a.nr ? r0 + q : a.nr - 1;                  // (a slot past the batch repeats the last replicate; not written)
        fq[q] = a.f ? a.f[(int64_t)r * a.fstride + s] : 0.0;
        ldq[q] = a.log_den + (int64_t)r * N;
        cq[q] = a.counts + (int64_t)(a.reps[r] - a.b0) * N;
    }
    double mraw[MBAR_BOOT_RB], m[MBAR_BOOT_RB], sum[MBAR_BOOT_RB];
    #pragma unroll
    for (int q = 0; q < MBAR_BOOT_RB; q++) { mraw[q] = 0.0; m[q] = 0.0; sum[q] = 0.0; }
    if (USE_MAX) {
        double mt[MBAR_BOOT_RB];
        #pragma unroll
        for (int q = 0; q < MBAR_BOOT_RB; q++) mt[q] = -INFINITY;
        for (int64_t n = n0 + threadIdx.x; n < n1; n += MBAR_BLOCK) {
            const double uu = us[n], la = Ar ? log(Ar[n]) : 0.0;
            #pragma unroll
            for (int q = 0; q < MBAR_BOOT_RB; q++)
                if (cq[q][n]) {
                    double t = (fq[q] - uu) - ldq[q][n];
                    if (Ar) t += la;
                    mt[q] = nanmax(mt[q], t);
                }
        }
        #pragma unroll
        for (int q = 0; q < MBAR_BOOT_RB; q++) { mraw[q] = block_nanmax(mt[q], sh); m[q] = mbar_guard(mraw[q]); }
    }
    for (int64_t n = n0 + threadIdx.x; n < n1; n += MBAR_BLOCK) {
        const double uu = us[n], la = Ar ? log(Ar[n]) : 0.0;
        #pragma unroll
        for (int q = 0; q < MBAR_BOOT_RB; q++) {
            const uint32_t c = cq[q][n];
            if (c) {
                double t = (fq[q] - uu) - ldq[q][n];
                if (Ar) t += la;
                sum[q] += (double)c * exp(t - m[q]);
            }
        }
    }
    #pragma unroll
    for (int q = 0; q < MBAR_BOOT_RB; q++) {
        const double t = block_sum(sum[q], sh);
        if (threadIdx.x == 0 && r0 + q < a.nr)
            a.pairs[((int64_t)(r0 + q) * a.R + row) * gridDim.x + blockIdx.x] = make_double2(mraw[q], t);
    }
}

// ---- Gram pass ------------------------------------------------------------------------------------------------------------------
struct mbar_boot_gram_args {
    const double* u; const double* log_den; const double* f;
    const int* srow; const int2* tiles; const int* reps; const uint32_t* counts;
    int Ks, K, b0, r_first;
    int64_t N, chunk;
    double* partial;             // [replicates of the launch][chunks][Ks][Ks], the lower triangle's tiles
};

// grid (tiles, chunks, replicates of the launch)
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_boot_gram_kernel(mbar_boot_gram_args a)
{
    __shared__ double As[MBAR_TSTEP][MBAR_LDS_STRIDE];
    __shared__ double Bs[MBAR_TSTEP][MBAR_LDS_STRIDE];
    __shared__ int list_n[MBAR_BOOT_SLAB];                        // the samples of the slab with c_n > 0, ascending (offset in the slab)
    __shared__ uint32_t list_c[MBAR_BOOT_SLAB];
    __shared__ int wave_count[4];
    const int2 tile = a.tiles[blockIdx.x];
    const int i0 = tile.x * MBAR_TILE, j0 = tile.y * MBAR_TILE;
    const int64_t N = a.N;
    const int64_t n0 = (int64_t)blockIdx.y * a.chunk;
    const int64_t n1 = n0 + a.chunk < N ? n0 + a.chunk : N;
    const int r = a.r_first + blockIdx.z;
    const uint32_t* __restrict__ cnt = a.counts + (int64_t)(a.reps[r] - a.b0) * N;
    const double* __restrict__ ld = a.log_den + (int64_t)r * N;
    const double* __restrict__ f = a.f + (int64_t)r * a.K;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int fs = t & (MBAR_TSTEP - 1), fc = t >> 4;             // the list entry and the first column this thread stages
    const int lane = t & 63, wave = t >> 6;
    int ka[4], kb[4];                                             // the rows of u of the columns this thread stages (-1: past Ks)
    double fa[4], fb[4];
    #pragma unroll
    for (int p = 0; p < 4; p++) {
        const int ci = i0 + fc + 16 * p, cj = j0 + fc + 16 * p;
        ka[p] = ci < a.Ks ? a.srow[ci] : -1;
        kb[p] = cj < a.Ks ? a.srow[cj] : -1;
        fa[p] = ka[p] >= 0 ? f[ka[p]] : 0.0;
        fb[p] = kb[p] >= 0 ? f[kb[p]] : 0.0;
    }
    double acc[4][4];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    for (int64_t slab = n0; slab < n1; slab += MBAR_BOOT_SLAB) {
        const int64_t nt = slab + t;
        const uint32_t cn = nt < n1 ? cnt[nt] : 0u;
        const unsigned long long ballot = __ballot(cn != 0u);
        if (lane == 0) wave_count[wave] = __popcll(ballot);
        __syncthreads();
        int base = 0, total = 0;
        #pragma unroll
        for (int w = 0; w < 4; w++) { if (w < wave) base += wave_count[w]; total += wave_count[w]; }
        if (cn) {
            const int at = base + __popcll(ballot & ((1ull << lane) - 1ull));
            list_n[at] = t;
            list_c[at] = cn;
        }
        __syncthreads();
        for (int e0 = 0; e0 < total; e0 += MBAR_TSTEP) {
            const int e = e0 + fs;
            const bool valid = e < total;
            const int64_t n = valid ? slab + list_n[e] : slab;
            const double w = valid ? (double)list_c[e] : 0.0;
            const double ldn = valid ? ld[n] : 0.0;
            #pragma unroll
            for (int p = 0; p < 4; p++) {
                const int cl = fc + 16 * p;
                As[fs][cl] = (valid && ka[p] >= 0) ? w * exp((fa[p] - a.u[(int64_t)ka[p] * N + n]) - ldn) : 0.0;
                Bs[fs][cl] = (valid && kb[p] >= 0) ? exp((fb[p] - a.u[(int64_t)kb[p] * N + n]) - ldn) : 0.0;
            }
            __syncthreads();
            #pragma unroll
            for (int s = 0; s < MBAR_TSTEP; s++) {
                double av[4], bv[4];
                #pragma unroll
                for (int i = 0; i < 4; i++) { av[i] = As[s][ty * 4 + i]; bv[i] = Bs[s][tx * 4 + i]; }
                #pragma unroll
                for (int i = 0; i < 4; i++)
                    #pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
            }
            __syncthreads();
        }
    }
    double* out = a.partial + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * a.Ks * a.Ks;
    for (int i = 0; i < 4; i++) {
        const int gi = i0 + ty * 4 + i;
        if (gi >= a.Ks) continue;
        for (int j = 0; j < 4; j++) {
            const int gj = j0 + tx * 4 + j;
            if (gj < a.Ks) out[(int64_t)gi * a.Ks + gj] = acc[i][j];
        }
    }
}

// grid (entries / 256, replicates of the launch): the lower triangle of a replicate's partials summed in chunk order, both halves written
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_boot_gram_sum_kernel(const double* __restrict__ partial, int C, int chunks, double* __restrict__ gram)
{
    const int64_t idx = (int64_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (idx >= (int64_t)C * C) return;
    const int i = (int)(idx / C), j = (int)(idx % C);
    if (j > i) return;
    const double* __restrict__ p = partial + (int64_t)blockIdx.y * chunks * C * C;
    double* __restrict__ g = gram + (int64_t)blockIdx.y * C * C;
    double s = 0.0;
    for (int c = 0; c < chunks; c++) s += p[(int64_t)c * C * C + idx];
    g[(int64_t)i * C + j] = s;
    g[(int64_t)j * C + i] = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static int boot_max_batch(const remd_mbar_ctx* m)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(REMD_MBAR_BOOTSTRAP_MAX_BATCH, REMD_MBAR_BOOTSTRAP_BATCH_ELEMENTS / m->N));
}

// samples per workgroup of the weighted Gram pass: set by N alone
static int64_t boot_gram_chunk(int64_t N)
{
    int64_t chunk = (N + MBAR_BOOT_GRAM_CHUNKS - 1) / MBAR_BOOT_GRAM_CHUNKS;
    chunk = (chunk + MBAR_BOOT_SLAB - 1) / MBAR_BOOT_SLAB * MBAR_BOOT_SLAB;
    return std::max<int64_t>(MBAR_BOOT_SLAB, chunk);
}

// checks a batched call, uploads reps[nr] and f_b[nr][K], sizes log_den[nr][N] and starts the clock
int boot_begin(remd_mbar m, const std::string& who, int nr, const int32_t* reps, const double* f_b)
{
    if (!m) return remd_fail(nullptr, -1, who + ": the problem is NULL");
    if (nr < 1) return remd_fail(nullptr, -1, who + ": nb = " + std::to_string(nr) + " replicates; at least 1 is needed");
    if (!reps || !f_b) return remd_fail(nullptr, -1, who + ": reps or f_b is NULL");
    mbar_bootstrap_state& b = m->boot;
    if (b.nb < 1) return remd_fail(nullptr, -1, who + ": no replicate has been drawn (remd_mbar_bootstrap_draw)");
    if (nr > b.nb) return remd_fail(nullptr, -1, who + ": " + std::to_string(nr) + " replicates asked of the " + std::to_string(b.nb) + " drawn");
    for (int i = 0; i < nr; i++)
        if (reps[i] < b.b0 || reps[i] >= b.b0 + b.nb)
            return remd_fail(nullptr, -1, who + ": replicate " + std::to_string(reps[i]) + " is outside the drawn range " + std::to_string(b.b0) +
                                          " ... " + std::to_string(b.b0 + b.nb - 1));
    for (int64_t i = 0; i < (int64_t)nr * m->K; i++)
        if (!std::isfinite(f_b[i]))
            return remd_fail(nullptr, -1, who + ": f_b of replicate " + std::to_string(reps[i / m->K]) + " holds a non-finite value");
    DEVICE_CHECK(hipSetDevice(m->tm.device));
    REMD_TRY(b.reps.grow(nullptr, (size_t)nr));
    REMD_TRY(b.f.grow(nullptr, (size_t)nr * m->K));
    REMD_TRY(b.log_den.grow(nullptr, (size_t)nr * m->N));
    REMD_TRY(b.col_partial.grow(nullptr, (size_t)nr * (size_t)((m->N + MBAR_BLOCK - 1) / MBAR_BLOCK)));
    REMD_TRY(b.phi_sum.grow(nullptr, (size_t)nr));
    DEVICE_CHECK(hipMemcpyAsync(b.reps, reps, sizeof(int) * nr, hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipMemcpyAsync(b.f, f_b, sizeof(double) * (size_t)nr * m->K, hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipStreamSynchronize(m->tm.stream));
    m->tm.ms = 0.0;
    return m->tm.begin();
}

int boot_end(remd_mbar m)
{
    REMD_TRY(m->tm.end());
    m->timed = true;
    return 0;
}

// log_den[nr][N] on the device, sum_n c_n log_den_n per replicate in phi_sum[nr]
int boot_column_pass(remd_mbar m, int nr)
{
    mbar_bootstrap_state& b = m->boot;
    const int64_t blocks = (m->N + MBAR_BLOCK - 1) / MBAR_BLOCK;
    const int groups = (nr + MBAR_BOOT_RB - 1) / MBAR_BOOT_RB;
    hipLaunchKernelGGL(mbar_boot_logden_kernel, dim3((unsigned)blocks, (unsigned)groups), dim3(MBAR_BLOCK), sizeof(double) * MBAR_BOOT_RB * m->Ks,
                       m->tm.stream, m->u.get(), b.f.get(), m->nk.get(), m->d_srow.get(), m->Ks, m->K, m->N, b.reps.get(), nr, b.b0, b.counts.get(),
                       b.log_den.get(), b.col_partial.get());
    hipLaunchKernelGGL(mbar_boot_sum_kernel, dim3((unsigned)nr), dim3(MBAR_BLOCK), 0, m->tm.stream, b.col_partial.get(), blocks, b.phi_sum.get());
    DEVICE_CHECK(hipGetLastError());
    return 0;
}

// phi[r] = sum_n c_n log_den_n - sum_k N_k f_k
static int boot_phi(remd_mbar m, int nr, const double* f_b, double* phi)
{
    std::vector<double> sum(nr);
    DEVICE_CHECK(hipMemcpy(sum.data(), m->boot.phi_sum, sizeof(double) * nr, hipMemcpyDeviceToHost));
    for (int r = 0; r < nr; r++) {
        double dot = 0.0;
        for (int j = 0; j < m->Ks; j++) dot += m->nk_all[m->srow[j]] * f_b[(int64_t)r * m->K + m->srow[j]];
        phi[r] = sum[r] - dot;
    }
    return 0;
}

// One row pass over `states` (R rows) for nr replicates into row_out[nr][R].  f: [nr][fstride] on the device or NULL; u_ln, A: device
// arrays of the call or NULL.  as_log: sign * ln of the weighted sum, else the sum itself (no maximum is taken).
static int boot_row_pass(remd_mbar m, int nr, const std::vector<int>& states, const double* f, int fstride, const double* u_ln, const double* A,
                         bool as_log, double sign)
{
    mbar_bootstrap_state& b = m->boot;
    const int R = (int)states.size();
    const int chunks = (int)((m->N + MBAR_ROW_CHUNK - 1) / MBAR_ROW_CHUNK);
    REMD_TRY(b.row_state.grow(nullptr, (size_t)R));
    REMD_TRY(b.pairs.grow(nullptr, (size_t)nr * R * chunks));
    REMD_TRY(b.row_out.grow(nullptr, (size_t)nr * R));
    DEVICE_CHECK(hipMemcpyAsync(b.row_state, states.data(), sizeof(int) * R, hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipStreamSynchronize(m->tm.stream));            // (the source may be a local)
    mbar_boot_row_args a;
    a.u = m->u; a.u_ln = u_ln; a.A = A; a.log_den = b.log_den; a.f = f; a.row_state = b.row_state; a.reps = b.reps; a.counts = b.counts;
    a.K = m->K; a.R = R; a.nr = nr; a.b0 = b.b0; a.fstride = fstride; a.N = m->N; a.pairs = b.pairs;
    const dim3 grid((unsigned)chunks, (unsigned)R, (unsigned)((nr + MBAR_BOOT_RB - 1) / MBAR_BOOT_RB));
    if (as_log) hipLaunchKernelGGL(mbar_boot_row_kernel<true>, grid, dim3(MBAR_BLOCK), 0, m->tm.stream, a);
    else        hipLaunchKernelGGL(mbar_boot_row_kernel<false>, grid, dim3(MBAR_BLOCK), 0, m->tm.stream, a);
    const int rows = nr * R;
    hipLaunchKernelGGL(mbar_row_merge_kernel, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, m->tm.stream, b.pairs.get(), rows, chunks, as_log ? 1 : 0,
                       sign, b.row_out.get());
    DEVICE_CHECK(hipGetLastError());
    return 0;
}

// the weighted Gram matrices over the sampled states into gram[nr][Ks][Ks], as many replicates per launch as the partials' cap allows
static int boot_gram_pass(remd_mbar m, int nr)
{
    mbar_bootstrap_state& b = m->boot;
    const int Ks = m->Ks;
    const int T = (Ks + MBAR_TILE - 1) / MBAR_TILE;
    std::vector<int2> tiles;
    for (int ti = 0; ti < T; ti++) for (int tj = 0; tj <= ti; tj++) tiles.push_back(make_int2(ti, tj));
    const int64_t chunk = boot_gram_chunk(m->N);
    const int chunks = (int)((m->N + chunk - 1) / chunk);
    const int64_t per_rep = (int64_t)chunks * Ks * Ks;
    const int per_launch = (int)std::max<int64_t>(1, std::min<int64_t>(nr, MBAR_BOOT_PARTIAL_CAP / per_rep));
    REMD_TRY(b.tiles.grow(nullptr, tiles.size()));
    REMD_TRY(b.gram.grow(nullptr, (size_t)nr * Ks * Ks));
    REMD_TRY(b.gram_partial.grow(nullptr, (size_t)per_launch * per_rep));
    DEVICE_CHECK(hipMemcpyAsync(b.tiles, tiles.data(), sizeof(int2) * tiles.size(), hipMemcpyHostToDevice, m->tm.stream));
    DEVICE_CHECK(hipStreamSynchronize(m->tm.stream));            // (the source is a local)
    mbar_boot_gram_args a;
    a.u = m->u; a.log_den = b.log_den; a.f = b.f; a.srow = m->d_srow; a.tiles = b.tiles; a.reps = b.reps; a.counts = b.counts;
    a.Ks = Ks; a.K = m->K; a.b0 = b.b0; a.N = m->N; a.chunk = chunk; a.partial = b.gram_partial;
    const int64_t entries = (int64_t)Ks * Ks;
    for (int first = 0; first < nr; first += per_launch) {
        const int count = std::min(per_launch, nr - first);
        a.r_first = first;
        hipLaunchKernelGGL(mbar_boot_gram_kernel, dim3((unsigned)tiles.size(), (unsigned)chunks, (unsigned)count), dim3(MBAR_BLOCK), 0, m->tm.stream, a);
        hipLaunchKernelGGL(mbar_boot_gram_sum_kernel, dim3((unsigned)((entries + MBAR_BLOCK - 1) / MBAR_BLOCK), (unsigned)count), dim3(MBAR_BLOCK), 0,
                           m->tm.stream, b.gram_partial.get(), Ks, chunks, b.gram.get() + (int64_t)first * entries);
    }
    DEVICE_CHECK(hipGetLastError());
    return 0;
}

extern "C" {

int remd_mbar_bootstrap_max_batch(remd_mbar m, int* nb)
{
    if (!m || !nb) return remd_fail(nullptr, -1, "remd_mbar_bootstrap_max_batch: the problem or nb is NULL");
    *nb = boot_max_batch(m);
    return 0;
}

int remd_mbar_bootstrap_draw(remd_mbar m, uint64_t seed, const int32_t* sample_states, int b0, int nb)
{
    const std::string who = "remd_mbar_bootstrap_draw";
    if (!m) return remd_fail(nullptr, -1, who + ": the problem is NULL");
    m->boot.nb = 0;                                              // (a refused draw leaves nothing resident)
    if (nb < 1) return remd_fail(nullptr, -1, who + ": nb = " + std::to_string(nb) + " replicates; at least 1 is needed");
    if (b0 < 0 || (int64_t)b0 + nb > INT32_MAX) return remd_fail(nullptr, -1, who + ": the replicates b0 ... b0 + nb - 1 must lie in 0 ... 2^31 - 1");
    if (nb > boot_max_batch(m))
        return remd_fail(nullptr, -1, who + ": nb = " + std::to_string(nb) + " exceeds the " + std::to_string(boot_max_batch(m)) +
                                      " replicates that may be resident at N = " + std::to_string(m->N) + " (remd_mbar_bootstrap_max_batch)");
    if (m->N > INT32_MAX) return remd_fail(nullptr, -1, who + ": N exceeds 2^31 - 1");
    const int K = m->K, Ks = m->Ks;
    const int64_t N = m->N;
    mbar_bootstrap_state& b = m->boot;
    // the samples of every sampled state in ascending order: sample_states, or pymbar's blocks
    std::vector<int> slot(K, -1), start(Ks + 1, 0), samples((size_t)N);
    for (int j = 0; j < Ks; j++) { slot[m->srow[j]] = j; start[j + 1] = start[j] + (int)m->nk_all[m->srow[j]]; }
    if (sample_states) {
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int64_t n = 0; n < N; n++) {
            const int k = sample_states[n];
            if (k < 0 || k >= K || slot[k] < 0)
                return remd_fail(nullptr, -1, who + ": sample_states[" + std::to_string(n) + "] = " + std::to_string(k) + " is not a sampled state");
            const int j = slot[k];
            if (fill[j] >= start[j + 1])
                return remd_fail(nullptr, -1, who + ": sample_states names state " + std::to_string(k) + " more often than N_k = " +
                                              std::to_string((int64_t)m->nk_all[k]));
            samples[fill[j]++] = (int)n;
        }                                                        // (N entries, none above its N_k, sum N_k = N: the histogram is N_k)
    } else {
        for (int64_t n = 0; n < N; n++) samples[n] = (int)n;
    }
    int most = 0;
    for (int j = 0; j < Ks; j++) most = std::max(most, start[j + 1] - start[j]);
    DEVICE_CHECK(hipSetDevice(m->tm.device));
    REMD_TRY(b.state_start.upload(nullptr, start));
    REMD_TRY(b.state_samples.upload(nullptr, samples));
    REMD_TRY(b.counts.grow(nullptr, (size_t)nb * N));
    m->tm.ms = 0.0;
    REMD_TRY(m->tm.begin());
    DEVICE_CHECK(hipMemsetAsync(b.counts, 0, sizeof(uint32_t) * (size_t)nb * N, m->tm.stream));
    const int calls = (most + 1) / 2;
    hipLaunchKernelGGL(mbar_boot_draw_kernel, dim3((unsigned)((calls + MBAR_BLOCK - 1) / MBAR_BLOCK), (unsigned)Ks, (unsigned)nb), dim3(MBAR_BLOCK), 0,
                       m->tm.stream, seed, m->d_srow.get(), b.state_start.get(), b.state_samples.get(), N, b0, b.counts.get());
    DEVICE_CHECK(hipGetLastError());
    REMD_TRY(boot_end(m));
    b.b0 = b0; b.nb = nb;
    return 0;
}

int remd_mbar_bootstrap_counts(remd_mbar m, int b0, int nb, uint32_t* counts)
{
    const std::string who = "remd_mbar_bootstrap_counts";
    if (!m || !counts) return remd_fail(nullptr, -1, who + ": the problem or counts is NULL");
    if (nb < 1) return remd_fail(nullptr, -1, who + ": nb = " + std::to_string(nb) + " replicates; at least 1 is needed");
    const mbar_bootstrap_state& b = m->boot;
    if (b0 < b.b0 || (int64_t)b0 + nb > (int64_t)b.b0 + b.nb)
        return remd_fail(nullptr, -1, who + ": replicates " + std::to_string(b0) + " ... " + std::to_string((int64_t)b0 + nb - 1) +
                                      " are outside the drawn range of " + std::to_string(b.nb) + " from " + std::to_string(b.b0));
    DEVICE_CHECK(hipSetDevice(m->tm.device));
    DEVICE_CHECK(hipMemcpy(counts, b.counts.get() + (int64_t)(b0 - b.b0) * m->N, sizeof(uint32_t) * (size_t)nb * m->N, hipMemcpyDeviceToHost));
    return 0;
}

int remd_mbar_bootstrap_log_denominator(remd_mbar m, int nr, const int32_t* reps, const double* f_b, double* log_den, double* phi)
{
    REMD_TRY(boot_begin(m, "remd_mbar_bootstrap_log_denominator", nr, reps, f_b));
    REMD_TRY(boot_column_pass(m, nr));
    REMD_TRY(boot_end(m));
    if (log_den) DEVICE_CHECK(hipMemcpy(log_den, m->boot.log_den, sizeof(double) * (size_t)nr * m->N, hipMemcpyDeviceToHost));
    if (phi) REMD_TRY(boot_phi(m, nr, f_b, phi));
    return 0;
}

int remd_mbar_bootstrap_self_consistent(remd_mbar m, int nr, const int32_t* reps, const double* f_b, double* f_new)
{
    const std::string who = "remd_mbar_bootstrap_self_consistent";
    if (!f_new) return remd_fail(nullptr, -1, who + ": an output array is NULL");
    REMD_TRY(boot_begin(m, who, nr, reps, f_b));
    std::vector<int> states(m->K);
    for (int k = 0; k < m->K; k++) states[k] = k;
    REMD_TRY(boot_column_pass(m, nr));
    REMD_TRY(boot_row_pass(m, nr, states, nullptr, 0, nullptr, nullptr, true, -1.0));
    REMD_TRY(boot_end(m));
    DEVICE_CHECK(hipMemcpy(f_new, m->boot.row_out, sizeof(double) * (size_t)nr * m->K, hipMemcpyDeviceToHost));
    return 0;
}

int remd_mbar_bootstrap_newton_parts(remd_mbar m, int nr, const int32_t* reps, const double* f_b, double* W_sum, double* gram, double* phi)
{
    const std::string who = "remd_mbar_bootstrap_newton_parts";
    if (!W_sum || !gram) return remd_fail(nullptr, -1, who + ": an output array is NULL");
    REMD_TRY(boot_begin(m, who, nr, reps, f_b));
    const int K = m->K, Ks = m->Ks;
    REMD_TRY(boot_column_pass(m, nr));
    REMD_TRY(boot_row_pass(m, nr, m->srow, m->boot.f, K, nullptr, nullptr, false, 1.0));
    REMD_TRY(boot_gram_pass(m, nr));
    REMD_TRY(boot_end(m));
    std::vector<double> ws((size_t)nr * Ks), g((size_t)nr * Ks * Ks);
    DEVICE_CHECK(hipMemcpy(ws.data(), m->boot.row_out, sizeof(double) * ws.size(), hipMemcpyDeviceToHost));
    DEVICE_CHECK(hipMemcpy(g.data(), m->boot.gram, sizeof(double) * g.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < (int64_t)nr * K; i++) W_sum[i] = 0.0;
    for (int64_t i = 0; i < (int64_t)nr * K * K; i++) gram[i] = 0.0;
    for (int r = 0; r < nr; r++)
        for (int a = 0; a < Ks; a++) {
            W_sum[(int64_t)r * K + m->srow[a]] = ws[(size_t)r * Ks + a];
            for (int c = 0; c < Ks; c++)
                gram[((int64_t)r * K + m->srow[a]) * K + m->srow[c]] = g[((size_t)r * Ks + a) * Ks + c];
        }
    if (phi) REMD_TRY(boot_phi(m, nr, f_b, phi));
    return 0;
}

int remd_mbar_bootstrap_rows(remd_mbar m, int nr, const int32_t* reps, const double* f_b, int L, const double* u_ln, int I, const double* A_in,
                             const int32_t* obs_state, double* f_l, double* log_cA)
{
    const std::string who = "remd_mbar_bootstrap_rows";
    if (!m) return remd_fail(nullptr, -1, who + ": the problem is NULL");
    if (L < 0 || I < 0) return remd_fail(nullptr, -1, who + ": L = " + std::to_string(L) + " or I = " + std::to_string(I) + " is negative");
    if (L == 0 && I == 0) return remd_fail(nullptr, -1, who + ": L and I are both 0");
    const int K = m->K;
    const int64_t N = m->N;
    if ((int64_t)K + L + I > 2 * REMD_MBAR_MAX_STATES)
        return remd_fail(nullptr, -1, who + ": K + L + I = " + std::to_string((int64_t)K + L + I) + " exceeds 2 x REMD_MBAR_MAX_STATES = " +
                                      std::to_string(2 * REMD_MBAR_MAX_STATES));
    if ((L > 0 && (!u_ln || !f_l)) || (I > 0 && (!A_in || !obs_state || !log_cA)))
        return remd_fail(nullptr, -1, who + ": an array of a non-zero count is NULL");
    for (int64_t i = 0; i < (int64_t)L * N; i++)
        if (u_ln[i] != u_ln[i] || u_ln[i] == -std::numeric_limits<double>::infinity())
            return remd_fail(nullptr, -1, who + ": u_ln of perturbed state " + std::to_string(i / N) + " holds a NaN or -inf");
    for (int i = 0; i < I; i++) {
        if (obs_state[i] < 0 || obs_state[i] >= K + L)
            return remd_fail(nullptr, -1, who + ": obs_state[" + std::to_string(i) + "] = " + std::to_string(obs_state[i]) + " is outside 0 ... " +
                                          std::to_string(K + L - 1));
        for (int64_t n = 0; n < N; n++) {
            const double v = A_in[(int64_t)i * N + n];
            if (!(v > 0.0) || !std::isfinite(v))
                return remd_fail(nullptr, -1, who + ": A_in of observable " + std::to_string(i) + " holds a non-positive or non-finite value");
        }
    }
    REMD_TRY(boot_begin(m, who, nr, reps, f_b));
    // the arrays of this call: freed when it returns
    dev_array<double> d_u_ln, d_A, d_f;
    REMD_TRY(d_u_ln.alloc(nullptr, (size_t)L * N));
    REMD_TRY(d_A.alloc(nullptr, (size_t)I * N));
    if (L) DEVICE_CHECK(hipMemcpy(d_u_ln, u_ln, sizeof(double) * (size_t)L * N, hipMemcpyHostToDevice));
    if (I) DEVICE_CHECK(hipMemcpy(d_A, A_in, sizeof(double) * (size_t)I * N, hipMemcpyHostToDevice));
    REMD_TRY(boot_column_pass(m, nr));
    std::vector<double> fcat((size_t)nr * (K + L), 0.0);         // f_b, then f_l, per replicate
    for (int r = 0; r < nr; r++)
        for (int k = 0; k < K; k++) fcat[(size_t)r * (K + L) + k] = f_b[(size_t)r * K + k];
    if (L) {                                                     // eq. 11 on the rows of u_ln
        std::vector<int> states(L);
        for (int l = 0; l < L; l++) states[l] = K + l;
        REMD_TRY(boot_row_pass(m, nr, states, nullptr, 0, d_u_ln, nullptr, true, -1.0));
        DEVICE_CHECK(hipMemcpyAsync(f_l, m->boot.row_out, sizeof(double) * (size_t)nr * L, hipMemcpyDeviceToHost, m->tm.stream));
        DEVICE_CHECK(hipStreamSynchronize(m->tm.stream));
        for (int r = 0; r < nr; r++)
            for (int l = 0; l < L; l++) {
                const double v = f_l[(size_t)r * L + l];
                if (!std::isfinite(v)) {
                    REMD_TRY(boot_end(m));
                    return remd_fail(nullptr, -1, who + ": perturbed state " + std::to_string(l) + " has no sample with a non-zero weight in replicate " +
                                                  std::to_string(reps[r]));
                }
                fcat[(size_t)r * (K + L) + K + l] = v;
            }
    }
    if (I) {
        REMD_TRY(d_f.upload(nullptr, fcat));
        std::vector<int> states(obs_state, obs_state + I);
        REMD_TRY(boot_row_pass(m, nr, states, d_f, K + L, d_u_ln, d_A, true, 1.0));
    }
    REMD_TRY(boot_end(m));
    if (I) DEVICE_CHECK(hipMemcpy(log_cA, m->boot.row_out, sizeof(double) * (size_t)nr * I, hipMemcpyDeviceToHost));
    return 0;
}

}
