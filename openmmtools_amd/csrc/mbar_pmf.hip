// Free energy surfaces over binned samples on the device (include/remd_hip_mbar.h, remd_mbar_pmf and remd_mbar_bootstrap_pmf).
// All f64, no floating-point atomics.
//
// The host groups the binned samples by bin, ascending in each bin (a stable counting sort), and cuts every bin's list into items of
// at most REMD_MBAR_PMF_CHUNK samples; an empty bin has no item.  Every kernel takes its samples through that list: u_n, log_den and
// the rows of u_kn (sample index fastest) are gathered reads, ascending inside an item.
//
//   sum pass     a workgroup per (item, replicate), one thread per sample: the (max, scaled sum) pair of  log w_n = -u_n - log_den_n
//                over the item, weighted by c_n for a replicate
//   bin merge    one thread per (replicate, bin) merges the pairs of the bin's items in item order: f_i
//   cross pass   a workgroup per item: the samples, their W_n,i = exp(f_i + log w_n) and log_den staged in LDS; sum W_n,i^2 by the
//                workgroup, then wave w takes the states w, w + 4, ...: lanes over the samples, sum W_nk W_n,i in lane order
//   cross merge  one thread per (row, bin) sums the items' partials in item order: cross[K][nbins] and diag[nbins]
//
// The items are set by bin_n alone: a result does not depend on the run, and a replicate's not on its batch.
#include "mbar_ctx.h"
#include <cmath>
#include <limits>
#include <algorithm>

static_assert(REMD_MBAR_PMF_CHUNK == MBAR_BLOCK, "one thread per sample of an item");

// item: (first entry of `order`, samples); order[M]: the binned samples, by bin, ascending in each
struct mbar_pmf_items {
    const int2* item; const int* order;
    const double* u_n;           // [N]
    int64_t N;
};

// grid (items, replicates): pairs[r * items + item] = (max over c_n > 0, sum c_n exp(term - guarded max)).  BOOT false: one
// "replicate", c_n = 1, log_den[N]
template <bool BOOT>
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_pmf_sum_kernel(mbar_pmf_items a, const double* __restrict__ log_den, const int* __restrict__ reps,
                                                                  int b0, const uint32_t* __restrict__ counts, double2* __restrict__ pairs)
{
    __shared__ double sh[4];
    const int2 it = a.item[blockIdx.x];
    const int r = blockIdx.y;
    const double* __restrict__ ld = log_den + (int64_t)r * a.N;
    double term = -INFINITY, w = 0.0;
    if ((int)threadIdx.x < it.y) {
        const int n = a.order[it.x + threadIdx.x];
        w = BOOT ? (double)counts[(int64_t)(reps[r] - b0) * a.N + n] : 1.0;
        if (w != 0.0) term = -a.u_n[n] - ld[n];
    }
    const double mraw = block_nanmax(term, sh);
    const double m = mbar_guard(mraw);
    const double t = block_sum(w != 0.0 ? w * exp(term - m) : 0.0, sh);
    if (threadIdx.x == 0) pairs[(int64_t)r * gridDim.x + blockIdx.x] = make_double2(mraw, t);
}

// one thread per (replicate, bin): the pairs of items bin_first[bin] .. bin_first[bin + 1] - 1 merged in item order (as
// mbar_row_merge_kernel merges its chunks); f[r * nbins + bin] = -(ln S + M), +inf for S = 0
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_pmf_bin_merge_kernel(const double2* __restrict__ pairs, const int* __restrict__ bin_first, int nbins,
                                                                        int items, int nr, double* __restrict__ f)
{
    const int64_t idx = (int64_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (idx >= (int64_t)nr * nbins) return;
    const int r = (int)(idx / nbins), bin = (int)(idx % nbins);
    const double2* p = pairs + (int64_t)r * items;
    const int c0 = bin_first[bin], c1 = bin_first[bin + 1];
    double M = -INFINITY;
    for (int c = c0; c < c1; c++) M = nanmax(M, p[c].x);
    M = mbar_guard(M);
    double S = 0.0;
    for (int c = c0; c < c1; c++)
        if (p[c].y != 0.0) S += p[c].y * exp(mbar_guard(p[c].x) - M);
    f[idx] = -(log(S) + M);
}

// grid (items): partial[item][K + 1]: slot k < K = sum over the item of W_nk W_n,i, slot K = sum of W_n,i^2.  An empty bin
// (f_i = +inf) gives zeros.
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_pmf_cross_kernel(mbar_pmf_items a, const int* __restrict__ item_bin, const double* __restrict__ u,
                                                                    const double* __restrict__ log_den, const double* __restrict__ f_k,
                                                                    const double* __restrict__ f_i, int K, double* __restrict__ partial)
{
    __shared__ double sh[4];
    __shared__ int sn[MBAR_BLOCK];
    __shared__ double sw[MBAR_BLOCK], sld[MBAR_BLOCK];
    const int2 it = a.item[blockIdx.x];
    const double fi = f_i[item_bin[blockIdx.x]];
    const int t = threadIdx.x;
    double wi = 0.0;
    if (t < it.y) {
        const int n = a.order[it.x + t];
        const double ld = log_den[n];
        if (isfinite(fi)) wi = exp(fi + (-a.u_n[n] - ld));
        sn[t] = n; sw[t] = wi; sld[t] = ld;
    }
    const double d = block_sum(wi * wi, sh);                      // (its barriers publish the staged item)
    double* __restrict__ out = partial + (int64_t)blockIdx.x * (K + 1);
    if (t == 0) out[K] = d;
    const int lane = t & 63, wave = t >> 6;
    for (int k = wave; k < K; k += MBAR_BLOCK / 64) {
        const double* __restrict__ uk = u + (int64_t)k * a.N;
        const double fk = f_k[k];
        double s = 0.0;
        for (int j = lane; j < it.y; j += 64) s += exp((fk - uk[sn[j]]) - sld[j]) * sw[j];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
        if (lane == 0) out[k] = s;
    }
}

// one thread per (row, bin), row K the diagonal: the items' partials of the bin summed in item order
__global__ __launch_bounds__(MBAR_BLOCK) void mbar_pmf_cross_merge_kernel(const double* __restrict__ partial, const int* __restrict__ bin_first, int nbins,
                                                                          int K, double* __restrict__ cross, double* __restrict__ diag)
{
    const int64_t idx = (int64_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (idx >= (int64_t)(K + 1) * nbins) return;
    const int row = (int)(idx / nbins), bin = (int)(idx % nbins);
    double s = 0.0;
    for (int c = bin_first[bin]; c < bin_first[bin + 1]; c++) s += partial[(int64_t)c * (K + 1) + row];
    if (row < K) cross[idx] = s; else diag[bin] = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// the samples of a call grouped by bin on the device, and u_n: freed when the call returns
struct mbar_pmf_call {
    int items = 0;
    dev_array<int2> item;
    dev_array<int> order, item_bin, bin_first;
    dev_array<double> u_n;
    mbar_pmf_items args(int64_t N) const { mbar_pmf_items a; a.item = item; a.order = order; a.u_n = u_n; a.N = N; return a; }
};

// checks u_n, bin_n and nbins; groups the samples (stable: ascending in each bin) and uploads the lists
static int pmf_prepare(remd_mbar m, const std::string& who, const double* u_n, const int32_t* bin_n, int nbins, mbar_pmf_call& call)
{
    if (!m) return remd_fail(nullptr, -1, who + ": the problem is NULL");
    if (!u_n || !bin_n) return remd_fail(nullptr, -1, who + ": u_n or bin_n is NULL");
    if (nbins < 1 || nbins > REMD_MBAR_PMF_MAX_BINS)
        return remd_fail(nullptr, -1, who + ": nbins = " + std::to_string(nbins) + " is outside 1 ... REMD_MBAR_PMF_MAX_BINS = " +
                                      std::to_string(REMD_MBAR_PMF_MAX_BINS));
    const int64_t N = m->N;
    if (N > INT32_MAX) return remd_fail(nullptr, -1, who + ": N exceeds 2^31 - 1");
    std::vector<int> start(nbins + 1, 0);
    for (int64_t n = 0; n < N; n++) {
        if (u_n[n] != u_n[n] || u_n[n] == -std::numeric_limits<double>::infinity())
            return remd_fail(nullptr, -1, who + ": u_n[" + std::to_string(n) + "] is a NaN or -inf");
        if (bin_n[n] < -1 || bin_n[n] >= nbins)
            return remd_fail(nullptr, -1, who + ": bin_n[" + std::to_string(n) + "] = " + std::to_string(bin_n[n]) + " is outside -1 ... " +
                                          std::to_string(nbins - 1));
        if (bin_n[n] >= 0) start[bin_n[n] + 1]++;
    }
    for (int i = 0; i < nbins; i++) start[i + 1] += start[i];
    std::vector<int> order((size_t)start[nbins]), fill(start.begin(), start.end() - 1);
    for (int64_t n = 0; n < N; n++)
        if (bin_n[n] >= 0) order[fill[bin_n[n]]++] = (int)n;
    std::vector<int2> item;
    std::vector<int> item_bin, bin_first(nbins + 1, 0);
    for (int i = 0; i < nbins; i++) {
        bin_first[i] = (int)item.size();
        for (int s = start[i]; s < start[i + 1]; s += REMD_MBAR_PMF_CHUNK) {
            item.push_back(make_int2(s, std::min(REMD_MBAR_PMF_CHUNK, start[i + 1] - s)));
            item_bin.push_back(i);
        }
    }
    bin_first[nbins] = (int)item.size();
    call.items = (int)item.size();
    DEVICE_CHECK(hipSetDevice(m->tm.device));
    REMD_TRY(call.item.upload(nullptr, item));
    REMD_TRY(call.item_bin.upload(nullptr, item_bin));
    REMD_TRY(call.bin_first.upload(nullptr, bin_first));
    REMD_TRY(call.order.upload(nullptr, order));
    REMD_TRY(call.u_n.alloc(nullptr, (size_t)N));
    DEVICE_CHECK(hipMemcpy(call.u_n, u_n, sizeof(double) * (size_t)N, hipMemcpyHostToDevice));
    return 0;
}

static unsigned pmf_blocks(int64_t n) { return (unsigned)((n + MBAR_BLOCK - 1) / MBAR_BLOCK); }

extern "C" {

int remd_mbar_pmf_chunk(remd_mbar m, int64_t* chunk)
{
    if (!m || !chunk) return remd_fail(nullptr, -1, "remd_mbar_pmf_chunk: the problem or chunk is NULL");
    *chunk = REMD_MBAR_PMF_CHUNK;
    return 0;
}

int remd_mbar_pmf(remd_mbar m, const double* f_k, const double* u_n, const int32_t* bin_n, int nbins, double* f_i, double* cross, double* diag,
                  double* all_parts)
{
    const std::string who = "remd_mbar_pmf";
    mbar_pmf_call call;
    if (m && f_k)
        for (int k = 0; k < m->K; k++)
            if (!std::isfinite(f_k[k])) return remd_fail(nullptr, -1, who + ": f_k[" + std::to_string(k) + "] is not finite");
    if (!f_i || !cross || !diag) return remd_fail(nullptr, -1, who + ": an output array is NULL");
    REMD_TRY(pmf_prepare(m, who, u_n, bin_n, nbins, call));
    const int K = m->K, T = call.items;
    dev_array<double> d_f_i, d_partial, d_cross, d_diag;
    dev_array<double2> d_pairs;
    REMD_TRY(d_f_i.alloc(nullptr, (size_t)nbins));
    REMD_TRY(d_pairs.alloc(nullptr, (size_t)T));
    REMD_TRY(d_partial.alloc(nullptr, (size_t)T * (K + 1)));
    REMD_TRY(d_cross.alloc(nullptr, (size_t)K * nbins));
    REMD_TRY(d_diag.alloc(nullptr, (size_t)nbins));
    REMD_TRY(mbar_begin(m, who.c_str(), f_k));
    REMD_TRY(mbar_column_pass(m));
    const mbar_pmf_items a = call.args(m->N);
    if (T)
        hipLaunchKernelGGL(mbar_pmf_sum_kernel<false>, dim3((unsigned)T, 1u), dim3(MBAR_BLOCK), 0, m->tm.stream, a, m->log_den.get(), (const int*)nullptr, 0,
                           (const uint32_t*)nullptr, d_pairs.get());
    hipLaunchKernelGGL(mbar_pmf_bin_merge_kernel, dim3(pmf_blocks(nbins)), dim3(MBAR_BLOCK), 0, m->tm.stream, d_pairs.get(), call.bin_first.get(), nbins, T,
                       1, d_f_i.get());
    if (T)
        hipLaunchKernelGGL(mbar_pmf_cross_kernel, dim3((unsigned)T), dim3(MBAR_BLOCK), 0, m->tm.stream, a, call.item_bin.get(), m->u.get(), m->log_den.get(),
                           m->f.get(), d_f_i.get(), K, d_partial.get());
    hipLaunchKernelGGL(mbar_pmf_cross_merge_kernel, dim3(pmf_blocks((int64_t)(K + 1) * nbins)), dim3(MBAR_BLOCK), 0, m->tm.stream, d_partial.get(),
                       call.bin_first.get(), nbins, K, d_cross.get(), d_diag.get());
    DEVICE_CHECK(hipGetLastError());
    REMD_TRY(mbar_end(m));
    DEVICE_CHECK(hipMemcpy(f_i, d_f_i, sizeof(double) * (size_t)nbins, hipMemcpyDeviceToHost));
    DEVICE_CHECK(hipMemcpy(cross, d_cross, sizeof(double) * (size_t)K * nbins, hipMemcpyDeviceToHost));
    DEVICE_CHECK(hipMemcpy(diag, d_diag, sizeof(double) * (size_t)nbins, hipMemcpyDeviceToHost));
    if (all_parts) {                                             // W_n,z = exp(f_z - f_i) W_n,i on the samples of bin i: the same sums, in bin order
        for (int64_t i = 0; i < 2 + (int64_t)K + nbins; i++) all_parts[i] = 0.0;
        double lo = std::numeric_limits<double>::infinity();
        for (int i = 0; i < nbins; i++) lo = std::min(lo, f_i[i]);
        all_parts[0] = lo;
        if (std::isfinite(lo)) {
            double s = 0.0;
            for (int i = 0; i < nbins; i++) if (std::isfinite(f_i[i])) s += std::exp(lo - f_i[i]);
            const double fz = lo - std::log(s);
            all_parts[0] = fz;
            for (int i = 0; i < nbins; i++) {
                if (!std::isfinite(f_i[i])) continue;
                const double e = std::exp(fz - f_i[i]);
                all_parts[1] += e * e * diag[i];
                for (int k = 0; k < K; k++) all_parts[2 + k] += e * cross[(int64_t)k * nbins + i];
                all_parts[2 + K + i] = e * diag[i];
            }
        }
    }
    return 0;
}

int remd_mbar_bootstrap_pmf(remd_mbar m, int nr, const int32_t* reps, const double* f_b, const double* u_n, const int32_t* bin_n, int nbins, double* f_i)
{
    const std::string who = "remd_mbar_bootstrap_pmf";
    mbar_pmf_call call;
    if (!f_i) return remd_fail(nullptr, -1, who + ": an output array is NULL");
    REMD_TRY(pmf_prepare(m, who, u_n, bin_n, nbins, call));
    REMD_TRY(boot_begin(m, who, nr, reps, f_b));
    const int T = call.items;
    mbar_bootstrap_state& b = m->boot;
    dev_array<double> d_f_i;
    dev_array<double2> d_pairs;
    REMD_TRY(d_f_i.alloc(nullptr, (size_t)nr * nbins));
    REMD_TRY(d_pairs.alloc(nullptr, (size_t)nr * T));
    REMD_TRY(boot_column_pass(m, nr));
    if (T)
        hipLaunchKernelGGL(mbar_pmf_sum_kernel<true>, dim3((unsigned)T, (unsigned)nr), dim3(MBAR_BLOCK), 0, m->tm.stream, call.args(m->N), b.log_den.get(),
                           b.reps.get(), b.b0, b.counts.get(), d_pairs.get());
    hipLaunchKernelGGL(mbar_pmf_bin_merge_kernel, dim3(pmf_blocks((int64_t)nr * nbins)), dim3(MBAR_BLOCK), 0, m->tm.stream, d_pairs.get(),
                       call.bin_first.get(), nbins, T, nr, d_f_i.get());
    DEVICE_CHECK(hipGetLastError());
    REMD_TRY(boot_end(m));
    DEVICE_CHECK(hipMemcpy(f_i, d_f_i, sizeof(double) * (size_t)nr * nbins, hipMemcpyDeviceToHost));
    return 0;
}

}
